"""The cases of tests/test_coverage_abi.py (the oracle alone: do the inputs exercise what they claim?) and
tests/test_coverage_gpu.py (rz_coverage and rz_outline against tests/coverage_ref.py, byte for byte).

Coverage cases: name -> (scene, width, height).
  reference   RayZen's own scene at 64 x 48: big and small instances, misses, instances that cover nothing
  instanced   sixteen small instances over a floor at 64 x 36: instances of a few pixels, tiles with many keys
  lattice     16 x 12 cubes of about a pixel each at 48 x 36: every one of the 192 visible, two dozen keys in one 8 x 8 tile --
              the wave's grouping loop runs two dozen times
  axis        two cubes on the view axis at 33 x 25, the far one hidden: an instance inside the frustum with an empty record
  ties        four coincident sheets (tests/tie_cases.py: "stack"): who owns a pixel depends on the visiting order
Outline cases: hand-made id images, OUTLINE_CASES."""
import numpy as np

import coverage_ref as CR
import tie_cases as TC
from rayzen_amd import scene as S
from tlas_shapes import set_transforms

F32 = np.float32


def lattice_scene():
    """16 x 12 cubes (S.make_cube scaled 0.18, 0.6 apart) at z = -6, two shared meshes alternating, every instance uploaded at
    identity and placed by its transform (as tlas_shapes.Shape.scene places its instances); camera at (0, 0, 3), aspect 4/3."""
    sc = S.Scene(camera=S.Camera(position=(0.0, 0.0, 3.0), aspect=4 / 3))
    a, b = sc.add_mesh(S.make_cube(0)), sc.add_mesh(S.make_cube(2))
    ids = [sc.add_object(b if i % 2 else a) for i in range(16 * 12)]
    sc.build(share_meshes=True)
    xf = [S.scale(S.translate(S.identity(), ((i % 16 - 7.5) * 0.6, (i // 16 - 5.5) * 0.6, -6.0)), (0.18, 0.18, 0.18)) for i in range(16 * 12)]
    set_transforms(sc, ids, np.stack(xf))
    return sc


def axis_scene():
    """Two cubes on the view axis: scale 1 at z = -2 hides scale 0.5 at z = -6."""
    sc = S.Scene(camera=S.Camera(position=(0.0, 0.0, 3.0), aspect=33 / 25))
    cube = sc.add_mesh(S.make_cube(0))
    sc.add_object(cube, S.translate(S.identity(), (0.0, 0.0, -2.0)))
    sc.add_object(cube, S.scale(S.translate(S.identity(), (0.0, 0.0, -6.0)), (0.5, 0.5, 0.5)))
    return sc.build(share_meshes=True)


CASES = {
    "reference": (lambda: S.reference_scene(), 64, 48),
    "instanced": (lambda: S.instanced_scene(n=12), 64, 36),
    "lattice": (lattice_scene, 48, 36),
    "axis": (axis_scene, 33, 25),
    "ties": (lambda: TC.scene("stack", 0), 64, 48),
}
PARTIAL = [(1, 1), (9, 7), (65, 5)]         # frames of partial tiles, on the reference scene

_cases, _images = {}, {}


def case(name):
    """(scene, w, h, ids, t): the built scene and the oracle's images of it (cached: the tests share them and leave them unchanged)."""
    if name not in _cases:
        make, w, h = CASES[name]
        sc = make()
        _cases[name] = (sc, w, h) + images(name, sc, w, h)
    return _cases[name]


def images(key, sc, w, h):
    if (key, w, h) not in _images:
        _images[key, w, h] = CR.oracle_images(sc.arrays, sc.camera, w, h)
    return _images[key, w, h]


def n_instances(sc):
    return len(sc.arrays[S.BIND_INSTANCES])


def tile_keys(ids, tile=8):
    """The most distinct keys (instances, and the miss) any tile x tile tile of the frame's grid holds."""
    h, w = ids.shape
    return max(len(np.unique(ids[y:y + tile, x:x + tile])) for y in range(0, h, tile) for x in range(0, w, tile))


def rectangles(w, h):
    """The rectangles every frame is asked for: the whole frame, a single pixel, one that crosses tile borders at coordinates that
    are no multiples of 8, one partly outside the frame, and two that are empty after clipping."""
    return {"whole": None, "stated": (0, 0, w, h), "pixel": (w // 2, h // 2, w // 2 + 1, h // 2 + 1), "crossing": (3, 1, 13, 4),
            "partly-outside": (w - 5, -3, w + 9, 3), "outside": (w, 0, w + 8, h), "degenerate": (5, 2, 5, 4)}


# ---------------------------------------------------------------------------------------------------------------------
# hand-made id images for rz_outline: name -> (ids (h, w) int32, n_instances, selected indices)

def _blank(h, w, fill=0):
    return np.full((h, w), fill, np.int32)


def _corner():
    ids = _blank(12, 14)
    ids[0, 0] = 5
    return ids, 8, [5]


def _border():
    ids = _blank(10, 20)
    ids[3:10, 15:20] = 2            # touches the right and the top border
    ids[0:2, 0:6] = 3               # and the bottom-left corner
    return ids, 4, [2, 3]


def _out_of_range():
    ids = _blank(9, 16, -1)
    ids[2:5, 2:6] = 40              # >= n_instances: unselected though bit 40 & 31 of word 1 would exist in a longer set
    ids[5:8, 8:12] = 7
    ids[1, 12] = 37                 # the last valid index of a set of 38
    ids[7, 1] = 38                  # the first invalid one
    ids[0, 15] = 0x7fffffff
    ids[8, 0] = -0x80000000
    return ids, 38, [7, 37, 6]


def _one_pixel():
    return np.array([[3]], np.int32), 4, [3]


def _one_pixel_unselected():
    return np.array([[3]], np.int32), 4, [1]


def _stripes(h, w):
    """Selected columns and dots spread over the tiles of a wide, low image: the halo crosses tile borders both ways."""
    ids = _blank(h, w)
    ids[:, ::37] = 9
    ids[h // 2, 5::29] = 70
    ids[0, w - 1] = 70
    return ids, 71, [9, 70]


OUTLINE_CASES = {
    "corner": _corner(), "border": _border(), "out-of-range": _out_of_range(), "one-pixel": _one_pixel(),
    "one-pixel-unselected": _one_pixel_unselected(), "nothing-selected": (_blank(6, 40, 2), 33, []),
    "65x5": _stripes(5, 65), "257x3": _stripes(3, 257),
}


def images_for(ids, seed=3):
    """An rgb32f and an rgba8 image of the id image's size with values below 0 and above 1 among the floats."""
    h, w = ids.shape
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(-0.25, 1.5, (h, w, 3)).astype(F32)
    rgba8 = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    return rgb, rgba8

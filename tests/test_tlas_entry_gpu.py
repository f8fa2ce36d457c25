"""A closest-hit query of the sample kernels' non-counting instantiations may enter the TLAS's pop-order list BEHIND its root
(rz_trace.h: RZ_TLAS_ENTRY): the root's box holds both its children's, so its step says nothing the
children's steps do not -- where the list's maker found that to hold (rz_scene_dev.h: tlas_entry_verdict) and no lane's
reciprocal direction is zero, infinite or NaN (rz_device_math.h: the wave test of rcp3).  The oracle knows no shortcut: every
frame here is compared with it bit for bit, whole frame, on the group code and on the compacting claims.

  1. lists of 1 (no shortcut: there is no child), 3, 13 and 39 records; an instance of an empty mesh, as in RayZen's own scene;
     a camera exactly on a plane of the root's box looking along an axis; a directional light exactly along -y over an
     axis-aligned floor (its shadow rays have zero components: infinite reciprocals, the guard's path); a camera inside a
     child's box; a camera outside the root looking away from it; a transparent scene;
  2. the list made again, by the host and by the device builder, after the instances have moved;
  3. on the CPU: each case's list gets the verdict its name says, from a numpy statement of the rule (tests/tlas_entry_ref.py)."""
import numpy as np
import pytest

from rayzen_amd import scene as S
import tlas_entry_ref as R
import tlas_front_cases as C

f32 = np.float32


def _scene(camera=None, lights=None, aspect=37 / 29):
    cam = camera or S.Camera(position=(0.5, 2.0, 7.0), target=(-0.05, -0.25, -1.0), aspect=aspect)
    return S.Scene(lights=lights, camera=cam)


def _floor(s, cube):
    return C.cube_at(s, cube, (0.0, -1.5, 0.0), (6.0, 0.25, 6.0))


def one():
    s = _scene()
    C.cube_at(s, s.add_mesh(S.make_cube(0)), (0.0, 0.0, 0.0), 1.0, 0.5)
    return s.build()


def two():
    s = _scene()
    cube = s.add_mesh(S.make_cube(4))
    _floor(s, cube)
    C.cube_at(s, s.add_mesh(S.make_cube(0)), (0.3, 0.0, 0.0), 1.0, 0.5)
    return s.build()


def several(n):
    """The floor and n - 1 cubes on a ring around the origin, turned, of three materials (one a mirror)."""
    s = _scene()
    _floor(s, s.add_mesh(S.make_cube(4)))
    meshes = [s.add_mesh(S.make_cube(m)) for m in (0, 1, 2)]
    for k in range(n - 1):
        a = 2.0 * np.pi * k / (n - 1)
        rad = 2.2 + 1.2 * (k % 3)
        C.cube_at(s, meshes[k % 3], (rad * np.cos(a), -0.6 + 0.35 * (k % 4), rad * np.sin(a)), 0.35 + 0.1 * (k % 2), 0.3 * k)
    return s.build()


def empty_mesh():
    s = _scene()
    _floor(s, s.add_mesh(S.make_cube(4)))
    C.cube_at(s, s.add_mesh(S.make_cube(0)), (0.3, 0.0, 0.0), 1.0, 0.5)
    s.add_object(s.add_mesh(S.make_cube(0)[:0]))
    C.cube_at(s, s.add_mesh(S.make_cube(1)), (-2.5, 0.0, -1.0), 0.7)
    return s.build()


def camera_on_root_plane():
    """Two axis-aligned cubes, x in [-3, -1] and [1, 3], y in [-1, 1]: the root's box ends at y = 1, where the camera stands,
    looking along -z."""
    s = _scene(S.Camera(position=(0.0, 1.0, 6.0), target=(0.0, 0.0, -1.0), aspect=37 / 29))
    cube = s.add_mesh(S.make_cube(0))
    C.cube_at(s, cube, (-2.0, 0.0, 0.0))
    C.cube_at(s, cube, (2.0, 0.0, 0.0))
    return s.build()


def light_along_minus_y():
    s = _scene(lights=C.light((0.0, 1.0, 0.0, 0.0), 2.0))
    _floor(s, s.add_mesh(S.make_cube(4)))
    C.cube_at(s, s.add_mesh(S.make_cube(0)), (0.3, 0.6, 0.0), (1.0, 0.2, 1.0))
    C.cube_at(s, s.add_mesh(S.make_cube(1)), (-2.0, -0.75, 1.0), 0.5)
    return s.build()


def camera_inside_child():
    """The camera stands inside the box (and the mesh) of a big cube, a small one beside it."""
    s = _scene(S.Camera(position=(0.5, 0.3, 2.0), target=(-0.2, -0.1, -1.0), aspect=37 / 29))
    C.cube_at(s, s.add_mesh(S.make_cube(4)), (0.0, 0.0, 0.0), 4.0)
    C.cube_at(s, s.add_mesh(S.make_cube(0)), (-0.5, -0.5, -1.5), 0.6, 0.4)
    return s.build()


def camera_looking_away():
    s = _scene(S.Camera(position=(0.0, 1.0, 9.0), target=(0.1, 0.2, 1.0), aspect=37 / 29))
    _floor(s, s.add_mesh(S.make_cube(4)))
    C.cube_at(s, s.add_mesh(S.make_cube(0)), (0.3, 0.0, 0.0), 1.0, 0.5)
    return s.build()


def glass():
    s = _scene()
    _floor(s, s.add_mesh(S.make_cube(4)))
    C.cube_at(s, s.add_mesh(S.make_cube(3)), (0.6, 0.0, 1.0), 0.9, 0.4)
    C.cube_at(s, s.add_mesh(S.make_cube(0)), (-0.8, -0.4, -1.5), 0.8, 0.2)
    return s.build()


# name -> (builder, the verdict its list must get: None = either, the frame decides)
CASES = {
    "one": (one, 0),
    "two": (two, 1),
    "seven": (lambda: several(7), 1),
    "twenty": (lambda: several(20), 1),
    "empty_mesh": (empty_mesh, None),
    "camera_on_root_plane": (camera_on_root_plane, 1),
    "light_along_minus_y": (light_along_minus_y, 1),
    "camera_inside_child": (camera_inside_child, 1),
    "camera_looking_away": (camera_looking_away, 1),
    "glass": (glass, 1),
}
_scenes = {}


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = CASES[name][0]()
    return _scenes[name]


def _render(monkeypatch, name, width, height, spp, bounces, claims):
    from rayzen_amd.renderer import Renderer
    C.claims_env(monkeypatch, claims)
    sc = scene_of(name)
    r = Renderer(0)
    r.upload_scene(sc)
    gpu = C.frame(r, sc, width, height, spp, bounces, claims)
    r.close()
    C.same_bits(gpu, C.reference(name, sc, width, height, spp, bounces), f"{name} {width}x{height}, {spp} spp, claims {claims}")


# ---- 1 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
# the claims at one pixel per wave, partial tiles | the group code at four pixels per wave
@pytest.mark.parametrize("width,height,spp,bounces,claims", [(37, 29, 64, 2, 4), (64, 48, 16, 3, None)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_matches_the_oracle(monkeypatch, name, width, height, spp, bounces, claims):
    _render(monkeypatch, name, width, height, spp, bounces, claims)


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", [(8, 8), (5, 3)])
@pytest.mark.parametrize("name", ["two", "camera_on_root_plane", "light_along_minus_y"])
def test_tiny_frames(monkeypatch, name, width, height):
    _render(monkeypatch, name, width, height, 64, 2, 4)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------

def _moved(sc, k):
    """Other transforms for every cube but the floor: state k of the scene `seven` (the host scene follows; its arrays are the oracle's)."""
    n = len(sc.arrays[S.BIND_INSTANCES])
    for i in range(1, n):
        a = 2.0 * np.pi * i / (n - 1) + 0.4 * k
        sc.set_transform(i, C.cube_xf((2.8 * np.cos(a), -0.3 + 0.2 * ((i + k) % 3), 2.8 * np.sin(a)), 0.45, 0.2 * i + k))
    sc.update_dynamic()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["host", "device"])
def test_list_made_again_after_the_instances_moved(monkeypatch, path):
    from rayzen_amd.renderer import Renderer
    C.claims_env(monkeypatch, 4)
    sc = several(7)
    r = Renderer(0)
    r.upload_scene(sc)
    W, H = 37, 29
    C.same_bits(C.frame(r, sc, W, H, 64, 2, 4), C.reference("seven", sc, W, H, 64, 2), "before the move")
    for k in (1, 2):
        _moved(sc, k)
        if path == "host":
            r.update_dynamic(sc)
        else:
            r.update_transforms(sc.arrays[S.BIND_INSTANCES]["transform"])
        assert R.entry_verdict(R.dfs_of(sc)) == 1
        C.same_bits(C.frame(r, sc, W, H, 64, 2, 4), C.reference(("seven moved", k), sc, W, H, 64, 2), f"{path} path, move {k}")
    r.close()


# ---- 3. the inputs do what they are for (CPU only) ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_each_case_has_the_verdict_its_name_says(name):
    sc = scene_of(name)
    dfs = R.dfs_of(sc)
    v = R.entry_verdict(dfs)
    print(f"{name}: {len(dfs)} records, verdict {v}")
    want = CASES[name][1]
    assert want is None or v == want, (name, v)
    assert len(dfs) == 2 * len(sc.arrays[S.BIND_INSTANCES]) - 1
    if name == "one":
        assert len(dfs) == 1
    if name == "light_along_minus_y":       # the shadow rays of its only light: two zero components, two infinite reciprocals
        d = np.asarray(sc.lights[0]["positionOrDirection"], f32)
        assert d[3] == 0.0 and d[0] == 0.0 and d[2] == 0.0 and d[1] > 0.0
    if name == "camera_on_root_plane":
        assert f32(sc.camera.position[1]) == dfs[0]["bmax"][1]
    if name in ("camera_inside_child", "camera_looking_away"):
        p = np.asarray(sc.camera.position, f32)
        inside = [bool((r["bmin"] <= p).all() and (p <= r["bmax"]).all()) for r in dfs]
        assert inside[0] == (name == "camera_inside_child")
        if name == "camera_inside_child":
            assert any(inside[1:])
        else:
            hits = R.primary_hits(sc, 37, 29)
            assert not hits.any()

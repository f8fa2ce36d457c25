"""rz_draw_lines without a GPU: the C-ABI structs and symbols, the numpy helpers of rayzen_amd/lines.py, the restatement
(lines_ref.py) on hand-made cases, the depth test against the CPU oracle's hits on the Cornell scene, and the kernels' cull
against the restatement's coverage.  Frames whose sizes are powers of two with view = proj = identity make every screen
coordinate below exact: sx = (x * 0.5 + 0.5) * W."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lines_ref as LR
from oracle import rzo
from rayzen_amd import _lib
from rayzen_amd import lines as LN
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, editor_rays
from coverage_ref import oracle_scene
from test_rays_abi import _kernel_metadata

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.eye(4, dtype=F32).reshape(16)
# clip.w = -z: a point at z = -1 has w = 1, a point at z = +1 lies behind the camera
PERSP = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1, 0, 0, 0, 0], F32)
WHITE, RED, BLUE = (255, 255, 255, 255), (255, 0, 0, 128), (0, 0, 255, 128)


def ndc(s, n):
    """The world coordinate that lands on screen coordinate s of n pixels under the identity matrices."""
    return s / n * 2.0 - 1.0


def seg(ax, ay, bx, by, color=WHITE, w=8, h=8, z=0.0):
    return LN.segments([(ndc(ax, w), ndc(ay, h), z)], [(ndc(bx, w), ndc(by, h), z)], color)


def black(w=8, h=8):
    return np.zeros((h, w, 3), F32), np.zeros((h, w, 4), np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the ABI

def _header_fields(name):
    text = open(os.path.join(ROOT, "include", "rayzen_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*\]", "", d.split()[-1]) for d in body.split(";") if d.strip()]


def test_structs_sizes_field_order_and_symbols():
    L = _lib.hip()
    assert (_lib.SIZEOF_LINE, _lib.SIZEOF_LINES_PARAMS) == (42, 43)
    assert L.rz_sizeof(42) == 32 == _lib.LINE_DTYPE.itemsize and L.rz_sizeof(43) == 32 == C.sizeof(_lib.LinesParams)
    assert L.rz_sizeof(41) == 0
    assert _header_fields("rz_line") == ["a", "color", "b", "instance"] == list(_lib.LINE_DTYPE.names)
    assert [_lib.LINE_DTYPE.fields[f][1] for f in _lib.LINE_DTYPE.names] == [0, 12, 16, 28]
    assert _header_fields("rz_lines_params") == [f for f, _ in _lib.LinesParams._fields_]
    assert [getattr(_lib.LinesParams, f).offset for f, _ in _lib.LinesParams._fields_] == [0, 4, 8, 12, 16, 20]
    d = _lib.LINES_DEFAULTS
    assert (d["width"], d["near_w"], d["depth_bias"], d["hidden_alpha"], d["smooth"]) == (1.5, 0.01, 2.0 ** -8, 0.0, 0) and d == LR.DEFAULTS
    assert _lib.LINES_HOST == 1 and _lib.LINES_MAX == 1 << 20
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5      # additive: the revision stays
    assert hasattr(C.CDLL(_lib.HIP_SO), "rz_draw_lines") and "rz_draw_lines" in _lib.HIP_SYMBOLS
    from rayzen_amd.renderer import LINE_DTYPE, Renderer
    assert LINE_DTYPE is _lib.LINE_DTYPE
    for m in ("draw_lines", "draw_lines_device"):
        assert callable(getattr(Renderer, m)), m
    # the colour bytes are r, g, b, alpha in memory order
    ln = LN.segments([(0, 0, 0)], [(1, 2, 3)], (1, 2, 3, 4), instance=7)
    assert ln.tobytes()[12:16] == bytes([1, 2, 3, 4]) and np.frombuffer(ln.tobytes(), np.int32)[7] == 7


def test_kernels_spill_nothing():
    meta = _kernel_metadata(_lib.HIP_SO)
    ours = {k: v for k, v in meta.items() if "rz_lines_" in k}
    assert len(ours) == 5, sorted(ours)                     # project, bin<count>, bin<fill>, scan, draw
    for name, (spill, priv) in ours.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


# ---------------------------------------------------------------------------------------------------------------------
# the numpy helpers

def test_mesh_edges_of_a_cube_and_the_box():
    cube = S.make_cube(0)
    assert len(cube) == 12
    e = LN.mesh_edges(cube, (255, 255, 0), instance=2)
    assert e.dtype == _lib.LINE_DTYPE and len(e) == 18 and (e["instance"] == 2).all() and (e["color"] == (255, 255, 0, 255)).all()
    keys = {frozenset((tuple(r["a"].tolist()), tuple(r["b"].tolist()))) for r in e}
    assert len(keys) == 18 and all(len(k) == 2 for k in keys)                  # each once, none degenerate
    # first-appearance order: the first triangle's three edges lead
    t0 = cube[0]
    assert [(tuple(r["a"].tolist()), tuple(r["b"].tolist())) for r in e[:3]] == \
        [(tuple(t0[p].tolist()), tuple(t0[q].tolist())) for p, q in (("v0", "v1"), ("v1", "v2"), ("v2", "v0"))]
    # a reversed duplicate and a repeated triangle add nothing
    assert len(LN.mesh_edges(np.concatenate([cube, cube[::-1]]), (1, 1, 1))) == 18
    b = LN.box((-1, -2, -3), (1, 2, 3), (0.0, 1.0, 0.0, 0.5))
    assert len(b) == 12 and (b["instance"] == -1).all() and (b["color"] == (0, 255, 0, 128)).all()
    bk = {frozenset((tuple(r["a"].tolist()), tuple(r["b"].tolist()))) for r in b}
    assert len(bk) == 12 and all(sum(p != q for p, q in zip(*sorted(k))) == 1 for k in bk)    # axis-parallel, each once
    assert len(LN.axes((0, 0, 0), 1.0)) == 3 and len(LN.grid(2.0, 0.5, (128, 128, 128))) == 18
    cam = S.Camera()
    f = LN.frustum(cam.inv_view, cam.inv_proj, (255, 255, 255))
    assert len(f) == 12 and np.isfinite(f["a"]).all() and np.isfinite(f["b"]).all()
    near = np.linalg.norm(f["a"][0] - cam.position)
    assert 0.09 < near < 0.2                                                    # a near corner lies about `near` from the eye


# ---------------------------------------------------------------------------------------------------------------------
# hand-made cases on the restatement alone

def test_the_edge_comparison_is_strict():
    rgb, _ = black()
    _, out, info = LR.draw(seg(0.5, 3.5, 7.5, 3.5), IDENT, IDENT, 8, 8, rgb32f=rgb, width=2.0)
    assert info["touched"][3].all()                                             # d = 0 on the row the line runs through
    assert not info["touched"][2].any() and not info["touched"][4].any()        # d == hw == 1 exactly: not covered
    assert (out[3] == 1.0).all() and out.sum() == 24.0
    _, _, wider = LR.draw(seg(0.5, 3.5, 7.5, 3.5), IDENT, IDENT, 8, 8, rgb32f=rgb, width=2.0 + 2.0 ** -20)
    assert wider["touched"][2].all() and wider["touched"][4].all()


def test_a_zero_length_line_is_a_dot():
    rgb, _ = black()
    _, _, info = LR.draw(seg(3.5, 3.5, 3.5, 3.5), IDENT, IDENT, 8, 8, rgb32f=rgb, width=2.0)
    assert np.argwhere(info["touched"]).tolist() == [[3, 3]]
    _, _, info = LR.draw(seg(3.5, 3.5, 3.5, 3.5), IDENT, IDENT, 8, 8, rgb32f=rgb, width=3.0)
    assert info["touched"].sum() == 9 and info["touched"][2:5, 2:5].all()       # sqrt(2) < 1.5


def test_lines_through_and_behind_the_camera_plane():
    w = h = 16
    rgb = np.zeros((h, w, 3), F32)
    # A in front at the centre of the screen, B behind the camera to the right: drawn from the centre to the right edge, where
    # the clipped end lies far outside; the mirror image of B (x / w with w < 0) would lie to the left
    one = LN.segments([(0.0, ndc(8.5, h), -1.0)], [(0.5, ndc(8.5, h), 1.0)], WHITE)
    P = LR.project(one, IDENT, PERSP, w, h)
    assert not P["drop"][0] and P["sax"][0] == 8.0 and P["sbx"][0] > 200.0 and P["ib"][0] == F32(1.0) / F32(0.01)
    _, _, info = LR.draw(one, IDENT, PERSP, w, h, rgb32f=rgb, width=1.0)
    cols = np.flatnonzero(info["touched"].any(axis=0))
    assert cols.tolist() == list(range(8, 16)) and not info["touched"][:, :8].any()
    swapped = LN.segments(one["b"], one["a"], WHITE)                             # "only B fails" and "only A fails" agree
    _, _, info2 = LR.draw(swapped, IDENT, PERSP, w, h, rgb32f=rgb, width=1.0)
    assert (info2["touched"] == info["touched"]).all()
    both = LN.segments([(0.0, 0.0, 1.0)], [(0.5, 0.1, 2.0)], WHITE)
    out8, out32, info = LR.draw(both, IDENT, PERSP, w, h, rgb32f=rgb, rgba8=np.full((h, w, 4), 7, np.uint8), width=16.0)
    assert LR.project(both, IDENT, PERSP, w, h)["drop"][0] and not info["touched"].any()
    assert (out8 == 7).all() and (out32 == 0).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_ends_touch_nothing(bad):
    rgb, _ = black()
    for k in range(3):
        for end in ("a", "b"):
            ln = seg(0.5, 3.5, 7.5, 3.5)
            ln[end][0, k] = bad
            for proj in (IDENT, PERSP):
                if proj is PERSP:
                    other = "b" if end == "a" else "a"
                    ln[other][0, 2] = -1.0
                _, out, info = LR.draw(ln, IDENT, proj, 8, 8, rgb32f=rgb, width=16.0, smooth=1)
                assert not info["touched"].any() and (out == 0).all(), (k, end, bad)     # (0 * z is a NaN in every row of m4v)


def test_the_smooth_ramp():
    rgb, _ = black()
    _, out, info = LR.draw(seg(-8.0, 3.5, 16.0, 3.5), IDENT, IDENT, 8, 8, rgb32f=rgb, width=2.0, smooth=1)
    assert (out[3] == 1.0).all() and (out[2] == 0.5).all() and (out[4] == 0.5).all()          # cov = clamp(1.5 - d): 1.5, 0.5
    assert not info["touched"][1].any() and not info["touched"][5].any()                     # d = 2: cov = 0, not covered
    _, out, _ = LR.draw(seg(-8.0, 3.75, 16.0, 3.75), IDENT, IDENT, 8, 8, rgb32f=rgb, width=2.0, smooth=1)
    assert [float(out[r, 0, 0]) for r in range(1, 7)] == [0.0, 0.25, 1.0, 0.75, 0.0, 0.0]    # d = 2.25, 1.25, 0.25, 0.75, 1.75, 2.75
    # the alpha byte scales it: 128 / 255 * 0.5
    _, out, _ = LR.draw(seg(-8.0, 3.5, 16.0, 3.5, (255, 255, 255, 128)), IDENT, IDENT, 8, 8, rgb32f=rgb, width=2.0, smooth=1)
    assert out[2, 0, 0] == F32(128) / F32(255) * F32(0.5)


def test_blending_runs_in_line_order():
    rgb, _ = black()
    cross = np.concatenate([seg(0.5, 0.5, 7.5, 7.5, RED), seg(0.5, 7.5, 7.5, 0.5, BLUE)])
    _, fwd, a = LR.draw(cross, IDENT, IDENT, 8, 8, rgb32f=rgb, width=2.0)
    _, rev, b = LR.draw(cross, IDENT, IDENT, 8, 8, rgb32f=rgb, width=2.0, order=[1, 0])
    both = np.argwhere((fwd != 0).all(axis=-1) | ((fwd[..., 0] != 0) & (fwd[..., 2] != 0)))
    assert len(both) >= 4 and (a["touched"] == b["touched"]).all()
    assert (fwd != rev).any() and (fwd[..., 0] != rev[..., 0])[tuple(both.T)].all()
    al = F32(128) / F32(255)
    y, x = both[0]
    assert fwd[y, x, 0] == (F32(0) * (F32(1) - al) + F32(1) * al) * (F32(1) - al) + F32(0) * al     # red first, then blue over it
    assert fwd[y, x, 2] == al * (F32(1) - al) * F32(0) + F32(1) * al or fwd[y, x, 2] == F32(0) * (F32(1) - al) + F32(1) * al


def test_rgba8_is_quantised_once():
    """Two lines over one pixel row.  Quantising after each line gives another byte than the definition, which converts the byte
    once, blends both lines in float and quantises once."""
    _, img = black()
    img[...] = (10, 200, 77, 9)
    two = np.concatenate([seg(0.5, 3.5, 7.5, 3.5, (200, 30, 90, 100)), seg(0.5, 3.5, 7.5, 3.5, (250, 250, 140, 100))])
    once, _, info = LR.draw(two, IDENT, IDENT, 8, 8, rgba8=img, width=1.0)
    each, _, _ = LR.draw(two, IDENT, IDENT, 8, 8, rgba8=img, width=1.0, quantise_each=True)
    assert info["touched"][3].all() and info["touched"].sum() == 8
    assert (once[..., 3] == 9).all() and (once[~info["touched"]] == (10, 200, 77, 9)).all()
    assert (once[3, 0, 0], each[3, 0, 0]) == (149, 150), (once[3, 0], each[3, 0])
    # by hand, channel 0
    al = F32(100) / F32(255)
    v = (F32(10) / F32(255)) * (F32(1) - al) + (F32(200) / F32(255)) * al
    v = v * (F32(1) - al) + (F32(250) / F32(255)) * al
    assert once[3, 0, 0] == int(np.rint(v * F32(255)))


# ---------------------------------------------------------------------------------------------------------------------
# the depth test against the oracle's hits on the Cornell scene

_HITS = {}


def cornell_hits(w, h, only=None):
    """rz_hit records of the pixel-centre rays from the CPU oracle (rzo.trace), a miss elsewhere; only: a mask of the pixels to
    trace (the others stay misses)."""
    key = (w, h, None if only is None else only.tobytes())
    if key not in _HITS:
        sc = S.cornell_scene()
        osc = oracle_scene(sc.arrays)
        rays = editor_rays(sc.camera, w, h)
        hits = np.zeros(w * h, HIT_DTYPE)
        hits["t"], hits["instance"], hits["material"], hits["triangle"], hits["prim"] = 1e30, -1, -1, -1, -1
        for k in (range(w * h) if only is None else np.flatnonzero(only.reshape(-1))):
            r = rzo.trace(osc, rays["origin"][k], rays["dir"][k])
            if r["hit"]:
                hits[k]["t"], hits[k]["point"], hits[k]["normal"] = r["t"], r["point"], r["normal"]
                hits[k]["instance"], hits[k]["material"] = r["instance"], r["material"]
        _HITS[key] = (sc, hits.reshape(h, w))
    return _HITS[key]


def test_a_line_behind_the_cube_is_hidden_there_and_visible_beside_it():
    w = h = 64
    sc, hits = cornell_hits(w, h)
    cam = sc.camera
    line = LN.segments([(-3.0, -0.5, -1.5)], [(3.0, -0.5, -1.5)], (255, 255, 0, 255))     # behind the cube, in front of the wall
    rgb = np.full((h, w, 3), 0.25, F32)
    _, out0, info = LR.draw(line, cam.view, cam.proj, w, h, hits=hits, rgb32f=rgb)
    assert info["occluded"].any() and info["visible"].any()
    assert (hits["instance"][info["occluded"]] == 2).all()                      # the cube hides it, nothing else
    assert not (info["touched"] & info["occluded"] & ~info["visible"]).any()    # hidden_alpha = 0: hidden pixels are not written
    # hidden_alpha = 0.25: the occluded pixels change, the visible ones do not
    _, out1, info1 = LR.draw(line, cam.view, cam.proj, w, h, hits=hits, rgb32f=rgb, hidden_alpha=0.25)
    occ = info["occluded"]
    assert (info1["occluded"] == occ).all() and (out1[occ] != out0[occ]).any(axis=-1).all()
    assert (out1[~occ] == out0[~occ]).all()
    # without hits nothing is occluded
    _, _, free = LR.draw(line, cam.view, cam.proj, w, h, rgb32f=rgb)
    assert not free["occluded"].any() and (free["visible"] == (info["visible"] | occ)).all()


def test_a_grid_on_the_floor_is_not_hidden_by_the_floor():
    """The grid lies in the floor's plane, so its depth and the floor's differ only by what a pixel's offset from the line is
    worth.  The camera looks along the floor from H = 2 above it with tan(fov / 2) = 0.7: one pixel up the screen is a relative
    step of 2 * 0.7 * w / (N * H) = 0.7 * w / N in depth.  With N = 768, the grid's far edge at w = 6 and a covered pixel at most
    hw = 0.5 px from its line that is 0.27 %, under the default bias of 2^-8 = 0.39 %."""
    n = 768
    sc = S.cornell_scene()
    cam = sc.camera
    grid = LN.grid(1.5, 0.5, (255, 255, 255, 255), y=-1.5)
    rgb = np.zeros((n, n, 3), F32)
    _, _, free = LR.draw(grid, cam.view, cam.proj, n, n, rgb32f=rgb, width=1.0)
    _, hits = cornell_hits(n, n, only=free["visible"])
    _, _, info = LR.draw(grid, cam.view, cam.proj, n, n, hits=hits, rgb32f=rgb, width=1.0)
    on_floor = hits["instance"] == 0
    assert (free["visible"] & on_floor).sum() > 1500
    assert not (info["occluded"] & on_floor).any()
    assert (info["occluded"] & (hits["instance"] == 2)).any()                   # the cube stands on some of it


# ---------------------------------------------------------------------------------------------------------------------
# the cull: rectangle, cells and tiles

def test_the_cull_misses_no_covered_pixel():
    """3 000 random screen-space lines through or near a frame of 2 x 2 cells whose ends lie 2^10 to 2^30 pixels away, widths 1
    and 16, hard and smooth: every pixel the restatement covers lies inside the line's rectangle, and its cell and its tile keep
    the line.  The tests must also reject something, or they prove nothing."""
    w, h = 150, 136
    rng = np.random.default_rng(20261021)
    n = 3000
    ex = rng.integers(10, 31, n)
    far = (2.0 ** ex * rng.uniform(0.5, 1.0, n)).astype(F32)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    ang[::7] = np.round(ang[::7] / (np.pi / 2)) * (np.pi / 2)                   # some axis-parallel ones
    px, py = rng.uniform(-20.0, w + 20.0, n), rng.uniform(-20.0, h + 20.0, n)
    one_sided = rng.random(n) < 0.5                                             # an end inside the frame, or both far away
    dx, dy = np.cos(ang), np.sin(ang)
    P = dict(drop=np.zeros(n, bool),
             sax=np.where(one_sided, px, px - far * dx).astype(F32), say=np.where(one_sided, py, py - far * dy).astype(F32),
             sbx=(px + far * dx).astype(F32), sby=(py + far * dy).astype(F32))
    assert np.abs(P["sbx"]).max() > 2.0 ** 28
    xs, ys = np.meshgrid(np.arange(w, dtype=F32) + F32(0.5), np.arange(h, dtype=F32) + F32(0.5))
    culls = {(wd, sm): LR.cull(P, wd, sm) for wd in (1.0, 16.0) for sm in (0, 1)}
    covered_lines = rejected_rect = rejected_cell = rejected_tile = 0
    for i in range(n):
        abx, aby = P["sbx"][i] - P["sax"][i], P["sby"][i] - P["say"][i]
        with np.errstate(all="ignore"):
            L = abx * abx + aby * aby
        _, d = LR.seg_t_d(xs, ys, P["sax"][i], P["say"][i], abx, aby, L)
        for (wd, sm), (rect, reach) in culls.items():
            hw = F32(wd) * F32(0.5)
            cov = ((hw + F32(0.5)) - d > 0) if sm else (d < hw)
            lox, loy, hix, hiy = rect[i]
            rejected_rect += bool(lox > 0.5 or hix < w - 0.5 or loy > 0.5 or hiy < h - 0.5)      # some pixel centre lies outside
            if (wd, sm) == (1.0, 0):
                for cy in range(0, h, LR.CELL):
                    for cx in range(0, w, LR.CELL):
                        rejected_cell += not LR.meets(P, rect, reach, i, cx, cy, LR.CELL_R)
            if not cov.any():
                continue
            covered_lines += 1
            yy, xx = np.nonzero(cov)
            cxs, cys = xs[yy, xx], ys[yy, xx]
            assert ((cxs >= lox) & (cxs <= hix) & (cys >= loy) & (cys <= hiy)).all(), (i, wd, sm)
            for cx, cy in {(int(x) // LR.CELL * LR.CELL, int(y) // LR.CELL * LR.CELL) for x, y in zip(xx, yy)}:
                assert LR.meets(P, rect, reach, i, cx, cy, LR.CELL_R), (i, wd, sm, cx, cy)
            tiles = {(int(x) // LR.TILE_W * LR.TILE_W, int(y) // LR.TILE_H * LR.TILE_H) for x, y in zip(xx, yy)}
            for tx, ty in tiles:
                assert LR.meets(P, rect, reach, i, tx, ty, LR.TILE_R), (i, wd, sm, tx, ty)
            if (wd, sm) == (1.0, 0) and i % 32 == 0:                            # the tiles it does not cross
                for tx in range(0, w, LR.TILE_W):
                    for ty in range(0, h, LR.TILE_H):
                        rejected_tile += (tx, ty) not in tiles and not LR.meets(P, rect, reach, i, tx, ty, LR.TILE_R)
    assert covered_lines > 4000 and rejected_rect > 1000 and rejected_cell > 1000 and rejected_tile > 1200, \
        (covered_lines, rejected_rect, rejected_cell, rejected_tile)
    # a dropped line has the empty rectangle
    P["drop"][0] = True
    rect, reach = LR.cull(P)
    assert not LR.meets(P, rect, reach, 0, 0, 0, LR.CELL_R) and rect[0].tolist() == [LR.BIG, LR.BIG, -LR.BIG, -LR.BIG]

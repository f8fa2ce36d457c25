"""Do the inputs of tests/present_cases.py bite?  With the oracle alone (no GPU): every box case draws a wire (or, behind the
camera, none), with the stated number of valid corners per box; every grazing case has wire pixels outside every box's cull
rectangle as it stood before the M * 2^-21 term, so a kernel with that rectangle cannot agree with the oracle there; every
branch-walk case has the path length and the nodeCount it was built for; and the rectangle rz_present.hip now states is
conservative for segments that reach from the screen out to 2^10 .. 2^40 px (tests/test_present_gpu.py holds the kernel to
the oracle on all of these).

Measured on these inputs: wire pixels outside every old rectangle -- grazing-right 7, -left 10, -top 7, -bottom 2; in the
sweep (3 000 segments, thickness 1.5 and 2) 352 segments have such pixels under the old rule, none under the new."""
import numpy as np
import pytest

import present_cases as P
import present_ref as R
from helpers import oracle_scene
from oracle import rzo
from rayzen_amd import scene as S

F32 = np.float32


def _grey(width, height):
    acc = np.zeros((height, width, 4), F32)
    acc[..., :3], acc[..., 3] = 0.5, 1.0
    return acc


def _present(case, **over):
    kw = dict(case.kw)
    kw.update(over)
    return rzo.present(oracle_scene(case.scene), _grey(case.width, case.height), case.camera.view, case.camera.proj, P.NUM_LIGHTS, **kw)[0]


def _changed(a, b):
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1)


@pytest.mark.parametrize("name", P.BOX_CASES)
def test_box_case_draws_a_wire_with_the_stated_valid_corners(name):
    case = P.box_case(name)
    valid = R.valid_corners(case.scene.arrays, case.camera.view, case.camera.proj, case.width, case.height)
    assert valid == P.VALID_CORNERS[name]
    wire = _changed(_present(case), _present(case, show_bvh=False))
    print(f"{name}: valid corners {valid}, {int(wire.sum())} wire pixels of {wire.size}")
    assert (wire.sum() == 0) if name == "behind" else (wire.sum() >= 1)


def test_cut_drops_edges_singly_and_flat_has_coincident_corners():
    assert any(0 < v < 8 and v != 4 for v in P.VALID_CORNERS["cut"])
    boxes = dict((n, (mn, mx)) for n, mn, mx, _ in R.scene_boxes(P.box_scene().arrays))
    mn, mx = boxes["root3"]                                  # the quad
    assert mn[1] == mx[1] and mn[0] < mx[0] and mn[2] < mx[2]
    inst = P.box_scene().arrays[S.BIND_INSTANCES]
    assert len(inst) == 6 and sorted(np.unique(inst["blasNodeOffset"], return_counts=True)[1].tolist()) == [1, 5]
    c = P.box_case("inside")
    eye = np.asarray(P.CAMERAS["inside"]["position"], F32)
    for name in ("root0", "tlas10"):                         # instance 0's root box, and its TLAS leaf
        mn, mx = boxes[name]
        assert (mn < eye).all() and (eye < mx).all(), name
    assert c.scene.arrays[S.BIND_TLAS_NODES][10]["count"] == 1


@pytest.mark.parametrize("name", ["overflow", "w_zero"])
def test_the_non_finite_cases_hold_what_they_claim(name):
    case = P.box_case(name)
    vp = R.view_proj(case.camera.view, case.camera.proj)
    boxes = dict((n, (mn, mx)) for n, mn, mx, _ in R.scene_boxes(case.scene.arrays))
    sx, sy, sw = R.project_corners(*boxes["root3"], vp, case.width, case.height)
    if name == "overflow":
        assert (sw > 0).all() and np.isposinf(sx[sw < 1]).all() and (sw < 1).sum() == 4 and np.isfinite(sx[sw >= 1]).all()
        assert R.cull_rect(sx, sy, sw, 2.0) == (-R.BIG, -R.BIG, R.BIG, R.BIG)
    else:
        assert (sw == 0).sum() == 4 and np.isinf(sx[sw == 0]).all() and np.isnan(sy[sw == 0]).any()


@pytest.mark.parametrize("side", sorted(P.GRAZING))
def test_grazing_case_has_wire_pixels_outside_every_old_rectangle(side):
    case = P.box_case("grazing-" + side)
    k = P.GRAZING[side]["k"]
    vp = R.view_proj(case.camera.view, case.camera.proj)
    boxes = R.scene_boxes(case.scene.arrays)
    root = next(b for b in boxes if b[0] == "root0")
    sx, sy, sw = R.project_corners(root[1], root[2], vp, case.width, case.height)
    assert sw[0] == F32(2.0 ** -k) and (sw > 0).all()                     # corner 0 = (-1, -1, -1)
    far = {"right": sx[0], "left": -sx[0], "top": sy[0], "bottom": -sy[0]}[side]
    assert 2.0 ** 26 <= far < 2.0 ** 30 and np.isfinite(sx).all() and np.isfinite(sy).all()
    on_screen = [c for c in (1, 3, 4) if 0 <= sx[c] <= case.width and 0 <= sy[c] <= case.height]    # the other ends of its three edges
    assert on_screen, (sx, sy)
    wire = _changed(_present(case), _present(case, show_bvh=False))
    xs, ys = R.pixel_centres(case.width, case.height)
    out_old, out_new = np.ones_like(wire), np.ones_like(wire)
    for _, mn, mx, thick in boxes:
        c = R.project_corners(mn, mx, vp, case.width, case.height)
        out_old &= R.outside(R.cull_rect(*c, thick, error_term=False), xs, ys)
        out_new &= R.outside(R.cull_rect(*c, thick), xs, ys)
    print(f"grazing-{side}: corner at {far:.4g} px, {int(wire.sum())} wire pixels, {int((wire & out_old).sum())} outside every old "
          f"rectangle, {int((wire & out_new).sum())} outside every new one")
    assert (wire & out_old).sum() >= 1
    assert (wire & out_new).sum() == 0


@pytest.mark.parametrize("k", range(len(P.BRANCH_CASES)), ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in P.BRANCH_CASES])
def test_branch_case_has_the_stated_path_and_node_count(k):
    name, blas, tri, want_len, want_count, what = P.BRANCH_CASES[k]
    case = P.branch_case(k)
    path, count = rzo.bvh_branch(oracle_scene(case.scene), blas, tri)
    assert (len(path), count) == (want_len, want_count), what
    wire = _changed(_present(case), _present(case, show_bvh=False))
    assert (wire.sum() >= 1) == (want_len > 0), what                     # a path shows in the frame


def test_branch_scenes_are_what_the_cases_assume():
    sc = P.branch_scene()
    inst = sc.arrays[S.BIND_INSTANCES]
    assert inst["blasNodeOffset"].tolist() == [0, 0, 231, 240, 231, 231, 0, 240, 0] and len(sc.arrays[S.BIND_BLAS_NODES]) == 241
    assert len(sc.arrays[S.BIND_TRIANGLES]) == 432 + 12 + 1
    signs = {int(np.sign(c[4])) for c in P.BRANCH_CASES if c[0] == "branch" and 0 <= c[1] < 9}
    assert signs == {-1, 0, 1}
    deep = P.deep_scene()
    assert deep.max_blas_depth == 35 and len(deep.arrays[S.BIND_TRIANGLES]) == 52 + 55 + 12
    for sc in (sc, deep):                                                   # valid scenes: they are path-traced on the GPU
        assert np.isfinite(sc.arrays[S.BIND_INSTANCES]["inverseTransform"]).all()
    assert np.isfinite(S.inverse(P.branch_transforms("deep")[0])).all()


def test_lights_bite():
    case = P.light_case()
    plain = _present(case, show_lights=False)
    lit = _present(case)
    marked = _changed(lit, plain)
    assert marked[:8, :8].any() and not marked[:12, :12].all()           # the marker cut by the frame's corner
    osc = oracle_scene(case.scene)
    lights = case.scene.lights

    def frame(order, n=P.NUM_LIGHTS):
        o = rzo.Scene(*[osc.arrays[k] if k != "lights" else np.ascontiguousarray(lights[order]) for k in
                        ("triangles", "materials", "lights", "tlas_nodes", "tlas_indices", "blas_nodes", "blas_indices", "instances")])
        return rzo.present(o, _grey(case.width, case.height), case.camera.view, case.camera.proj, n, **case.kw)[0]

    every = list(range(len(lights)))
    assert not _changed(frame(every), lit).any()
    assert _changed(frame([0, 2, 1, 3, 4, 5, 6, 7]), lit).any()                 # the two overlapping markers: the mix order shows
    assert _changed(frame(every, n=len(lights)), lit).any()                     # the light beyond num_lights would show
    for k, what in ((4, "behind the camera"), (5, "directional")):
        gone = [j for j in every if j != k] + [k]                               # moved past num_lights
        assert not _changed(frame(gone, n=P.NUM_LIGHTS - 1), lit).any(), what
    assert lit.max() > 1.0 and lit.min() < 0.0                                  # the colour outside [0, 1] reaches the float output


def test_fps_values_bite():
    frames = {f: _present(P.fps_case(f)) for f in P.FPS_DEFINED + P.FPS_UNDEFINED if f == f}
    nan = _present(P.fps_case(float("nan")))
    zero = frames[0.0]
    for f in P.FPS_UNDEFINED:
        assert not _changed(nan if f != f else frames[f], zero).any(), f            # the rule: 000.0
    assert not _changed(frames[2147483520.0], _present(P.fps_case(520.0))).any()   # the last three digits of 2147483520
    assert not _changed(frames[-3.2], _present(P.fps_case(0.7))).any()            # -3 % 10 < 0 -> 0; fract(-3.2) = 0.8 - 1 ulp -> 7
    assert not _changed(frames[59.999996], _present(P.fps_case(59.9))).any()      # tenths truncate
    assert _changed(frames[9.96], frames[99.95]).any() and _changed(frames[999.94], frames[1000.0]).any()


@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_combined_sizes_run_and_cut_the_fps_box(size):
    case = P.combined_case(*size)
    full = _present(case)
    assert full.shape == (size[1], size[0], 3)
    box = _changed(full, _present(case, show_fps=False))
    # the box spans x in 7 .. 103 and y in H - 25 .. H - 9: wholly below row 0 where H <= 9, right of a frame 7 wide or less
    assert box.any() == (size[0] > 7 and size[1] > 9)
    if size == (97, 61):
        assert box[:, 80:].any() and not box[:, :8].any()                 # the last digit's cell (x in 80 .. 96) ends at the frame's edge
    assert size[0] % 256 != 0 and (size[0] * size[1]) % 256 != 0


def test_the_stated_rectangle_is_conservative_for_far_endpoints():
    """Segments with one end on a 97 x 61 screen and the other 2^10 .. 2^40 px off one of its four sides, in either order of
    the endpoints: no pixel outside the rectangle of rz_present.hip's comment has dist < thickness; under the rule before it
    (thickness + 1) most of the far segments have such pixels."""
    rng = np.random.default_rng(20261019)
    xs, ys = R.pixel_centres(P.W, P.H)
    n, missed_new, missed_old = 3000, 0, 0
    for j in range(n):
        near = (F32(rng.uniform(0, P.W)), F32(rng.uniform(0, P.H)))
        mag = F32(2.0 ** rng.uniform(10, 40) * (1 if j % 4 < 2 else -1))
        other = F32(rng.uniform(-2, 2) * abs(float(mag)) if j % 3 == 0 else rng.uniform(-40, 140))
        far = (mag, other) if j % 2 else (other, mag)
        a, b = (near, far) if (j // 4) % 2 else (far, near)
        thick = 2.0 if j % 5 else 1.5
        sx, sy, sw = np.array([a[0], b[0]], F32), np.array([a[1], b[1]], F32), np.ones(2, F32)
        hit = R.seg_dist(xs, ys, a[0], a[1], b[0], b[1]) < F32(thick)
        missed_new += int((hit & R.outside(R.cull_rect(sx, sy, sw, thick), xs, ys)).any())
        missed_old += int((hit & R.outside(R.cull_rect(sx, sy, sw, thick, error_term=False), xs, ys)).any())
    print(f"{n} segments: {missed_old} with a drawn pixel outside the old rectangle, {missed_new} outside the new one")
    assert missed_new == 0
    assert missed_old >= 100

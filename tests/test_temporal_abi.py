"""Temporal accumulation and the variance-guided filter (rz_denoise_temporal): the C-ABI struct, the kernels' register budget,
properties of the float64 restatement (temporal_ref.py), its quality on frames of the CPU oracle and the ambiguity cap on the
inputs the GPU tests use -- everything that can be checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as DR
import helpers
import temporal_ref as TR
from oracle import rzo
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, editor_rays
from test_rays_abi import _kernel_metadata


def test_temporal_params_size_and_offsets():
    L = _lib.hip()
    assert L.rz_sizeof(12) == 64 and C.sizeof(_lib.TemporalParams) == 64
    want = {"alpha": 0, "alpha_moments": 4, "max_history": 8, "normal_cos": 12, "plane_tol": 16, "iterations": 20, "sigma_l": 24,
            "sigma_normal": 28, "sigma_plane": 32, "demodulate": 36, "reserved": 40}
    assert [f for f, _ in _lib.TemporalParams._fields_] == list(want)
    for f, off in want.items():
        assert getattr(_lib.TemporalParams, f).offset == off, f
    assert (_lib.TEMPORAL_HOST, _lib.TEMPORAL_KEEP) == (1, 4)
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5       # additive: the revision stays
    for name in ("rz_denoise_temporal", "rz_present_temporal", "rz_temporal_reset", "rz_debug_read_temporal"):
        assert hasattr(L, name) and name in _lib.HIP_SYMBOLS
    assert _lib.TEMPORAL_DEFAULTS == TR.DEFAULTS
    assert L.rz_sizeof(11) == 32 and L.rz_sizeof(13) == 0


def test_temporal_kernels_spill_nothing():
    meta = _kernel_metadata(_lib.HIP_SO)
    mine = {k: v for k, v in meta.items() if "rz_temporal_" in k}
    for part, count in (("rz_temporal_instances", 1), ("rz_temporal_accumulate", 1), ("rz_temporal_variance", 1), ("rz_temporal_atrous", 2)):
        assert len([k for k in mine if part in k]) == count, sorted(mine)
    for name, (spill, priv) in mine.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


# ---------------------------------------------------------------------------------------------------------------------
# properties of the restatement, on synthetic guides: a camera at `cam` looking down -z at the plane z = -depth

def _look(cam=(0.0, 0.0, 0.0), fov=90.0, aspect=1.0):
    return S.Camera(position=cam, target=(0.0, 0.0, -1.0), fov=fov, aspect=aspect)


def _plane_guides(cam, W, H, depth=5.0, inst=0, mat=0):
    """What a camera sees of the plane z = -depth (normal +z): exact hit points of the pixel-centre rays."""
    rays = editor_rays(cam, W, H)
    d = rays["dir"].astype(np.float64).reshape(H, W, 3)
    o = np.asarray(cam.position, np.float64)
    t = (-depth - o[2]) / d[..., 2]
    g = np.zeros((H, W), HIT_DTYPE)
    g["t"] = t
    g["point"] = o + d * t[..., None]
    g["normal"] = (0.0, 0.0, 1.0)
    g["material"], g["instance"] = mat, inst
    return g, rays["dir"].reshape(H, W, 3)


def _mats(*albedos):
    m = np.zeros(len(albedos), S.MATERIAL)
    for i, a in enumerate(albedos):
        m[i] = (a, 0.0, 1.0, 0.0, 0.0, 1.5)
    return m


IDENT = np.zeros((1, 2, 4, 3), np.float32)
IDENT[:, :, 0, 0] = IDENT[:, :, 1, 1] = IDENT[:, :, 2, 2] = 1.0


def _step(hist, c, g, md, cam, inst=IDENT, mats=None, **kw):
    mats = _mats((1.0, 1.0, 1.0)) if mats is None else mats
    return TR.step(hist, c, g, mats, cam.view, cam.proj, cam.inv_proj, cam.position, inst, md, TR.params(**kw))


def _texture(points):
    """A smooth colour as a function of the world point: what a textured plane shows."""
    x, y = points[..., 0], points[..., 1]
    return np.stack([0.5 + 0.4 * np.sin(1.3 * x), 0.5 + 0.4 * np.cos(0.9 * y), 0.5 + 0.2 * np.sin(x + y)], -1)


def test_ref_static_sequence_is_a_running_mean():
    rng = np.random.default_rng(1)
    H, W = 12, 16
    cam = _look()
    g, md = _plane_guides(cam, W, H)
    frames = rng.random((6, H, W, 3))
    hist = None
    for k in range(6):
        r, hist = _step(hist, frames[k], g, md, cam, alpha=0.0, alpha_moments=0.0, iterations=0)
        assert (r["N"] == k + 1).all() and not r["ambiguous"].any()
        assert np.allclose(r["D"], frames[:k + 1].mean(0), rtol=1e-12)
        assert np.array_equal(r["out"], r["D"] * r["alpha"]) if k else np.array_equal(r["out"], frames[0])
        assert (r["var"] >= 0).all()
    # the cap: N stops at max_history and the blend becomes exponential
    hist = None
    for k in range(5):
        r, hist = _step(hist, frames[k], g, md, cam, alpha=0.0, max_history=3, iterations=0)
    assert (r["N"] == 3).all()


def test_ref_colour_never_crosses_a_hit_miss_edge_or_an_instance():
    H, W = 16, 16
    cam0, cam1 = _look(), _look(cam=(0.07, 0.0, 0.0))
    inst = np.repeat(IDENT, 2, 0)

    def guides(cam):
        g, md = _plane_guides(cam, W, H)
        left = g["point"][..., 0] < -0.5
        right = g["point"][..., 0] > 0.5
        g["instance"][left] = -1                # sky on the left
        g["t"][left] = 1e30
        g["point"][left] = 0
        g["normal"][left] = 0
        g["instance"][right] = 1                # another instance on the right (same plane)
        return g, md

    g0, md0 = guides(cam0)
    g1, md1 = guides(cam1)
    region = lambda g: np.where(g["instance"] < 0, 0, g["instance"] + 1)
    col = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    _, hist = _step(None, col[region(g0)], g0, md0, cam0, inst=inst, iterations=0)
    r, _ = _step(hist, col[region(g1)], g1, md1, cam1, inst=inst, iterations=0, alpha=0.0)
    assert r["accepted"].mean() > 0.8 and (r["N"][r["accepted"]] > 1).all()
    assert np.array_equal(r["D"], col[region(g1)])          # every pixel still has exactly its own region's colour
    # and through the filter: a hit and a miss never mix (instances on one plane may, as in rz_denoise)
    r, _ = _step(hist, col[region(g1)], g1, md1, cam1, inst=inst, iterations=3, alpha=0.0)
    assert (r["out"][g1["instance"] < 0] == col[0]).all() and (r["out"][g1["instance"] >= 0][:, 0] == 0).all()


def test_ref_translated_camera_finds_the_same_surface_point():
    H, W = 24, 32
    cam0, cam1 = _look(aspect=W / H), _look(cam=(0.23, -0.11, 0.4), aspect=W / H)
    g0, md0 = _plane_guides(cam0, W, H)
    g1, md1 = _plane_guides(cam1, W, H)
    # the history's "colour" is the world point itself: bilinear interpolation of a linear function is exact
    _, hist = _step(None, g0["point"].astype(np.float64), g0, md0, cam0, iterations=0, demodulate=0)
    r, _ = _step(hist, np.zeros((H, W, 3)), g1, md1, cam1, iterations=0, demodulate=0, alpha=1e-30, max_history=1 << 20)
    acc = r["accepted"]
    assert acc.mean() > 0.5
    # D = D_h + (1 / 2) (0 - D_h): the history's colour is 2 D
    want = g1["point"].astype(np.float64)
    full = (r["S"] > 1 - 1e-9) & ~r["ambiguous"]          # all four taps counted
    assert full.mean() > 0.4
    assert np.abs(2 * r["D"][full] - want[full]).max() < 1e-5      # (the guide's points are float32: 1e-9 needs exact ones)
    # with points that are exact in float64 -- the plane seen through the inverse of the very view and proj the step projects
    # with, so that a history pixel's point projects onto its centre: the same surface point to 1e-9
    f64 = np.dtype([(n, "<f8" if HIT_DTYPE[n].base.kind == "f" else "<i4", HIT_DTYPE[n].shape) for n in HIT_DTYPE.names])

    def exact(cam):
        inv = np.linalg.inv(cam.proj.astype(np.float64).reshape(4, 4).T @ cam.view.astype(np.float64).reshape(4, 4).T)
        eye = np.linalg.inv(cam.view.astype(np.float64).reshape(4, 4).T)[:3, 3]
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ndc = np.stack([(xs + 0.5) / W * 2 - 1, (ys + 0.5) / H * 2 - 1, np.zeros((H, W)), np.ones((H, W))], -1)
        far = ndc @ inv.T
        d = far[..., :3] / far[..., 3:] - eye
        g = g0.astype(f64)
        g["point"] = eye + d * ((-5.0 - eye[2]) / d[..., 2])[..., None]
        return g

    e0, e1 = exact(cam0), exact(cam1)
    h2 = dict(hist, guide=e0, col=np.concatenate([e0["point"], np.ones((H, W, 1))], -1))
    r, _ = _step(h2, np.zeros((H, W, 3)), e1, md1, cam1, iterations=0, demodulate=0, max_history=1 << 20)
    inner = r["S"] > 1 - 1e-9                               # all four taps counted
    assert inner.mean() > 0.4
    assert np.abs(2 * r["D"][inner] - e1["point"][inner]).max() < 1e-9


def test_ref_moved_instance_is_followed_through_its_previous_transform():
    H, W = 24, 24
    cam = _look()
    shift = np.array([0.31, -0.17, 0.0])

    def packed(offset):
        m = IDENT.copy()
        m[0, 1, 3] = offset
        m[0, 0, 3] = -np.asarray(offset)
        return m

    # the plane's object points are world - offset; its texture lives in object space
    g0, md = _plane_guides(cam, W, H)
    g1 = g0.copy()                  # same camera, same plane z = -5: the same world points are hit, the object has slid in x, y
    obj0 = g0["point"].astype(np.float64)
    obj1 = g1["point"].astype(np.float64) - shift
    _, hist = _step(None, obj0, g0, md, cam, inst=packed((0, 0, 0)), iterations=0, demodulate=0)
    r, _ = _step(hist, np.zeros((H, W, 3)), g1, md, cam, inst=packed(shift), iterations=0, demodulate=0, max_history=1 << 20)
    inner = r["S"] > 1 - 1e-9
    assert inner.mean() > 0.5
    assert np.abs(2 * r["D"][inner] - obj1[inner]).max() < 1e-5     # the history of the OBJECT point, not of the pixel
    # unchanged transform: the shortcut, every pixel its own history
    r, _ = _step(hist, np.zeros((H, W, 3)), g0, md, cam, inst=packed((0, 0, 0)), iterations=0, demodulate=0)
    assert (r["N"] == 2).all() and np.array_equal(2 * r["D"], obj0)


def test_ref_disocclusion_restarts_at_one():
    H, W = 16, 32
    cam0, cam1 = _look(aspect=2.0), _look(cam=(0.5, 0.0, 0.0), aspect=2.0)
    g0, md0 = _plane_guides(cam0, W, H, depth=5.0)
    near, _ = _plane_guides(cam0, W, H, depth=2.0, inst=0)
    occl0 = np.abs(near["point"][..., 0]) < 0.4            # a strip in front, at depth 2
    g0[occl0] = near[occl0]
    g1, md1 = _plane_guides(cam1, W, H, depth=5.0)
    near1, _ = _plane_guides(cam1, W, H, depth=2.0, inst=0)
    occl1 = np.abs(near1["point"][..., 0]) < 0.4
    g1[occl1] = near1[occl1]
    hist = None
    for _ in range(3):
        r, hist = _step(hist, np.full((H, W, 3), 0.5), g0, md0, cam0, iterations=0)
    assert (r["N"] == 3).all()
    r, _ = _step(hist, np.full((H, W, 3), 0.5), g1, md1, cam1, iterations=0)
    # background points the strip hid in frame 0: they project onto the strip's pixels there and fail the plane test
    bx = g1["point"][..., 0].astype(np.float64)
    proj_x = bx * (2.0 / 5.0)                               # where the ray from cam0 to the point crosses z = -2
    hidden = ~occl1 & (np.abs(proj_x) < 0.35)
    assert hidden.any() and (r["N"][hidden] == 1).all()
    seen = ~occl1 & (np.abs(proj_x) > 0.6) & r["accepted"]
    assert seen.any() and (r["N"][seen] > 3).all()


def test_ref_variance_and_filter_weights():
    rng = np.random.default_rng(5)
    H, W = 20, 24
    cam = _look(aspect=W / H)
    g, md = _plane_guides(cam, W, H)
    g["instance"][:, :5] = -1
    hist = None
    for k in range(6):
        c = 0.5 + 0.2 * rng.standard_normal((H, W, 3))
        r, hist = _step(hist, c, g, md, cam, iterations=0)
        assert (r["var"] >= 0).all() and np.isfinite(r["var"]).all()
        assert np.array_equal(r["out"], r["D"] * r["alpha"]) if k else np.array_equal(r["out"], c)
    assert (r["N"] == 6).all()
    p = TR.params(sigma_l=4.0)              # (SVGF's value: the noise of this input is brought down by half and more)
    d, v = r["D"], r["var"]
    for i in range(4):
        d2, v2, ws = TR.atrous_pass(d, v, g, cam.inv_proj, i, p, want_weights=True)
        assert np.allclose(sum(ws.values()), 1.0, atol=1e-12) and all((w >= 0).all() for w in ws.values())
        assert (ws[(0, 0)] > 0).all() and (v2 >= 0).all()
        d, v = d2, v2
    assert np.std(lum := TR.lum(d)[:, 5:]) < 0.5 * np.std(TR.lum(r["D"])[:, 5:]) and lum.size
    # a constant colour stays constant, whatever the variance says
    const = np.full((H, W, 3), 0.3)
    out, _ = TR.atrous_pass(const, rng.random((H, W)), g, cam.inv_proj, 1, p)
    assert np.allclose(out, 0.3, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# non-finite samples (include/rayzen_hip.h, "Non-finite samples"): a bad sample never outlives its frame

BAD_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def bad_pattern(H, W):
    """An isolated interior pixel, the corner (0, 0) and a 5 x 5 block: 27 pixels."""
    m = np.zeros((H, W), bool)
    m[5, 20] = m[0, 0] = True
    m[12:17, 8:13] = True
    return m


def _bad_sequence(value, K, frames=5, bad_frames=(0, 2)):
    """32 x 24, the camera moving 0.05 to the left per frame (the previous position of every pixel but the rightmost columns is
    inside the frame), the 27 pixels of bad_pattern set to `value` in bad_frames (one channel; the isolated pixel all three).
    Yields (frame, bad mask, result, history)."""
    rng = np.random.default_rng(21)
    H, W = 24, 32
    mats = _mats((0.5, 0.6, 0.7))
    hist = None
    for fr in range(frames):
        cam = _look(cam=(-0.05 * fr, 0.0, 0.0), aspect=W / H)
        g, md = _plane_guides(cam, W, H)
        c = (0.2 + rng.random((H, W, 3))).astype(np.float32)
        bad = bad_pattern(H, W) if fr in bad_frames else np.zeros((H, W), bool)
        c[bad, 1] = BAD_VALUES[value]
        if bad.any():
            c[5, 20] = BAD_VALUES[value]
        r, hist = _step(hist, c, g, md, cam, mats=mats, iterations=K)
        assert np.array_equal(r["bad"], bad)
        yield fr, bad, r, hist


@pytest.mark.parametrize("value", sorted(BAD_VALUES))
def test_ref_bad_samples_do_not_outlive_their_frame(value):
    for fr, bad, r, hist in _bad_sequence(value, 5):
        for k in ("D", "N", "M", "var", "out", "scale", "S"):
            assert np.isfinite(r[k]).all(), (value, fr, k)
        assert np.isfinite(hist["col"]).all() and np.isfinite(hist["mom"]).all()
        if fr == 0:
            assert (r["D"][bad] == 0).all() and (r["N"] == 1).all() and (r["M"][bad] == 0).all()
        if fr == 2:
            assert r["accepted"][bad].all() and (r["N"][bad] > 2.5).all()        # N counts on
    for fr, bad, r, hist in _bad_sequence(value, 0):
        shows = ~np.isfinite(r["out"]).all(-1)
        assert np.array_equal(shows, bad & ~r["accepted"])
        assert shows.sum() == (27 if fr == 0 else 0)
        assert np.isfinite(hist["col"]).all() and np.isfinite(hist["mom"]).all()


def test_ref_bad_sample_equals_a_sample_of_the_history_colour():
    """With d_p := D_h the call stores what a call whose sample was D_h stores: D, N and the moments, bit for bit."""
    rng = np.random.default_rng(22)
    H, W = 24, 32
    cam0, cam1 = _look(aspect=W / H), _look(cam=(-0.05, 0.02, 0.0), aspect=W / H)
    g0, md0 = _plane_guides(cam0, W, H)
    g1, md1 = _plane_guides(cam1, W, H)
    _, hist = _step(None, rng.random((H, W, 3)).astype(np.float32), g0, md0, cam0, iterations=0)
    c = rng.random((H, W, 3)).astype(np.float32)
    bad = bad_pattern(H, W)
    cb = c.copy()
    cb[bad, 2] = np.nan
    r, _ = _step(hist, cb, g1, md1, cam1, iterations=0)          # (albedo 1: d = c)
    assert r["accepted"][bad].all()
    assert np.array_equal(r["out"][bad], r["D"][bad])           # K = 0 with history: D alpha, not the sample
    sub = c.astype(np.float64)
    sub[bad] = r["D"][bad]                                       # = D_h there
    r2, _ = _step(hist, sub, g1, md1, cam1, iterations=0)
    for k in ("D", "N", "M", "var", "accepted"):
        assert np.array_equal(r[k], r2[k]), k
    clean, _ = _step(hist, c, g1, md1, cam1, iterations=0)
    assert np.array_equal(r["D"][~bad], clean["D"][~bad]) and np.array_equal(r["N"], clean["N"])
    # without history: black, N = 1
    r0, _ = _step(None, cb, g1, md1, cam1, iterations=0)
    assert (r0["D"][bad] == 0).all() and (r0["M"][bad] == 0).all() and (r0["N"] == 1).all()
    assert np.isnan(r0["out"][bad][:, 2]).all() and np.isfinite(r0["out"][~bad]).all()


def test_ref_equals_its_former_self_on_finite_input(monkeypatch):
    """accumulate() before the bad-pixel rule (restatement_before.py), run beside the current one on every call the tests of
    this file make with a finite input (the synthetic ones and the cornell orbit of the GPU tests): equal bit for bit."""
    import restatement_before as RB
    new_acc = TR.accumulate
    calls = [0]

    def both(hist, color, *a, **kw):
        res = new_acc(hist, color, *a, **kw)
        assert not res["bad"].any()
        old = RB.accumulate(hist, color, *a, **kw)
        for k, v in old.items():
            if k == "ambiguous_parts":
                assert all(np.array_equal(v[m], res[k][m]) for m in v)
            else:
                assert np.array_equal(v, res[k]), k
        calls[0] += 1
        return res

    monkeypatch.setattr(TR, "accumulate", both)
    test_ref_static_sequence_is_a_running_mean()
    test_ref_colour_never_crosses_a_hit_miss_edge_or_an_instance()
    test_ref_translated_camera_finds_the_same_surface_point()
    test_ref_moved_instance_is_followed_through_its_previous_transform()
    test_ref_disocclusion_restarts_at_one()
    test_ref_variance_and_filter_weights()
    make, W, H, step_deg, transforms = gpu_sequences()["cornell"]
    run_sequence(make(), W, H, GPU_FRAMES, step_deg, TR.params(), transforms, CORNELL_PIVOT, CORNELL_LIFT)
    assert calls[0] >= 30, calls


# ---------------------------------------------------------------------------------------------------------------------
# quality on the oracle's frames (the GPU's frames equal the oracle's bit for bit), and the ambiguity cap

QW, QH, FRAMES = 160, 120, 16


def oracle_guides(sc, osc, W, H):
    rays = editor_rays(sc.camera, W, H)
    g = np.zeros(W * H, HIT_DTYPE)
    g["t"], g["material"], g["instance"], g["triangle"], g["prim"] = 1e30, -1, -1, -1, -1
    for k in range(W * H):
        h = rzo.trace(osc, rays["origin"][k], rays["dir"][k])
        if h["hit"]:
            g[k]["t"], g[k]["point"], g[k]["normal"] = h["t"], h["point"], h["normal"]
            g[k]["material"], g[k]["instance"] = h["material"], h["instance"]
    return g.reshape(H, W), rays["dir"].reshape(H, W, 3)


def orbit_camera(base, angle, pivot=(0.0, 0.0, 0.0), lift=0.0):
    """`base` turned by `angle` radians about the vertical axis through `pivot` (position and view direction alike), then
    raised by `lift` and moved forward by 1.5 `lift` along -z.  (A pure turn about a vertical axis leaves v where it was for the
    whole column of pixels whose depth does not change: a band of pixels with floor(v) undecided.)"""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    pv = np.asarray(pivot, np.float64)
    return S.Camera(position=tuple(R @ (np.asarray(base.position, np.float64) - pv) + pv + np.array([0.0, lift, -1.5 * lift])), target=tuple(R @ np.asarray(base.target, np.float64)),
                    up=tuple(base.up), fov=base.fov, aspect=base.aspect, near=base.near, far=base.far)


def run_sequence(sc, W, H, frames, step_deg, p, transforms=None, pivot=(0.0, 0.0, 0.0), lift_step=0.0):
    """`frames` oracle frames of 1 spp (sample_base = frame), the camera orbiting by step_deg per frame and ending at the
    scene's own camera; transforms(frame) -> the instances' 4 x 4 transforms of that frame, or None.  Returns the last frame's
    (colour, guide, result of the restatement) and the largest ambiguous share of any frame."""
    helpers.sync_oracle_flavour()
    base = sc.camera
    hist, worst = None, 0.0
    for fr in range(frames):
        if transforms is not None:
            for oid, t in zip(sc.instance_ids, transforms(fr)):
                sc.set_transform(oid, t)
            sc.update_dynamic()
        sc.camera = orbit_camera(base, np.radians(step_deg) * (fr - (frames - 1)), pivot, lift_step * (fr - (frames - 1))) if step_deg else base
        cam = sc.camera
        osc = helpers.oracle_scene(sc)
        c = DR.resolve(rzo.render(osc, rzo.make_frame(W, H, cam.inv_view, cam.inv_proj, cam.position, len(sc.lights), 5, 1, fr), nthreads=8))
        g, md = oracle_guides(sc, osc, W, H)
        r, hist = TR.step(hist, c, g, sc.materials, cam.view, cam.proj, cam.inv_proj, cam.position,
                          TR.inst_pack(sc.arrays[S.BIND_INSTANCES]), md, p, want_filter=fr == frames - 1)
        worst = max(worst, float(r["ambiguous_var"].mean()))
    sc.camera = base
    return c, g, r, worst


@pytest.fixture(scope="module")
def cornell_target():
    sc = S.cornell_scene()
    return DR.resolve(helpers.oracle_render(sc, QW, QH, 256, 5))


# Measured with the restatement, MSE(raw last frame, 256 spp) / MSE(output, 256 spp), cornell_scene at 160 x 120,
# 5 bounces, 16 frames of 1 spp with sample_base = frame:
#   (a) static camera, alpha = 0, K = 0:   RATIO_STATIC_MEASURED, and equal to the running mean's ratio to 1e-9 relative
#   (b) orbit of ORBIT_STEP_DEG degrees per frame, defaults:   RATIO_ORBIT_MEASURED; rz_denoise's tuned setting on the same
#       last frame gives RATIO_TUNED_MEASURED
# The asserted floors are the measured values / 1.25 (slack for the scene helpers changing by a rounding).
RATIO_STATIC_MEASURED = 22.9
RATIO_ORBIT_MEASURED = 3.82
RATIO_TUNED_MEASURED = 0.772
ORBIT_STEP_DEG = 0.25


def test_quality_static_camera_reproduces_the_running_mean(cornell_target):
    sc = S.cornell_scene()
    c, g, r, worst = run_sequence(sc, QW, QH, FRAMES, 0.0, TR.params(alpha=0.0, alpha_moments=0.0, iterations=0))
    assert worst == 0.0 and (r["N"] == FRAMES).all()
    osc = helpers.oracle_scene(sc)
    cam = sc.camera
    frames = [DR.resolve(rzo.render(osc, rzo.make_frame(QW, QH, cam.inv_view, cam.inv_proj, cam.position, len(sc.lights), 5, 1, fr),
                                    nthreads=8)).astype(np.float64) for fr in range(FRAMES)]
    raw = DR.mse(c, cornell_target)
    ratio, mean_ratio = raw / DR.mse(r["out"], cornell_target), raw / DR.mse(np.mean(frames, 0), cornell_target)
    print(f"static: raw {raw:.4g}, ratio {ratio:.3f}, running mean's {mean_ratio:.3f}")
    assert abs(ratio - mean_ratio) <= 1e-6 * mean_ratio
    assert ratio >= 20.0                                    # the issue's measurement
    assert ratio >= RATIO_STATIC_MEASURED / 1.25


def test_quality_orbiting_camera_beats_the_spatial_filter(cornell_target):
    sc = S.cornell_scene()
    c, g, r, worst = run_sequence(sc, QW, QH, FRAMES, ORBIT_STEP_DEG, TR.params())
    raw = DR.mse(c, cornell_target)
    ratio = raw / DR.mse(r["out"], cornell_target)
    tuned = raw / DR.mse(DR.denoise(c, g, sc.materials, sc.camera.inv_proj, iterations=5, sigma_color=1.0, demodulate=False), cornell_target)
    print(f"orbit {ORBIT_STEP_DEG} deg: raw {raw:.4g}, temporal {ratio:.3f}, rz_denoise tuned {tuned:.3f}, ambiguous {worst * 100:.3f} %")
    assert ratio > 1.0 and ratio > tuned
    assert ratio >= RATIO_ORBIT_MEASURED / 1.25


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (test_temporal_gpu.py: SEQUENCES): the restatement on the oracle's guides marks at most 0.5 % of a
# frame ambiguous

def gpu_sequences():
    """name -> (scene factory, W, H, orbit step in degrees, transforms(frame) or None): what test_temporal_gpu.py runs."""
    return {
        "reference": (lambda: S.reference_scene(aspect=4 / 3), 200, 150, 0.0, None),
        "instanced": (lambda: S.instanced_scene(n=24, count=16, aspect=16 / 9), 192, 108, 0.0,
                      lambda fr: S.instanced_transforms(fr, 16)),
        "cornell": (lambda: S.cornell_scene(), 32, 32, 0.5, None),
    }


CORNELL_PIVOT = (0.0, 0.0, -8.0)        # behind the back wall: every visible point moves on the screen
CORNELL_LIFT = 0.013                    # ... and up and forward a little every frame


GPU_FRAMES = 6


@pytest.mark.parametrize("name", sorted(gpu_sequences()))
def test_ambiguity_cap_on_the_gpu_tests_inputs(name):
    make, W, H, step_deg, transforms = gpu_sequences()[name]
    _, _, r, worst = run_sequence(make(), W, H, GPU_FRAMES, step_deg, TR.params(), transforms, CORNELL_PIVOT, CORNELL_LIFT)
    print(f"{name}: ambiguous at most {worst * 100:.3f} % of a frame; history accepted on {r['accepted'].mean() * 100:.1f} %")
    assert worst <= 0.005, worst
    assert r["accepted"].mean() > 0.5

"""The display stage (rz_display, rz_present_display; rz_display.hip) on the GPU: with the reference's settings it reproduces
rz_present's bytes; the metering against the integer restatement (display_ref.py), exactly; target and adaptation; the tone
curves against float64; isolation from the render state, errors and a speed ceiling."""
import ctypes as C

import numpy as np
import pytest

import display_ref as R
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer, frame_params
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

F32 = np.float32
AUTO = dict(auto=True)


def _setup(sc, W, H, spp=1, bounces=5, render=True):
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), bounces, spp, 0))
    if render:
        r.render()
    return r


_CAMERA = S.cornell_scene().camera


def _frame_only(W, H):
    """A context with a frame and no scene: all rz_display needs."""
    r = Renderer(0)
    r.set_frame(frame_params(_CAMERA, W, H, 0, 5, 1, 0))
    return r


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _key(st):
    return tuple(v.tobytes() if hasattr(v, "tobytes") else v for v in st.values())


# ---------------------------------------------------------------------------------------------------------------------
# 1 the anchor: the reference's display through the new path

@pytest.mark.parametrize("overlays", [False, True])
def test_no_display_parameters_reproduce_present(overlays):
    sc = S.reference_scene(aspect=4 / 3)
    W, H = 200, 150
    kw = dict(fps=57.3, show_fps=overlays, show_lights=overlays, show_bvh=overlays)
    r = _setup(sc, W, H)
    assert _same(r.present(**kw), r.present_display(**kw))
    assert _same(r.present(**kw), r.present_display("accum", **kw))
    for k in (0, 2):
        assert _same(r.present_denoised(iterations=k, **kw), r.present_display("denoise", filter=dict(iterations=k), **kw)), k
    assert not _same(r.present(**kw), r.present_display("denoise", filter=dict(iterations=2), **kw))
    # the temporal source advances its history: two contexts with fresh histories, one call each
    r2 = _setup(sc, W, H)
    assert r.debug_read_temporal(0) is None and r2.debug_read_temporal(0) is None
    assert _same(r.present_temporal(**kw), r2.present_display("temporal", **kw))
    for which in range(5):
        assert r.debug_read_temporal(which).tobytes() == r2.debug_read_temporal(which).tobytes(), which
    # and the parameters do something
    assert not _same(r.present(**kw), r.present_display(curve="aces", transfer="srgb", **kw))
    r.close()
    r2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2 the histogram, exact

EDGES = np.array([2.0 ** -16, np.nextafter(F32(2.0 ** -16), F32(0)), 1.0, 1.25, np.nextafter(F32(1.25), F32(0)), 65535.996, 65536.0,
                  np.inf, np.nan, 0.0, -0.0, -1.0, 1e-40, -1e-40], F32)


def _synthetic(W, H, seed, edges=True):
    rng = np.random.default_rng(seed)
    lum = np.exp(rng.normal(-1.0, 2.0, (H, W, 1)))
    img = (lum * rng.uniform(0.5, 1.5, (H, W, 3))).astype(F32)
    if edges:                       # the edge values at the first and the last pixels, as many as fit
        flat = img.reshape(-1, 3)
        k = min(len(EDGES), len(flat))
        head = (k + 1) // 2
        flat[:head] = EDGES[:head, None]
        if k > head:
            flat[-(k - head):] = EDGES[head:k, None]
    return img


def _assert_metered(st, img, what):
    hist, below, above = R.meter(R.luminance(img))
    assert np.array_equal(st["histogram"], hist), f"{what}: bins {np.nonzero(st['histogram'] != hist)[0].tolist()} differ"
    assert (st["below"], st["above"], st["counted"]) == (below, above, int(hist.sum())), what
    assert st["counted"] + st["below"] + st["above"] == img.shape[0] * img.shape[1], what


HIST_SIZES = [(1, 1), (64, 4), (256, 1), (67, 37), (513, 3)]


@pytest.mark.parametrize("W,H", HIST_SIZES)
def test_histogram_equals_restatement(W, H):
    hip = Hip()
    r = _frame_only(W, H)
    for seed in (1, 2):
        img = _synthetic(W, H, seed)
        r.display(img, **AUTO)                                          # the host path
        _assert_metered(r.display_state(), img, f"host {W}x{H}")
        r.display_reset()
        buf = hip.upload(np.concatenate([np.zeros(1, F32), img.reshape(-1)]))
        hip.ok(hip.L.hipMemcpy(buf, img.ctypes.data, img.nbytes, 1))
        r.display_device(buf, **AUTO)                                   # device memory, 16-byte aligned: vector loads
        _assert_metered(r.display_state(), img, f"device {W}x{H}")
        hip.ok(hip.L.hipMemcpy(buf + 4, img.ctypes.data, img.nbytes, 1))
        r.display_device(buf + 4, **AUTO)                               # a base that is only 4-byte aligned
        _assert_metered(r.display_state(), img, f"device + 4 {W}x{H}")
    # the accumulation as the input: sum and count, counts 0..3
    rng = np.random.default_rng(3)
    img = _synthetic(W, H, 4, edges=False)
    cnt = rng.integers(0, 4, (H, W, 1)).astype(F32)
    acc = np.concatenate([img * np.where(cnt > 0, cnt, 1), cnt], -1).astype(F32)
    r.bind_accum(hip.upload(acc), acc.nbytes)
    rgb, rgba8 = r.display(**AUTO)
    st = r.display_state()
    _assert_metered(st, R.resolve(acc), f"accumulation {W}x{H}")
    assert np.abs(rgb - R.tone(R.resolve(acc), st["exposure"])).max() <= 1e-6
    r.close()
    hip.close()


def test_histogram_of_a_constant_image():
    """Every lane of every wave on one bin."""
    W, H = 67, 37
    r = _frame_only(W, H)
    img = np.full((H, W, 3), 0.18, F32)
    rgb, _ = r.display(img, **AUTO)
    st = r.display_state()
    _assert_metered(st, img, "constant")
    assert st["histogram"][53] == W * H
    assert abs(float(st["exposure"]) - 1.0516) < 5e-5
    assert np.abs(rgb - R.tone(img, st["exposure"])).max() <= 1e-6
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3 the target

def _assert_target(st, img, **kw):
    """`target` to a relative 2.5e-7 -- two binary32 ulps: everything before the exp2 is exact integers and binary64 sums stated
    term by term, so the device's binary64 exp2 can only move the final rounding to binary32."""
    want, mean = R.target(R.meter(R.luminance(img))[0], **kw)
    print(f"target {float(st['target'])!r} want {float(want)!r} log2_mean {float(st['log2_mean'])!r} want {mean!r}")
    assert abs(float(st["target"]) - float(want)) <= 2.5e-7 * float(want), (st["target"], want)
    assert abs(float(st["log2_mean"]) - mean) <= 2.5e-7 * abs(mean) + 1e-7
    return want


def test_target_matches_restatement():
    W, H = 67, 37
    r = _frame_only(W, H)
    img = _synthetic(W, H, 5)
    for low, high in ((0, 0), (100, 50), (500, 499)):
        r.display(img, auto=True, low=low / 1000, high=high / 1000)
        st = r.display_state()
        _assert_target(st, img, low_permille=low, high_permille=high)
        assert st["exposure"] == st["target"]                          # adapt = 1: a jump
    e = r.display_state()["exposure"]
    # an all-black frame leaves the exposure where it was
    black = np.zeros((H, W, 3), F32)
    rgb, _ = r.display(black, **AUTO)
    st = r.display_state()
    assert (st["counted"], st["below"], st["above"]) == (0, W * H, 0) and st["exposure"] == e and st["target"] == e
    assert st["log2_mean"] == 0 and not rgb.any()
    r.display_reset()
    r.display(black, **AUTO)
    st = r.display_state()
    assert st["exposure"] == 1 and st["target"] == 1 and st["below"] == W * H
    # ... and does not use up the jump of a fresh state
    r.display(img, auto=True, adapt=0.25)
    st = r.display_state()
    assert st["exposure"] == st["target"] != 1
    # the clamps
    free = float(R.target(R.meter(R.luminance(img))[0])[0])
    for lo, hi, want in ((free * 2, free * 4, free * 2), (free / 4, free / 2, free / 2), (2.0, 2.0, 2.0)):
        r.display(img, auto=True, min_exposure=lo, max_exposure=hi)
        st = r.display_state()
        assert st["target"] == F32(want) and st["exposure"] == F32(want), (lo, hi)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4 adaptation and the state

def test_adaptation_keep_reset_and_manual_commit():
    W, H = 64, 40
    r = _frame_only(W, H)
    base = _synthetic(W, H, 6, edges=False)
    imgs = [base, base * F32(8), base * F32(0.1)]
    st0 = r.display_state()
    assert st0["exposure"] == 1 and st0["target"] == 1 and st0["counted"] == 0 and not st0["histogram"].any()
    prev = None
    for k, img in enumerate(imgs):
        rgb, rgba8 = r.display(img, auto=True, adapt=0.25, curve="reinhard")
        st = r.display_state()
        _assert_target(st, img)
        want = R.adapt(prev, st["target"], 0.25)                       # binary32, from the reported target
        assert st["exposure"].tobytes() == want.tobytes(), (k, st["exposure"], want)
        assert np.abs(rgb - R.tone(img, st["exposure"], "reinhard")).max() <= 1e-6
        prev = st["exposure"]
    assert prev != st["target"]
    # RZ_DISPLAY_KEEP: the same pixels, the state as it was
    before = r.display_state()
    kept = r.display(imgs[0], auto=True, adapt=0.25, keep=True)
    assert _key(r.display_state()) == _key(before)
    kept_manual = r.display(imgs[0], exposure=3.0, keep=True)
    assert _key(r.display_state()) == _key(before)
    assert _same(kept, r.display(imgs[0], auto=True, adapt=0.25))
    st = r.display_state()
    assert st["exposure"].tobytes() == R.adapt(before["exposure"], st["target"], 0.25).tobytes() and _key(st) != _key(before)
    # a manual call commits its exposure
    assert _same(kept_manual, r.display(imgs[0], exposure=3.0))
    st = r.display_state()
    assert st["exposure"] == 3 and st["target"] == 3 and st["log2_mean"] == 0
    r.display(imgs[1], auto=True, adapt=0.25)
    st = r.display_state()
    assert st["exposure"].tobytes() == R.adapt(F32(3.0), st["target"], 0.25).tobytes()
    # after a reset the exposure jumps to its target
    r.display_reset()
    st = r.display_state()
    assert st["exposure"] == 1 and st["counted"] == 0 and not st["histogram"].any()
    r.display(imgs[2], auto=True, adapt=0.25)
    st = r.display_state()
    assert st["exposure"] == st["target"]
    # a frame of another size does not touch the state
    r.set_frame(frame_params(_CAMERA, 32, 16, 0, 5, 1, 0))
    assert _key(r.display_state()) == _key(st)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5 the curves
#
# Bounds: |rgb32f - float64 restatement| <= 1e-6 with the linear transfer (the numpy binary32 evaluation of the same expressions
# is within 2.5e-7 of float64 on these inputs: a handful of roundings of values <= 1), and <= 4e-6 with the sRGB transfer (that
# error times the OETF's largest slope, 12.92, plus powf's ulps).
# Measured on an MI355X (profiles/display/README.md): at most 2.35e-7 linear (ACES, E = 0.5), 2.19e-7 sRGB.

CURVE_BOUND = {"linear": 1e-6, "srgb": 4e-6}


def test_curves_match_restatement():
    W, H = 96, 64
    rng = np.random.default_rng(7)
    img = np.exp(rng.uniform(np.log(1e-4), np.log(64.0), (H, W, 3))).astype(F32)
    img[0, :8] = 0.0
    img[1, :8] = -np.exp(rng.uniform(np.log(1e-6), np.log(1e-2), (8, 3))).astype(F32)
    img[2, 0] = (1e-4, 64.0, 0.0031308)
    r = _frame_only(W, H)
    worst = {"linear": 0.0, "srgb": 0.0}
    for curve in ("clamp", "reinhard", "aces"):
        for transfer in ("linear", "srgb"):
            for exposure in (0.5, 3.0):
                what = f"{curve} {transfer} E={exposure}"
                rgb, rgba8 = r.display(img, exposure=exposure, curve=curve, transfer=transfer, white=6.0)
                want = R.tone(img, exposure, curve, 6.0, transfer)
                err = float(np.abs(rgb.astype(np.float64) - want).max())
                print(f"{what}: worst |err| {err:.3g}")
                worst[transfer] = max(worst[transfer], err)
                bound = CURVE_BOUND[transfer]
                assert err <= bound, what
                assert rgb.min() >= 0 and rgb.max() <= 1
                # the bytes: the quantisation of the call's own floats exactly; against the restatement at most one step, and
                # only where the restatement is within the bound of a rounding boundary
                assert np.array_equal(rgba8, R.quantise(rgb)), what
                ref8 = R.quantise(want)
                d = np.abs(rgba8.astype(int) - ref8.astype(int))[..., :3]
                assert d.max() <= 1, what
                scaled = 255.0 * want
                near = np.abs(scaled - (np.floor(scaled) + 0.5)) <= 255.0 * bound
                assert near[d == 1].all(), what
    print(f"worst |err|: linear {worst['linear']:.3g}, srgb {worst['srgb']:.3g}")
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6 isolation

def test_leaves_the_render_state_alone():
    sc = S.bunny_scene(n=24, aspect=16 / 9)
    W, H = 96, 54

    def run(with_display):
        r = _setup(sc, W, H, spp=4, bounces=4)
        r.denoise_temporal()                            # a history to leave alone
        plan = r.debug_last_plan()
        acc0 = r.read_accum()
        tmp = [r.debug_read_temporal(k).tobytes() for k in range(5)]
        if with_display:
            r.display(auto=True, curve="aces", transfer="srgb")
            r.display(r.denoise(iterations=1), auto=True, adapt=0.5)
            r.present_display(auto=True, curve="reinhard")
            r.present_display("denoise", auto=True, transfer="srgb", filter=dict(iterations=2))
            assert r.debug_last_plan() == plan
            assert r.read_accum().tobytes() == acc0.tobytes()
            assert [r.debug_read_temporal(k).tobytes() for k in range(5)] == tmp
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 4, 4))
        r.render()
        acc = r.read_accum()
        r.close()
        return acc0, acc

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 7 errors

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    W, H = 16, 8
    n = W * H
    r = _setup(sc, W, H)
    r.display(r.denoise(iterations=0), auto=True, adapt=0.5)           # a state to leave alone
    before = _key(r.display_state())
    pin = hip.upload(_synthetic(W, H, 8))
    p32, p8 = hip.alloc(n * 12 + 16, fill=0x5A), hip.alloc(n * 4 + 16, fill=0x5A)

    def call(ctx, params=None, args=(pin, n * 12, p32, n * 12, p8, n * 4), flags=0):
        a = list(args)
        return L.rz_display(ctx, params, C.c_void_p(a[0]), a[1], C.c_void_p(a[2]), a[3], C.c_void_p(a[4]), a[5], flags)

    def params(**kw):
        p = _lib.DisplayParams(1, 1.0, 0.18, 1 / 64, 64.0, 0.5, 0, 0, 1, 4.0, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    nan, inf = float("nan"), float("inf")
    assert call(None) == -1
    bad_fields = [dict(exposure_mode=2), dict(exposure_mode=-1), dict(exposure_mode=0, exposure=0.0), dict(exposure_mode=0, exposure=inf),
                  dict(exposure_mode=0, exposure=nan), dict(exposure_mode=0, exposure=-2.0),
                  dict(key=0.0), dict(key=nan), dict(key=inf), dict(min_exposure=0.0), dict(min_exposure=nan), dict(max_exposure=inf),
                  dict(min_exposure=2.0, max_exposure=1.0), dict(adapt=-0.1), dict(adapt=1.5), dict(adapt=nan),
                  dict(low_permille=-1), dict(high_permille=-1), dict(low_permille=500, high_permille=500), dict(low_permille=1000),
                  dict(curve=3), dict(curve=-1), dict(white=0.0), dict(white=nan), dict(white=inf), dict(transfer=2), dict(transfer=-1)]
    for bad in bad_fields:
        assert call(r._c, params(**bad)) == -1, bad
    p = _lib.DisplayParams(1, 1.0, 0.18, 1 / 64, 64.0, 0.5, 0, 0, 1, 4.0, 1)
    p.reserved[4] = 1
    assert call(r._c, C.byref(p)) == -1 and b"reserved" in L.rz_last_error(r._c)
    assert call(r._c, params(), flags=0x2) == -1 and call(r._c, params(), flags=0x8) == -1
    assert call(r._c, params(), args=(pin + 2, n * 12, p32, n * 12, p8, n * 4)) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert call(r._c, params(), args=(pin, n * 12, p32 + 1, n * 12, p8, n * 4)) == -1
    assert call(r._c, params(), args=(pin, n * 12, p32, n * 12, p8 + 2, n * 4)) == -1
    assert call(r._c, params(), args=(pin, n * 12 - 4, p32, n * 12, p8, n * 4)) == -7
    assert call(r._c, params(), args=(pin, n * 12, p32, n * 12 - 4, p8, n * 4)) == -7
    assert call(r._c, params(), args=(pin, n * 12, p32, n * 12, p8, n * 4 - 1)) == -7
    # rz_present_display
    pp = _lib.PresentParams()
    buf8, buf32 = np.zeros(n * 4, np.uint8), np.zeros(n * 3, F32)

    def present(present_params=C.byref(pp), display=None, source=0, filt=None, n8=buf8.nbytes, n32=buf32.nbytes):
        return L.rz_present_display(r._c, present_params, display, source, filt, buf8.ctypes.data, n8, buf32.ctypes.data, n32)

    assert L.rz_present_display(None, C.byref(pp), None, 0, None, None, 0, None, 0) == -1
    assert present(present_params=None) == -1
    assert present(source=3) == -1 and present(source=-1) == -1
    dn = _lib.DenoiseParams(5, 0.5, 128.0, 1.0, 1)
    assert present(source=0, filt=C.byref(dn)) == -1 and b"source 0" in L.rz_last_error(r._c)
    assert present(display=params(curve=7)) == -1
    dn.iterations = 12
    assert present(source=1, filt=C.byref(dn)) == -1
    tp = _lib.TemporalParams(**{k: v for k, v in _lib.TEMPORAL_DEFAULTS.items()})
    tp.max_history = 0
    assert present(source=2, filt=C.byref(tp)) == -1
    assert present(n8=n * 4 - 1) == -7 and present(n32=n * 12 - 4) == -7
    assert L.rz_display_state(r._c, None) == -1 and L.rz_display_state(None, None) == -1 and L.rz_display_reset(None) == -1
    r.sync()
    for ptr, nb in ((p32, n * 12 + 16), (p8, n * 4 + 16)):
        assert (hip.download(ptr, nb) == 0x5A).all()                    # nothing was launched
    assert not buf8.any() and not buf32.any()
    assert _key(r.display_state()) == before                           # and the state is as it was
    assert r.debug_read_temporal(0) is None                            # (the refused temporal source made no history)
    # the context stays usable; each output alone, and none at all (which still meters)
    assert call(r._c, params()) == 0
    r.sync()
    both32, both8 = hip.download(p32, n * 12).copy(), hip.download(p8, n * 4).copy()
    assert (both8.reshape(-1, 4)[:, 3] == 255).all()
    r.display_reset()
    q32, q8 = hip.alloc(n * 12, fill=0), hip.alloc(n * 4, fill=0)
    assert call(r._c, params(), args=(pin, n * 12, q32, n * 12, None, 0)) == 0
    r.display_reset()
    assert call(r._c, params(), args=(pin, n * 12, None, 0, q8, n * 4)) == 0
    r.display_reset()
    assert call(r._c, params(), args=(pin, n * 12, None, 0, None, 0)) == 0
    r.sync()
    assert r.display_state()["counted"] > 0
    # (the first successful call adapted half-way from the state left alone above; these three started fresh, so compare them
    #  with a fresh call)
    r.display_reset()
    assert call(r._c, params()) == 0
    r.sync()
    assert hip.download(p32, n * 12).tobytes() == hip.download(q32, n * 12).tobytes()
    assert hip.download(p8, n * 4).tobytes() == hip.download(q8, n * 4).tobytes()
    assert both32.tobytes() != hip.download(p32, n * 12).tobytes()
    # in place: rgb32f may be rgb_in
    inplace = hip.upload(hip.download(pin, n * 12))
    r.display_reset()
    assert call(r._c, params(), args=(inplace, n * 12, inplace, n * 12, None, 0)) == 0
    r.sync()
    assert hip.download(inplace, n * 12).tobytes() == hip.download(q32, n * 12).tobytes()
    # the accumulation of a tile of a group frame: refused; a caller's buffer is not
    r.set_frame(frame_params(sc.camera, W, H, 2, 5, 1, 0, 0, 2))
    assert call(r._c, params(), args=(None, 0, p32, n * 12, p8, n * 4)) == -1 and b"whole frame" in L.rz_last_error(r._c)
    assert call(r._c, params()) == 0
    r.close()
    # no frame
    nof = Renderer(0)
    nof.upload_scene(sc)
    assert call(nof._c) == -5
    info = _lib.DisplayInfo()
    assert L.rz_display_state(nof._c, C.byref(info)) == 0 and info.exposure == 1 and info.target == 1 and info.counted == 0
    assert L.rz_display_reset(nof._c) == 0
    nof.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8 speed

# Recorded medians on an MI355X (profiles/display/README.md): rz_display (auto, ACES, sRGB) 800 x 600: 0.033 ms,
# 1920 x 1080: 0.063 ms (rz_present_denoised with K = 0 in the same run: 0.21 and 0.67 ms).  The ceilings are three times the
# recorded medians: margin for a shared machine.
@pytest.mark.parametrize("W,H,ceiling", [(800, 600, 3 * 0.033), (1920, 1080, 3 * 0.063)])
def test_speed_ceiling(W, H, ceiling):
    """One rz_display call (meter, expose, tone: auto exposure, ACES, sRGB; rgb32f and rgba8 written) on device buffers, beside
    rz_present_denoised with K = 0 -- the existing path that moves the same pixels without the display stage (it ends in a copy
    to the host).  Medians of 25, device events."""
    hip = Hip()
    sc = S.reference_scene(aspect=W / H)
    r = _setup(sc, W, H)
    n = W * H
    din, d32, d8 = hip.upload(r.denoise(iterations=0)), hip.alloc(n * 12), hip.alloc(n * 4)
    stream = hip.stream()
    r.set_stream(stream)
    a, b = hip.event(), hip.event()
    kw = dict(auto=True, adapt=0.5, curve="aces", transfer="srgb")

    def timed(fn):
        fn()
        r.sync()
        out = []
        for _ in range(25):
            hip.ok(hip.L.hipEventRecord(a, stream))
            fn()
            hip.ok(hip.L.hipEventRecord(b, stream))
            hip.ok(hip.L.hipEventSynchronize(b))
            ms = C.c_float()
            hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
            out.append(ms.value)
        return float(np.median(out))

    t = timed(lambda: r.display_device(din, d32, d8, **kw))
    t_present = timed(lambda: r.present_denoised(iterations=0))
    r.set_stream(0)
    r.close()
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    hip.L.hipStreamDestroy(stream)
    hip.close()
    print(f"display {W}x{H}: rz_display {t:.4f} ms; rz_present_denoised K=0 {t_present:.4f} ms")
    assert t <= ceiling, t

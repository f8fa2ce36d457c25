"""Edge anti-aliasing (rz_antialias, rz_present_antialiased; rz_antialias.hip) on the GPU: the edge mask against the restatement
(antialias_ref.py) bit for bit, given the GPU's own frame-size guides; the guides against rz_trace_rays; flat pixels bit-equal to
the input and edge pixels bit-equal to the binary32 box mean of rz_upscale's own output on the same context; the whole frame
against the float64 restatement; non-finite input, factor 1, the present call, host and device paths, isolation from the
render, temporal and display state, errors, the backstop, the C++ front end, and the cost next to rz_upscale."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import antialias_ref as AR
import denoise_ref as DR
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, RayZenError, Renderer, frame_params
from test_denoise_gpu import _assert_same_hits, _setup, _trace_pixels
from test_display_gpu import _key
from test_rays_gpu import Hip
from test_upscale_gpu import _bad_patterns, _filled, _median_ms, _window_max, sliver_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SCENES = {"cornell": S.cornell_scene, "glass": lambda: S.reference_scene(aspect=4 / 3), "sliver": sliver_scene}
FRAMES = [(1, 1), (3, 2), (65, 5), (33, 17), (100, 75)]         # 65 and 100 wide: more than one unit per row
FACTORS = (2, 3, 4)


def _box_min(m, s):
    H, W = m.shape[:2]
    return m.reshape(H // s, s, W // s, s, -1).min(axis=(1, 3))


# Tolerance (test_upscale_gpu.py's rule): |gpu - ref| <= 1e-4 (|ref| + m) + 1e-7, m the largest |c| of the pixel's 4 x 4 window.
# An edge pixel is the mean of s^2 sub-pixels, each held to that rule in its own window; m here is the SMALLEST of the sub-pixels'
# window maxima, the strictest reading.  A flat pixel is compared bit for bit elsewhere and passes this with error 0.
def _assert_close(got, want, c, s, what=""):
    m = _box_min(_window_max(c, s), s)
    err = np.abs(got.astype(np.float64) - want)
    scale = np.abs(want) + m
    worst = float((err / (scale + 1e-30)).max())
    print(f"{what}: worst relative error {worst:.3g}")
    ok = err <= 1e-4 * scale + 1e-7
    assert ok.all(), f"{what}: {int((~ok).any(-1).sum())} pixels off; worst relative {worst:.3g}"


def _mean_of_upscale(r, c, s, **kw):
    """The binary32 box mean, in the stated order, of rz_upscale's own rgb32f at factor s on the same context; and its guides."""
    up, g_hi = r.upscale(c, factor=s, guides=True, **kw)
    return AR.box_mean32(up, s), g_hi


# ---------------------------------------------------------------------------------------------------------------------
# edges, guides and colours

@pytest.mark.parametrize("w,h", FRAMES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_edges_guides_and_colours(name, w, h):
    sc = SCENES[name]()
    r = _setup(sc, w, h, spp=2)
    c_acc = DR.resolve(r.read_accum())
    rng = np.random.default_rng(w * 100 + h)
    c_syn = (np.exp(rng.normal(-1.0, 1.5, (h, w, 1))) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(F32)
    shares = []
    for s in FACTORS:
        got, g, edge = r.antialias(factor=s, guides=True, edges=True)          # rgb_in NULL: the accumulation
        if s == FACTORS[0]:
            _assert_same_hits(g, _trace_pixels(r, sc.camera, w, h), name)
            g0 = g
        assert g.tobytes() == g0.tobytes()
        assert np.array_equal(edge, AR.edge_mask(c_acc, g, sc.materials, sc.camera.inv_proj))
        shares.append(float(edge.mean()))
        assert got[~edge].tobytes() == c_acc[~edge].tobytes()                   # flat: c exactly
        for demod in (True, False):
            got = r.antialias(factor=s, demodulate=demod)
            mean32, g_hi = _mean_of_upscale(r, None, s, demodulate=demod)
            assert got[~edge].tobytes() == c_acc[~edge].tobytes()
            assert got[edge].tobytes() == mean32[edge].tobytes(), f"{name} {w}x{h} s={s} demodulate={demod}: the box mean's bits"
            want, _ = AR.antialias(c_acc, g, g_hi, sc.materials, sc.camera.inv_proj, factor=s, demodulate=demod)
            _assert_close(got, want, c_acc, s, f"{name} {w}x{h} s={s} demodulate={demod} accumulation")
            assert r.antialias(c_acc, factor=s, demodulate=demod).tobytes() == got.tobytes()    # the same colour handed over
            assert r.antialias(factor=s, demodulate=demod).tobytes() == got.tobytes()           # two calls, the same bytes
            assert np.isfinite(got).all()
        # non-default sigmas and edge thresholds, on a colour of its own
        kw = dict(sigma_normal=16.0, sigma_plane=0.5)
        got, edge2 = r.antialias(c_syn, factor=s, edge_normal=0.99, edge_plane=0.25, edges=True, **kw)
        assert np.array_equal(edge2, AR.edge_mask(c_syn, g, sc.materials, sc.camera.inv_proj, edge_normal=0.99, edge_plane=0.25))
        assert (edge2 >= edge).all()
        mean32, g_hi = _mean_of_upscale(r, c_syn, s, **kw)
        assert got[~edge2].tobytes() == c_syn[~edge2].tobytes() and got[edge2].tobytes() == mean32[edge2].tobytes()
        want, _ = AR.antialias(c_syn, g, g_hi, sc.materials, sc.camera.inv_proj, factor=s, edge_normal=0.99, edge_plane=0.25, **kw)
        _assert_close(got, want, c_syn, s, f"{name} {w}x{h} s={s} rgb_in")
    r.close()
    print(f"{name} {w}x{h}: edge share {shares[0]:.3f}")
    if (name, w, h) in (("glass", 100, 75), ("sliver", 33, 17)):
        # a wave takes 64 / s^2 pixels at a time: some 64-pixel run of a row fills its queue more than once (s = 4: 4 pixels)
        per_unit = max(int(edge[y, x:x + 64].sum()) for y in range(h) for x in range(0, w, 64))
        assert per_unit > 2 * (64 // 16), per_unit


# ---------------------------------------------------------------------------------------------------------------------
# non-finite input at 65 x 5: the patterns of test_nonfinite_gpu.py's kind, sized for five rows

def test_bad_pixels_are_edges_and_contained():
    w, h, s = 65, 5, 2
    sc = S.cornell_scene()
    r = _setup(sc, w, h, render=False)
    rgb0, g, edge0 = r.antialias(np.zeros((h, w, 3), F32), guides=True, edges=True)
    g_hi = r.upscale(np.zeros((h, w, 3), F32), guides=True)[1]
    rng = np.random.default_rng(21)
    clean = rng.uniform(0.1, 2.0, (h, w, 3)).astype(F32)
    vals = [np.nan, np.inf, -np.inf]
    for pname, mask in _bad_patterns(g, rng).items():
        c = clean.copy()
        for y, x in zip(*np.nonzero(mask)):             # NaN, +Inf and -Inf in turn, in one channel or in all three
            v = vals[int(rng.integers(3))]
            if rng.random() < 0.5:
                c[y, x] = v
            else:
                c[y, x, int(rng.integers(3))] = v
        assert np.array_equal(DR.bad_pixels(c), mask), pname
        for demod in (True, False):
            got, edge = r.antialias(c, demodulate=demod, edges=True)
            want, edge_ref = AR.antialias(c, g, g_hi, sc.materials, sc.camera.inv_proj, demodulate=demod)
            assert np.array_equal(edge, edge_ref) and np.array_equal(edge, edge0 | mask), pname
            assert np.isfinite(got).all(), f"{pname}: {int((~np.isfinite(got)).any(-1).sum())} pixels not finite"
            _assert_close(got, want, c, s, f"{pname} demodulate={demod}")
            if pname == "all":
                assert not got.view(np.uint32).any()    # no tap anywhere, stage 3 on a bad pixel: exactly 0
            # containment: where no bad pixel lies within two pixels, the bytes are the clean frame's
            near = np.zeros((h, w), bool)
            for y, x in zip(*np.nonzero(mask)):
                near[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = True
            ref_clean = r.antialias(clean, demodulate=demod)
            assert got[~near].tobytes() == ref_clean[~near].tobytes(), pname
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# factor 1, present

def test_factor_1_is_c_itself_and_still_classifies():
    sc = S.reference_scene(aspect=4 / 3)
    w, h = 65, 5
    r = _setup(sc, w, h, spp=2)
    c = DR.resolve(r.read_accum())
    assert r.antialias(factor=1).tobytes() == c.tobytes()
    out, g, edge = r.antialias(factor=1, guides=True, edges=True)
    assert out.tobytes() == c.tobytes()
    _assert_same_hits(g, _trace_pixels(r, sc.camera, w, h), "factor 1")
    assert np.array_equal(edge, AR.edge_mask(c, g, sc.materials, sc.camera.inv_proj)) and edge.any() and not edge.all()
    x = c.copy()
    x[2, 7] = np.nan
    x[0, 0, 1] = -np.inf
    assert r.antialias(x, factor=1).tobytes() == x.tobytes()            # bad or not
    out, edge_x = r.antialias(x, factor=1, edges=True)
    assert out.tobytes() == x.tobytes() and edge_x[2, 7] and edge_x[0, 0]
    r.close()


@pytest.mark.parametrize("source", ["accum", "denoise", "temporal"])
def test_present_antialiased_factor_1_equals_present_display(source):
    sc = S.reference_scene(aspect=4 / 3)
    w, h = 100, 75
    kw = dict(fps=57.3, show_fps=True, show_lights=True, show_bvh=True)
    filt = None if source == "accum" else dict(iterations=2)
    outs = []
    for aa in (False, True):
        r = _setup(sc, w, h, spp=2)                     # (a context each: source "temporal" advances the history)
        for disp in (dict(), dict(auto=True, curve="aces", transfer="srgb")):
            if aa:
                outs.append(r.present_antialiased(source, factor=1, filter=filt, **kw, **disp))
            else:
                outs.append(r.present_display(source, filter=filt, **kw, **disp))
        r.close()
    for a, b in zip(outs[:2], outs[2:]):
        assert a[0].shape == (h, w, 3) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_present_antialiased_equals_present_display_of_the_antialiased_colour():
    hip = Hip()
    sc = S.reference_scene(aspect=4 / 3)
    w, h, s = 100, 75, 2
    kw = dict(fps=12.5, show_fps=True, show_lights=True, show_bvh=True)
    r = _setup(sc, w, h, spp=2)
    aa = r.antialias(factor=s)
    rgb, rgba8 = r.present_antialiased("accum", factor=s, **kw)
    assert rgb.shape == (h, w, 3) and rgba8.shape == (h, w, 4)
    # sources 1 and 2: the denoisers run first, then the same pass
    for source, den in (("denoise", r.denoise(iterations=2)), ("temporal", r.denoise_temporal(iterations=2, keep=True))):
        a = r.present_antialiased(source, factor=s, filter=dict(iterations=2), show_fps=False)
        want = np.clip(r.antialias(den, factor=s), 0.0, 1.0)
        assert a[0].tobytes() == want.tobytes(), source
    # ... and it commits its exposure to the display state as rz_present_display does
    r.display_reset()
    shown = r.present_antialiased("accum", factor=s, auto=True, adapt=0.5, curve="aces", transfer="srgb", **kw)
    state = r.display_state()
    r.close()
    # rz_present / rz_present_display on a context whose accumulation is (anti-aliased, 1)
    buf = np.concatenate([aa, np.ones((h, w, 1), F32)], -1)
    dbuf = hip.upload(buf)
    hip.ok(hip.L.hipDeviceSynchronize())
    r2 = Renderer(0)
    r2.upload_scene(sc)
    r2.bind_accum(dbuf, buf.nbytes)
    r2.set_frame(frame_params(sc.camera, w, h, len(sc.lights), 5, 1, 0))
    rgb2, rgba82 = r2.present(**kw)
    plain = r2.present(show_fps=False)
    shown2 = r2.present_display("accum", auto=True, adapt=0.5, curve="aces", transfer="srgb", **kw)
    state2 = r2.display_state()
    r2.close()
    hip.close()
    assert rgba8.tobytes() == rgba82.tobytes() and rgb.tobytes() == rgb2.tobytes()
    assert rgba8.tobytes() != plain[1].tobytes()        # the overlays are there, drawn after the pass
    assert state["exposure"] != 1.0 and _key(state) == _key(state2)
    assert shown[0].tobytes() == shown2[0].tobytes() and shown[1].tobytes() == shown2[1].tobytes()


def test_present_antialiased_source_2_advances_the_history_as_present_temporal_does():
    sc = S.reference_scene(aspect=4 / 3)
    w, h = 64, 48
    hist = []
    for aa in (False, True):
        r = _setup(sc, w, h)
        for _ in range(2):
            if aa:
                r.present_antialiased("temporal", factor=2)
            else:
                r.present_temporal()
        hist.append([r.debug_read_temporal(k).tobytes() for k in range(5)])
        r.close()
    assert hist[0] == hist[1]


# ---------------------------------------------------------------------------------------------------------------------
# paths, state

def test_host_and_device_paths_agree_and_null_outputs():
    hip = Hip()
    sc = S.reference_scene(aspect=4 / 3)
    w, h, s = 65, 5, 3
    n = w * h
    r = _setup(sc, w, h, spp=2)
    rgb, g, edge = r.antialias(factor=s, guides=True, edges=True)
    e8 = edge.astype(np.uint8)
    d32, dg, de = _filled(hip, n * 12, 0x5A), _filled(hip, n * 48, 0x5A), _filled(hip, n + 3, 0x5A)
    r.antialias_device(None, d32, dg, de + 1, factor=s)                 # edges needs no alignment
    r.sync()
    assert hip.download(d32, n * 12).tobytes() == rgb.tobytes()
    assert hip.download(dg, n * 48).tobytes() == g.tobytes()
    raw = hip.download(de, n + 3)
    assert raw[1:n + 1].tobytes() == e8.tobytes() and (raw[[0, n + 1, n + 2]] == 0x5A).all()
    # the input from device memory
    c = DR.resolve(r.read_accum())
    din = hip.upload(c)
    d32b = _filled(hip, n * 12, 0)
    r.antialias_device(din, d32b, None, None, factor=s)
    r.sync()
    assert hip.download(d32b, n * 12).tobytes() == rgb.tobytes()
    # factor 1 on the device: a copy
    d1 = _filled(hip, n * 12, 0)
    r.antialias_device(din, d1, None, None, factor=1)
    r.sync()
    assert hip.download(d1, n * 12).tobytes() == c.tobytes() == hip.download(din, n * 12).tobytes()
    # NULL outputs: each alone, and none
    p32, pg, pe = _filled(hip, n * 12, 0), _filled(hip, n * 48, 0), _filled(hip, n, 0x5A)
    r.antialias_device(None, None, pg, None, factor=s)
    r.sync()
    assert not hip.download(p32, n * 12).any() and hip.download(pg, n * 48).tobytes() == g.tobytes()
    r.antialias_device(None, None, None, pe, factor=s)
    r.sync()
    assert hip.download(pe, n).tobytes() == e8.tobytes() and not hip.download(p32, n * 12).any()
    r.antialias_device(None, p32, None, None, factor=s)
    r.antialias_device(None, None, None, None, factor=s)
    r.sync()
    assert hip.download(p32, n * 12).tobytes() == rgb.tobytes()
    r.close()
    hip.close()


def test_leaves_render_temporal_display_state_and_the_upsampler_alone():
    sc = S.bunny_scene(n=24, aspect=16 / 9, bunny_material=3)           # glass: currentIor is live state
    w, h = 96, 54

    def run(with_aa):
        r = _setup(sc, w, h, spp=4, bounces=4)
        r.denoise_temporal()                            # a history and a display state to leave alone
        r.display(auto=True, adapt=0.5)
        plan = r.debug_last_plan()
        acc0 = r.read_accum()
        tmp = [r.debug_read_temporal(k).tobytes() for k in range(5)]
        disp = _key(r.display_state())
        up0 = [a.tobytes() for a in r.upscale(factor=3, guides=True)]
        if with_aa:
            r.antialias(guides=True, edges=True)
            r.antialias(r.denoise(iterations=1), factor=3)
            assert _key(r.display_state()) == disp
            r.present_antialiased("accum")
            r.present_antialiased("denoise", factor=3, filter=dict(iterations=1))
            assert r.debug_last_plan() == plan
            assert r.read_accum().tobytes() == acc0.tobytes()
            assert [r.debug_read_temporal(k).tobytes() for k in range(5)] == tmp        # sources 0 and 1
        assert [a.tobytes() for a in r.upscale(factor=3, guides=True)] == up0
        r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), 4, 4, 4))
        r.render()
        acc = r.read_accum()
        r.close()
        return acc0, acc

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# errors, the backstop

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 16, 8
    n = w * h
    r = _setup(sc, w, h)
    pin = hip.upload(DR.resolve(r.read_accum()))
    p32, pg, pe = _filled(hip, n * 12 + 16, 0x5A), _filled(hip, n * 48 + 16, 0x5A), _filled(hip, n + 16, 0x5A)

    def call(ctx, params=None, args=(None, 0, p32, n * 12, pg, n * 48, pe, n), flags=0):
        a = list(args)
        return L.rz_antialias(ctx, params, C.c_void_p(a[0]), a[1], C.c_void_p(a[2]), a[3], C.c_void_p(a[4]), a[5], C.c_void_p(a[6]), a[7],
                              flags)

    def params(**kw):
        p = _lib.AntialiasParams(2, 128.0, 1.0, 1, 0.9, 1.0)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    nan, inf = float("nan"), float("inf")
    assert call(None) == -1
    for bad in (dict(factor=0), dict(factor=5), dict(factor=-2), dict(sigma_plane=0.0), dict(sigma_plane=-1.0), dict(sigma_plane=inf),
                dict(sigma_normal=-1.0), dict(sigma_normal=nan), dict(sigma_normal=inf), dict(sigma_plane=nan), dict(demodulate=2),
                dict(edge_normal=1.5), dict(edge_normal=-1.5), dict(edge_normal=nan), dict(edge_normal=inf), dict(edge_normal=-inf),
                dict(edge_plane=-0.5), dict(edge_plane=nan), dict(edge_plane=inf)):
        assert call(r._c, params(**bad)) == -1, bad
    for ok in (dict(edge_normal=1.0), dict(edge_normal=-1.0), dict(edge_plane=0.0)):
        assert call(r._c, params(**ok)) == 0, ok
    r.sync()
    for ptr, nb in ((p32, n * 12), (pg, n * 48), (pe, n)):              # (those three wrote: fill again)
        hip.ok(hip.L.hipMemset(C.c_void_p(ptr), 0x5A, nb))
    hip.ok(hip.L.hipDeviceSynchronize())
    for k in range(2):
        p = _lib.AntialiasParams(2, 128.0, 1.0, 1, 0.9, 1.0)
        p.reserved[k] = 7
        assert call(r._c, C.byref(p)) == -1
    assert call(r._c, flags=0x4) == -1 and call(r._c, flags=0x2) == -1
    assert call(r._c, args=(pin + 2, n * 12, p32, n * 12, pg, n * 48, pe, n)) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert call(r._c, args=(None, 0, p32 + 2, n * 12, pg, n * 48, pe, n)) == -1
    assert call(r._c, args=(None, 0, p32, n * 12, pg + 4, n * 48, pe, n)) == -1
    assert call(r._c, args=(pin, n * 12, pin, n * 12, pg, n * 48, pe, n)) == -1 and b"rgb_in" in L.rz_last_error(r._c)     # in place
    assert call(r._c, params(factor=1), args=(pin, n * 12, pin, n * 12, None, 0, None, 0)) == -1
    assert call(r._c, args=(pin, n * 12 - 1, p32, n * 12, pg, n * 48, pe, n)) == -7
    assert call(r._c, args=(None, 0, p32, n * 12 - 1, pg, n * 48, pe, n)) == -7
    assert call(r._c, args=(None, 0, p32, n * 12, pg, n * 48 - 1, pe, n)) == -7
    assert call(r._c, args=(None, 0, p32, n * 12, pg, n * 48, pe, n - 1)) == -7
    pp = _lib.PresentParams()
    buf8 = np.zeros(n * 4, np.uint8)
    buf32 = np.zeros(n * 3, F32)

    def present(ctx, present_p=C.byref(pp), aa=None, disp=None, source=0, filt=None, n8=buf8.nbytes, n32=buf32.nbytes):
        return L.rz_present_antialiased(ctx, present_p, aa, disp, source, filt, buf8.ctypes.data, n8, buf32.ctypes.data, n32)

    assert present(None) == -1 and present(r._c, present_p=None) == -1
    assert present(r._c, aa=params(factor=5)) == -1 and present(r._c, aa=params(factor=0)) == -1
    assert present(r._c, aa=params(edge_normal=2.0)) == -1 and present(r._c, aa=params(edge_plane=-1.0)) == -1
    assert present(r._c, source=3) == -1 and present(r._c, source=-1) == -1
    assert present(r._c, source=0, filt=params()) == -1                 # filter_params with source 0
    dn = _lib.DenoiseParams(12, 0.5, 128.0, 1.0, 1)
    assert present(r._c, source=1, filt=C.byref(dn)) == -1
    dd = _lib.DisplayParams(0, 1.0, 0.18, 1 / 64, 64.0, 1.0, 0, 0, 7, 4.0, 0)
    assert present(r._c, disp=C.byref(dd)) == -1
    assert present(r._c, n8=n * 4 - 1) == -7 and present(r._c, n32=n * 12 - 1) == -7
    assert not buf8.any() and not buf32.any()
    r.sync()
    for ptr, nb in ((p32, n * 12 + 16), (pg, n * 48 + 16), (pe, n + 16)):
        assert (hip.download(ptr, nb) == 0x5A).all()            # nothing was launched
    # the context stays usable
    assert call(r._c) == 0 and present(r._c) == 0
    r.sync()
    assert buf8.any() and (hip.download(pe, n) <= 1).all()
    # a tile of a group frame: refused
    r.set_frame(frame_params(sc.camera, w, h, 2, 5, 1, 0, 0, 2))
    assert call(r._c) == -1 and b"whole frame" in L.rz_last_error(r._c)
    assert present(r._c) == -1
    r.close()
    # no frame / no scene / no materials
    nof = Renderer(0)
    nof.upload_scene(sc)
    assert call(nof._c) == -5 and present(nof._c) == -5
    nof.close()
    empty = Renderer(0)
    empty.set_frame(frame_params(sc.camera, w, h, 2, 5, 1, 0))
    assert call(empty._c) == -5 and present(empty._c) == -5
    empty.close()
    nomat = Renderer(0)
    for b in S.BINDING_DTYPES:
        nomat.upload(b, sc.arrays[b][:0] if b == S.BIND_MATERIALS else sc.arrays[b])
    nomat.set_frame(frame_params(sc.camera, w, h, 2, 5, 1, 0))
    assert call(nomat._c) == -5 and b"material" in L.rz_last_error(nomat._c)
    nomat.close()
    hip.close()


def test_backstop_host_path_reports_and_device_path_leaves_it_to_sync():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 16, 8
    r = _setup(sc, w, h)
    before = r.antialias(guides=True, edges=True)
    r.sync()
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    with pytest.raises(RayZenError) as e:
        r.antialias(guides=True, edges=True)
    message = str(e.value).split("): ", 1)[1]
    assert e.value.code == -9 and message.startswith("rz_antialias: ") and "0x8" in message, str(e.value)
    r.sync()                                            # reported once, then clear
    after = r.antialias(guides=True, edges=True)
    assert [a.tobytes() for a in after] == [b.tobytes() for b in before]
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    with pytest.raises(RayZenError) as e:
        r.present_antialiased("accum")
    assert e.value.code == -9 and "rz_present_antialiased: " in str(e.value)
    # the device path returns at once and leaves the word to rz_sync
    d32 = _filled(hip, w * h * 12, 0)
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    r.antialias_device(None, d32, None, None)
    with pytest.raises(RayZenError) as e:
        r.sync()
    assert e.value.code == -9
    r.sync()
    assert hip.download(d32, w * h * 12).tobytes() == before[0].tobytes()
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# the C++ front end: presentDisplay(..., &antialias) against the Python binding

def test_cpp_present_display_antialiased_equals_python(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    header = os.path.join(ROOT, "rayzen_amd", "csrc", "host")
    exe = str(tmp_path / "antialias_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", header,
                           os.path.join(ROOT, "tests", "cpp", "antialias_driver.cpp"), "-L", lib, "-lrayzen_host", "-lrayzen_hip",
                           f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"antialias_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    fp = _lib.FrameParams.from_buffer_copy(raw("fp"))
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt).copy())
    r.set_frame(fp)
    r.render()
    kw = dict(fps=0.0, show_fps=False)
    plain = r.present_display("accum", **kw)[1].tobytes()
    aa2 = r.present_antialiased("accum", factor=2, sigma_normal=128.0, sigma_plane=1.0, demodulate=True, edge_normal=0.9,
                                edge_plane=1.0, **kw)[1].tobytes()
    aa3 = r.present_antialiased("denoise", factor=3, sigma_normal=64.0, sigma_plane=0.5, demodulate=False, edge_normal=0.95,
                                edge_plane=0.5, filter=dict(iterations=2), exposure=1.5, curve="aces", transfer="srgb", **kw)[1].tobytes()
    edge = r.antialias(edges=True)[1]
    r.close()
    assert 0.02 < edge.mean() < 0.5                      # the driver's camera does see silhouettes
    assert raw("plain") == plain and raw("aa2") == aa2 and raw("aa3") == aa3 and raw("aa1") == plain
    assert aa2 != plain


# ---------------------------------------------------------------------------------------------------------------------
# cost

def test_costs_less_than_the_upsampler_that_casts_every_sub_ray():
    """rz_antialias at factor 2 against rz_upscale at factor 2 from the same 1920 x 1080 frame of bunny_scene, in one process,
    device events, medians of 25.  rz_upscale casts all four sub-rays of every pixel (and the frame-size guide); rz_antialias
    casts the frame-size guide and four sub-rays on the edge pixels only.  No margin: measured in profiles/antialias/README.md.
    At this size a wave works through several units, so its queue carries pixels from one unit to the next: the mask and the
    colours are held to the restatement and to rz_upscale's own output here too."""
    hip = Hip()
    W, H, s = 1920, 1080, 2
    sc = S.bunny_scene(aspect=W / H)
    r = _setup(sc, W, H)
    c = DR.resolve(r.read_accum())
    got, g, edge = r.antialias(factor=s, guides=True, edges=True)
    assert np.array_equal(edge, AR.edge_mask(c, g, sc.materials, sc.camera.inv_proj)) and 1e-3 < edge.mean() < 0.15
    print(f"edge share {edge.mean():.4f}")
    mean32 = AR.box_mean32(r.upscale(factor=s), s)
    assert got[~edge].tobytes() == c[~edge].tobytes() and got[edge].tobytes() == mean32[edge].tobytes()
    del mean32
    d_aa, d_up = hip.alloc(W * H * 12), hip.alloc(W * H * s * s * 12)
    stream = hip.stream()
    r.set_stream(stream)
    t_up = _median_ms(hip, r, stream, lambda: r.upscale_device(None, d_up, None, factor=s))
    t_aa = _median_ms(hip, r, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s))
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()
    print(f"1920x1080 bunny_scene, factor 2: rz_antialias {t_aa:.3f} ms, rz_upscale {t_up:.3f} ms, ratio {t_up / t_aa:.2f}")
    assert t_aa < t_up, (t_aa, t_up)

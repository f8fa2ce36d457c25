"""Guided upsampling (rz_upscale, rz_present_upscaled; rz_upscale.hip) on the GPU: the high-size guide against rz_trace_rays on the
pixel-centre rays, bit for bit; the colours against the float64 restatement (upscale_ref.py) given the GPU's own guides;
non-finite input, factor 1, rz_present_upscaled against rz_present_display and rz_present, host and device paths, isolation from
the render, temporal and display state, errors, and the cost next to one a-trous pass."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as DR
import upscale_ref as UR
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, Renderer, frame_params
from test_denoise_gpu import _assert_same_hits, _setup, _trace_pixels
from test_display_gpu import _key
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

F32 = np.float32


def sliver_scene():
    """cornell_scene without its back wall, plus a post 0.04 wide in front of the sky: at 33 x 17 it is thinner than a low
    pixel (0.106 at its distance) and wider than a high pixel of s = 4 (0.027), and no low pixel centre lands on it."""
    s = S.Scene(camera=S.Camera(position=(0.0, 0.5, 4.5), aspect=1.0))
    floor = s.add_mesh(S.make_quad((-4, -1.5, 4), (4, -1.5, 4), (4, -1.5, -4), (-4, -1.5, -4), 4))
    cube = s.add_mesh(S.make_cube(0))
    post = s.add_mesh(S.make_quad((0.03, -1.5, 2.0), (0.07, -1.5, 2.0), (0.07, 4.5, 2.0), (0.03, 4.5, 2.0), 1))
    s.add_object(floor)
    s.add_object(cube, S.rotate(S.translate(S.identity(), (0.3, -0.5, 0.0)), 0.6, (0.0, 1.0, 0.0)))
    s.add_object(post)
    s.name = "sliver"
    return s.build()


SCENES = {"cornell": S.cornell_scene, "glass": lambda: S.reference_scene(aspect=4 / 3), "sliver": sliver_scene}
CASES = [(1, 1, 4), (3, 2, 3), (65, 5, 2), (33, 17, 4)]        # w, h, s


def _filled(hip, nbytes, fill):
    """Device memory set to a byte value, with the fill DONE.  Hip.alloc fills with hipMemset on the NULL stream, which returns
    before the device has written; a context's own stream is non-blocking, so it is not ordered behind the NULL stream, and a
    call that writes the buffer from its first operation (a guide cast's hit records, the factor-1 copy) could be overtaken by the
    fill and read back as the fill value.  Waiting here orders the fill before everything the test enqueues afterwards."""
    p = hip.alloc(nbytes, fill=fill)
    hip.ok(hip.L.hipDeviceSynchronize())
    return p


def _low_guides(r):
    """The guide at the frame's own size: rz_denoise's, which is what the upscaler casts at w x h."""
    return r.denoise(iterations=0, guides=True)[1]


def _window_max(c, s):
    """m per high pixel: the largest finite |c| among its 4 x 4 low window (the part inside the image)."""
    h, w = c.shape[:2]
    a = np.where(DR.bad_pixels(c), 0.0, np.abs(c.astype(np.float64)).max(-1))
    i0, _ = UR.footprint(np.arange(w * s), s)
    j0, _ = UR.footprint(np.arange(h * s), s)
    m = np.zeros((h * s, w * s))
    for b in range(-1, 3):
        for k in range(-1, 3):
            m = np.maximum(m, a[np.ix_(np.clip(j0 + b, 0, h - 1), np.clip(i0 + k, 0, w - 1))])
    return m[..., None]


# Tolerance (test_denoise_gpu.py's): |gpu - ref| <= 1e-4 (|ref| + m) + 1e-7, m the largest |c| of the pixel's 4 x 4 low window.
# The kernel evaluates the weights in binary32: max(0, n.n)^128 carries ~128 ulp (1e-5) and exp of an argument of at most 9.2 (a
# larger one is under the floor) a few ulp, so the weighted mean is good to ~1e-5 of the spread of what it averages.  No pixel is
# exempt: which stage a pixel takes depends on integers, hit flags and bit patterns only.
def _assert_close(got, want, c, s, what=""):
    m = _window_max(c, s)
    err = np.abs(got.astype(np.float64) - want)
    scale = np.abs(want) + m
    worst = float((err / (scale + 1e-30)).max())
    print(f"{what}: worst relative error {worst:.3g}")
    ok = err <= 1e-4 * scale + 1e-7
    assert ok.all(), f"{what}: {int((~ok).any(-1).sum())} pixels off; worst relative {worst:.3g}"


# ---------------------------------------------------------------------------------------------------------------------
# the guide

@pytest.mark.parametrize("name,w,h,s", [("glass", 100, 75, 2), ("cornell", 33, 17, 4), ("sliver", 65, 5, 3)])
def test_guides_equal_trace_rays(name, w, h, s):
    sc = SCENES[name]()
    r = _setup(sc, w, h, render=False)
    rgb, g = r.upscale(factor=s, guides=True)
    assert g.shape == (h * s, w * s) and rgb.shape == (h * s, w * s, 3)
    _assert_same_hits(g, _trace_pixels(r, sc.camera, w * s, h * s), name)
    assert (g["instance"] >= 0).any()
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# the colours against the restatement, which is given the GPU's own guides

@pytest.mark.parametrize("w,h,s", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_colours_match_restatement(name, w, h, s):
    sc = SCENES[name]()
    r = _setup(sc, w, h, spp=2)
    g_lo = _low_guides(r)
    c_acc = DR.resolve(r.read_accum())
    rng = np.random.default_rng(w * 100 + h)
    c_syn = (np.exp(rng.normal(-1.0, 1.5, (h, w, 1))) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(F32)
    stages = set()
    for demod in (True, False):
        got, g_hi = r.upscale(factor=s, demodulate=demod, guides=True)                 # rgb_in NULL: the accumulation
        want, stage = UR.upscale(c_acc, g_lo, g_hi, sc.materials, sc.camera.inv_proj, factor=s, demodulate=demod, want_stage=True)
        stages |= set(np.unique(stage))
        _assert_close(got, want, c_acc, s, f"{name} {w}x{h} s={s} demodulate={demod} accumulation")
        assert r.upscale(c_acc, factor=s, demodulate=demod).tobytes() == got.tobytes()  # ... and the same colour handed over
        got = r.upscale(c_syn, factor=s, demodulate=demod, sigma_normal=16.0, sigma_plane=0.5)
        want = UR.upscale(c_syn, g_lo, g_hi, sc.materials, sc.camera.inv_proj, factor=s, demodulate=demod, sigma_normal=16.0,
                          sigma_plane=0.5)
        _assert_close(got, want, c_syn, s, f"{name} {w}x{h} s={s} demodulate={demod} rgb_in")
        assert np.isfinite(got).all()
    r.close()
    if name == "sliver" and (w, h, s) == (33, 17, 4):
        assert stages == {1, 2, 3}                      # the post: no low tap hits it


# ---------------------------------------------------------------------------------------------------------------------
# non-finite input at 65 x 5: the patterns of test_nonfinite_gpu.py's kind, sized for five rows

def _bad_patterns(g, rng):
    h, w = g.shape
    iso = np.zeros((h, w), bool)
    iso[2, int(rng.integers(8, w - 8))] = True
    corners = np.zeros((h, w), bool)
    corners[0, 0] = corners[-1, -1] = True
    block = np.zeros((h, w), bool)
    x = int(rng.integers(4, w - 10))
    block[:, x:x + 5] = True                            # 5 x 5: the whole height
    row = np.zeros((h, w), bool)
    row[int(rng.integers(1, h - 1))] = True
    hit = g["instance"] >= 0
    edge = np.zeros((h, w), bool)
    ys, xs = np.nonzero(hit[:, :-1] != hit[:, 1:])
    for k in range(min(4, len(ys))):
        edge[ys[k], xs[k]] = edge[ys[k], xs[k] + 1] = True
    return {"isolated": iso, "corners": corners, "block": block, "row": row, "edge": edge, "sprinkle": rng.random((h, w)) < 0.05,
            "all": np.ones((h, w), bool)}


def test_bad_low_pixels_are_contained():
    w, h, s = 65, 5, 2
    sc = S.cornell_scene()
    r = _setup(sc, w, h, render=False)
    rgb0, g_hi = r.upscale(np.zeros((h, w, 3), F32), guides=True)
    g_lo = _low_guides(r)
    rng = np.random.default_rng(21)
    clean = rng.uniform(0.1, 2.0, (h, w, 3)).astype(F32)
    vals = [np.nan, np.inf, -np.inf]
    for pname, mask in _bad_patterns(g_lo, rng).items():
        c = clean.copy()
        for y, x in zip(*np.nonzero(mask)):             # NaN, +Inf and -Inf in turn, in one channel or in all three
            v = vals[int(rng.integers(3))]
            if rng.random() < 0.5:
                c[y, x] = v
            else:
                c[y, x, int(rng.integers(3))] = v
        assert np.array_equal(DR.bad_pixels(c), mask), pname
        for demod in (True, False):
            got = r.upscale(c, demodulate=demod)
            want, stage = UR.upscale(c, g_lo, g_hi, sc.materials, sc.camera.inv_proj, demodulate=demod, want_stage=True)
            assert np.isfinite(got).all(), f"{pname}: {int((~np.isfinite(got)).any(-1).sum())} pixels not finite"
            _assert_close(got, want, c, s, f"{pname} demodulate={demod}")
            zero = (stage == 3) & np.repeat(np.repeat(mask, s, 0), s, 1)       # stage 3 on a bad pixel: exactly 0
            assert not got[zero].view(np.uint32).any()
            if pname == "all":
                assert zero.all()
            # containment: where no bad pixel lies in the 4 x 4 window, the bytes are the clean frame's
            near = _window_max(np.where(mask[..., None], F32(1), F32(0)) * np.ones(3, F32), s)[..., 0] > 0
            ref_clean = r.upscale(clean, demodulate=demod)
            assert got[~near].tobytes() == ref_clean[~near].tobytes(), pname
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# factor 1, present

def test_factor_1_is_c_itself():
    sc = S.reference_scene(aspect=4 / 3)
    w, h = 65, 5
    r = _setup(sc, w, h, spp=2)
    c = DR.resolve(r.read_accum())
    out, g = r.upscale(factor=1, guides=True)
    assert out.tobytes() == c.tobytes()
    _assert_same_hits(g, _trace_pixels(r, sc.camera, w, h), "factor 1")
    x = c.copy()
    x[2, 7] = np.nan
    x[0, 0, 1] = -np.inf
    assert r.upscale(x, factor=1).tobytes() == x.tobytes()              # bad or not
    r.close()


@pytest.mark.parametrize("overlays", [False, True])
@pytest.mark.parametrize("source", ["accum", "denoise", "temporal"])
def test_present_upscaled_factor_1_equals_present_display(source, overlays):
    sc = S.reference_scene(aspect=4 / 3)
    w, h = 100, 75
    kw = dict(fps=57.3, show_fps=overlays, show_lights=overlays, show_bvh=overlays)
    filt = None if source == "accum" else dict(iterations=2)
    outs = []
    for upscaled in (False, True):
        r = _setup(sc, w, h, spp=2)                     # (a context each: source "temporal" advances the history)
        for disp in (dict(), dict(auto=True, curve="aces", transfer="srgb")):
            if upscaled:
                outs.append(r.present_upscaled(source, factor=1, filter=filt, **kw, **disp))
            else:
                outs.append(r.present_display(source, filter=filt, **kw, **disp))
        r.close()
    for a, b in zip(outs[:2], outs[2:]):
        assert a[0].shape == (h, w, 3) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_present_upscaled_equals_present_of_the_upscaled_colour():
    hip = Hip()
    sc = S.reference_scene(aspect=4 / 3)
    w, h, s = 100, 75, 2
    W, H = w * s, h * s
    kw = dict(fps=12.5, show_fps=True, show_lights=True, show_bvh=True)
    r = _setup(sc, w, h, spp=2)
    up = r.upscale(factor=s)
    rgb, rgba8 = r.present_upscaled("accum", factor=s, **kw)
    assert rgb.shape == (H, W, 3) and rgba8.shape == (H, W, 4)
    # sources 1 and 2: the denoisers run at the low size, then the same upscale
    for source, den in (("denoise", r.denoise(iterations=2)), ("temporal", r.denoise_temporal(iterations=2, keep=True))):
        a = r.present_upscaled(source, factor=s, filter=dict(iterations=2), show_fps=False)
        want = np.clip(r.upscale(den, factor=s), 0.0, 1.0)
        assert a[0].tobytes() == want.tobytes(), source
    # ... and it commits its exposure to the display state as rz_present_display does, metered from the W x H colour
    r.display_reset()
    shown = r.present_upscaled("accum", factor=s, auto=True, adapt=0.5, curve="aces", transfer="srgb", **kw)
    state = r.display_state()
    r.close()
    # rz_present on a context whose frame is W x H and whose accumulation is (upscaled, 1)
    buf = np.concatenate([up, np.ones((H, W, 1), F32)], -1)
    dbuf = hip.upload(buf)
    hip.ok(hip.L.hipDeviceSynchronize())
    r2 = Renderer(0)
    r2.upload_scene(sc)
    r2.bind_accum(dbuf, buf.nbytes)
    r2.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 5, 1, 0))
    rgb2, rgba82 = r2.present(**kw)
    plain = r2.present(show_fps=False)
    shown2 = r2.present_display("accum", auto=True, adapt=0.5, curve="aces", transfer="srgb", **kw)
    state2 = r2.display_state()
    r2.close()
    hip.close()
    assert rgba8.tobytes() == rgba82.tobytes() and rgb.tobytes() == rgb2.tobytes()
    assert rgba8.tobytes() != plain[1].tobytes()        # the overlays are there, at the high size
    assert state["counted"] == W * H - state["below"] - state["above"] and state["exposure"] != 1.0
    assert _key(state) == _key(state2)
    assert shown[0].tobytes() == shown2[0].tobytes() and shown[1].tobytes() == shown2[1].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# paths, streams, state

def test_host_and_device_paths_agree_and_null_outputs():
    hip = Hip()
    sc = S.reference_scene(aspect=4 / 3)
    w, h, s = 65, 5, 3
    n, N = w * h, w * h * s * s
    r = _setup(sc, w, h, spp=2)
    rgb, g = r.upscale(factor=s, guides=True)
    d32, dg = _filled(hip, N * 12, 0x5A), _filled(hip, N * 48, 0x5A)
    r.upscale_device(None, d32, dg, factor=s)
    r.sync()
    assert hip.download(d32, N * 12).tobytes() == rgb.tobytes()
    assert hip.download(dg, N * 48).tobytes() == g.tobytes()
    # the input from device memory
    c = DR.resolve(r.read_accum())
    din = hip.upload(c)
    d32b = _filled(hip, N * 12, 0)
    r.upscale_device(din, d32b, None, factor=s)
    r.sync()
    assert hip.download(d32b, N * 12).tobytes() == rgb.tobytes()
    # factor 1 on the device: in place is allowed, and a copy otherwise
    d1 = _filled(hip, n * 12, 0)
    r.upscale_device(din, d1, None, factor=1)
    r.upscale_device(din, din, None, factor=1)
    r.sync()
    assert hip.download(d1, n * 12).tobytes() == c.tobytes() == hip.download(din, n * 12).tobytes()
    # NULL outputs: each alone, and none
    p32, pg = _filled(hip, N * 12, 0), _filled(hip, N * 48, 0)
    r.upscale_device(None, None, pg, factor=s)
    r.sync()
    assert not hip.download(p32, N * 12).any() and hip.download(pg, N * 48).tobytes() == g.tobytes()
    r.upscale_device(None, p32, None, factor=s)
    r.upscale_device(None, None, None, factor=s)
    r.sync()
    assert hip.download(p32, N * 12).tobytes() == rgb.tobytes()
    r.close()
    hip.close()


def test_on_a_user_stream_after_update_transforms():
    hip = Hip()
    sc = S.instanced_scene(n=24, count=16, aspect=16 / 9)
    w, h, s = 96, 54, 2
    W, H = w * s, h * s
    r = _setup(sc, w, h)
    _, before = r.upscale(guides=True)
    stream = hip.stream()
    r.set_stream(stream)
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(t, F32).reshape(16) for t in S.instanced_transforms(11, 16)])
    r.update_transforms(xf)
    d32, dg = hip.alloc(W * H * 12), hip.alloc(W * H * 48)
    r.upscale_device(None, d32, dg)
    r.sync()
    got = hip.download(dg, W * H * 48).view(HIT_DTYPE).reshape(H, W)
    rgb = hip.download(d32, W * H * 12).view(F32).reshape(H, W, 3)
    tr = _trace_pixels(r, sc.camera, W, H)
    g_lo = _low_guides(r)
    c = DR.resolve(r.read_accum())
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()
    _assert_same_hits(got, tr, "after update_transforms")
    assert (got["t"] != before["t"]).any()
    _assert_close(rgb, UR.upscale(c, g_lo, got, sc.materials, sc.camera.inv_proj), c, s, "on a user stream")


def test_leaves_render_temporal_and_display_state_alone():
    sc = S.bunny_scene(n=24, aspect=16 / 9, bunny_material=3)           # glass: currentIor is live state
    w, h = 96, 54

    def run(with_upscale):
        r = _setup(sc, w, h, spp=4, bounces=4)
        r.denoise_temporal()                            # a history and a display state to leave alone
        r.display(auto=True, adapt=0.5)
        plan = r.debug_last_plan()
        acc0 = r.read_accum()
        tmp = [r.debug_read_temporal(k).tobytes() for k in range(5)]
        disp = _key(r.display_state())
        if with_upscale:
            r.upscale(guides=True)
            r.upscale(r.denoise(iterations=1), factor=3)
            assert _key(r.display_state()) == disp
            r.present_upscaled("accum")
            r.present_upscaled("denoise", factor=3, filter=dict(iterations=1))
            assert r.debug_last_plan() == plan
            assert r.read_accum().tobytes() == acc0.tobytes()
            assert [r.debug_read_temporal(k).tobytes() for k in range(5)] == tmp        # sources 0 and 1
        r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), 4, 4, 4))
        r.render()
        acc = r.read_accum()
        r.close()
        return acc0, acc

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_present_upscaled_source_2_advances_the_history_as_present_temporal_does():
    sc = S.reference_scene(aspect=4 / 3)
    w, h = 64, 48
    hist = []
    for upscaled in (False, True):
        r = _setup(sc, w, h)
        for _ in range(2):
            if upscaled:
                r.present_upscaled("temporal", factor=2)
            else:
                r.present_temporal()
        hist.append([r.debug_read_temporal(k).tobytes() for k in range(5)])
        r.close()
    assert hist[0] == hist[1]


# ---------------------------------------------------------------------------------------------------------------------
# errors

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h, s = 16, 8, 2
    n, N = w * h, w * h * s * s
    r = _setup(sc, w, h)
    pin = hip.upload(DR.resolve(r.read_accum()))
    p32, pg = _filled(hip, N * 12 + 16, 0x5A), _filled(hip, N * 48 + 16, 0x5A)

    def call(ctx, params=None, args=(None, 0, p32, N * 12, pg, N * 48), flags=0):
        a = list(args)
        return L.rz_upscale(ctx, params, C.c_void_p(a[0]), a[1], C.c_void_p(a[2]), a[3], C.c_void_p(a[4]), a[5], flags)

    def params(**kw):
        p = _lib.UpscaleParams(2, 128.0, 1.0, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    nan, inf = float("nan"), float("inf")
    assert call(None) == -1
    for bad in (dict(factor=0), dict(factor=5), dict(factor=-2), dict(sigma_plane=0.0), dict(sigma_plane=-1.0), dict(sigma_plane=inf),
                dict(sigma_normal=-1.0), dict(sigma_normal=nan), dict(sigma_normal=inf), dict(sigma_plane=nan), dict(demodulate=2)):
        assert call(r._c, params(**bad)) == -1, bad
    for k in range(4):
        p = _lib.UpscaleParams(2, 128.0, 1.0, 1)
        p.reserved[k] = 7
        assert call(r._c, C.byref(p)) == -1
    assert call(r._c, flags=0x4) == -1 and call(r._c, flags=0x2) == -1
    assert call(r._c, args=(pin + 2, n * 12, p32, N * 12, pg, N * 48)) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert call(r._c, args=(None, 0, p32 + 2, N * 12, pg, N * 48)) == -1
    assert call(r._c, args=(None, 0, p32, N * 12, pg + 4, N * 48)) == -1
    assert call(r._c, args=(pin, n * 12 - 1, p32, N * 12, pg, N * 48)) == -7
    assert call(r._c, args=(None, 0, p32, N * 12 - 1, pg, N * 48)) == -7
    assert call(r._c, args=(None, 0, p32, N * 12, pg, N * 48 - 1)) == -7
    assert call(r._c, params(factor=3)) == -7                           # the outputs are sized for s = 2
    pp = _lib.PresentParams()
    buf8 = np.zeros(N * 4, np.uint8)
    buf32 = np.zeros(N * 3, F32)

    def present(ctx, present_p=C.byref(pp), up=None, disp=None, source=0, filt=None, n8=buf8.nbytes, n32=buf32.nbytes):
        return L.rz_present_upscaled(ctx, present_p, up, disp, source, filt, buf8.ctypes.data, n8, buf32.ctypes.data, n32)

    assert present(None) == -1 and present(r._c, present_p=None) == -1
    assert present(r._c, up=params(factor=5)) == -1 and present(r._c, up=params(factor=0)) == -1
    assert present(r._c, source=3) == -1 and present(r._c, source=-1) == -1
    assert present(r._c, source=0, filt=params()) == -1                 # filter_params with source 0
    dn = _lib.DenoiseParams(12, 0.5, 128.0, 1.0, 1)
    assert present(r._c, source=1, filt=C.byref(dn)) == -1
    dd = _lib.DisplayParams(0, 1.0, 0.18, 1 / 64, 64.0, 1.0, 0, 0, 7, 4.0, 0)
    assert present(r._c, disp=C.byref(dd)) == -1
    assert present(r._c, n8=N * 4 - 1) == -7 and present(r._c, n32=N * 12 - 1) == -7
    assert not buf8.any() and not buf32.any()
    r.sync()
    for ptr, nb in ((p32, N * 12 + 16), (pg, N * 48 + 16)):
        assert (hip.download(ptr, nb) == 0x5A).all()            # nothing was launched
    # the context stays usable
    assert call(r._c) == 0 and present(r._c) == 0
    r.sync()
    assert buf8.any()
    # a tile of a group frame: refused
    r.set_frame(frame_params(sc.camera, w, h, 2, 5, 1, 0, 0, 2))
    assert call(r._c) == -1 and b"whole frame" in L.rz_last_error(r._c)
    assert present(r._c) == -1
    r.close()
    # out of host memory inside the call: the first call of a context derives the scene layout
    fresh = Renderer(0)
    fresh.upload_scene(sc)
    fresh.set_frame(frame_params(sc.camera, w, h, 2, 5, 1, 0))
    fresh.debug_fail_alloc(1)
    assert call(fresh._c) == -8
    fresh.debug_fail_alloc(0)
    assert call(fresh._c) == 0
    fresh.sync()
    out = fresh.upscale(guides=True)[1]
    assert hip.download(pg, N * 48).tobytes() == out.tobytes()
    fresh.close()
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


# ---------------------------------------------------------------------------------------------------------------------
# speed

def _median_ms(hip, r, stream, fn, runs=25):
    a, b = hip.event(), hip.event()
    fn()
    r.sync()
    out = []
    for _ in range(runs):
        hip.ok(hip.L.hipEventRecord(a, stream))
        fn()
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        out.append(ms.value)
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    return float(np.median(out))


def test_costs_no_more_than_one_atrous_pass():
    """rz_upscale 960 x 540 -> 1920 x 1080 against rz_denoise with K = 1 at 1920 x 1080, in one process, device events, medians
    of 25.  The bound is 1.25: the upscaler casts 1.25 times the guide rays (full plus quarter size) and gathers at most 16 taps
    where the a-trous pass gathers 25.  Measured: profiles/upscale/README.md."""
    hip = Hip()
    W, H, s = 1920, 1080, 2
    sc = S.reference_scene(aspect=W / H)
    times = {}
    for what in ("upscale", "denoise"):
        r = _setup(sc, W // s, H // s) if what == "upscale" else _setup(sc, W, H)
        d32 = hip.alloc(W * H * 12)
        stream = hip.stream()
        r.set_stream(stream)
        if what == "upscale":
            times[what] = _median_ms(hip, r, stream, lambda: r.upscale_device(None, d32, None, factor=s))
        else:
            times[what] = _median_ms(hip, r, stream, lambda: r.denoise_device(d32, iterations=1))
        r.set_stream(0)
        r.close()
        hip.L.hipStreamDestroy(stream)
    hip.close()
    ratio = times["upscale"] / times["denoise"]
    print(f"rz_upscale 960x540 -> 1920x1080: {times['upscale']:.3f} ms; rz_denoise K=1 at 1920x1080: {times['denoise']:.3f} ms; "
          f"ratio {ratio:.3f}")
    assert ratio <= 1.25, times

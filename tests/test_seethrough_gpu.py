"""See-through guides for the upsampler (rz_upscale_seethrough, rz_present_upscaled_seethrough; rz_seethrough.hip) on the GPU: the
guides and chains against the binary32 restatement (seethrough_ref.py) around the device's own query, bit for bit; the colours
against the float64 restatement given the GPU's own records; the anchors at which the calls must return their first-hit twins'
bytes; present, non-finite input, errors, isolation, and the C++ front end against the Python binding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as DR
import seethrough_ref as SR
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import CHAIN_DTYPE, Renderer, frame_params
from test_denoise_gpu import _assert_same_hits, _setup
from test_display_gpu import _key
from test_rays_gpu import Hip
from test_upscale_gpu import _assert_close, _filled, _window_max

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERA = (3.0, 0.8, 7.0)


def glass_scene(W, H, extras=True):
    """408 triangles: the floor, the blob, a glass blob (material 3) and a mirror cube (material 2), seen from the glass's side."""
    return S.bunny_scene(n=4, aspect=W / H, extras=extras, camera_position=CAMERA)


# w, h, s: the high sizes 48 x 36 (by every factor) and 66 x 10, and the low frames 1 x 1, 3 x 2 and 65 x 5
CASES = [(24, 18, 2), (16, 12, 3), (12, 9, 4), (33, 5, 2), (1, 1, 4), (3, 2, 3), (65, 5, 2)]

_REF = {}           # (W, H, max_depth) -> the restatement's chain around the device's query; computed once, never changed


def _ref_chain(W, H, md):
    key = (W, H, md)
    if key not in _REF:
        sc = glass_scene(W, H)
        r = _setup(sc, W, H, render=False)
        g, T, k, first = SR.pixel_chain(sc.camera, W, H, sc.materials, lambda o, d: r.trace_rays(o, d), md)
        r.close()
        for a in (g, T, k, first):
            a.setflags(write=False)
        _REF[key] = (g, T, k, first)
    return _REF[key]


def _cls(ch):
    return SR.split_records(ch)[3]


def _specular(materials, m):
    tr, rf = materials["transparency"][m], materials["reflectivity"][m]
    return (tr > 0) | (rf >= 1)


# ---------------------------------------------------------------------------------------------------------------------
# 0 the preconditions: the camera does look through the glass and into the mirror

def test_the_scene_has_the_chains_the_tests_rely_on():
    sc = glass_scene(48, 36)
    g, T, k, first = _ref_chain(48, 36, 8)
    hit = g["instance"] >= 0
    print("48 x 36: chain pixels %.3f; hit ends by k %s; miss ends by k %s" %
          ((k > 0).mean(), sorted(set(k[hit & (k > 0)])), sorted(set(k[~hit & (k > 0)]))))
    assert (k > 0).mean() >= 0.10
    assert (hit & (k > 0)).any() and (~hit & (k > 0)).any() and (k >= 5).any()
    g1, _, k1, _ = _ref_chain(48, 36, 1)
    h1 = g1["instance"] >= 0
    exhausted = h1 & (k1 == 1) & _specular(sc.materials, np.clip(g1["material"], 0, len(sc.materials) - 1))
    print("48 x 36, max_depth 1: %d chains exhausted on a specular surface" % exhausted.sum())
    assert exhausted.sum() >= 100
    k2 = _ref_chain(66, 10, 8)[2]
    print("66 x 10: chain pixels %.3f" % (k2 > 0).mean())
    assert (k2 > 0).mean() >= 0.03


# ---------------------------------------------------------------------------------------------------------------------
# 1 guides and chains, bit for bit

@pytest.mark.parametrize("md", [1, 2, 8])
@pytest.mark.parametrize("w,h,s", [(24, 18, 2), (33, 5, 2)], ids=lambda v: str(v))
def test_guides_and_chains_equal_the_restatement(w, h, s, md):
    W, H = w * s, h * s
    g_ref, T, k, first = _ref_chain(W, H, md)
    want = SR.chain_records(T, k, first)
    hip = Hip()
    r = _setup(glass_scene(W, H), w, h, render=False)
    rgb, g, ch = r.upscale(np.zeros((h, w, 3), F32), factor=s, see_through=md, guides=True, chains=True)
    assert g.shape == (H, W) and ch.shape == (H, W) and ch.dtype == CHAIN_DTYPE
    _assert_same_hits(g, g_ref.reshape(-1), f"{W}x{H} max_depth {md}")
    assert ch.tobytes() == want.tobytes(), f"{int((ch['word'] != want['word']).sum())} chain words differ"
    # the device path
    N = W * H
    dg, dc, d32 = _filled(hip, N * 48, 0x5A), _filled(hip, N * 16, 0x5A), _filled(hip, N * 12, 0x5A)
    din = hip.upload(np.zeros((h, w, 3), F32))
    r.upscale_device(din, d32, dg, factor=s, see_through=md, chains_ptr=dc)
    r.sync()
    assert hip.download(dg, N * 48).tobytes() == g.tobytes() and hip.download(dc, N * 16).tobytes() == ch.tobytes()
    assert hip.download(d32, N * 12).tobytes() == rgb.tobytes()
    # each output alone
    pc = _filled(hip, N * 16, 0)
    r.upscale_device(None, None, None, factor=s, see_through=md, chains_ptr=pc)
    r.sync()
    assert hip.download(pc, N * 16).tobytes() == ch.tobytes()
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2 the colours against the float64 restatement, which is given the GPU's own records

@pytest.mark.parametrize("w,h,s", CASES, ids=lambda v: str(v))
def test_colours_match_restatement(w, h, s):
    sc = glass_scene(w, h)
    r = _setup(sc, w, h, spp=2)
    c_acc = DR.resolve(r.read_accum())
    rng = np.random.default_rng(w * 100 + h)
    c_syn = (np.exp(rng.normal(-1.0, 1.5, (h, w, 1))) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(F32)
    _, g_lo, ch_lo = r.upscale(factor=1, see_through=8, guides=True, chains=True)       # the records at the frame's own size
    stages = np.zeros(4, int)
    for demod in (True, False):
        got, g_hi, ch_hi = r.upscale(factor=s, demodulate=demod, see_through=8, guides=True, chains=True)
        args = (g_lo, g_hi, ch_lo["throughput"], ch_hi["throughput"], _cls(ch_lo), _cls(ch_hi), sc.materials, sc.camera.inv_proj)
        want, stage = SR.upscale(c_acc, *args, factor=s, demodulate=demod, want_stage=True)
        stages += np.bincount(stage.ravel(), minlength=4)
        _assert_close(got, want, c_acc, s, f"{w}x{h} s={s} demodulate={demod} accumulation")
        near = c_acc[np.ix_(np.arange(h * s) // s, np.arange(w * s) // s)]
        assert got[stage == 3].tobytes() == near[stage == 3].tobytes()                   # stage 3: the nearest low pixel, as it is
        assert r.upscale(c_acc, factor=s, demodulate=demod, see_through=8).tobytes() == got.tobytes()
        got = r.upscale(c_syn, factor=s, demodulate=demod, sigma_normal=16.0, sigma_plane=0.5, see_through=8)
        want = SR.upscale(c_syn, *args, factor=s, demodulate=demod, sigma_normal=16.0, sigma_plane=0.5)
        _assert_close(got, want, c_syn, s, f"{w}x{h} s={s} demodulate={demod} rgb_in")
        assert np.isfinite(got).all()
    print(f"{w}x{h} s={s}: pixels by stage {stages[1:]}; chain pixels {(_cls(ch_hi) != 0).mean():.3f}")
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3 the anchors: the first-hit twins' bytes

SOURCES = ("accum", "denoise", "temporal")


def _both(sc, w, h, s, md):
    """(rz_upscale's colour and guide, rz_upscale_seethrough's colour, guide and chains, and per source both presents)."""
    out = []
    for see in (None, md):
        r = _setup(sc, w, h, spp=2)                     # (a context each: source "temporal" advances the history)
        res = [r.upscale(factor=s, guides=True, **({} if see is None else dict(see_through=see, chains=True)))]
        for source in SOURCES:
            filt = None if source == "accum" else dict(iterations=2)
            res.append(r.present_upscaled(source, factor=s, filter=filt, fps=31.0, show_lights=True, auto=True, curve="aces",
                                          transfer="srgb", see_through=see))
        r.close()
        out.append(res)
    return out


def _assert_twins(first, see):
    assert see[0][0].tobytes() == first[0][0].tobytes() and see[0][1].tobytes() == first[0][1].tobytes()
    for a, b in zip(first[1:], see[1:]):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("w,h,s", [(24, 18, 2), (65, 5, 3)], ids=lambda v: str(v))
def test_max_depth_0_is_the_first_hit_call(w, h, s):
    first, see = _both(glass_scene(w, h), w, h, s, 0)
    _assert_twins(first, see)
    ch = see[0][2]
    assert (ch["throughput"] == 1).all() and ((ch["word"] & 0xFF) == 0).all() and (ch["word"] != 0).any()
    hit = see[0][1]["instance"] >= 0
    assert ((ch["word"] == 0) == ~hit).all()            # 0 for a primary miss, m_first + 1 << 8 for a hit


def test_a_scene_in_which_no_chain_moves_is_the_first_hit_call():
    w, h, s = 24, 18, 2
    first, see = _both(glass_scene(w, h, extras=False), w, h, s, 8)
    _assert_twins(first, see)
    assert ((see[0][2]["word"] & 0xFF) == 0).all()


@pytest.mark.parametrize("md", [0, 8])
def test_factor_1_is_c_itself(md):
    w, h = 65, 5
    sc = glass_scene(w, h)
    first, see = _both(sc, w, h, 1, md)
    assert see[0][0].tobytes() == first[0][0].tobytes()
    for a, b in zip(first[1:], see[1:]):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    r = _setup(sc, w, h, spp=2)
    c = DR.resolve(r.read_accum())
    assert see[0][0].tobytes() == c.tobytes()
    x = c.copy()
    x[2, 7] = np.nan
    x[0, 0, 1] = -np.inf
    assert r.upscale(x, factor=1, see_through=md).tobytes() == x.tobytes()
    r.close()
    if md == 8:         # ... and the guide asked for at factor 1 is the chain's
        g_ref, T, k, first_m = _ref_chain(w, h, 8)
        _assert_same_hits(see[0][1], g_ref.reshape(-1), "factor 1")
        assert see[0][2].tobytes() == SR.chain_records(T, k, first_m).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 4 present

def test_present_equals_present_of_the_clamped_see_through_colour():
    hip = Hip()
    w, h, s = 24, 18, 2
    W, H = w * s, h * s
    sc = glass_scene(w, h)
    kw = dict(fps=12.5, show_fps=True, show_lights=True, show_bvh=True)
    r = _setup(sc, w, h, spp=2)
    up = r.upscale(factor=s, see_through=8)
    assert up.tobytes() != r.upscale(factor=s).tobytes()            # the chains do change the colour here
    rgb, rgba8 = r.present_upscaled("accum", factor=s, see_through=8, **kw)
    assert rgb.shape == (H, W, 3) and rgba8.shape == (H, W, 4)
    # sources 1 and 2: the denoisers run at the low size with their first-hit guides, then the same upscale
    for source, den in (("denoise", r.denoise(iterations=2)), ("temporal", r.denoise_temporal(iterations=2, keep=True))):
        a = r.present_upscaled(source, factor=s, filter=dict(iterations=2), show_fps=False, see_through=8)
        want = np.clip(r.upscale(den, factor=s, see_through=8), 0.0, 1.0)
        assert a[0].tobytes() == want.tobytes(), source
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
    r2.close()
    hip.close()
    assert rgba8.tobytes() == rgba82.tobytes() and rgb.tobytes() == rgb2.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5 non-finite low pixels

def test_bad_low_pixels_are_contained():
    w, h, s = 65, 5, 2
    sc = glass_scene(w, h)
    r = _setup(sc, w, h, render=False)
    zero = np.zeros((h, w, 3), F32)
    _, g_hi, ch_hi = r.upscale(zero, see_through=8, guides=True, chains=True)
    _, g_lo, ch_lo = r.upscale(zero, factor=1, see_through=8, guides=True, chains=True)
    args = (g_lo, g_hi, ch_lo["throughput"], ch_hi["throughput"], _cls(ch_lo), _cls(ch_hi), sc.materials, sc.camera.inv_proj)
    assert (_cls(ch_lo) != 0).any()
    rng = np.random.default_rng(21)
    clean = rng.uniform(0.1, 2.0, (h, w, 3)).astype(F32)
    vals = [np.nan, np.inf, -np.inf]
    moved = _cls(ch_lo) != 0
    patterns = {"isolated": np.zeros((h, w), bool), "chain pixels": moved.copy(), "block": np.zeros((h, w), bool),
                "sprinkle": rng.random((h, w)) < 0.05, "all": np.ones((h, w), bool)}
    patterns["isolated"][2, 30] = patterns["isolated"][0, 0] = patterns["isolated"][-1, -1] = True
    patterns["block"][:, 20:25] = True
    for pname, mask in patterns.items():
        c = clean.copy()
        for y, x in zip(*np.nonzero(mask)):             # NaN, +Inf and -Inf in turn, in one channel or in all three
            v = vals[int(rng.integers(3))]
            if rng.random() < 0.5:
                c[y, x] = v
            else:
                c[y, x, int(rng.integers(3))] = v
        assert np.array_equal(DR.bad_pixels(c), mask), pname
        for demod in (True, False):
            got = r.upscale(c, demodulate=demod, see_through=8)
            want, stage = SR.upscale(c, *args, demodulate=demod, want_stage=True)
            assert np.isfinite(got).all(), f"{pname}: {int((~np.isfinite(got)).any(-1).sum())} pixels not finite"
            _assert_close(got, want, c, s, f"{pname} demodulate={demod}")
            dead = (stage == 3) & np.repeat(np.repeat(mask, s, 0), s, 1)       # stage 3 on a bad pixel: exactly 0
            assert not got[dead].view(np.uint32).any()
            if pname == "all":
                assert dead.all()
            near = _window_max(np.where(mask[..., None], F32(1), F32(0)) * np.ones(3, F32), s)[..., 0] > 0
            assert got[~near].tobytes() == r.upscale(clean, demodulate=demod, see_through=8)[~near].tobytes(), pname
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6 errors

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    w, h, s = 16, 8, 2
    sc = glass_scene(w, h)
    n, N = w * h, w * h * s * s
    r = _setup(sc, w, h)
    pin = hip.upload(DR.resolve(r.read_accum()))
    p32, pg, pc = _filled(hip, N * 12 + 16, 0x5A), _filled(hip, N * 48 + 16, 0x5A), _filled(hip, N * 16 + 16, 0x5A)

    def call(ctx, params=None, see=None, args=(None, 0, p32, N * 12, pg, N * 48, pc, N * 16), flags=0):
        a = list(args)
        return L.rz_upscale_seethrough(ctx, params, see, C.c_void_p(a[0]), a[1], C.c_void_p(a[2]), a[3], C.c_void_p(a[4]), a[5],
                                       C.c_void_p(a[6]), a[7], flags)

    def params(**kw):
        p = _lib.UpscaleParams(2, 128.0, 1.0, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def see(max_depth=8, word=None):
        p = _lib.SeethroughParams(max_depth)
        if word is not None:
            p.reserved[word] = 1
        return C.byref(p)

    nan, inf = float("nan"), float("inf")
    assert call(None) == -1
    for md in (-1, 9, 1 << 20, -(1 << 31)):
        assert call(r._c, see=see(md)) == -1 and b"max_depth" in L.rz_last_error(r._c), md
    for k in range(7):
        assert call(r._c, see=see(word=k)) == -1, k
    for bad in (dict(factor=0), dict(factor=5), dict(factor=-2), dict(sigma_plane=0.0), dict(sigma_plane=-1.0), dict(sigma_plane=inf),
                dict(sigma_normal=-1.0), dict(sigma_normal=nan), dict(sigma_normal=inf), dict(sigma_plane=nan), dict(demodulate=2)):
        assert call(r._c, params(**bad)) == -1, bad
    for k in range(4):
        p = _lib.UpscaleParams(2, 128.0, 1.0, 1)
        p.reserved[k] = 7
        assert call(r._c, C.byref(p)) == -1
    assert call(r._c, flags=0x4) == -1 and call(r._c, flags=0x2) == -1
    full = (None, 0, p32, N * 12, pg, N * 48, pc, N * 16)

    def with_(i, v):
        a = list(full)
        a[i] = v
        return tuple(a)

    assert call(r._c, args=(pin + 2, n * 12) + full[2:]) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert call(r._c, args=with_(2, p32 + 2)) == -1 and call(r._c, args=with_(4, pg + 4)) == -1 and call(r._c, args=with_(6, pc + 8)) == -1
    assert call(r._c, args=(pin, n * 12 - 1) + full[2:]) == -7
    assert call(r._c, args=with_(3, N * 12 - 1)) == -7 and call(r._c, args=with_(5, N * 48 - 1)) == -7
    assert call(r._c, args=with_(7, N * 16 - 1)) == -7 and b"chains" in L.rz_last_error(r._c)
    assert call(r._c, params(factor=3)) == -7                           # the outputs are sized for s = 2
    pp = _lib.PresentParams()
    buf8 = np.zeros(N * 4, np.uint8)
    buf32 = np.zeros(N * 3, F32)

    def present(ctx, present_p=C.byref(pp), up=None, st=None, disp=None, source=0, filt=None, n8=buf8.nbytes, n32=buf32.nbytes):
        return L.rz_present_upscaled_seethrough(ctx, present_p, up, st, disp, source, filt, buf8.ctypes.data, n8, buf32.ctypes.data, n32)

    assert present(None) == -1 and present(r._c, present_p=None) == -1
    assert present(r._c, st=see(9)) == -1 and present(r._c, st=see(-1)) == -1 and present(r._c, st=see(word=6)) == -1
    assert present(r._c, up=params(factor=1), st=see(9)) == -1          # ... at factor 1 too
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
    for ptr, nb in ((p32, N * 12 + 16), (pg, N * 48 + 16), (pc, N * 16 + 16)):
        assert (hip.download(ptr, nb) == 0x5A).all()            # nothing was launched
    # the context stays usable
    assert call(r._c) == 0 and present(r._c) == 0
    r.sync()
    assert buf8.any() and (hip.download(pc, N * 16) != 0x5A).any()
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
    # the binding's own checks
    r = _setup(sc, w, h, render=False)
    with pytest.raises(ValueError):
        r.upscale(chains=True)
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7 isolation

def test_leaves_render_temporal_and_display_state_and_the_first_hit_path_alone():
    w, h = 48, 36
    sc = glass_scene(w, h)                              # glass in view: currentIor is live state

    def run(with_calls):
        r = _setup(sc, w, h, spp=4, bounces=4)
        r.denoise_temporal()                            # a history and a display state to leave alone
        r.display(auto=True, adapt=0.5)
        plan = r.debug_last_plan()
        acc0 = r.read_accum()
        tmp = [r.debug_read_temporal(k).tobytes() for k in range(5)]
        disp = _key(r.display_state())
        first = [x.tobytes() for x in r.upscale(guides=True)]
        first3 = r.upscale(r.denoise(iterations=1), factor=3).tobytes()
        if with_calls:
            r.upscale(see_through=8, guides=True, chains=True)
            r.upscale(r.denoise(iterations=1), factor=3, see_through=2)
            assert _key(r.display_state()) == disp
            assert r.debug_last_plan() == plan
            assert r.read_accum().tobytes() == acc0.tobytes()
            assert [r.debug_read_temporal(k).tobytes() for k in range(5)] == tmp
            # a first-hit call after see-through calls returns its earlier bytes
            assert [x.tobytes() for x in r.upscale(guides=True)] == first
            assert r.upscale(r.denoise(iterations=1), factor=3).tobytes() == first3
            r.present_upscaled("accum", see_through=8)
            r.present_upscaled("denoise", factor=3, filter=dict(iterations=1), see_through=8)
            assert r.debug_last_plan() == plan
            assert r.read_accum().tobytes() == acc0.tobytes()
            assert [r.debug_read_temporal(k).tobytes() for k in range(5)] == tmp        # sources 0 and 1
            assert [x.tobytes() for x in r.upscale(guides=True)] == first
        else:           # what the first-hit twins touch: the display state commits an exposure
            r.present_upscaled("accum")
            r.present_upscaled("denoise", factor=3, filter=dict(iterations=1))
        r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), 4, 4, 4))
        r.render()
        acc = r.read_accum()
        r.close()
        return acc0.tobytes(), acc.tobytes()

    assert run(False) == run(True)


def test_present_source_2_advances_the_history_as_the_first_hit_call_does():
    w, h = 32, 24
    sc = glass_scene(w, h)
    hist = []
    for see in (None, 8):
        r = _setup(sc, w, h)
        for _ in range(2):
            r.present_upscaled("temporal", factor=2, see_through=see)
        hist.append([r.debug_read_temporal(k).tobytes() for k in range(5)])
        r.close()
    assert hist[0] == hist[1]


# ---------------------------------------------------------------------------------------------------------------------
# 8 the C++ front end: presentUpscaled(..., &seeThrough) against the Python binding

def test_cpp_present_upscaled_see_through_equals_python(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    header = os.path.join(ROOT, "rayzen_amd", "csrc", "host")
    exe = str(tmp_path / "seethrough_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", header,
                           os.path.join(ROOT, "tests", "cpp", "seethrough_driver.cpp"), "-L", lib, "-lrayzen_host", "-lrayzen_hip",
                           f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"seethrough_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    fp = _lib.FrameParams.from_buffer_copy(raw("fp"))
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt).copy())
    r.set_frame(fp)
    r.render()
    kw = dict(fps=0.0, show_fps=False)
    first = r.present_upscaled("accum", factor=3, **kw)[1].tobytes()
    see8 = r.present_upscaled("accum", factor=3, see_through=8, **kw)[1].tobytes()
    see0 = r.present_upscaled("accum", factor=3, see_through=0, **kw)[1].tobytes()
    see_null = r.present_upscaled("accum", see_through=2, **kw)[1].tobytes()
    chains = r.upscale(factor=3, see_through=8, chains=True)[1]
    r.close()
    assert ((chains["word"] & 0xFF) > 0).mean() > 0.01          # the driver's camera does see the glass and the mirror
    assert raw("first") == first and raw("see8") == see8 and raw("see0") == see0 and raw("see_null") == see_null
    assert see0 == first and see8 != first

"""rz_bloom / rz_present_bloomed on the GPU.  Every operation of the definition is one binary32 operation, so the images are
compared for equality with tests/bloom_ref.py.  Around that: the accumulation as input, determinism, the state the calls must
leave alone, rz_present_bloomed against its building blocks and against rz_present_display, errors, the C++ free functions and
the cost beside one a-trous pass."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import bloom_ref as BR
import display_ref as DR
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import RayZenError, Renderer, frame_params
from test_rays_gpu import Hip
from test_upscale_gpu import _median_ms

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 67 x 35 and 130 x 70 cross a 16 x 16 output tile in both axes, at level 0 and at level 1
FRAMES = [(1, 1), (2, 1), (9, 7), (33, 9), (65, 5), (67, 35), (130, 70)]
INF = float("inf")
_CAMERA = S.cornell_scene().camera
NO_OVERLAYS = dict(fps=0.0, show_fps=False, show_lights=False, show_bvh=False)


def _frame_only(W, H):
    """A context with a frame and no scene: all rz_bloom needs."""
    r = Renderer(0)
    r.set_frame(frame_params(_CAMERA, W, H, 0, 5, 1, 0))
    return r


def _setup(sc, W, H, spp=1, bounces=5):
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), bounces, spp, 0))
    r.render()
    return r


def _same(got, want, what, bad=None):
    """Bit for bit; at the pixels of `bad` (a mask) only the class of each value -- NaN, +Inf, -Inf -- is compared."""
    got, want = np.ascontiguousarray(got, F32).reshape(want.shape), np.ascontiguousarray(want, F32)
    differ = (got.view(np.uint32) != want.view(np.uint32)).any(axis=-1)
    if bad is not None:
        with np.errstate(invalid="ignore"):
            same_class = ((np.isnan(got) & np.isnan(want)) | (got == want)).all(axis=-1)
        differ &= ~(bad & same_class)
    at = np.argwhere(differ)
    assert not len(at), f"{what}: differs on {len(at)} pixels; first (y, x) {at[0].tolist()}: {got[tuple(at[0])]} != {want[tuple(at[0])]}"


def _f32(hip, ptr, shape):
    return hip.download(ptr, int(np.prod(shape)) * 4).view(F32).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit for bit

GRID = list(itertools.product((1, 2, 6, 8), (0.0, 0.5), (0.5, 1.0, 2.0), (4.0, INF)))


@pytest.mark.parametrize("w,h", FRAMES, ids=lambda v: str(v))
def test_host_form_equals_the_restatement(w, h):
    """levels 1, 2, 6, 8 x knee 0, 0.5 x spread 0.5, 1, 2 x a limit that binds (4; the frames reach 64) and none."""
    r = _frame_only(w, h)
    c = BR.frame(w, h)
    for levels, knee, spread, limit in GRID:
        kw = dict(levels=levels, knee=knee, spread=spread, limit=limit)
        out, glare = r.bloom(c, glare=True, **kw)
        want_out, want_glare, _ = BR.bloom(c, **kw)
        _same(glare, want_glare, f"glare {kw}")
        _same(out, want_out, f"rgb32f {kw}")
    # threshold, intensity; the output alone; intensity 0
    kw = dict(threshold=0.25, knee=1.0, intensity=2.0)
    _same(r.bloom(c, **kw), BR.bloom(c, **kw)[0], f"rgb32f alone {kw}")
    out, glare = r.bloom(c, glare=True, intensity=0.0)
    assert out.tobytes() == c.tobytes()
    _same(glare, BR.bloom(c)[1], "glare with intensity 0")
    assert r.bloom(c, intensity=0.0).tobytes() == c.tobytes()
    r.close()


@pytest.mark.parametrize("w,h", [(9, 7), (67, 35), (130, 70)], ids=lambda v: str(v))
def test_device_forms_equal_the_restatement(w, h):
    """Out of place and in place, each output alone, from a 16-byte aligned base and from one that is only 4-byte aligned."""
    hip = Hip()
    r = _frame_only(w, h)
    c = BR.frame(w, h, seed=2)
    nb = c.nbytes
    kw = dict(knee=0.25, spread=2.0, levels=8)
    want_out, want_glare, _ = BR.bloom(c, **kw)
    shape = c.shape
    for off in (0, 4):
        base = hip.alloc(nb + 32)
        assert base % 16 == 0
        din = base + off
        hip.ok(hip.L.hipMemcpy(din, c.ctypes.data, nb, 1))
        d32, dgl = hip.alloc(nb + 32, fill=0x5A) + off, hip.alloc(nb + 32, fill=0x5A) + off
        r.bloom_device(din, d32, dgl, **kw)
        r.sync()
        _same(_f32(hip, d32, shape), want_out, f"rgb32f, base + {off}")
        _same(_f32(hip, dgl, shape), want_glare, f"glare, base + {off}")
        assert (hip.download(d32 + nb, 16) == 0x5A).all() and (hip.download(dgl + nb, 16) == 0x5A).all()    # nothing past the end
        assert hip.download(din, nb).tobytes() == c.tobytes()
        only32, onlygl = hip.alloc(nb + 32, fill=0) + off, hip.alloc(nb + 32, fill=0) + off
        r.bloom_device(din, only32, None, **kw)
        r.bloom_device(din, None, onlygl, **kw)
        r.sync()
        _same(_f32(hip, only32, shape), want_out, f"rgb32f alone, base + {off}")
        _same(_f32(hip, onlygl, shape), want_glare, f"glare alone, base + {off}")
        # in place, with the glare beside it; then intensity 0 in place (nothing to do) and out of place (a copy)
        r.bloom_device(din, din, dgl, **kw)
        r.sync()
        _same(_f32(hip, din, shape), want_out, f"in place, base + {off}")
        _same(_f32(hip, dgl, shape), want_glare, f"glare of the in-place call, base + {off}")
        hip.ok(hip.L.hipMemcpy(din, c.ctypes.data, nb, 1))
        r.bloom_device(din, din, None, intensity=0.0)
        r.bloom_device(din, d32, None, intensity=0.0)
        r.sync()
        assert hip.download(din, nb).tobytes() == c.tobytes() and hip.download(d32, nb).tobytes() == c.tobytes()
    r.close()
    hip.close()


@pytest.mark.parametrize("w,h", [(33, 9), (67, 35)], ids=lambda v: str(v))
def test_bad_pixels_add_nothing(w, h):
    hip = Hip()
    r = _frame_only(w, h)
    c, bad, neg = BR.with_bad_pixels(BR.frame(w, h))
    mask = np.zeros((h, w), bool)
    for at in bad:
        mask[at] = True
    want_out, want_glare, _ = BR.bloom(c)
    out, glare = r.bloom(c, glare=True)
    _same(glare, want_glare, "glare, host")
    _same(out, want_out, "rgb32f, host", bad=mask)
    assert np.isfinite(glare).all() and np.isfinite(out[~mask]).all() and not np.isfinite(out[mask]).all(axis=-1).any()
    din, d32 = hip.upload(c), hip.alloc(c.nbytes)
    r.bloom_device(din, d32, None)
    r.sync()
    _same(_f32(hip, d32, c.shape), want_out, "rgb32f, device", bad=mask)
    # intensity 0 hands the bad pixels on as they are, NaN payloads and -0.0 included
    c.view(np.uint32)[1, 1] = (0x7FC12345, 0xFFC00001, 0x7F800001)
    c[0, 3] = (-0.0, 0.0, -0.0)
    assert r.bloom(c, intensity=0.0).tobytes() == c.tobytes()
    r.close()
    hip.close()


_BIG = {}


def _big():
    """The 1920 x 1080 seeded frame and its restatement, computed once."""
    if not _BIG:
        c = BR.frame(1920, 1080)
        _BIG["c"] = c
        _BIG["out"], _BIG["glare"], _ = BR.bloom(c)
    return _BIG


def test_full_hd_frame_equals_the_restatement_twice():
    """1920 x 1080 with the defaults on device pointers; a second call gives the same bytes."""
    hip = Hip()
    W, H = 1920, 1080
    big = _big()
    c = big["c"]
    r = _frame_only(W, H)
    din, d32, dgl = hip.upload(c), hip.alloc(c.nbytes), hip.alloc(c.nbytes)
    r.bloom_device(din, d32, dgl)
    r.sync()
    out, glare = _f32(hip, d32, c.shape).copy(), _f32(hip, dgl, c.shape).copy()
    _same(glare, big["glare"], "glare")
    _same(out, big["out"], "rgb32f")
    hip.ok(hip.L.hipMemset(d32, 0, c.nbytes))
    hip.ok(hip.L.hipMemset(dgl, 0, c.nbytes))
    r.bloom_device(din, d32, dgl)
    r.sync()
    assert _f32(hip, d32, c.shape).tobytes() == out.tobytes() and _f32(hip, dgl, c.shape).tobytes() == glare.tobytes()
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the accumulation as input; the state around the call

def test_rgb_in_null_reads_the_resolved_accumulation():
    sc = S.cornell_scene()
    W, H = 67, 35
    r = _setup(sc, W, H, spp=2)
    c = DR.resolve(r.read_accum())
    kw = dict(threshold=0.25, knee=0.25)
    a_out, a_glare = r.bloom(glare=True, **kw)
    b_out, b_glare = r.bloom(c, glare=True, **kw)
    assert a_out.tobytes() == b_out.tobytes() and a_glare.tobytes() == b_glare.tobytes()
    assert (a_glare > 0).any() and a_out.tobytes() != c.tobytes()
    _same(a_out, BR.bloom(c, **kw)[0], "rgb32f of the accumulation")
    # twice: the same bytes
    again = r.bloom(glare=True, **kw)
    assert again[0].tobytes() == a_out.tobytes() and again[1].tobytes() == a_glare.tobytes()
    r.close()


def _key(st):
    return tuple(v.tobytes() if hasattr(v, "tobytes") else v for v in st.values())


def test_leaves_every_state_alone():
    sc = S.cornell_scene()
    W, H = 48, 27
    r = _setup(sc, W, H, spp=2)
    r.denoise_temporal()                                # a history and
    r.display(auto=True, adapt=0.5)                     # an exposure to leave alone
    plan, acc = r.debug_last_plan(), r.read_accum().tobytes()
    tmp = [r.debug_read_temporal(k).tobytes() for k in range(5)]
    st = _key(r.display_state())
    r.bloom()
    r.bloom(BR.frame(W, H), glare=True, levels=8, spread=2.0)
    r.bloom(intensity=0.0)
    assert r.debug_last_plan() == plan and r.read_accum().tobytes() == acc
    assert [r.debug_read_temporal(k).tobytes() for k in range(5)] == tmp
    assert _key(r.display_state()) == st
    assert (r.width, r.height) == (W, H)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. rz_present_bloomed

def _pair(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("source", ["accum", "denoise", "temporal"])
def test_present_bloomed_with_intensity_zero_is_present_display(source):
    sc = S.cornell_scene()
    W, H = 64, 36
    kw = dict(fps=57.3, show_fps=True, show_lights=True, show_bvh=True, auto=True, curve="aces", transfer="srgb")
    filt = dict(iterations=2) if source != "accum" else None
    r, twin = _setup(sc, W, H), _setup(sc, W, H)
    got = r.present_bloomed(source, bloom=dict(intensity=0.0), filter=filt, **kw)
    want = twin.present_display(source, filter=filt, **kw)
    assert _pair(got, want)
    assert _key(r.display_state()) == _key(twin.display_state())
    assert not _pair(r.present_bloomed(source, bloom=dict(threshold=0.1, intensity=1.0), filter=filt, **kw), want)
    r.close()
    twin.close()


@pytest.mark.parametrize("display", [dict(auto=True, key=0.3, curve="reinhard", transfer="srgb"), dict(exposure=1.5, curve="aces")],
                         ids=["auto", "manual"])
def test_present_bloomed_is_display_of_bloom(display):
    """Every overlay off: both outputs are rz_display's on rz_bloom's output of the accumulation.  With auto exposure the metering
    sees the bloomed colour: the exposure differs from the one the plain frame meters."""
    sc = S.cornell_scene()
    W, H = 67, 35
    bl = dict(threshold=0.25, intensity=1.0)
    r, twin, plain = _setup(sc, W, H), _setup(sc, W, H), _setup(sc, W, H)
    rgb, rgba8 = r.present_bloomed(bloom=bl, **NO_OVERLAYS, **display)
    want32, want8 = twin.display(twin.bloom(**bl), **display)
    assert rgb.tobytes() == want32.tobytes() and rgba8.tobytes() == want8.tobytes()
    assert _key(r.display_state()) == _key(twin.display_state())
    # the defaults too
    r.display_reset()
    twin.display_reset()
    rgb, rgba8 = r.present_bloomed(**NO_OVERLAYS, **display)
    want32, want8 = twin.display(twin.bloom(), **display)
    assert rgb.tobytes() == want32.tobytes() and rgba8.tobytes() == want8.tobytes()
    if display.get("auto"):
        r.display_reset()
        r.present_bloomed(bloom=bl, **NO_OVERLAYS, **display)
        plain.present_display(**NO_OVERLAYS, **display)
        assert r.display_state()["exposure"] < plain.display_state()["exposure"]       # more light was metered
    for x in (r, twin, plain):
        x.close()


def test_present_bloomed_draws_the_overlays_on_top():
    sc = S.cornell_scene()
    W, H = 96, 54
    on = dict(fps=57.3, show_fps=True, show_lights=True, show_bvh=True)
    # The overlays are mixed into the colour with weights between 0 and 1, so the float output is compared: in bytes a faint
    # wire over a dark pixel rounds away in one image and not in the other.  A pixel that is exactly black would hide a black
    # wire in the plain image alone (the glare reaches every pixel), hence 8 samples and the check that there is none; a pixel
    # clamped to 1 would hide a white glyph in the bloomed image alone, hence the dark exposure and the check that none is.
    disp = dict(exposure=0.005)
    bl = dict(threshold=0.1, intensity=1.0)
    r = _setup(sc, W, H, spp=8)
    b_on, b_off = r.present_bloomed(bloom=bl, **on, **disp)[0], r.present_bloomed(bloom=bl, **NO_OVERLAYS, **disp)[0]
    d_on, d_off = r.present_display(**on, **disp)[0], r.present_display(**NO_OVERLAYS, **disp)[0]
    assert (d_off.max(axis=-1) > 0).all(), int((d_off.max(axis=-1) == 0).sum())
    where_b, where_d = (b_on != b_off).any(axis=-1), (d_on != d_off).any(axis=-1)
    assert where_d.sum() > 20 and (b_off != d_off).any() and b_off.max() < 1.0
    odd = np.argwhere(where_b != where_d)
    assert not len(odd), (len(odd), [(tuple(p), b_on[tuple(p)], b_off[tuple(p)], d_on[tuple(p)], d_off[tuple(p)]) for p in odd[:4]])
    r.close()


def test_source_two_advances_the_history_as_present_temporal_does():
    sc = S.cornell_scene()
    W, H = 64, 36
    r, twin = _setup(sc, W, H), _setup(sc, W, H)
    assert r.debug_read_temporal(0) is None and twin.debug_read_temporal(0) is None
    for _ in range(2):
        r.present_bloomed("temporal", **NO_OVERLAYS)
        twin.present_temporal(**NO_OVERLAYS)
        for which in range(5):
            assert r.debug_read_temporal(which).tobytes() == twin.debug_read_temporal(which).tobytes(), which
    r.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. errors

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    W, H = 16, 8
    n = W * H
    r = _setup(sc, W, H)
    pin = hip.upload(BR.frame(W, H))
    p32, pgl = hip.alloc(n * 12 + 16, fill=0x5A), hip.alloc(n * 12 + 16, fill=0x5A)

    def call(ctx, params=None, args=(pin, n * 12, p32, n * 12, pgl, n * 12), flags=0):
        a = list(args)
        return L.rz_bloom(ctx, params, C.c_void_p(a[0]), a[1], C.c_void_p(a[2]), a[3], C.c_void_p(a[4]), a[5], flags)

    def params(**kw):
        p = _lib.BloomParams(**_lib.BLOOM_DEFAULTS)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    nan = float("nan")
    assert call(None) == -1
    for bad in (dict(threshold=-0.5), dict(threshold=nan), dict(threshold=INF), dict(knee=-1.0), dict(knee=nan), dict(knee=INF),
                dict(limit=0.0), dict(limit=-1.0), dict(limit=nan), dict(intensity=-0.1), dict(intensity=nan), dict(intensity=INF),
                dict(spread=0.0), dict(spread=-1.0), dict(spread=4.0001), dict(spread=nan), dict(spread=INF), dict(levels=0),
                dict(levels=9), dict(levels=-1)):
        assert call(r._c, params(**bad)) == -1, bad
    for k in (0, 1):
        p = _lib.BloomParams(**_lib.BLOOM_DEFAULTS)
        p.reserved[k] = 1
        assert call(r._c, C.byref(p)) == -1 and b"reserved" in L.rz_last_error(r._c)
    assert call(r._c, flags=0x2) == -1 and call(r._c, flags=0x4) == -1 and call(r._c, flags=0x80000000) == -1
    for k in (0, 2, 4):
        a = [pin, n * 12, p32, n * 12, pgl, n * 12]
        a[k] += 2
        assert call(r._c, args=tuple(a)) == -1 and b"aligned" in L.rz_last_error(r._c), k
    assert call(r._c, args=(pin, n * 12, None, 0, None, 0)) == -1 and b"neither" in L.rz_last_error(r._c)
    assert call(r._c, args=(pin, n * 12, p32, n * 12, pin, n * 12)) == -1 and b"alias" in L.rz_last_error(r._c)
    assert call(r._c, args=(pin, n * 12, None, 0, pin + 12, n * 12)) == -1 and b"alias" in L.rz_last_error(r._c)
    assert call(r._c, args=(pin, n * 12 - 4, p32, n * 12, pgl, n * 12)) == -7
    assert call(r._c, args=(pin, n * 12, p32, n * 12 - 4, pgl, n * 12)) == -7
    assert call(r._c, args=(pin, n * 12, p32, n * 12, pgl, n * 12 - 4)) == -7
    # rz_present_bloomed
    pp = _lib.PresentParams()
    buf8, buf32 = np.zeros(n * 4, np.uint8), np.zeros(n * 3, F32)

    def present(present_params=C.byref(pp), display=None, bloom=None, source=0, filt=None, n8=buf8.nbytes, n32=buf32.nbytes):
        return L.rz_present_bloomed(r._c, present_params, display, bloom, source, filt, buf8.ctypes.data, n8, buf32.ctypes.data, n32)

    assert L.rz_present_bloomed(None, C.byref(pp), None, None, 0, None, None, 0, None, 0) == -1
    assert present(present_params=None) == -1
    assert present(source=3) == -1 and present(source=-1) == -1
    dn = _lib.DenoiseParams(5, 0.5, 128.0, 1.0, 1)
    assert present(source=0, filt=C.byref(dn)) == -1 and b"source 0" in L.rz_last_error(r._c)
    dp = _lib.DisplayParams(0, 1.0, 0.18, 1 / 64, 64.0, 1.0, 0, 0, 7, 4.0, 0)
    assert present(display=C.byref(dp)) == -1
    assert present(bloom=params(spread=5.0)) == -1 and b"spread" in L.rz_last_error(r._c)
    tp = _lib.TemporalParams(**_lib.TEMPORAL_DEFAULTS)
    tp.max_history = 0
    assert present(source=2, filt=C.byref(tp)) == -1
    assert present(n8=n * 4 - 1) == -7 and present(n32=n * 12 - 4) == -7
    r.sync()
    for ptr in (p32, pgl):
        assert (hip.download(ptr, n * 12 + 16) == 0x5A).all()           # nothing was launched
    assert not buf8.any() and not buf32.any()
    assert r.debug_read_temporal(0) is None                            # (the refused temporal source made no history)
    # the context stays usable and writes nothing past the buffers
    assert call(r._c) == 0 and present() == 0
    r.sync()
    assert (hip.download(p32 + n * 12, 16) == 0x5A).all() and (hip.download(pgl + n * 12, 16) == 0x5A).all()
    assert (hip.download(p32, n * 12) != 0x5A).any() and buf8.any()
    # the accumulation of a tile of a group frame: refused; a caller's buffer is not
    r.set_frame(frame_params(sc.camera, W, H, 2, 5, 1, 0, 0, 2))
    assert call(r._c, args=(None, 0, p32, n * 12, pgl, n * 12)) == -1 and b"whole frame" in L.rz_last_error(r._c)
    assert present() == -1 and b"whole frame" in L.rz_last_error(r._c)
    assert call(r._c) == 0
    r.close()
    # no frame
    nof = Renderer(0)
    nof.upload_scene(sc)
    assert call(nof._c) == -5
    assert L.rz_present_bloomed(nof._c, C.byref(pp), None, None, 0, None, buf8.ctypes.data, buf8.nbytes, None, 0) == -5
    nof.close()
    hip.close()


def test_a_failed_workspace_allocation_returns_the_error_and_writes_nothing():
    """rz_debug_fail_alloc fails the call's one allocation site, the pyramid: RZ_ERR_NO_MEMORY, nothing launched, and the next
    call is right."""
    hip = Hip()
    w, h = 67, 35
    r = _frame_only(w, h)
    c = BR.frame(w, h)
    din, d32, dgl = hip.upload(c), hip.alloc(c.nbytes, fill=0x5A), hip.alloc(c.nbytes, fill=0x5A)
    r.debug_fail_alloc(1)
    with pytest.raises(RayZenError) as e:
        r.bloom_device(din, d32, dgl)
    assert e.value.code == -8, str(e.value)
    r.sync()
    assert (hip.download(d32, c.nbytes) == 0x5A).all() and (hip.download(dgl, c.nbytes) == 0x5A).all()
    r.debug_fail_alloc(1)
    with pytest.raises(RayZenError) as e:
        r.bloom(c)
    assert e.value.code == -8, str(e.value)
    r.debug_fail_alloc(0)
    r.bloom_device(din, d32, dgl)
    r.sync()
    want_out, want_glare, _ = BR.bloom(c)
    _same(_f32(hip, d32, c.shape), want_out, "rgb32f after the failures")
    _same(_f32(hip, dgl, c.shape), want_glare, "glare after the failures")
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the C++ front end

def test_cpp_free_functions_equal_the_python_binding(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    exe = str(tmp_path / "bloom_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rayzen_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "bloom_driver.cpp"), "-L", lib, "-lrayzen_host", "-lrayzen_hip",
                           f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"bloom_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    fp = _lib.FrameParams.from_buffer_copy(raw("fp"))
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt).copy())
    r.set_frame(fp)
    r.render()
    wide = dict(threshold=0.5, knee=0.25, limit=8.0, intensity=0.5, spread=2.0, levels=3)
    aces = dict(exposure=1.5, curve="aces", transfer="srgb")
    o, g = r.bloom(glare=True)
    assert raw("out") == o.tobytes() and raw("glare") == g.tobytes() and (g > 0).any()
    assert raw("out2") == r.bloom(o, **wide).tobytes()
    plain = r.present_display("accum", **NO_OVERLAYS, **aces)[1].tobytes()
    assert raw("plain") == plain and raw("zero") == plain
    b32, b8 = r.present_bloomed(**NO_OVERLAYS, **aces)
    assert raw("bloomed") == b8.tobytes() and raw("bloomed32") == b32.tobytes() and b8.tobytes() != plain
    assert raw("denoised") == r.present_bloomed("denoise", bloom=wide, filter=dict(iterations=2), **NO_OVERLAYS, **aces)[1].tobytes()
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. cost

# Measured on an MI355X (profiles/bloom/README.md): rz_bloom 0.069 ms, the a-trous pass 0.313 ms, ratio 0.220.  The bound is that
# ratio times 1.5, rounded up to one decimal: margin for a shared machine.
RATIO_BOUND = 0.4


def test_costs_less_than_one_atrous_pass():
    """rz_bloom with the defaults on a 1920 x 1080 frame of device memory against one a-trous pass (rz_denoise, K = 1) on the
    same frame, in one process, device events, medians of 25."""
    hip = Hip()
    W, H = 1920, 1080
    sc = S.reference_scene(aspect=W / H)
    r = _setup(sc, W, H)
    c = _big()["c"]
    din, d32 = hip.upload(c), hip.alloc(c.nbytes)
    stream = hip.stream()
    r.set_stream(stream)
    bloom = _median_ms(hip, r, stream, lambda: r.bloom_device(din, d32, None))
    atrous = _median_ms(hip, r, stream, lambda: r.denoise_device(d32, iterations=1))
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()
    ratio = bloom / atrous
    print(f"rz_bloom 1920x1080: {bloom:.3f} ms; rz_denoise K=1 at 1920x1080: {atrous:.3f} ms; ratio {ratio:.3f}")
    assert ratio <= RATIO_BOUND, (bloom, atrous)

"""Edge anti-aliasing on see-through guides (rz_antialias_seethrough, rz_present_antialiased_seethrough;
rz_antialias_seethrough.hip) on the GPU: the frame-size records against rz_upscale_seethrough at factor 1 bit for bit; the edge
mask against the restatement (antialias_seethrough_ref.py) bit for bit, given those records; flat pixels bit-equal to the input
and edge pixels bit-equal to the binary32 box mean of rz_upscale_seethrough's own output on the same context; the whole frame
against the float64 restatement; the anchors (max_depth 0, a scene without specular surfaces, factor 1); the present call,
non-finite input, host and device paths, isolation from the render, temporal and display state, errors, the backstop, the C++
front end, and the cost next to rz_upscale_seethrough."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import antialias_ref as AR
import antialias_seethrough_ref as ASR
import denoise_ref as DR
import seethrough_ref as SR
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import CHAIN_DTYPE, RayZenError, Renderer, frame_params
from test_antialias_gpu import _assert_close
from test_denoise_gpu import _setup
from test_display_gpu import _key
from test_rays_gpu import Hip
from test_seethrough_gpu import glass_scene
from test_upscale_gpu import _bad_patterns, _filled, _median_ms, sliver_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SCENES = {"glass": lambda w, h: glass_scene(w, h), "reference": lambda w, h: S.reference_scene(aspect=4 / 3),
          "sliver": lambda w, h: sliver_scene()}
FRAMES = [(1, 1), (3, 2), (65, 5), (33, 17), (24, 18)]          # 65 wide: more than one unit per row
CASES = [(n, w, h) for n in sorted(SCENES) for w, h in FRAMES] + [("glass", 100, 75)]
FACTORS = (2, 3, 4)
SOURCES = ("accum", "denoise", "temporal")


def _cls(ch):
    return SR.split_records(ch)[3]


def _records(r, md):
    """The chain records at the frame's own size, as rz_upscale_seethrough returns them at factor 1."""
    _, g, ch = r.upscale(factor=1, see_through=md, guides=True, chains=True)
    return g, ch


def _ref(c, g, ch, g_hi, ch_hi, sc, **kw):
    return ASR.antialias(c, g, ch["throughput"], _cls(ch), g_hi, ch_hi["throughput"], _cls(ch_hi), sc.materials, sc.camera.inv_proj, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# records, edges and colours

@pytest.mark.parametrize("name,w,h", CASES, ids=lambda v: str(v))
def test_records_edges_and_colours(name, w, h):
    sc = SCENES[name](w, h)
    r = _setup(sc, w, h, spp=2)
    c_acc = DR.resolve(r.read_accum())
    rng = np.random.default_rng(w * 100 + h)
    c_syn = (np.exp(rng.normal(-1.0, 1.5, (h, w, 1))) * rng.uniform(0.5, 1.5, (h, w, 3))).astype(F32)
    for md in (8, 1, 2):
        g_lo, ch_lo = _records(r, md)
        cls = _cls(ch_lo)
        for s in (FACTORS if md == 8 else (2,)):
            got, g, ch, edge = r.antialias(factor=s, see_through=md, guides=True, chains=True, edges=True)    # rgb_in NULL: the accumulation
            assert ch.dtype == CHAIN_DTYPE and g.tobytes() == g_lo.tobytes() and ch.tobytes() == ch_lo.tobytes()
            assert np.array_equal(edge, ASR.edge_mask(c_acc, g, cls, sc.materials, sc.camera.inv_proj))
            assert got[~edge].tobytes() == c_acc[~edge].tobytes()               # flat: c exactly
            for demod in (True, False):
                got = r.antialias(factor=s, demodulate=demod, see_through=md)
                up, g_hi, ch_hi = r.upscale(factor=s, demodulate=demod, see_through=md, guides=True, chains=True)
                mean32 = AR.box_mean32(up, s)
                assert got[~edge].tobytes() == c_acc[~edge].tobytes()
                assert got[edge].tobytes() == mean32[edge].tobytes(), f"{name} {w}x{h} s={s} md={md} demodulate={demod}: the box mean's bits"
                want, _ = _ref(c_acc, g, ch, g_hi, ch_hi, sc, factor=s, demodulate=demod)
                _assert_close(got, want, c_acc, s, f"{name} {w}x{h} s={s} md={md} demodulate={demod} accumulation")
                assert r.antialias(c_acc, factor=s, demodulate=demod, see_through=md).tobytes() == got.tobytes()   # the same colour handed over
                assert r.antialias(factor=s, demodulate=demod, see_through=md).tobytes() == got.tobytes()          # two calls, the same bytes
                assert np.isfinite(got).all()
            # non-default sigmas and edge thresholds, on a colour of its own
            kw = dict(sigma_normal=16.0, sigma_plane=0.5)
            got, edge2 = r.antialias(c_syn, factor=s, edge_normal=0.99, edge_plane=0.25, edges=True, see_through=md, **kw)
            assert np.array_equal(edge2, ASR.edge_mask(c_syn, g, cls, sc.materials, sc.camera.inv_proj, edge_normal=0.99, edge_plane=0.25))
            assert (edge2 >= edge).all()
            up, g_hi, ch_hi = r.upscale(c_syn, factor=s, see_through=md, guides=True, chains=True, **kw)
            mean32 = AR.box_mean32(up, s)
            assert got[~edge2].tobytes() == c_syn[~edge2].tobytes() and got[edge2].tobytes() == mean32[edge2].tobytes()
            want, _ = _ref(c_syn, g, ch, g_hi, ch_hi, sc, factor=s, edge_normal=0.99, edge_plane=0.25, **kw)
            _assert_close(got, want, c_syn, s, f"{name} {w}x{h} s={s} md={md} rgb_in")
        if md == 8:
            first = r.antialias(edges=True)[1]
            chain_edge = edge & (cls != 0)
            print(f"{name} {w}x{h}: edge share {edge.mean():.3f} (first-hit {first.mean():.3f}), chain edges {chain_edge.mean():.3f}, "
                  f"see-through edges that are first-hit flat {int((edge & ~first).sum())}")
            if (name, w, h) == ("glass", 100, 75):
                # a wave takes 64 / s^2 pixels at a time: some 64-pixel run of a row holds more chain edge pixels than two of
                # s = 4's batches, so one unit's edge pixels go to several batches and their chains go on
                per_unit = max(int(chain_edge[y, x:x + 64].sum()) for y in range(h) for x in range(0, w, 64))
                assert per_unit > 2 * (64 // 16), per_unit
                assert (edge & ~first).sum() >= 20
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# the anchors

@pytest.mark.parametrize("w,h", [(65, 5), (24, 18)], ids=lambda v: str(v))
def test_max_depth_0_is_rz_antialias(w, h):
    sc = glass_scene(w, h)
    r = _setup(sc, w, h, spp=2)
    rng = np.random.default_rng(7)
    c_syn = rng.uniform(0.05, 2.0, (h, w, 3)).astype(F32)
    for s in FACTORS:
        for c in (None, c_syn):
            for demod in (True, False):
                a = r.antialias(c, factor=s, demodulate=demod, guides=True, edges=True)
                b = r.antialias(c, factor=s, demodulate=demod, guides=True, edges=True, see_through=0, chains=True)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[3])
                assert (b[2]["word"] == np.where(b[1]["instance"] >= 0, (np.clip(b[1]["material"], 0, len(sc.materials) - 1) + 1) << 8, 0)).all()
                assert (b[2]["throughput"] == 1).all()
    assert a[2].any() and not a[2].all()
    r.close()


def test_a_scene_without_specular_surfaces_is_rz_antialias():
    w, h = 33, 17
    sc = glass_scene(w, h, extras=False)
    r = _setup(sc, w, h, spp=2)
    for s in FACTORS:
        a = r.antialias(factor=s, guides=True, edges=True)
        b = r.antialias(factor=s, guides=True, edges=True, see_through=8, chains=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[3])
        assert (b[2]["word"] & 0xFF == 0).all() and a[2].any()
    r.close()


def test_factor_1_is_c_itself_and_still_classifies():
    w, h = 65, 5
    sc = glass_scene(w, h)
    r = _setup(sc, w, h, spp=2)
    c = DR.resolve(r.read_accum())
    g_lo, ch_lo = _records(r, 8)
    assert r.antialias(factor=1, see_through=8).tobytes() == c.tobytes()
    out, g, ch, edge = r.antialias(factor=1, see_through=8, guides=True, chains=True, edges=True)
    assert out.tobytes() == c.tobytes() and g.tobytes() == g_lo.tobytes() and ch.tobytes() == ch_lo.tobytes()
    assert np.array_equal(edge, ASR.edge_mask(c, g, _cls(ch), sc.materials, sc.camera.inv_proj)) and edge.any() and not edge.all()
    x = c.copy()
    x[2, 7] = np.nan
    x[0, 0, 1] = -np.inf
    out, edge_x = r.antialias(x, factor=1, edges=True, see_through=8)
    assert out.tobytes() == x.tobytes() and edge_x[2, 7] and edge_x[0, 0]
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# present

def test_present_equals_present_display_of_the_calls_own_colour():
    hip = Hip()
    w, h, s = 100, 75, 2
    sc = glass_scene(w, h)
    kw = dict(fps=12.5, show_fps=True, show_lights=True, show_bvh=True)
    r = _setup(sc, w, h, spp=2)
    aa = r.antialias(factor=s, see_through=8)
    assert aa.tobytes() != r.antialias(factor=s).tobytes()
    rgb, rgba8 = r.present_antialiased("accum", factor=s, see_through=8, **kw)
    # sources 1 and 2: the denoisers run first, then the same pass
    for source, den in (("denoise", r.denoise(iterations=2)), ("temporal", r.denoise_temporal(iterations=2, keep=True))):
        a = r.present_antialiased(source, factor=s, filter=dict(iterations=2), show_fps=False, see_through=8)
        want = np.clip(r.antialias(den, factor=s, see_through=8), 0.0, 1.0)
        assert a[0].tobytes() == want.tobytes(), source
    # see_through = 0: rz_present_antialiased's bytes; factor 1: rz_present_display's
    for source in SOURCES:
        filt = None if source == "accum" else dict(iterations=2)
        outs = []
        for call in (lambda: r.present_antialiased(source, factor=s, filter=filt, see_through=0, **kw),
                     lambda: r.present_antialiased(source, factor=s, filter=filt, **kw),
                     lambda: r.present_antialiased(source, factor=1, filter=filt, see_through=8, **kw),
                     lambda: r.present_display(source, filter=filt, **kw)):
            if source == "temporal":
                r.temporal_reset()
            outs.append(call())
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), source
        assert outs[2][0].tobytes() == outs[3][0].tobytes() and outs[2][1].tobytes() == outs[3][1].tobytes(), source
    r.display_reset()
    shown = r.present_antialiased("accum", factor=s, auto=True, adapt=0.5, curve="aces", transfer="srgb", see_through=8, **kw)
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
    shown2 = r2.present_display("accum", auto=True, adapt=0.5, curve="aces", transfer="srgb", **kw)
    state2 = r2.display_state()
    r2.close()
    hip.close()
    assert rgba8.tobytes() == rgba82.tobytes() and rgb.tobytes() == rgb2.tobytes()
    assert state["exposure"] != 1.0 and _key(state) == _key(state2)
    assert shown[0].tobytes() == shown2[0].tobytes() and shown[1].tobytes() == shown2[1].tobytes()


def test_present_source_2_advances_the_history_as_present_temporal_does():
    w, h = 64, 48
    sc = glass_scene(w, h)
    hist = []
    for aa in (False, True):
        r = _setup(sc, w, h)
        for _ in range(2):
            if aa:
                r.present_antialiased("temporal", factor=2, see_through=8)
            else:
                r.present_temporal()
        hist.append([r.debug_read_temporal(k).tobytes() for k in range(5)])
        r.close()
    assert hist[0] == hist[1]


# ---------------------------------------------------------------------------------------------------------------------
# non-finite input at 65 x 5

def test_bad_pixels_are_edges_and_contained():
    w, h, s = 65, 5, 2
    sc = glass_scene(w, h)
    r = _setup(sc, w, h, render=False)
    zero = np.zeros((h, w, 3), F32)
    _, g, ch, edge0 = r.antialias(zero, guides=True, chains=True, edges=True, see_through=8)
    _, g_hi, ch_hi = r.upscale(zero, guides=True, chains=True, see_through=8)
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
            got, edge = r.antialias(c, demodulate=demod, edges=True, see_through=8)
            want, edge_ref = _ref(c, g, ch, g_hi, ch_hi, sc, demodulate=demod)
            assert np.array_equal(edge, edge_ref) and np.array_equal(edge, edge0 | mask), pname
            assert np.isfinite(got).all(), f"{pname}: {int((~np.isfinite(got)).any(-1).sum())} pixels not finite"
            _assert_close(got, want, c, s, f"{pname} demodulate={demod}")
            if pname == "all":
                assert not got.view(np.uint32).any()    # no tap anywhere, stage 3 on a bad pixel: exactly 0
            near = np.zeros((h, w), bool)
            for y, x in zip(*np.nonzero(mask)):
                near[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = True
            ref_clean = r.antialias(clean, demodulate=demod, see_through=8)
            assert got[~near].tobytes() == ref_clean[~near].tobytes(), pname
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# paths, state

def test_host_and_device_paths_agree_and_null_outputs():
    hip = Hip()
    w, h, s = 65, 5, 3
    sc = glass_scene(w, h)
    n = w * h
    r = _setup(sc, w, h, spp=2)
    rgb, g, ch, edge = r.antialias(factor=s, guides=True, chains=True, edges=True, see_through=8)
    e8 = edge.astype(np.uint8)
    assert (ch["word"] & 0xFF).any()
    d32, dg, dc, de = _filled(hip, n * 12, 0x5A), _filled(hip, n * 48, 0x5A), _filled(hip, n * 16, 0x5A), _filled(hip, n + 3, 0x5A)
    r.antialias_device(None, d32, dg, de + 1, factor=s, see_through=8, chains_ptr=dc)       # edges needs no alignment
    r.sync()
    assert hip.download(d32, n * 12).tobytes() == rgb.tobytes()
    assert hip.download(dg, n * 48).tobytes() == g.tobytes() and hip.download(dc, n * 16).tobytes() == ch.tobytes()
    raw = hip.download(de, n + 3)
    assert raw[1:n + 1].tobytes() == e8.tobytes() and (raw[[0, n + 1, n + 2]] == 0x5A).all()
    # the input from device memory
    c = DR.resolve(r.read_accum())
    din = hip.upload(c)
    d32b = _filled(hip, n * 12, 0)
    r.antialias_device(din, d32b, None, None, factor=s, see_through=8)
    r.sync()
    assert hip.download(d32b, n * 12).tobytes() == rgb.tobytes()
    # factor 1 on the device: a copy
    d1 = _filled(hip, n * 12, 0)
    r.antialias_device(din, d1, None, None, factor=1, see_through=8)
    r.sync()
    assert hip.download(d1, n * 12).tobytes() == c.tobytes() == hip.download(din, n * 12).tobytes()
    # NULL outputs: each alone, and none
    p32, pg, pc, pe = _filled(hip, n * 12, 0), _filled(hip, n * 48, 0), _filled(hip, n * 16, 0), _filled(hip, n, 0x5A)
    r.antialias_device(None, None, pg, None, factor=s, see_through=8)
    r.sync()
    assert not hip.download(p32, n * 12).any() and hip.download(pg, n * 48).tobytes() == g.tobytes()
    r.antialias_device(None, None, None, None, factor=s, see_through=8, chains_ptr=pc)
    r.sync()
    assert hip.download(pc, n * 16).tobytes() == ch.tobytes() and not hip.download(p32, n * 12).any()
    r.antialias_device(None, None, None, pe, factor=s, see_through=8)
    r.sync()
    assert hip.download(pe, n).tobytes() == e8.tobytes() and not hip.download(p32, n * 12).any()
    r.antialias_device(None, p32, None, None, factor=s, see_through=8)
    r.antialias_device(None, None, None, None, factor=s, see_through=8)
    r.sync()
    assert hip.download(p32, n * 12).tobytes() == rgb.tobytes()
    # the host path, each output alone
    assert r.antialias(factor=s, see_through=8, chains=True)[1].tobytes() == ch.tobytes()
    assert np.array_equal(r.antialias(factor=s, see_through=8, edges=True)[1], edge)
    r.close()
    hip.close()


def test_leaves_render_temporal_display_state_and_the_other_passes_alone():
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
        up0 = [a.tobytes() for a in r.upscale(factor=3, guides=True, see_through=8, chains=True)]
        aa0 = [a.tobytes() for a in r.antialias(factor=3, guides=True, edges=True)]
        if with_aa:
            r.antialias(guides=True, chains=True, edges=True, see_through=8)
            r.antialias(r.denoise(iterations=1), factor=3, see_through=2)
            assert _key(r.display_state()) == disp
            r.present_antialiased("accum", see_through=8)
            r.present_antialiased("denoise", factor=3, filter=dict(iterations=1), see_through=8)
            assert r.debug_last_plan() == plan
            assert r.read_accum().tobytes() == acc0.tobytes()
            assert [r.debug_read_temporal(k).tobytes() for k in range(5)] == tmp        # sources 0 and 1
        assert [a.tobytes() for a in r.upscale(factor=3, guides=True, see_through=8, chains=True)] == up0
        assert [a.tobytes() for a in r.antialias(factor=3, guides=True, edges=True)] == aa0
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
    w, h = 16, 8
    sc = glass_scene(w, h)
    n = w * h
    r = _setup(sc, w, h)
    pin = hip.upload(DR.resolve(r.read_accum()))
    p32, pg, pc, pe = (_filled(hip, n * 12 + 16, 0x5A), _filled(hip, n * 48 + 16, 0x5A), _filled(hip, n * 16 + 16, 0x5A),
                       _filled(hip, n + 16, 0x5A))
    full = (None, 0, p32, n * 12, pg, n * 48, pc, n * 16, pe, n)

    def call(ctx, params=None, st=None, args=full, flags=0):
        a = list(args)
        return L.rz_antialias_seethrough(ctx, params, st, C.c_void_p(a[0]), a[1], C.c_void_p(a[2]), a[3], C.c_void_p(a[4]), a[5],
                                         C.c_void_p(a[6]), a[7], C.c_void_p(a[8]), a[9], flags)

    def params(**kw):
        p = _lib.AntialiasParams(2, 128.0, 1.0, 1, 0.9, 1.0)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def depth(md, reserved=None):
        p = _lib.SeethroughParams(md)
        if reserved is not None:
            p.reserved[reserved] = 1
        return C.byref(p)

    def swap(k, v):
        a = list(full)
        a[k] = v
        return tuple(a)

    nan = float("nan")
    assert call(None) == -1
    # the new cases: max_depth, the reserved words of rz_seethrough_params
    for md in (-1, 9, 100):
        assert call(r._c, st=depth(md)) == -1 and b"max_depth" in L.rz_last_error(r._c), md
    for k in range(7):
        assert call(r._c, st=depth(8, k)) == -1 and b"reserved" in L.rz_last_error(r._c)
    # rz_antialias' own
    for bad in (dict(factor=0), dict(factor=5), dict(sigma_plane=0.0), dict(sigma_normal=nan), dict(demodulate=2), dict(edge_normal=1.5),
                dict(edge_normal=nan), dict(edge_plane=-0.5), dict(edge_plane=nan)):
        assert call(r._c, params(**bad)) == -1, bad
    for k in range(2):
        p = _lib.AntialiasParams(2, 128.0, 1.0, 1, 0.9, 1.0)
        p.reserved[k] = 7
        assert call(r._c, C.byref(p)) == -1             # rz_antialias_params.reserved stays must-be-zero
    assert call(r._c, flags=0x4) == -1 and call(r._c, flags=0x2) == -1
    assert call(r._c, args=(pin + 2, n * 12) + full[2:]) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert call(r._c, args=swap(2, p32 + 2)) == -1
    assert call(r._c, args=swap(4, pg + 4)) == -1
    assert call(r._c, args=swap(6, pc + 4)) == -1 and b"chains" in L.rz_last_error(r._c)       # a misaligned chains pointer
    assert call(r._c, args=swap(6, pc + 8)) == -1
    assert call(r._c, args=(pin, n * 12, pin, n * 12) + full[4:]) == -1 and b"rgb_in" in L.rz_last_error(r._c)     # in place
    assert call(r._c, args=(pin, n * 12 - 1) + full[2:]) == -7
    assert call(r._c, args=swap(3, n * 12 - 1)) == -7
    assert call(r._c, args=swap(5, n * 48 - 1)) == -7
    assert call(r._c, args=swap(7, n * 16 - 1)) == -7 and b"chains" in L.rz_last_error(r._c)
    assert call(r._c, args=swap(9, n - 1)) == -7
    pp = _lib.PresentParams()
    buf8 = np.zeros(n * 4, np.uint8)
    buf32 = np.zeros(n * 3, F32)

    def present(ctx, present_p=C.byref(pp), aa=None, st=None, disp=None, source=0, filt=None, n8=buf8.nbytes, n32=buf32.nbytes):
        return L.rz_present_antialiased_seethrough(ctx, present_p, aa, st, disp, source, filt, buf8.ctypes.data, n8, buf32.ctypes.data, n32)

    assert present(None) == -1 and present(r._c, present_p=None) == -1
    assert present(r._c, st=depth(9)) == -1 and present(r._c, st=depth(-1)) == -1 and present(r._c, st=depth(8, 3)) == -1
    assert present(r._c, aa=params(factor=1), st=depth(9)) == -1         # checked before the factor-1 short cut
    assert present(r._c, aa=params(factor=5)) == -1 and present(r._c, aa=params(edge_normal=2.0)) == -1
    assert present(r._c, source=3) == -1 and present(r._c, source=0, filt=params()) == -1
    assert present(r._c, n8=n * 4 - 1) == -7 and present(r._c, n32=n * 12 - 1) == -7
    assert not buf8.any() and not buf32.any()
    r.sync()
    for ptr, nb in ((p32, n * 12 + 16), (pg, n * 48 + 16), (pc, n * 16 + 16), (pe, n + 16)):
        assert (hip.download(ptr, nb) == 0x5A).all()            # nothing was launched
    # the context stays usable; the defaults (both NULL) are factor 2 and max_depth 8
    assert call(r._c) == 0 and present(r._c) == 0
    r.sync()
    assert buf8.any() and (hip.download(pe, n) <= 1).all()
    assert hip.download(pc, n * 16).tobytes() == r.antialias(see_through=8, chains=True)[1].tobytes()
    for md in (0, 8):
        assert call(r._c, st=depth(md)) == 0
    # a tile of a group frame: refused
    r.set_frame(frame_params(sc.camera, w, h, 2, 5, 1, 0, 0, 2))
    assert call(r._c) == -1 and b"whole frame" in L.rz_last_error(r._c)
    assert present(r._c) == -1
    r.close()
    # no frame / no scene: NOT_READY
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
    w, h = 16, 8
    sc = glass_scene(w, h)
    r = _setup(sc, w, h)
    before = r.antialias(guides=True, chains=True, edges=True, see_through=8)
    r.sync()
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    with pytest.raises(RayZenError) as e:
        r.antialias(guides=True, chains=True, edges=True, see_through=8)
    message = str(e.value).split("): ", 1)[1]
    assert e.value.code == -9 and message.startswith("rz_antialias_seethrough: ") and "0x8" in message, str(e.value)
    r.sync()                                            # reported once, then clear
    after = r.antialias(guides=True, chains=True, edges=True, see_through=8)
    assert [a.tobytes() for a in after] == [b.tobytes() for b in before]
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    with pytest.raises(RayZenError) as e:
        r.present_antialiased("accum", see_through=8)
    assert e.value.code == -9 and "rz_present_antialiased_seethrough: " in str(e.value)
    # the device path returns at once and leaves the word to rz_sync
    d32 = _filled(hip, w * h * 12, 0)
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    r.antialias_device(None, d32, None, None, see_through=8)
    with pytest.raises(RayZenError) as e:
        r.sync()
    assert e.value.code == -9
    r.sync()
    assert hip.download(d32, w * h * 12).tobytes() == before[0].tobytes()
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# the C++ front end: presentDisplay(..., &antialias, &seeThrough) against the Python binding

def test_cpp_present_display_antialiased_see_through_equals_python(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    header = os.path.join(ROOT, "rayzen_amd", "csrc", "host")
    exe = str(tmp_path / "antialias_seethrough_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", header,
                           os.path.join(ROOT, "tests", "cpp", "antialias_seethrough_driver.cpp"), "-L", lib, "-lrayzen_host",
                           "-lrayzen_hip", f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"antialias_seethrough_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    fp = _lib.FrameParams.from_buffer_copy(raw("fp"))
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt).copy())
    r.set_frame(fp)
    r.render()
    kw = dict(fps=0.0, show_fps=False)
    a2 = dict(factor=2, sigma_normal=128.0, sigma_plane=1.0, demodulate=True, edge_normal=0.9, edge_plane=1.0)
    plain = r.present_display("accum", **kw)[1].tobytes()
    first = r.present_antialiased("accum", **a2, **kw)[1].tobytes()
    see8 = r.present_antialiased("accum", see_through=8, **a2, **kw)[1].tobytes()
    see3 = r.present_antialiased("denoise", factor=3, sigma_normal=64.0, sigma_plane=0.5, demodulate=False, edge_normal=0.95,
                                 edge_plane=0.5, filter=dict(iterations=2), exposure=1.5, curve="aces", transfer="srgb", see_through=2,
                                 **kw)[1].tobytes()
    ch, edge = r.antialias(see_through=8, chains=True, edges=True)[1:]
    r.close()
    assert (edge & ((ch["word"] & 0xFF) > 0)).mean() > 0.01             # the driver's camera does see edges behind glass or in the mirror
    assert raw("plain") == plain and raw("first") == first and raw("see8") == see8 and raw("see3") == see3
    assert raw("see0") == first and raw("see_null") == see8 and raw("see1") == plain
    assert see8 != first


# ---------------------------------------------------------------------------------------------------------------------
# cost

@pytest.mark.parametrize("extras", [False, True], ids=["c2", "c2g"])
def test_costs_no_more_than_the_upsampler_that_casts_every_sub_pixels_chain(extras):
    """rz_antialias_seethrough at factor 2 against rz_upscale_seethrough at factor 2, both at max_depth 8, from the same
    1920 x 1080 frame, in one process, device events, medians of 25: bunny_scene as test_antialias_gpu.py's cost test renders it
    (c2: nothing specular in view) and with its glass blob and mirror cube (c2g).  The upsampler casts the chain of all four
    sub-pixels of every pixel (and the frame-size records); this pass casts the frame-size records and four chains on the edge
    pixels only.  No margin.  At this size every wave of the grid classifies several units and the edge pixels' batches are
    numbered across all segments: the mask and the colours are held to the restatement and to rz_upscale_seethrough's own
    output here too.

    MEASURED (profiles/antialias_seethrough/README.md): c2 0.40 ms against 0.77 ms, c2g 1.41 ms against 2.04 ms (edge share
    1.54 %, 1.10 % of the frame edge pixels whose chain moves).  The first form of the pass, in which the wave that classified a
    unit also ran its edge pixels' chains, missed this on c2g (2.51 ms): the time was the sequential queries of its busiest
    wave.  The edge pixels are now handed out evenly between the two kernels."""
    hip = Hip()
    W, H, s = 1920, 1080, 2
    sc = S.bunny_scene(aspect=W / H, extras=extras)
    r = _setup(sc, W, H)
    c = DR.resolve(r.read_accum())
    got, g, ch, edge = r.antialias(factor=s, guides=True, chains=True, edges=True, see_through=8)
    cls = _cls(ch)
    assert np.array_equal(edge, ASR.edge_mask(c, g, cls, sc.materials, sc.camera.inv_proj)) and 1e-3 < edge.mean() < 0.25
    print(f"edge share {edge.mean():.4f}, chain edge share {(edge & (cls != 0)).mean():.4f}")
    assert (edge & (cls != 0)).any() == extras
    mean32 = AR.box_mean32(r.upscale(factor=s, see_through=8), s)
    assert got[~edge].tobytes() == c[~edge].tobytes() and got[edge].tobytes() == mean32[edge].tobytes()
    del mean32
    d_aa, d_up = hip.alloc(W * H * 12), hip.alloc(W * H * s * s * 12)
    stream = hip.stream()
    r.set_stream(stream)
    t_up = _median_ms(hip, r, stream, lambda: r.upscale_device(None, d_up, None, factor=s, see_through=8))
    t_aa = _median_ms(hip, r, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s, see_through=8))
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()
    print(f"1920x1080 bunny_scene{' + glass + mirror' if extras else ''}, factor 2, max_depth 8: rz_antialias_seethrough {t_aa:.3f} ms, "
          f"rz_upscale_seethrough {t_up:.3f} ms, ratio {t_up / t_aa:.2f}")
    assert t_aa <= t_up, (t_aa, t_up)

"""Non-finite samples in both denoisers on the GPU (include/rayzen_hip.h, "Non-finite samples"): a pixel whose resolved colour has
a NaN or infinite channel is contained by pass 0 of rz_denoise and by the accumulation step of rz_denoise_temporal.  Bad pixels
enter through rgba_in (patterns from fixed seeds) or through the one scene of the suite that renders NaN (a glass material with
ior = NaN); every result is held to the float64 restatements (denoise_ref.py, temporal_ref.py) with the tolerances
test_denoise_gpu.py and test_temporal_gpu.py justify, bad and good pixels alike.  Then both denoisers against their restatements
on frames smaller than the taps' reach and at grid tails, with finite input.

Measured on an MI355X (printed by the tests; profiles/denoise/README.md, profiles/temporal/README.md), against the tolerances the
two files derive: rz_denoise 3.1e-7 over the patterns, 3.3e-7 for the count channel, 1.7e-6 at 333 x 187 (1e-4); the temporal
stage 1.8e-5 (TOL 4e-4) and its K = 5 filter 2.1e-6 (TOL_FILTER 1e-4); the small frames 1.5e-6 and 9.4e-7."""
import numpy as np
import pytest

import denoise_ref as DR
import temporal_ref as TR
from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer, editor_rays, frame_params
from test_denoise_gpu import _assert_close, _setup
from test_rays_gpu import Hip
from test_temporal_abi import gpu_sequences
from test_temporal_gpu import TOL, TOL_FILTER, _advance, _check_frame, _filter_close, _frame, _history, _rel, _renderer

pytestmark = pytest.mark.gpu

F32 = np.float32
W0, H0 = 96, 54
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
KS = (1, 2, 5)


# ---------------------------------------------------------------------------------------------------------------------
# bad-pixel patterns: (H, W) bool masks from fixed seeds, the guide deciding where a surface or an edge is

def _isolated(g, rng):
    m = np.zeros(g.shape, bool)
    m[int(rng.integers(8, g.shape[0] - 8)), int(rng.integers(8, g.shape[1] - 8))] = True
    return m


def _corners(g, rng):
    m = np.zeros(g.shape, bool)
    m[0, 0] = m[-1, -1] = True
    return m


def _block(g, rng):
    """A 5 x 5 block inside one surface: every pixel of it and of its one-pixel rim a hit on one instance."""
    inst = g["instance"]
    H, W = g.shape
    spots = [(y, x) for y in range(1, H - 6) for x in range(1, W - 6)
             if inst[y, x] >= 0 and (inst[y - 1:y + 6, x - 1:x + 6] == inst[y, x]).all()]
    assert spots
    y, x = spots[int(rng.integers(len(spots)))]
    m = np.zeros(g.shape, bool)
    m[y:y + 5, x:x + 5] = True
    return m


def _row(g, rng):
    m = np.zeros(g.shape, bool)
    m[int(rng.integers(2, g.shape[0] - 2))] = True
    return m


def _edge(g, rng):
    """Pairs of horizontal neighbours of which one is a hit and the other a miss: both sides of the edge."""
    hit = g["instance"] >= 0
    ys, xs = np.nonzero(hit[:, :-1] != hit[:, 1:])
    assert len(ys) >= 6
    m = np.zeros(g.shape, bool)
    for k in rng.choice(len(ys), 6, replace=False):
        m[ys[k], xs[k]] = m[ys[k], xs[k] + 1] = True
    assert (m & hit).any() and (m & ~hit).any()
    return m


def _sprinkle(g, rng):
    m = rng.random(g.shape) < 0.01
    assert m.any()
    return m


PATTERNS = {"isolated": _isolated, "corners": _corners, "block": _block, "row": _row, "edge": _edge, "sprinkle": _sprinkle}


def _poke(acc, mask, value, channels):
    """acc with the masked pixels' sum set to `value` in one channel (a different one from pixel to pixel) or in all three."""
    out = np.array(acc, F32)
    ys, xs = np.nonzero(mask)
    if channels == 3:
        out[ys, xs, :3] = value
    else:
        out[ys, xs, (ys + xs) % 3] = value
    assert np.array_equal(DR.bad_pixels(DR.resolve(out)), mask | DR.bad_pixels(DR.resolve(acc)))
    return out


def _mixed(acc, mask, seed):
    """The masked pixels set to NaN, +Inf and -Inf in turn, in one channel or in all three, from a fixed seed."""
    rng = np.random.default_rng(seed)
    out = np.array(acc, F32)
    vals = list(VALUES.values())
    for y, x in zip(*np.nonzero(mask)):
        v = vals[int(rng.integers(3))]
        if rng.random() < 0.5:
            out[y, x, :3] = v
        else:
            out[y, x, int(rng.integers(3))] = v
    assert np.array_equal(DR.bad_pixels(DR.resolve(out)), mask)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rz_denoise

@pytest.fixture(scope="module")
def frame():
    """One rendered 1-spp frame of the instanced scene (sky and several instances), its guide, and the renderer."""
    sc = S.instanced_scene(n=24, count=16, aspect=16 / 9)
    r = _setup(sc, W0, H0)
    acc = r.read_accum()
    _, g = r.denoise(iterations=0, guides=True)
    assert np.isfinite(acc).all() and (g["instance"] < 0).any() and len(np.unique(g["instance"])) > 3
    acc.setflags(write=False)
    g.setflags(write=False)
    yield sc, r, acc, g
    r.close()


def _denoise_case(sc, r, g, x, what, ks=KS):
    """rz_denoise on the buffer x for K = 0 and K in ks, with and without demodulation, against the restatement."""
    c = DR.resolve(x)
    assert r.denoise(rgba_in=x, iterations=0).tobytes() == c.tobytes()         # K = 0: c_p exactly, bad or not
    for demod in (True, False):
        for K in ks:
            got = r.denoise(rgba_in=x, iterations=K, demodulate=demod)
            want, den = DR.denoise(c, g, sc.materials, sc.camera.inv_proj, iterations=K, demodulate=demod, want_den=True)
            assert np.isfinite(got).all(), f"{what} K={K} demodulate={demod}: {int((~np.isfinite(got)).any(-1).sum())} pixels not finite"
            _assert_close(got, want, f"{what} K={K} demodulate={demod}")
            if K == 1:
                assert not got[den == 0].view(np.uint32).any()                  # every tap dropped: exactly 0


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_denoise_contains_bad_pixels(frame, pattern):
    sc, r, acc, g = frame
    mask = PATTERNS[pattern](g, np.random.default_rng(sorted(PATTERNS).index(pattern) + 100))
    for name, value in VALUES.items():
        for channels in (1, 3):
            _denoise_case(sc, r, g, _poke(acc, mask, value, channels), f"{pattern} {name} x{channels}")


def test_denoise_block_centre_and_whole_frame_are_exactly_zero(frame):
    sc, r, acc, g = frame
    mask = _block(g, np.random.default_rng(7))
    x = _poke(acc, mask, np.nan, 3)
    ys, xs = np.nonzero(mask)
    cy, cx = ys.min() + 2, xs.min() + 2
    got = r.denoise(rgba_in=x, iterations=1)
    _, den = DR.denoise(DR.resolve(x), g, sc.materials, sc.camera.inv_proj, iterations=1, want_den=True)
    assert den[cy, cx] == 0 and (den[mask] == 0).sum() == 1
    assert not got[cy, cx].view(np.uint32).any() and np.isfinite(got).all()
    # every pixel bad: no tap is left anywhere, whatever K
    allbad = _poke(acc, np.ones(g.shape, bool), -np.inf, 1)
    for K in KS:
        assert not r.denoise(rgba_in=allbad, iterations=K).view(np.uint32).any()


def test_denoise_count_channel(frame):
    """The divide is part of the definition: n = 0 and n = NaN count as 1, a finite sum over n = +Inf is c = 0 (not bad)."""
    sc, r, acc, g = frame
    rng = np.random.default_rng(8)
    x = np.array(acc, F32)
    a, b, c = (np.unravel_index(k, g.shape) for k in rng.choice(H0 * W0, 36, replace=False).reshape(3, 12))
    x[a[0], a[1], 3] = 0.0                          # n = 0 with an infinite sum: n = 1, bad
    x[a[0], a[1], 1] = np.inf
    x[b[0], b[1], 3] = np.nan                       # n = NaN: n = 1, c = the sum
    x[c[0], c[1], 3] = np.inf                       # a finite sum over n = +Inf: c = 0
    res = DR.resolve(x)
    want_bad = np.zeros(g.shape, bool)
    want_bad[a] = True
    assert np.array_equal(DR.bad_pixels(res), want_bad)
    assert res[b].tobytes() == x[b][:, :3].tobytes() and (res[c] == 0).all()
    _denoise_case(sc, r, g, x, "count channel")


def test_denoise_partial_tiles():
    """333 x 187: neither a multiple of the 64 x 4 workgroup; a 1 % sprinkle of mixed bad values on a random finite buffer."""
    W, H = 333, 187
    sc = S.instanced_scene(n=24, count=16, aspect=16 / 9)
    r = _setup(sc, W, H, render=False)
    _, g = r.denoise(iterations=0, guides=True)
    rng = np.random.default_rng(9)
    x = rng.random((H, W, 4)).astype(F32)
    x[..., 3] = rng.integers(1, 4, (H, W))
    x = _mixed(x, rng.random((H, W)) < 0.01, 10)
    x[H - 1, W - 1, 0] = np.nan
    _denoise_case(sc, r, g, x, "333x187 sprinkle", ks=(1, 5))
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# rz_denoise_temporal

def _temporal_mask(g, seed):
    rng = np.random.default_rng(seed)
    return _isolated(g, rng) | _corners(g, rng) | _block(g, rng) | _sprinkle(g, rng)


@pytest.mark.parametrize("name", ["cornell", "instanced"])
def test_temporal_contains_bad_pixels(name):
    """Four frames of the sequence test_temporal_gpu.py runs; bad pixels in frames 0 and 2 only.  Every frame is checked by
    _check_frame (the history read back, the restatement stepped from it, TOL), the K = 5 output by the filter stage's method
    (TOL_FILTER)."""
    make, W, H, _, _ = gpu_sequences()[name]
    sc = make()
    base = sc.camera
    r = _renderer(sc, W, H)
    p = TR.params()
    worst = worst_f = 0.0
    for fr in range(4):
        xf = _advance(sc, name, fr, base)
        if xf is not None:
            r.update_transforms(xf)
        _frame(r, sc, W, H, fr)
        x = r.read_accum()
        assert np.isfinite(x).all()
        bad = np.zeros((H, W), bool)
        if fr in (0, 2):
            _, g = r.denoise(iterations=0, guides=True)
            bad = _temporal_mask(g, 40 + fr)
            x = _mixed(x, bad, 50 + fr)
        out5, g, st = r.denoise_temporal(rgba_in=x, keep=True, guides=True, stats=True)          # K = 5
        assert np.isfinite(out5).all() and np.isfinite(st).all(), f"{name} frame {fr}"
        shows = ~np.isfinite(r.denoise_temporal(rgba_in=x, keep=True, iterations=0)).all(-1)
        w, share, ref = _check_frame(r, sc, W, H, p, f"{name} frame {fr} ({int(bad.sum())} bad)", rgba_in=x)
        worst = max(worst, w)
        ok = ~ref["ambiguous"]
        assert np.array_equal(ref["bad"], bad) and (bad & ok).sum() >= 0.9 * bad.sum()      # bad pixels are compared, not excused
        col, mom = r.debug_read_temporal(0), r.debug_read_temporal(1)
        assert np.isfinite(col).all() and np.isfinite(mom).all(), f"{name} frame {fr}: the stored history"
        # K = 0: the non-finite outputs are exactly the bad pixels without accepted history
        assert np.array_equal(shows[ok], (bad & ~ref["accepted"])[ok]) and not (shows & ~bad).any()
        if fr == 0:
            assert np.array_equal(shows, bad)
        if fr == 2:
            assert (bad & ref["accepted"] & ok).sum() >= 0.5 * bad.sum()        # most of them do have history to stand in
        # the filter stage from the D just stored and the call's own variance
        alpha = np.where((g["instance"] >= 0)[..., None], DR.albedo(g, sc.materials), 1.0)
        want = TR.filter_from(col[..., :3], st[..., 1], alpha, g, sc.camera.inv_proj, p)
        worst_f = max(worst_f, _filter_close(out5, want, f"{name} frame {fr} K = 5"))
    print(f"{name} with bad pixels: worst relative error, temporal stage {worst:.3g} (TOL {TOL:g}), filter {worst_f:.3g} (TOL_FILTER {TOL_FILTER:g})")
    r.close()


def test_temporal_bad_pixel_over_a_history_keeps_the_history_colour():
    """One bad pixel in frame 1 over the history of frame 0: D there is the reprojected D_h, N is N_h + 1."""
    make, W, H, _, _ = gpu_sequences()["cornell"]
    sc = make()
    base = sc.camera
    r = _renderer(sc, W, H)
    _advance(sc, "cornell", 0, base)
    _frame(r, sc, W, H, 0)
    r.denoise_temporal(iterations=0)
    _advance(sc, "cornell", 1, base)
    _frame(r, sc, W, H, 1)
    cam = sc.camera
    hist = _history(r)
    acc = r.read_accum()
    _, g = r.denoise_temporal(keep=True, guides=True, iterations=0)
    md = editor_rays(cam, W, H)["dir"].reshape(H, W, 3)
    inst = TR.inst_pack(sc.arrays[S.BIND_INSTANCES])

    def step(c):
        return TR.step(hist, c, g, sc.materials, cam.view, cam.proj, cam.inv_proj, cam.position, inst, md, TR.params(iterations=0))[0]

    clean = step(DR.resolve(acc))
    full = clean["accepted"] & ~clean["ambiguous"] & (clean["S"] > 0.99) & (g["instance"] >= 0)
    full[:4] = full[-4:] = full[:, :4] = full[:, -4:] = False
    ys, xs = np.nonzero(full)
    assert len(ys)
    y, x = ys[len(ys) // 2], xs[len(ys) // 2]
    out_clean = r.denoise_temporal(rgba_in=acc, keep=True, iterations=0)
    others = np.ones((H, W), bool)
    others[y, x] = False
    for value in VALUES.values():
        xin = np.array(acc, F32)
        xin[y, x, 1] = value
        out = r.denoise_temporal(rgba_in=xin, keep=True, iterations=0)
        assert out[others].tobytes() == out_clean[others].tobytes()            # no other pixel moved
        ref = step(DR.resolve(xin))
        assert ref["bad"].sum() == 1 and ref["bad"][y, x] and ref["accepted"][y, x]
        # the restatement's D at the pixel IS its reprojected D_h, and N_h + 1 = 2 exactly (every tap has N = 1)
        assert ref["N"][y, x] == 2.0
        # (... which the clean frame gives away: its D = D_h + (d - D_h) / 2, so D_h = 2 D - d)
        assert np.allclose(ref["D"][y, x], 2.0 * clean["D"][y, x] - clean["d"][y, x], rtol=1e-12, atol=1e-15)
        err = _rel(out[y, x], ref["out0"][y, x], ref["scale"][y, x])
        assert err.max() <= TOL, err
        assert np.isfinite(out).all()
    # committing: D and N as stored
    xin = np.array(acc, F32)
    xin[y, x] = np.nan
    r.denoise_temporal(rgba_in=xin, iterations=0)
    col = r.debug_read_temporal(0)
    ref = step(DR.resolve(xin))
    assert col[y, x, 3] == 2.0 and _rel(col[y, x, :3], ref["D"][y, x], ref["scale"][y, x]).max() <= TOL
    assert np.isfinite(col).all() and np.isfinite(r.debug_read_temporal(1)).all()
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the scene of the suite whose accumulation holds NaN

def _present_of(hip, sc, W, H, rgb):
    """rz_present on a context whose accumulation is (rgb, 1)."""
    buf = np.concatenate([rgb, np.ones((H, W, 1), F32)], -1)
    dbuf = hip.upload(buf)
    r2 = Renderer(0)
    r2.upload_scene(sc)
    r2.bind_accum(dbuf, buf.nbytes)
    r2.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 5, 1, 0))
    out = r2.present()
    r2.close()
    return out


def test_nan_ior_frame_through_every_presenting_call():
    """test_gpu_configs_full.py's NaN-ior scene (48 x 28, 4 spp, 5 bounces): NaN reaches the accumulation; every presenting call
    that filters returns finite colour at its default K, and its bytes are rz_present's of that colour."""
    hip = Hip()
    sc = S.bunny_scene(n=8, bunny_material=3, floor_material=0)
    sc.materials["ior"][3] = np.nan
    W, H, spp, b = 48, 28, 4, 5
    r = Renderer(0)
    r.upload_scene(sc)

    def render(fr):
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), b, spp, fr * spp))
        r.clear_accum()
        r.render()
        acc = r.read_accum()
        assert np.isnan(acc).any()                  # the precondition: NaN really reaches pixels
        return acc

    def check(out, colour, what):
        """out: a presenting call's (rgb, rgba8); colour: the filter's own float output the call presented."""
        assert np.isfinite(colour).all() and np.isfinite(out[0]).all(), what
        rgb2, rgba82 = _present_of(hip, sc, W, H, colour)
        assert out[1].tobytes() == rgba82.tobytes() and out[0].tobytes() == rgb2.tobytes(), what

    acc = render(0)
    bad = DR.bad_pixels(DR.resolve(acc))
    print(f"NaN-ior frame: {int(bad.sum())} of {W * H} pixels bad")
    assert np.array_equal(~np.isfinite(r.denoise(iterations=0)).all(-1), bad)          # K = 0 shows them
    den = r.denoise()
    check(r.present_denoised(), den, "present_denoised")
    check(r.present_display(source="denoise"), den, "present_display denoise")
    for fr in range(3):
        if fr:
            render(fr)
        out = r.denoise_temporal(keep=True)
        check(r.present_temporal(), out, f"present_temporal frame {fr}")
        assert np.isfinite(r.debug_read_temporal(0)).all() and np.isfinite(r.debug_read_temporal(1)).all()
    render(3)
    out = r.denoise_temporal(keep=True)
    check(r.present_display(source="temporal"), out, "present_display temporal")
    assert np.isfinite(r.debug_read_temporal(0)).all() and r.debug_read_temporal(0)[..., 3].max() == 4
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# frames smaller than the taps' reach, and grid tails (finite input)

SMALL = [(1, 1), (1, 7), (7, 1), (5, 3), (65, 5)]


@pytest.mark.parametrize("W,H", SMALL, ids=lambda v: str(v))
def test_small_frames_match_the_restatements(W, H):
    sc = S.cornell_scene()
    base = sc.camera
    rng = np.random.default_rng(1000 * W + H)

    def buffer():
        x = rng.random((H, W, 4)).astype(F32)
        x[..., 3] = rng.integers(1, 4, (H, W))
        return x

    r = _setup(sc, W, H, render=False)
    x = buffer()
    _, g = r.denoise(iterations=0, guides=True)
    assert g.shape == (H, W)
    for K in (0, 1, 3, 5):
        for demod in (True, False):
            got = r.denoise(rgba_in=x, iterations=K, demodulate=demod)
            if K == 0:
                assert got.tobytes() == DR.resolve(x).tobytes()
            else:
                _assert_close(got, DR.denoise(DR.resolve(x), g, sc.materials, sc.camera.inv_proj, iterations=K, demodulate=demod),
                              f"{W}x{H} K={K} demodulate={demod}")
    # temporal: two frames, the camera slightly moved between them -- sideways, up, forward and turned in yaw and pitch, by amounts
    # for which the restatement leaves no pixel of these five sizes ambiguous (at 1 x 1 one such pixel is the whole frame; a
    # pure yaw keeps v of the sky's middle row at an integer)
    p = TR.params()
    moved = S.Camera(position=tuple(np.asarray(base.position, np.float64) + (0.21, 0.13, -0.17)),
                     target=tuple(np.asarray(base.target, np.float64) + (0.37, 0.29, 0.0)), up=tuple(base.up), fov=base.fov,
                     aspect=base.aspect, near=base.near, far=base.far)
    for fr in range(2):
        sc.camera = moved if fr else base
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 5, 1, fr))
        x = buffer()
        out5, g, st = r.denoise_temporal(rgba_in=x, keep=True, guides=True, stats=True)
        _, share, ref = _check_frame(r, sc, W, H, p, f"{W}x{H} frame {fr}", rgba_in=x)
        assert share == 0 and (fr == 0 or ref["accepted"].any())
        col = r.debug_read_temporal(0)
        alpha = np.where((g["instance"] >= 0)[..., None], DR.albedo(g, sc.materials), 1.0)
        _filter_close(out5, TR.filter_from(col[..., :3], st[..., 1], alpha, g, sc.camera.inv_proj, p), f"{W}x{H} frame {fr} K = 5")
    sc.camera = base
    r.close()

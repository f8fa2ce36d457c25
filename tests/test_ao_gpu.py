"""rz_ambient_occlusion on the GPU.  raw is the CPU oracle's two queries (rzo.trace for the guide, rzo.shadow for a walk) put
together by tests/ao_ref.py, and everything after it is a handful of binary32 operations per pixel, so every output is compared
for equality with the restatement.  The timing test at the end states its own bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_ref as AR
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import VISIBILITY_DTYPE, HIT_DTYPE, RayZenError, Renderer, frame_params
from refit_ref import wobble
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES, RADII = (1, 4, 16), (0.5, 2.0)


def _frame(sc, w, h):
    return frame_params(sc.camera, w, h, len(sc.lights), 1, 1)


def _setup(sc, w=None, h=None, flags=0):
    r = Renderer(0, flags)
    r.upload_scene(sc)
    if w:
        r.set_frame(_frame(sc, w, h))
    return r


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        first = tuple(bad[0]) if len(bad) else None
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first at {first}: "
                             f"{got[first] if first else got.ravel()[0]!r} != {want[first] if first else want.ravel()[0]!r}")


def _image(h, w, seed=5):
    """An rgb32f image with values below 0 and above 1 among the floats."""
    return np.random.default_rng(seed).uniform(-0.25, 1.5, (h, w, 3)).astype(F32)


class _Arrays:
    """A scene as the context holds it now: the eight bindings read back."""

    def __init__(self, r):
        self.arrays = {b: r.read_binding(b) for b in S.BINDING_DTYPES}


# ---------------------------------------------------------------------------------------------------------------------
# 1. raw is the oracle's

@pytest.mark.parametrize("name", sorted(AR.CASES))
def test_raw_equals_the_restatement(name):
    sc, w, h = AR.scene(name), 32, 24
    r = _setup(sc)                          # no rz_set_frame: the call is given its frame
    fp = _frame(sc, w, h)
    for n in SAMPLES:
        for radius in RADII:
            got = r.ambient_occlusion(fp, samples=n, radius=radius, smooth=False)["ao"]
            _same(got, AR.raw(name, w, h, n, radius)[0], f"{name} N = {n} radius {radius}")
    r.close()


@pytest.mark.parametrize("w,h", AR.PARTIAL, ids=lambda v: str(v))
def test_raw_on_partial_tiles(w, h):
    sc = AR.scene("reference")
    r = _setup(sc)
    fp = _frame(sc, w, h)
    for n in SAMPLES:
        for radius in RADII:
            got = r.ambient_occlusion(fp, samples=n, radius=radius, smooth=False)["ao"]
            _same(got, AR.raw("reference", w, h, n, radius)[0], f"{w}x{h} N = {n} radius {radius}")
    r.close()


def test_raw_equals_the_librarys_own_queries_on_many_tiles():
    """240 x 135 (30 x 17 tiles, the top row of tiles partial), N = 8: the guide is rz_denoise's, the walks rz_shadow_rays' on the
    restatement's rays -- the same kernels' loop, asked ray by ray instead of tile by tile."""
    sc = S.bunny_scene(n=24, extras=True)
    w, h, n, radius = 240, 135, 8, 2.0
    r = _setup(sc, w, h)
    got = r.ambient_occlusion(samples=n, radius=radius, smooth=False)["ao"]
    _, hits = r.denoise(iterations=0, guides=True)
    g = AR.guide_of_hits(hits, sc.camera, w, h)
    rays, walked = AR.sample_rays(g, n, radius)
    lit, visibility = r.shadow_rays(rays["origin"], rays["dir"], rays["max_dist"])
    r.close()
    assert 0.3 * w * h < g.hit.sum() < w * h
    vis = np.zeros(len(rays), VISIBILITY_DTYPE)
    vis["lit"], vis["visibility"] = lit, visibility
    a = AR.visibility_of(vis, walked)
    _same(got, AR.raw_image(g, a), "240 x 135")
    assert ((a > 0) & (a < 1)).sum() > 100 and (got < 1).sum() > 1000


# ---------------------------------------------------------------------------------------------------------------------
# 2. the gather and the outputs

@pytest.mark.parametrize("name", sorted(AR.CASES))
def test_smoothed_outputs_equal_the_restatement(name):
    sc, w, h = AR.scene(name), 32, 24
    g = AR.guide(name, w, h)
    raw = AR.raw(name, w, h, 4, 2.0)[0]
    ao = AR.smooth(g, raw, sc.camera.inv_proj)
    assert ao.tobytes() != raw.tobytes()
    rgb = _image(h, w)
    r = _setup(sc)
    fp = _frame(sc, w, h)
    for strength in (0.0, 0.5, 1.0):
        for src in (rgb, None):
            got = r.ambient_occlusion(fp, src, samples=4, radius=2.0, strength=strength, want=("ao", "rgb32f", "rgba8"))
            what = f"{name} strength {strength} {'white' if src is None else 'image'}"
            _same(got["ao"], ao, what)
            want = AR.modulate(ao, src, strength)
            _same(got["rgb32f"], want, what)
            _same(got["rgba8"], AR.quantise(want), what)
    # the unsmoothed colour, and a gather with other thresholds
    got = r.ambient_occlusion(fp, rgb, samples=4, radius=2.0, smooth=False, want=("ao", "rgb32f", "rgba8"))
    _same(got["ao"], raw, name)
    _same(got["rgb32f"], AR.modulate(raw, rgb), name)
    _same(got["rgba8"], AR.quantise(AR.modulate(raw, rgb)), name)
    got = r.ambient_occlusion(fp, samples=4, radius=2.0, normal_cos=0.5, plane_tol=0.25)["ao"]
    _same(got, AR.smooth(g, raw, sc.camera.inv_proj, 0.5, 0.25), f"{name} other thresholds")
    r.close()


@pytest.mark.parametrize("w,h", AR.PARTIAL, ids=lambda v: str(v))
def test_smoothed_on_partial_tiles(w, h):
    sc = AR.scene("reference")
    raw = AR.raw("reference", w, h, 4, 2.0)[0]
    ao = AR.smooth(AR.guide("reference", w, h), raw, sc.camera.inv_proj)
    r = _setup(sc)
    got = r.ambient_occlusion(_frame(sc, w, h), samples=4, radius=2.0, want=("ao", "rgba8"))
    r.close()
    _same(got["ao"], ao, f"{w}x{h}")
    _same(got["rgba8"], AR.quantise(AR.modulate(ao)), f"{w}x{h}")


def test_each_output_alone_and_the_device_form():
    """Each output alone gives the bytes all three give together, with and without smoothing, and the device form gives the host
    form's bytes and writes nothing past its buffers."""
    hip = Hip()
    sc, w, h = AR.scene("bunny"), 65, 21
    np_ = w * h
    rgb = _image(h, w)
    r = _setup(sc)
    fp = _frame(sc, w, h)
    d_in = hip.upload(rgb)
    for smooth in (True, False):
        kw = dict(samples=2, radius=1.5, smooth=smooth, strength=0.75)
        both = r.ambient_occlusion(fp, rgb, want=("ao", "rgb32f", "rgba8"), **kw)
        for k in both:
            _same(r.ambient_occlusion(fp, rgb, want=(k,), **kw)[k], both[k], f"{k} alone, smooth {smooth}")
        sizes = {"ao": np_ * 4, "rgb32f": np_ * 12, "rgba8": np_ * 4}
        dev = {k: hip.alloc(b + 16, 0x5A) for k, b in sizes.items()}
        r.ambient_occlusion_device(fp, d_in, dev["ao"], dev["rgb32f"], dev["rgba8"], **kw)
        r.sync()
        for k, b in sizes.items():
            got = hip.download(dev[k], b + 16)
            assert got[:b].tobytes() == both[k].tobytes(), f"{k}, device form, smooth {smooth}"
            assert (got[b:] == 0x5A).all(), k
        for k, b in sizes.items():          # ... and each alone on the device
            p = hip.alloc(b, 0x5A)
            r.ambient_occlusion_device(fp, d_in, **{f"{k}_ptr": p}, **kw)
            r.sync()
            assert hip.download(p, b).tobytes() == both[k].tobytes(), f"{k} alone, device form, smooth {smooth}"
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the occlusion follows the scene

def _expect(arrays, camera, w, h, n, radius):
    g = AR.oracle_guide(arrays, camera, w, h)
    raw = AR.oracle_raw(arrays, g, n, radius)[0]
    return raw, AR.smooth(g, raw, camera.inv_proj)


def test_after_update_transforms():
    sc, w, h = AR.scene("instanced"), 32, 24
    r = _setup(sc, w, h)
    before = r.ambient_occlusion(samples=4, radius=2.0)["ao"]
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(m, F32).reshape(16) for m in S.instanced_transforms(7, 16)])
    r.update_transforms(xf)
    got_raw = r.ambient_occlusion(samples=4, radius=2.0, smooth=False)["ao"]
    got = r.ambient_occlusion(samples=4, radius=2.0)["ao"]
    now = _Arrays(r)
    r.close()
    raw, ao = _expect(now.arrays, sc.camera, w, h, 4, 2.0)
    _same(got_raw, raw, "after update_transforms")
    _same(got, ao, "after update_transforms")
    assert got.tobytes() != before.tobytes()


def test_after_a_refit():
    sc = S.bunny_scene(n=12, aspect=4 / 3)
    w, h = 24, 18
    r = _setup(sc, w, h)
    before = r.ambient_occlusion(samples=4, radius=2.0)["ao"]
    _same(before, _expect(sc.arrays, sc.camera, w, h, 4, 2.0)[1], "built")
    r.refit_geometry(wobble(S.make_blob(12, 2.8, 0), 0.5), first=12)
    got_raw = r.ambient_occlusion(samples=4, radius=2.0, smooth=False)["ao"]
    got = r.ambient_occlusion(samples=4, radius=2.0)["ao"]
    now = _Arrays(r)
    r.close()
    raw, ao = _expect(now.arrays, sc.camera, w, h, 4, 2.0)
    _same(got_raw, raw, "after the refit")
    _same(got, ao, "after the refit")
    assert got.tobytes() != before.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 4. isolation

def test_the_call_leaves_render_temporal_and_display_state_alone():
    hip = Hip()
    sc = S.reference_scene()                                # (its glass carries currentIor from chunk to chunk)
    w, h, spp, bounces = 40, 30, 2, 5
    nl = len(sc.lights)

    def state(r):
        d = r.display_state()
        return (b"".join(r.debug_read_temporal(k).tobytes() for k in range(5)),
                b"".join(np.asarray(d[k]).tobytes() for k in sorted(d)))

    def run(with_calls):
        r = Renderer(0, 0)
        r.upload_scene(sc)
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, 0))
        r.render()
        first = r.read_accum()
        r.denoise_temporal()
        r.display(auto=True, curve="reinhard")
        if with_calls:
            plan, kernel, ms, before = r.debug_last_plan(), r.last_kernel_name(), r.last_render_ms(), state(r)
            got = r.ambient_occlusion(rgb=first[..., :3], samples=4, radius=2.0, want=("ao", "rgb32f", "rgba8"))
            _same(got["ao"], _expect(sc.arrays, sc.camera, w, h, 4, 2.0)[1], "between two chunks")
            r.ambient_occlusion(_frame(sc, 65, 5), samples=16, smooth=False)       # another frame: the one of rz_set_frame stays
            d_ao = hip.alloc(w * h * 4)
            r.ambient_occlusion_device(ao_ptr=d_ao)
            r.sync()
            assert r.read_accum().tobytes() == first.tobytes()
            assert (r.debug_last_plan(), r.last_kernel_name(), r.last_render_ms()) == (plan, kernel, ms)
            assert state(r) == before
            assert (r.width, r.height) == (w, h)
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, spp))
        r.render()
        r.sync()
        out = r.read_accum(), len(r.render_history_ms()), r.denoise_temporal(), r.display(auto=True, curve="reinhard")[1], state(r)
        r.close()
        return out

    plain, mixed = run(False), run(True)
    hip.close()
    assert mixed[0].tobytes() == plain[0].tobytes() and mixed[1] == plain[1] == 2
    assert mixed[2].tobytes() == plain[2].tobytes() and mixed[3].tobytes() == plain[3].tobytes() and mixed[4] == plain[4]


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors and the backstop

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 16, 8
    np_ = w * h
    r = _setup(sc)
    fp = _frame(sc, w, h)
    d_in, d_ao, d_rgb, d_8 = (hip.alloc(b + 16, 0x5A) for b in (np_ * 12, np_ * 4, np_ * 12, np_ * 4))
    full = (d_in, np_ * 12, d_ao, np_ * 4, d_rgb, np_ * 12, d_8, np_ * 4)

    def params(samples=4, radius=1.0, smooth=1, strength=1.0, normal_cos=0.9, plane_tol=2.0, reserved=None):
        p = _lib.AoParams(samples, radius, smooth, strength, normal_cos, plane_tol)
        if reserved is not None:
            p.reserved[reserved] = 1
        return C.byref(p)

    def ao(ctx, frame=fp, p=None, args=full, flags=0):
        return L.rz_ambient_occlusion(ctx, None if frame is None else C.byref(frame), p, *args, flags)

    nan, inf = float("nan"), float("inf")
    assert ao(None) == -1 and ao(r._c, frame=None) == -1
    assert ao(r._c, flags=2) == -1 and ao(r._c, flags=0x80000000) == -1
    for bad in ((0, 8), (16, 0), (-1, 8), (1 << 16, 1 << 16)):
        assert ao(r._c, frame=frame_params(sc.camera, bad[0], bad[1], 2, 1, 1)) == -1, bad
    for bad in (dict(samples=0), dict(samples=3), dict(samples=32), dict(samples=-4), dict(radius=0.0), dict(radius=-1.0),
                dict(radius=inf), dict(radius=nan), dict(smooth=2), dict(smooth=-1), dict(strength=-0.01), dict(strength=1.01),
                dict(strength=nan), dict(normal_cos=1.5), dict(normal_cos=nan), dict(plane_tol=0.0), dict(plane_tol=inf),
                dict(plane_tol=nan), dict(reserved=0), dict(reserved=1)):
        assert ao(r._c, p=params(**bad)) == -1, bad
    assert b"reserved" in L.rz_last_error(r._c)
    assert ao(r._c, args=(d_in, np_ * 12, None, 0, None, 0, None, 0)) == -1 and b"none of" in L.rz_last_error(r._c)
    for k in range(4):
        a = list(full)
        a[2 * k] += 2
        assert ao(r._c, args=tuple(a)) == -1 and b"aligned" in L.rz_last_error(r._c), k
    for k in range(4):
        a = list(full)
        a[2 * k + 1] -= 1
        assert ao(r._c, args=tuple(a)) == -7, k
    host = np.full(np_, 0x5A5A5A5A, np.int32)
    assert L.rz_ambient_occlusion(r._c, C.byref(fp), None, None, 0, host.ctypes.data, np_ * 4 - 1, None, 0, None, 0, _lib.AO_HOST) == -7
    assert L.rz_ambient_occlusion(r._c, C.byref(fp), params(samples=5), None, 0, host.ctypes.data, np_ * 4, None, 0, None, 0, _lib.AO_HOST) == -1
    assert (host == 0x5A5A5A5A).all()
    # nothing was launched
    r.sync()
    for p, b in ((d_ao, np_ * 4), (d_rgb, np_ * 12), (d_8, np_ * 4)):
        assert (hip.download(p, b + 16) == 0x5A).all()
    # the context stays usable; every valid N passes; nothing is written past the buffers
    hip.ok(hip.L.hipMemset(d_in, 0, np_ * 12))
    for n in (1, 2, 4, 8, 16):
        assert ao(r._c, p=params(samples=n)) == 0, n
    assert ao(r._c) == 0
    r.sync()
    for p, b in ((d_ao, np_ * 4), (d_rgb, np_ * 12), (d_8, np_ * 4)):
        assert (hip.download(p, b + 16)[b:] == 0x5A).all()
    assert hip.download(d_ao, np_ * 4).tobytes() == r.ambient_occlusion(fp)["ao"].tobytes()
    r.close()
    # no scene, a scene without its instances, a scene without materials
    empty = Renderer(0)
    assert ao(empty._c) == -5 and b"no scene" in L.rz_last_error(empty._c)
    empty.close()
    part = Renderer(0)
    for b in S.BINDING_DTYPES:
        if b != S.BIND_INSTANCES:
            part.upload(b, sc.arrays[b])
    assert ao(part._c) == -5 and b"no scene" in L.rz_last_error(part._c)
    part.close()
    nomat = Renderer(0)
    for b in S.BINDING_DTYPES:
        nomat.upload(b, sc.arrays[b][:0] if b == S.BIND_MATERIALS else sc.arrays[b])
    assert ao(nomat._c) == -5 and b"no materials" in L.rz_last_error(nomat._c)
    nomat.close()
    hip.close()


def test_backstop_host_path_reports_and_device_path_leaves_it_to_sync():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 16, 8
    r = _setup(sc, w, h)
    before = r.ambient_occlusion()["ao"]
    r.sync()
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    with pytest.raises(RayZenError) as e:
        r.ambient_occlusion()
    message = str(e.value).split("): ", 1)[1]
    assert e.value.code == -9 and message.startswith("rz_ambient_occlusion: ") and "0x8" in message, str(e.value)
    r.sync()                                                # reported once, then clear
    assert r.ambient_occlusion()["ao"].tobytes() == before.tobytes()
    d_ao = hip.alloc(w * h * 4, 0)
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    r.ambient_occlusion_device(ao_ptr=d_ao)
    with pytest.raises(RayZenError) as e:
        r.sync()
    assert e.value.code == -9
    r.sync()
    assert hip.download(d_ao, w * h * 4).tobytes() == before.tobytes()
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the C++ front end

def test_cpp_free_functions_equal_the_python_binding(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    exe = str(tmp_path / "ao_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rayzen_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "ao_driver.cpp"), "-L", lib, "-lrayzen_host", "-lrayzen_hip",
                           f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"ao_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    assert raw("dirs") == AR.directions().tobytes()
    fp = _lib.FrameParams.from_buffer_copy(raw("frame"))
    w, h = fp.width, fp.height
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt))
    in32 = np.frombuffer(raw("in32"), F32).reshape(h, w, 3)
    got = r.ambient_occlusion(fp, in32, want=("ao", "rgb32f", "rgba8"))
    raw8 = r.ambient_occlusion(fp, samples=8, radius=3.0, smooth=False)["ao"]
    white = r.ambient_occlusion(fp, strength=0.5, want=("rgb32f",))["rgb32f"]
    r.close()
    for k in ("ao", "rgb32f", "rgba8"):
        assert got[k].tobytes() == raw(k), k
    assert raw8.tobytes() == raw("raw8") and white.tobytes() == raw("white")
    assert (raw8 < 1).sum() > 20 and raw("rgb32f") != raw("in32")


# ---------------------------------------------------------------------------------------------------------------------
# 7. what the call costs

def _alternate(hip, stream, calls, rounds):
    """GPU time (ms, a HIP event pair on the context's stream) of each call of `calls`, alternating them `rounds` times after a
    warm-up round that is dropped."""
    a, b = hip.event(), hip.event()
    times = [[] for _ in calls]
    for k in range(rounds + 1):
        for i, call in enumerate(calls):
            hip.ok(hip.L.hipEventRecord(a, stream))
            call()
            hip.ok(hip.L.hipEventRecord(b, stream))
            hip.ok(hip.L.hipEventSynchronize(b))
            ms = C.c_float()
            hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
            if k:
                times[i].append(float(ms.value))
    for e in (a, b):
        hip.L.hipEventDestroy(e)
    return times


def test_the_call_costs_no_more_than_the_two_calls_it_replaces():
    """reference_scene() at 1920 x 1080, N = 4, radius 2, smooth = 0, device pointers: rz_ambient_occlusion (ao only) against the
    sum of rz_denoise with K = 0 and guides only and rz_shadow_rays on the identical rays -- the restatement's, built from those
    guides and already in device memory -- with the faster of its two scheduling flags.  The call runs the same walks and moves
    40 B per ray less (no 32-B ray read, no 8-B record written), so it must not take longer than the sum by more than the
    run-to-run spread.  The four calls alternate in one process, 25 rounds after a warm-up round, medians; the pair is measured
    twice and the spread is the larger relative difference between the two runs' medians of either side; the bound is
    max(1.10, 1 + spread) on the medians over both runs.  The figures this test printed are in profiles/ao/README.md.
    Measured: rz_ambient_occlusion 0.872 ms (runs 0.872, 0.873) against 0.115 + 0.738 = 0.852 ms (runs 0.854, 0.851), ratio
    1.023, spread 0.003, bound 1.10.  Three earlier forms missed the bound -- row-major lanes in the tile 1.46, lanes ordered by
    pattern with one counter for whole tiles 1.26, a fixed share of tiles per wave 1.25 (profiles/ao/README.md)."""
    hip = Hip()
    L = _lib.hip()
    sc = S.reference_scene()
    w, h, n, radius = 1920, 1080, 4, 2.0
    r = _setup(sc, w, h)
    d_guides, d_ao = hip.alloc(w * h * 48), hip.alloc(w * h * 4)
    r.denoise_device(guides_ptr=d_guides, iterations=0)
    r.sync()
    hits = np.frombuffer(hip.download(d_guides, w * h * 48).tobytes(), HIT_DTYPE)
    g = AR.guide_of_hits(hits, sc.camera, w, h)
    rays, walked = AR.sample_rays(g, n, radius)
    d_rays, d_vis = hip.upload(rays), hip.alloc(len(rays) * 8)
    stream = L.rz_stream_handle(r._c)
    calls = [lambda: r.ambient_occlusion_device(ao_ptr=d_ao, samples=n, radius=radius, smooth=False),
             lambda: r.denoise_device(guides_ptr=d_guides, iterations=0),
             lambda: r.shadow_rays_device(d_rays, d_vis, len(rays), incoherent=False),
             lambda: r.shadow_rays_device(d_rays, d_vis, len(rays), incoherent=True)]
    runs = [_alternate(hip, stream, calls, 25) for _ in range(2)]
    r.sync()
    got = np.frombuffer(hip.download(d_ao, w * h * 4).tobytes(), F32).reshape(h, w)
    vis = np.frombuffer(hip.download(d_vis, len(rays) * 8).tobytes(), VISIBILITY_DTYPE)
    r.close()
    hip.close()
    _same(got, AR.raw_image(g, AR.visibility_of(vis, walked)), "1920 x 1080 against the library's own queries")

    def sides(t):
        med = [float(np.median(x)) for x in t]
        return med[0], med[1] + min(med[2], med[3])

    (a1, b1), (a2, b2) = sides(runs[0]), sides(runs[1])
    spread = max(abs(a1 - a2) / min(a1, a2), abs(b1 - b2) / min(b1, b2))
    a, b = sides([x + y for x, y in zip(*runs)])
    med = [float(np.median(x + y)) for x, y in zip(*runs)]
    bound = max(1.10, 1.0 + spread)
    print(f"1920x1080 reference, N = {n}, {len(rays)} walks of {int(g.hit.sum())} hit pixels: rz_ambient_occlusion {a:.3f} ms "
          f"(runs {a1:.3f}, {a2:.3f}); guides {med[1]:.3f} + rz_shadow_rays {min(med[2], med[3]):.3f} (coherent {med[2]:.3f}, "
          f"incoherent {med[3]:.3f}) = {b:.3f} ms (runs {b1:.3f}, {b2:.3f}); ratio {a / b:.3f}; spread {spread:.3f}; bound {bound:.3f}")
    assert a <= bound * b, (runs[0][0], runs[1][0])

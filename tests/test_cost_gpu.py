"""The per-pixel traversal cost map on the GPU (rz_render_cost, rz_cost_view, rz_present_cost).  The records are integers and the
CPU oracle counts the same events, so they are compared for equality, pixel by pixel and counter by counter: the oracle's
single-pixel crops (cost_ref.oracle_records) are the reference.  The linear ramp and the statistics equal cost_ref bit for bit;
the logarithmic ramp is held to 1e-5 absolute (log2 on the device is good to about 1 ulp, so u is off by a few 1e-7; the ramp's
slope is at most 4 per unit u, so a channel is off by about 2e-6 at most; 1e-5 leaves a five-fold margin).  Measured on an MI355X
(printed by the view tests; profiles/cost/README.md): 4.77e-07 at worst."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cost_ref as CR
from helpers import oracle_scene
from oracle import rzo
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import PIXEL_COST_DTYPE, RayZenError, Renderer, frame_params
from refit_ref import wobble
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEGAKERNEL = 1                      # RZ_FLAG_MEGAKERNEL
METRICS = ("bytes", "nodes", "triangles", "traversals", "instances")
COUNTERS = _lib.COUNTER_FIELDS


def _setup(sc, w, h, spp, bounces, flags=0, render=False):
    r = Renderer(0, flags)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), bounces, spp))
    if render:
        r.render()
        r.sync()
    return r


def _assert_records(got, want, what):
    assert got.dtype == PIXEL_COST_DTYPE and got.shape == want.shape, what
    for f in CR.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert not len(bad), f"{what}: {f} differs on {len(bad)} pixels; first (y, x) {bad[0].tolist()}: {got[f][tuple(bad[0])]} != {want[f][tuple(bad[0])]}"


class _Arrays:
    """A scene as the context holds it now: the eight bindings read back, with the camera and lights of the scene it came from."""

    def __init__(self, r, sc):
        self.arrays = {b: r.read_binding(b) for b in S.BINDING_DTYPES}
        self.camera, self.lights = sc.camera, sc.lights


# ---------------------------------------------------------------------------------------------------------------------
# 1. the records are the oracle's single-pixel crops

@pytest.mark.parametrize("name", sorted(CR.CASES))
def test_records_equal_the_oracle_crops(name):
    sc, w, h, spp, bounces, want, total = CR.case(name)
    r = _setup(sc, w, h, spp, bounces)
    got, totals = r.render_cost(totals=True)
    r.close()
    _assert_records(got, want, name)
    assert {n: totals[n] for n in COUNTERS[:10]} == {n: total[n] for n in COUNTERS[:10]}


@pytest.mark.parametrize("w,h", [(1, 1), (9, 7), (65, 5)], ids=lambda v: str(v))
def test_records_on_partial_tiles(w, h):
    sc = CR.case("reference")[0]
    want, _ = CR.oracle_records(sc, w, h, 2, 5)
    r = _setup(sc, w, h, 2, 5)
    got = r.render_cost()
    again = r.render_cost(spp=2)                        # the frame's spp, stated
    one = r.render_cost(spp=1)
    r.close()
    _assert_records(got, want, f"{w}x{h}")
    assert again.tobytes() == got.tobytes()
    _assert_records(one, CR.oracle_records(sc, w, h, 1, 5)[0], f"{w}x{h} at 1 spp")


# ---------------------------------------------------------------------------------------------------------------------
# 2. totals

@pytest.mark.parametrize("name", ["bunny", "reference"])
def test_totals_equal_render_counted_and_the_column_sums(name):
    sc, w, h, spp, bounces, _, _ = CR.case(name)
    seen = []
    for flags in (0, MEGAKERNEL):
        r = _setup(sc, w, h, spp, bounces, flags)
        rec, totals = r.render_cost(totals=True)
        counted = r.render_counted()
        r.sync()
        r.close()
        assert totals == counted, (flags, totals, counted)
        for f in CR.FIELDS:
            assert totals[f] == int(rec[f].sum(dtype=np.uint64)), f
        assert totals["samples"] == w * h * spp and totals["pixels"] == w * h
        seen.append((rec.tobytes(), totals))
    assert seen[0] == seen[1]


# ---------------------------------------------------------------------------------------------------------------------
# 3. isolation

@pytest.mark.parametrize("flags", [0, MEGAKERNEL], ids=["samples", "pixels"])
def test_render_cost_leaves_the_render_state_alone(flags):
    sc, w, h, spp, bounces, want, _ = CR.case("reference")        # (its glass carries currentIor from chunk to chunk)
    nl = len(sc.lights)

    def run(with_cost):
        r = Renderer(0, flags)
        r.upload_scene(sc)
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, 0))
        r.render()
        first = r.read_accum()
        if with_cost:
            plan, kernel, ms = r.debug_last_plan(), r.last_kernel_name(), r.last_render_ms()
            _assert_records(r.render_cost(), want, "between two chunks")
            r.render_cost(spp=3)
            assert r.read_accum().tobytes() == first.tobytes()
            assert (r.debug_last_plan(), r.last_kernel_name(), r.last_render_ms()) == (plan, kernel, ms)
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, spp))
        r.render()
        r.sync()
        out = r.read_accum(), len(r.render_history_ms())
        r.close()
        return out

    plain, n_plain = run(False)
    mixed, n_mixed = run(True)
    assert mixed.tobytes() == plain.tobytes()
    assert n_mixed == n_plain == 2


# ---------------------------------------------------------------------------------------------------------------------
# 4. the cost follows edits

def test_records_after_update_transforms():
    sc, w, h, spp, bounces, before, _ = CR.case("instanced")
    r = _setup(sc, w, h, spp, bounces)
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(t, F32).reshape(16) for t in S.instanced_transforms(7, 16)])
    r.update_transforms(xf)
    got = r.render_cost()
    want, _ = CR.oracle_records(_Arrays(r, sc), w, h, spp, bounces)
    r.close()
    _assert_records(got, want, "after update_transforms")
    assert got.tobytes() != before.tobytes()


def test_records_after_a_refit():
    sc = S.bunny_scene(n=12, aspect=4 / 3)
    w, h, spp, bounces = 24, 18, 1, 3
    r = _setup(sc, w, h, spp, bounces)
    before = r.render_cost()
    _assert_records(before, CR.oracle_records(sc, w, h, spp, bounces)[0], "built")
    r.refit_geometry(wobble(S.make_blob(12, 2.8, 0), 0.5), first=12)
    got = r.render_cost()
    want, _ = CR.oracle_records(_Arrays(r, sc), w, h, spp, bounces)
    r.close()
    _assert_records(got, want, "after the refit")
    b0, b1 = (int(CR.value(x).sum()) for x in (before, got))
    print(f"frame bytes: built {b0}, wobbled and refitted {b1}")
    assert got.tobytes() != before.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the view

def _synthetic(h=19, w=70):
    """Zeros, ties for the maximum, values above 2^24, everything in between; 1330 pixels: more than one workgroup of the view
    kernel each way and two of the reduction's first stage (1024 pixels each)."""
    rng = np.random.default_rng(9)
    cols = rng.integers(0, 900, (h, w, 8)).astype(np.uint64)
    cols[0, :5] = 0
    cols[2, 3:9, 4] = (1 << 24) + np.arange(6)          # blas_nodes above 2^24
    cols[3, 7] = cols[6, 60] = cols[18, 69] = 0xFFFFFFF0    # ties for the maximum of every metric: (3, 7) has the lowest index
    return CR.records(cols)


def _check_view(r, rec, src, what):
    worst = 0.0
    for metric in METRICS:
        top = int(CR.value(rec, metric).max())
        for scale in (0.0, float(F32(top * 0.37)), float(F32(top) * F32(2))):
            got, st = r.cost_view(src, metric=metric, scale=scale, stats=True)
            want = CR.colour(rec, metric, "linear", scale)
            assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), f"{what}: {metric} scale {scale}: the linear ramp's bits"
            assert st == CR.stats(rec, metric, scale), f"{what}: {metric} scale {scale}: {st}"
            if 0 < scale < top:
                assert (got == 1).all(axis=-1).any()        # a caller scale below the maximum: white pixels
            log = r.cost_view(src, metric=metric, curve="log", scale=scale)
            err = float(np.abs(log.astype(np.float64) - CR.colour(rec, metric, "log", scale).astype(np.float64)).max())
            worst = max(worst, err)
            assert err <= 1e-5, f"{what}: {metric} scale {scale}: the log ramp is off by {err:.3g}"
    print(f"{what}: worst absolute error of the logarithmic ramp {worst:.3g}")
    return worst


def test_view_matches_the_restatement_on_gpu_made_records():
    sc, w, h, spp, bounces, want, _ = CR.case("bunny")
    r = _setup(sc, w, h, spp, bounces)
    rec = r.render_cost()
    _assert_records(rec, want, "bunny")
    _check_view(r, rec, None, "the context's map")
    _check_view(r, rec, rec, "the same map handed over")
    r.close()


def test_view_matches_the_restatement_on_synthetic_records():
    rec = _synthetic()
    h, w = rec.shape
    sc = S.cornell_scene()
    r = _setup(sc, w, h, 1, 1)
    st = CR.stats(rec)
    assert (st["max_x"], st["max_y"]) == (7, 3) and st["max_value"] > (1 << 32)
    _check_view(r, rec, rec, "synthetic")
    zero = np.zeros((h, w), PIXEL_COST_DTYPE)
    for metric in METRICS:
        got, st = r.cost_view(zero, metric=metric, stats=True)
        assert st == CR.stats(zero, metric) and got.tobytes() == CR.colour(zero, metric).tobytes(), metric
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. present_cost

def test_present_cost_matches_the_oracle_present_of_the_heat_map():
    sc, w, h, spp, bounces, _, _ = CR.case("bunny")
    r = _setup(sc, w, h, spp, bounces, render=True)
    acc = r.read_accum()
    r.render_cost()
    osc = oracle_scene(sc)
    for view in (dict(), dict(metric="nodes", scale=50.0), dict(metric="triangles", curve="log")):
        heat = r.cost_view(**view)
        as_accum = np.concatenate([heat, np.ones((h, w, 1), F32)], axis=-1)
        for kw in (dict(show_fps=False), dict(fps=48.5, show_fps=True, show_lights=True, show_bvh=True),
                   dict(show_fps=False, show_bvh=True, bvh_mode=1, selected_blas=1, selected_tri=5)):
            rgb, rgba8 = r.present_cost(**view, **kw)
            want_rgb, want_rgba8 = rzo.present(osc, as_accum, sc.camera.view, sc.camera.proj, len(sc.lights), **kw)
            assert rgb.view(np.uint32).tobytes() == want_rgb.view(np.uint32).tobytes(), (view, kw)
            assert rgba8.tobytes() == want_rgba8.tobytes(), (view, kw)
        assert r.present_cost(**view, show_fps=False)[0].tobytes() == heat.tobytes()
    assert r.read_accum().tobytes() == acc.tobytes()
    assert r.present(show_fps=False)[0].tobytes() != r.present_cost(show_fps=False)[0].tobytes()
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. host and device pointers

def test_host_and_device_paths_give_the_same_bytes():
    hip = Hip()
    sc, w, h, spp, bounces, want, _ = CR.case("bunny")
    n = w * h
    r = _setup(sc, w, h, spp, bounces)
    host, host_totals = r.render_cost(totals=True)
    d_cost = hip.alloc(n * 32, 0x5A)
    assert r.render_cost_device(d_cost, totals=True) == host_totals
    r.sync()
    assert hip.download(d_cost, n * 32).tobytes() == host.tobytes()
    # cost = None keeps the context's copy, and cost_view finds it
    r2 = _setup(sc, w, h, spp, bounces)
    assert r2.render_cost_device(None) is None
    r2.sync()
    assert r2.cost_view(metric="nodes").tobytes() == r.cost_view(host, metric="nodes").tobytes()
    r2.close()
    # the view: device cost in, device colour and statistics out
    d_rgb, d_stats = hip.alloc(n * 12, 0x5A), hip.alloc(32, 0x5A)
    for src in (d_cost, None):
        r.cost_view_device(d_rgb, d_stats, src, metric="triangles", curve="log", scale=30.0)
        r.sync()
        rgb, st = r.cost_view(host, metric="triangles", curve="log", scale=30.0, stats=True)
        assert hip.download(d_rgb, n * 12).tobytes() == rgb.tobytes()
        ds = _lib.CostStats.from_buffer_copy(hip.download(d_stats, 32).tobytes())
        assert (ds.max_value, ds.sum_value, ds.max_x, ds.max_y, ds.scale_used, ds.reserved) == \
               (st["max_value"], st["sum_value"], st["max_x"], st["max_y"], st["scale_used"], 0)
    # each output alone
    hip.ok(hip.L.hipMemset(C.c_void_p(d_rgb), 0x5A, n * 12))
    r.cost_view_device(None, d_stats, None)
    r.sync()
    assert (hip.download(d_rgb, n * 12) == 0x5A).all()
    assert _lib.CostStats.from_buffer_copy(hip.download(d_stats, 32).tobytes()).sum_value == CR.stats(want)["sum_value"]
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 16, 8
    n = w * h
    r = _setup(sc, w, h, 1, 2)
    d_cost, d_rgb, d_stats = hip.alloc(n * 32 + 16, 0x5A), hip.alloc(n * 12 + 16, 0x5A), hip.alloc(48, 0x5A)
    totals = _lib.Counters()

    def cost(ctx, params=None, args=None, flags=0, tot=None):
        return L.rz_render_cost(ctx, params, *(args if args is not None else (d_cost, n * 32)), tot, flags)

    def view(ctx, params=None, args=None, flags=0):
        return L.rz_cost_view(ctx, params, *(args if args is not None else (d_cost, n * 32, d_rgb, n * 12, d_stats)), flags)

    def cp(spp=0, reserved=None):
        p = _lib.CostParams(spp)
        if reserved is not None:
            p.reserved[reserved] = 1
        return C.byref(p)

    def vp(metric=0, curve=0, scale=0.0, reserved=None):
        p = _lib.CostViewParams(metric, curve, scale)
        if reserved is not None:
            p.reserved[reserved] = 1
        return C.byref(p)

    nan, inf = float("nan"), float("inf")
    # before any rz_render_cost: nothing to view
    assert view(r._c, args=(None, 0, d_rgb, n * 12, d_stats)) == -5 and b"rz_render_cost has not been called" in L.rz_last_error(r._c)
    pp = _lib.PresentParams()
    buf8, buf32 = np.zeros(n * 4, np.uint8), np.zeros(n * 3, F32)

    def present(ctx, present_p=C.byref(pp), params=None, n8=buf8.nbytes, n32=buf32.nbytes):
        return L.rz_present_cost(ctx, present_p, params, buf8.ctypes.data, n8, buf32.ctypes.data, n32)

    assert present(r._c) == -5
    # invalid arguments
    assert cost(None) == -1 and view(None) == -1 and present(None) == -1 and present(r._c, present_p=None) == -1
    for spp in (-1, 1025, 1 << 20):
        assert cost(r._c, cp(spp)) == -1, spp
    for k in range(7):
        assert cost(r._c, cp(reserved=k)) == -1, k
    for k in range(5):
        assert view(r._c, vp(reserved=k)) == -1 and present(r._c, params=vp(reserved=k)) == -1, k
    for bad in (dict(metric=-1), dict(metric=5), dict(curve=-1), dict(curve=2), dict(scale=-1.0), dict(scale=nan), dict(scale=inf),
                dict(scale=-inf)):
        assert view(r._c, vp(**bad)) == -1 and present(r._c, params=vp(**bad)) == -1, bad
    assert cost(r._c, flags=2) == -1 and cost(r._c, flags=0x80000000) == -1 and view(r._c, flags=4) == -1
    assert cost(r._c, args=(d_cost + 8, n * 32)) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert view(r._c, args=(d_cost + 8, n * 32, d_rgb, n * 12, d_stats)) == -1
    assert view(r._c, args=(d_cost, n * 32, d_rgb + 2, n * 12, d_stats)) == -1
    assert view(r._c, args=(d_cost, n * 32, d_rgb, n * 12, d_stats + 4)) == -1
    # buffers too small
    assert cost(r._c, args=(d_cost, n * 32 - 1)) == -7
    assert view(r._c, args=(d_cost, n * 32 - 1, d_rgb, n * 12, d_stats)) == -7
    assert view(r._c, args=(d_cost, n * 32, d_rgb, n * 12 - 1, d_stats)) == -7
    host_cost = np.full(n, 0x5A5A5A5A, np.uint32).repeat(8)
    assert L.rz_render_cost(r._c, None, host_cost.ctypes.data, n * 32 - 1, C.byref(totals), _lib.COST_HOST) == -7
    assert (host_cost == 0x5A5A5A5A).all() and totals.samples == 0
    # nothing was launched, nothing was kept
    r.sync()
    for ptr, nb in ((d_cost, n * 32 + 16), (d_rgb, n * 12 + 16), (d_stats, 48)):
        assert (hip.download(ptr, nb) == 0x5A).all()
    assert view(r._c, args=(None, 0, d_rgb, n * 12, d_stats)) == -5
    assert not buf8.any() and not buf32.any()
    # the context stays usable
    assert cost(r._c, tot=C.byref(totals)) == 0 and totals.pixels == n and view(r._c, args=(None, 0, d_rgb, n * 12, d_stats)) == 0
    assert present(r._c) == 0 and buf8.any()
    assert present(r._c, n8=n * 4 - 1) == -7 and present(r._c, n32=n * 12 - 1) == -7
    r.sync()
    assert (hip.download(d_cost, n * 32 + 16)[n * 32:] == 0x5A).all() and (hip.download(d_rgb, n * 12 + 16)[n * 12:] == 0x5A).all()
    # a resolution change: the kept map is of another size
    r.set_frame(frame_params(sc.camera, w, h + 1, 2, 2, 1))
    assert view(r._c, args=(None, 0, None, 0, d_stats)) == -5 and b"16x8" in L.rz_last_error(r._c)
    assert present(r._c, n8=(n + w) * 4, n32=0) == -5
    r.set_frame(frame_params(sc.camera, w, h, 2, 2, 1))
    assert view(r._c, args=(None, 0, None, 0, d_stats)) == 0
    # a tile of a group frame: refused
    r.set_frame(frame_params(sc.camera, w, h, 2, 2, 1, 0, 0, 2))
    assert cost(r._c) == -1 and b"whole frame" in L.rz_last_error(r._c)
    assert view(r._c) == -1 and present(r._c) == -1
    r.sync()
    r.close()
    # no frame / no scene / no materials
    nof = Renderer(0)
    nof.upload_scene(sc)
    assert cost(nof._c) == -5 and view(nof._c) == -5 and present(nof._c) == -5
    nof.close()
    empty = Renderer(0)
    empty.set_frame(frame_params(sc.camera, w, h, 2, 2, 1))
    assert cost(empty._c) == -5
    empty.close()
    nomat = Renderer(0)
    for b in S.BINDING_DTYPES:
        nomat.upload(b, sc.arrays[b][:0] if b == S.BIND_MATERIALS else sc.arrays[b])
    nomat.set_frame(frame_params(sc.camera, w, h, 2, 2, 1))
    assert cost(nomat._c) == -5 and b"material" in L.rz_last_error(nomat._c)
    nomat.close()
    hip.close()


def test_backstop_host_path_reports_and_device_path_leaves_it_to_sync():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 16, 8
    r = _setup(sc, w, h, 1, 2)
    before = r.render_cost()
    r.sync()
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    with pytest.raises(RayZenError) as e:
        r.render_cost()
    message = str(e.value).split("): ", 1)[1]
    assert e.value.code == -9 and message.startswith("rz_render_cost: ") and "0x8" in message, str(e.value)
    r.sync()                                            # reported once, then clear
    assert r.render_cost().tobytes() == before.tobytes()
    # the device path returns at once and leaves the word to rz_sync
    d_cost = hip.alloc(w * h * 32, 0)
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    r.render_cost_device(d_cost)
    with pytest.raises(RayZenError) as e:
        r.sync()
    assert e.value.code == -9
    r.sync()
    assert hip.download(d_cost, w * h * 32).tobytes() == before.tobytes()
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the C++ front end

def test_cpp_free_functions_equal_the_python_binding(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    exe = str(tmp_path / "cost_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rayzen_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "cost_driver.cpp"), "-L", lib, "-lrayzen_host", "-lrayzen_hip",
                           f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"cost_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    fp = _lib.FrameParams.from_buffer_copy(raw("frame"))
    w, h = fp.width, fp.height
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt))
    r.set_frame(fp)
    rec, totals = r.render_cost(totals=True)
    assert rec.tobytes() == raw("cost") and len(raw("cost")) == w * h * 32
    ct = _lib.Counters.from_buffer_copy(raw("totals"))
    assert {n: int(getattr(ct, n)) for n in COUNTERS} == totals and totals["pixels"] == w * h
    rgb, st = r.cost_view(stats=True)
    assert rgb.tobytes() == raw("view")
    cs = _lib.CostStats.from_buffer_copy(raw("stats"))
    assert (cs.max_value, cs.sum_value, cs.max_x, cs.max_y, cs.scale_used) == (st["max_value"], st["sum_value"], st["max_x"], st["max_y"], st["scale_used"])
    assert st == CR.stats(rec)
    assert r.cost_view(rec, metric="nodes", curve="log", scale=40.0).tobytes() == raw("view_log")
    _, rgba8 = r.present_cost(metric="nodes", curve="log", scale=40.0, fps=59.5, show_fps=True, show_lights=True, show_bvh=True)
    assert rgba8.tobytes() == raw("present")
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. what the call costs

def test_render_cost_takes_at_most_twice_the_counted_pixel_render():
    """bunny_scene(n=76) at 480 x 270, 1 spp: the GPU time of rz_render_cost (a HIP event pair on the context's stream) against
    rz_last_render_ms of rz_render_counted in a RZ_FLAG_MEGAKERNEL context -- the same path loop, which only adds its tallies to
    the frame's counters.  The cost kernel stores 32 B per pixel on top; more than twice the time would mean that its path loop
    was compiled into something else.  Measured: profiles/cost/README.md."""
    hip = Hip()
    L = _lib.hip()
    sc = S.bunny_scene(n=76)
    w, h, bounces = 480, 270, 4
    r = _setup(sc, w, h, 1, bounces, MEGAKERNEL)
    stream = L.rz_stream_handle(r._c)
    a, b = hip.event(), hip.event()
    cost_ms, counted_ms = [], []
    for k in range(4):                                  # (the first round warms both up and is dropped)
        hip.ok(hip.L.hipEventRecord(a, stream))
        r.render_cost_device(None)
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        r.clear_accum()
        r.render_counted()
        r.sync()
        if k:
            cost_ms.append(float(ms.value))
            counted_ms.append(r.last_render_ms()[0])
    r.close()
    for e in (a, b):
        hip.L.hipEventDestroy(e)
    hip.close()
    c, m = float(np.median(cost_ms)), float(np.median(counted_ms))
    print(f"480x270, 1 spp, {bounces} bounces, bunny 69 312: rz_render_cost {c:.3f} ms {cost_ms}, rz_render_counted (pixel kernel) {m:.3f} ms {counted_ms}; ratio {c / m:.2f}")
    assert c <= 2.0 * m, (cost_ms, counted_ms)

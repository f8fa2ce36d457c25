"""rz_render_adaptive on the GPU.  The render kernels are rz_render's own and a path's arithmetic does not depend on the launch that
runs it, so everything is compared for equality: the accumulation (rgb and a), the per-tile batches and errors and the per-batch
records against the restatement (adaptive_ref.py: the CPU oracle driven batch by batch, the meter in np.float32, the plan in plain
Python), and -- independently of the rule -- every pixel against the oracle's one-shot frame at that pixel's own sample count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as AR
from helpers import oracle_frame, oracle_scene
from oracle import rzo
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import RayZenError, Renderer, frame_params
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEGAKERNEL = 1                      # RZ_FLAG_MEGAKERNEL
RECORDS = ("batches", "tiles_active", "tiles_rendered", "runs", "samples_traced", "samples_uniform")


def _setup(sc, w, h, bounces, flags=0, spp=3, sample_base=0):
    """(the frame's spp and sample_base are there to be ignored)"""
    r = Renderer(0, flags)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), bounces, spp, sample_base))
    return r


def _kw(over):
    return {**AR.SETTINGS, **over}


def _assert_equals(got, want, what):
    info, batches, error, accum = got
    assert accum.view(np.uint32).tobytes() == want["accum"].view(np.uint32).tobytes(), f"{what}: the accumulation"
    assert batches.dtype == np.int32 and batches.tobytes() == want["tile_batches"].tobytes(), f"{what}: tile_batches"
    assert error.dtype == F32 and error.view(np.uint32).tobytes() == want["tile_error"].view(np.uint32).tobytes(), f"{what}: tile_error"
    assert {k: info[k] for k in RECORDS} == {k: want[k] for k in RECORDS}, f"{what}: the records"
    assert info["n_tiles"] == batches.size and info["render_ms"] > 0 and info["meter_ms"] >= 0


def _both_forms_both_backends(sc, w, h, bounces, want, what, **kw):
    hip = Hip()
    n = ((w + 7) // 8) * ((h + 7) // 8)
    for flags in (0, MEGAKERNEL):
        r = _setup(sc, w, h, bounces, flags)
        info, batches, error = r.render_adaptive(**kw)
        _assert_equals((info, batches, error, r.read_accum()), want, f"{what}, flags {flags}, host form")
        r.clear_accum()
        d_b, d_e = hip.alloc(n * 4 + 16, 0x5A), hip.alloc(n * 4 + 16, 0x5A)
        info = r.render_adaptive_device(d_b, d_e, **kw)
        got_b, got_e = hip.download(d_b, n * 4 + 16), hip.download(d_e, n * 4 + 16)
        assert (got_b[n * 4:] == 0x5A).all() and (got_e[n * 4:] == 0x5A).all()
        shape = want["tile_batches"].shape
        _assert_equals((info, np.frombuffer(got_b[:n * 4].tobytes(), np.int32).reshape(shape),
                        np.frombuffer(got_e[:n * 4].tobytes(), F32).reshape(shape), r.read_accum()), want, f"{what}, flags {flags}, device form")
        r.sync()
        r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement, bit for bit

@pytest.mark.parametrize("s", [4, 1])
@pytest.mark.parametrize("name", ["cornell", "bunny", "reference"])
def test_equals_the_restatement(name, s):
    sc, w, h, bounces, want = AR.case(name, batch_spp=s)
    kw = _kw(dict(batch_spp=s, threshold=AR.THRESHOLD[name]))
    _both_forms_both_backends(sc, w, h, bounces, want, f"{name}, s = {s}", **kw)


@pytest.mark.parametrize("s", [4, 1])
@pytest.mark.parametrize("w,h", [(1, 1), (9, 7), (65, 5)], ids=lambda v: str(v))
def test_equals_the_restatement_on_partial_tiles(w, h, s):
    """A frame of one pixel, one of four partial tiles and one of nine tiles in a row, the last a column of 1 x 5 pixels."""
    sc, _, _, bounces, want = AR.case("reference", size=(w, h), batch_spp=s, merge_gap=0)
    _both_forms_both_backends(sc, w, h, bounces, want, f"{w}x{h}, s = {s}", **_kw(dict(batch_spp=s, merge_gap=0)))


def test_equals_the_restatement_with_several_runs_per_batch():
    sc, w, h, bounces, want = AR.case("cornell", merge_gap=0)
    assert max(want["runs"]) >= 5
    _both_forms_both_backends(sc, w, h, bounces, want, "cornell unmerged", **_kw(dict(merge_gap=0)))
    # max_runs 2 merges across gaps of any length
    sc, w, h, bounces, want = AR.case("cornell", merge_gap=0, max_runs=2)
    assert max(want["runs"]) == 2
    r = _setup(sc, w, h, bounces)
    info, batches, error = r.render_adaptive(**_kw(dict(merge_gap=0, max_runs=2)))
    _assert_equals((info, batches, error, r.read_accum()), want, "cornell, max_runs 2")
    r.close()


class _Arrays:
    """A scene as the context holds it now: the eight bindings read back, with the camera and lights of the scene it came from."""

    def __init__(self, r, sc):
        self.arrays = {b: r.read_binding(b) for b in S.BINDING_DTYPES}
        self.camera, self.lights = sc.camera, sc.lights


def test_after_update_transforms():
    sc = S.instanced_scene(n=8, count=16, aspect=16 / 9)
    w, h, bounces = 48, 27, 3
    kw = _kw(dict(merge_gap=1))
    r = _setup(sc, w, h, bounces)
    before = r.render_adaptive(**kw)[1]
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(t, F32).reshape(16) for t in S.instanced_transforms(7, 16)])
    r.update_transforms(xf)
    info, batches, error = r.render_adaptive(**kw)
    accum = r.read_accum()
    now = _Arrays(r, sc)
    r.close()
    want = AR.render_adaptive(now, w, h, bounces, **kw)
    _assert_equals((info, batches, error, accum), want, "after update_transforms")
    assert len(set(batches.ravel().tolist())) >= 2 and before.shape == batches.shape


# ---------------------------------------------------------------------------------------------------------------------
# 2. independently of the rule: every pixel is the one-shot frame at its own sample count

@pytest.mark.parametrize("flags", [0, MEGAKERNEL], ids=["samples", "pixels"])
@pytest.mark.parametrize("name", ["cornell", "bunny", "reference"])
def test_every_pixel_is_the_oracles_frame_at_its_own_spp(name, flags):
    sc, w, h, bounces = AR.scene(name)
    r = _setup(sc, w, h, bounces, flags)
    info, batches, _ = r.render_adaptive(**_kw(dict(threshold=AR.THRESHOLD[name], merge_gap=1)))
    accum = r.read_accum()
    r.close()
    spp = AR.pixel_spp(accum)
    assert (spp == np.repeat(np.repeat(batches, 8, axis=0), 8, axis=1)[:h, :w] * 4).all()
    assert len(np.unique(spp)) >= 2 and int(spp.sum()) == info["samples_traced"]
    want = AR.one_shot_at_own_spp(sc, w, h, bounces, accum)
    assert accum.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. anchors

def _oracle(sc, w, h, spp, bounces):
    return rzo.render(oracle_scene(sc), oracle_frame(sc, w, h, spp, bounces), nthreads=8)


@pytest.mark.parametrize("name", ["cornell", "reference"])
def test_anchor_no_tile_retires(name):
    """threshold -1: rz_render chunked at s up to max_batches * s, and the oracle at that spp."""
    sc, w, h, bounces = AR.scene(name)
    r = _setup(sc, w, h, bounces)
    info, batches, _ = r.render_adaptive(batch_spp=4, min_batches=2, max_batches=5, threshold=-1.0)
    got = r.read_accum()
    assert info["batches"] == 5 and info["tiles_active"] == [batches.size] * 5 and info["runs"] == [1] * 5
    assert info["samples_traced"] == info["samples_uniform"] == w * h * 20 and (batches == 5).all()
    r.render_scene(sc, w, h, 20, bounces, chunk=4)
    chunked = r.read_accum()
    r.close()
    assert got.tobytes() == chunked.tobytes()
    assert got.view(np.uint32).tobytes() == _oracle(sc, w, h, 20, bounces).view(np.uint32).tobytes()


def test_anchor_every_tile_retires_at_min_batches():
    sc, w, h, bounces = AR.scene("reference")
    r = _setup(sc, w, h, bounces)
    info, batches, error = r.render_adaptive(batch_spp=4, min_batches=3, max_batches=8, threshold=float("inf"))
    got = r.read_accum()
    r.close()
    assert info["batches"] == 3 and info["tiles_active"] == [batches.size, batches.size, 0] and (batches == 3).all()
    assert np.isfinite(error).all()
    assert got.view(np.uint32).tobytes() == _oracle(sc, w, h, 12, bounces).view(np.uint32).tobytes()


def test_anchor_the_merge_gap_changes_only_the_sample_counts():
    sc, w, h, bounces = AR.scene("cornell")
    outs = []
    for gap in (0, 1000):
        r = _setup(sc, w, h, bounces)
        info, batches, _ = r.render_adaptive(**_kw(dict(merge_gap=gap)))
        accum = r.read_accum()
        r.close()
        want = AR.one_shot_at_own_spp(sc, w, h, bounces, accum)
        assert accum.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), gap
        outs.append((info, batches, accum))
    (i0, b0, a0), (i1, b1, a1) = outs
    assert i0["tiles_active"] == i1["tiles_active"]         # who retires does not depend on the plan
    assert (b0 <= b1).all() and (b0 < b1).any() and set(i1["runs"]) == {1} and max(i0["runs"]) >= 5
    same = a0[..., 3] == a1[..., 3]
    assert a0[same].tobytes() == a1[same].tobytes() and not same.all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. presenting an adaptive accumulation; a bound accumulation

def test_present_and_present_display_divide_per_pixel():
    sc, w, h, bounces, want = AR.case("bunny")
    r = _setup(sc, w, h, bounces)
    r.render_adaptive(**_kw(dict(threshold=AR.THRESHOLD["bunny"])))
    accum = r.read_accum()
    assert len(np.unique(accum[..., 3])) >= 3
    kw = dict(fps=57.3, show_fps=True, show_lights=True, show_bvh=True)
    rgb, rgba8 = r.present(**kw)
    rgb_d, rgba8_d = r.present_display(**kw)
    resolved = r.resolve_rgba8()
    r.close()
    want_rgb, want_8 = rzo.present(oracle_scene(sc), accum, sc.camera.view, sc.camera.proj, len(sc.lights), **kw)
    assert rgb.view(np.uint32).tobytes() == want_rgb.view(np.uint32).tobytes() and rgba8.tobytes() == want_8.tobytes()
    assert rgb_d.tobytes() == rgb.tobytes() and rgba8_d.tobytes() == rgba8.tobytes()
    want = np.rint(np.clip(accum[..., :3] / accum[..., 3:4], 0.0, 1.0) * F32(255.0)).astype(np.uint8)      # (as test_resolve_rgba8)
    assert (resolved[..., :3] == want).all() and (resolved[..., 3] == 255).all()


def test_a_bound_accumulation():
    hip = Hip()
    sc, w, h, bounces, want = AR.case("cornell")
    r = _setup(sc, w, h, bounces)
    d = hip.alloc(w * h * 16 + 16, 0x5A)
    r.bind_accum(d, w * h * 16)
    info, batches, error = r.render_adaptive(**_kw({}))
    got = hip.download(d, w * h * 16 + 16)
    assert (got[w * h * 16:] == 0x5A).all()
    _assert_equals((info, batches, error, np.frombuffer(got[:w * h * 16].tobytes(), F32).reshape(h, w, 4)), want, "bound accumulation")
    r.bind_accum(d, w * h * 16 - 1)
    with pytest.raises(RayZenError) as e:
        r.render_adaptive()
    assert e.value.code == -7
    r.bind_accum(None, 0)
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. isolation, determinism

@pytest.mark.parametrize("flags", [0, MEGAKERNEL], ids=["samples", "pixels"])
def test_the_call_leaves_temporal_display_and_frame_alone_and_a_render_follows_as_on_a_fresh_context(flags):
    sc, w, h, bounces = AR.scene("reference")                # (its glass carries currentIor from chunk to chunk)
    nl = len(sc.lights)
    spp = 3

    def state(r):
        d = r.display_state()
        return (b"".join(r.debug_read_temporal(k).tobytes() for k in range(5)),
                b"".join(np.asarray(d[k]).tobytes() for k in sorted(d)))

    def run(with_call):
        r = Renderer(0, flags)
        r.upload_scene(sc)
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, 0))
        r.render()
        r.denoise_temporal()
        r.display(auto=True, curve="reinhard")
        if with_call:
            before, frame = state(r), bytes(r._frame)
            r.render_adaptive(**_kw({}))
            assert state(r) == before and bytes(r._frame) == frame and (r.width, r.height) == (w, h)
        # the frame of rz_set_frame is still the one set: its spp and sample_base decide this render
        r.render()
        first = r.read_accum()
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, spp))
        r.render()
        r.sync()
        out = first, r.read_accum(), len(r.render_history_ms()), r.denoise_temporal(), r.display(auto=True, curve="reinhard")[1], state(r)
        r.close()
        return out

    plain, mixed = run(False), run(True)
    assert mixed[0].tobytes() == plain[0].tobytes() and mixed[1].tobytes() == plain[1].tobytes()
    assert mixed[2] == plain[2] == 3                        # the ring of render times holds the renders only
    assert mixed[3].tobytes() == plain[3].tobytes() and mixed[4].tobytes() == plain[4].tobytes() and mixed[5] == plain[5]
    assert plain[0].view(np.uint32).tobytes() == _oracle(sc, w, h, spp, bounces).view(np.uint32).tobytes()


def test_two_runs_give_the_same_bytes():
    sc, w, h, bounces = AR.scene("bunny")
    r = _setup(sc, w, h, bounces)
    outs = []
    for _ in range(2):
        info, batches, error = r.render_adaptive(**_kw(dict(threshold=AR.THRESHOLD["bunny"], merge_gap=1)))
        outs.append(({k: info[k] for k in RECORDS}, batches.tobytes(), error.tobytes(), r.read_accum().tobytes()))
    # ... and after a frame of another size in between (the per-pixel state is the call's own: it starts afresh)
    r.set_frame(frame_params(sc.camera, 24, 16, len(sc.lights), bounces, 1))
    r.render_adaptive(batch_spp=1, min_batches=2, max_batches=3)
    r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), bounces, 1))
    info, batches, error = r.render_adaptive(**_kw(dict(threshold=AR.THRESHOLD["bunny"], merge_gap=1)))
    outs.append(({k: info[k] for k in RECORDS}, batches.tobytes(), error.tobytes(), r.read_accum().tobytes()))
    r.close()
    assert outs[0] == outs[1] == outs[2]


def test_the_defaults():
    sc, w, h, bounces = AR.scene("cornell")
    r = _setup(sc, w, h, bounces)
    info, batches, error = r.render_adaptive()
    accum = r.read_accum()
    r.close()
    want = AR.render_adaptive(sc, w, h, bounces, **AR.DEFAULTS)
    _assert_equals((info, batches, error, accum), want, "defaults")


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors and the backstop word

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h, n = 20, 12, 6
    r = _setup(sc, w, h, 2)
    d_b, d_e = hip.alloc(n * 4 + 16, 0x5A), hip.alloc(n * 4 + 16, 0x5A)

    def call(ctx, p=None, tb=d_b, tb_bytes=n * 4, te=d_e, te_bytes=n * 4, **fields):
        if fields:
            p = _lib.AdaptiveParams()
            for k, v in fields.items():
                setattr(p, k, v)
        return L.rz_render_adaptive(ctx, None if p is None else C.byref(p), None, tb, tb_bytes, te, te_bytes)

    nan, inf = float("nan"), float("inf")
    assert call(None) == -1
    for bad in (dict(flags=2), dict(flags=0x80000000), dict(batch_spp=-1), dict(batch_spp=1025), dict(min_batches=1), dict(min_batches=-2),
                dict(min_batches=65), dict(max_batches=3), dict(min_batches=6, max_batches=5), dict(max_batches=65), dict(max_batches=-1),
                dict(threshold=nan), dict(luminance_floor=-0.01), dict(luminance_floor=inf), dict(luminance_floor=nan), dict(merge_gap=-2),
                dict(max_runs=-1)):
        assert call(r._c, **bad) == -1, bad
    assert b"max_runs" in L.rz_last_error(r._c)
    assert call(r._c, tb=d_b + 2) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert call(r._c, te=d_e + 1) == -1
    assert call(r._c, tb_bytes=n * 4 - 1) == -7 and b"tile_batches" in L.rz_last_error(r._c)
    assert call(r._c, te_bytes=n * 4 - 1) == -7 and b"tile_error" in L.rz_last_error(r._c)
    host = np.full(n, 0x5A5A5A5A, np.int32)
    assert call(r._c, tb=host.ctypes.data, tb_bytes=n * 4 - 1, te=None, te_bytes=0, flags=_lib.ADAPTIVE_HOST) == -7
    assert (host == 0x5A5A5A5A).all()
    # a frame that is one of several tile ranks
    r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), 2, 1, 0, 1, 2))
    assert call(r._c) == -1 and b"tile 1 of 2" in L.rz_last_error(r._c)
    r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), 2, 1))
    # nothing was launched: the accumulation is as set_frame left it, the buffers untouched
    assert not r.read_accum().any()
    assert (hip.download(d_b, n * 4 + 16) == 0x5A).all() and (hip.download(d_e, n * 4 + 16) == 0x5A).all()
    # the context stays usable; both outputs are optional; nothing is written past the buffers
    assert call(r._c) == 0
    assert call(r._c, tb=None, tb_bytes=0, te=None, te_bytes=0) == 0
    assert call(r._c, threshold=inf) == 0 and call(r._c, threshold=-inf) == 0 and call(r._c, merge_gap=-1, max_runs=1) == 0
    assert (hip.download(d_b, n * 4 + 16)[n * 4:] == 0x5A).all() and (hip.download(d_e, n * 4 + 16)[n * 4:] == 0x5A).all()
    r.close()
    # before rz_set_frame; without a scene
    fresh = Renderer(0)
    fresh.upload_scene(sc)
    assert call(fresh._c) == -5 and b"rz_set_frame" in L.rz_last_error(fresh._c)
    fresh.close()
    empty = Renderer(0)
    empty.set_frame(frame_params(sc.camera, w, h, 2, 2, 1))
    assert call(empty._c) == -5
    empty.close()
    hip.close()


def test_the_backstop_word_is_left_to_sync_as_in_render():
    L = _lib.hip()
    sc, w, h, bounces, want = AR.case("cornell")
    r = _setup(sc, w, h, bounces)
    r.render()
    r.sync()
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    info, batches, error = r.render_adaptive(**_kw({}))     # returns as rz_render does
    _assert_equals((info, batches, error, r.read_accum()), want, "with the word set")
    with pytest.raises(RayZenError) as e:
        r.sync()
    assert e.value.code == -9
    r.sync()                                                # reported once, then clear
    r.close()


def test_a_tile_with_non_finite_samples_stays_active_to_the_end():
    """The NaN-ior scene of test_nonfinite_gpu.py: NaN reaches the accumulation of some pixels.  With threshold +inf every tile of
    finite samples retires at min_batches; a tile that holds a NaN pixel has E = NaN, for which `E <= threshold` is false, and is
    sampled until max_batches.  Tiles, records and the finite pixels equal the restatement bit for bit; a NaN is a NaN there too."""
    sc = S.bunny_scene(n=8, bunny_material=3, floor_material=0)
    sc.materials["ior"][3] = np.nan
    w, h, bounces = 48, 28, 5
    kw = dict(batch_spp=2, min_batches=2, max_batches=4, threshold=float("inf"), merge_gap=0, max_runs=64)
    want = AR.render_adaptive(sc, w, h, bounces, luminance_floor=0.01, **kw)
    bad = ~np.isfinite(want["accum"]).all(-1)
    bad_tiles = np.array([[bad[y:y + 8, x:x + 8].any() for x in range(0, w, 8)] for y in range(0, h, 8)])
    print(f"NaN-ior frame: {int(bad.sum())} bad pixels in {int(bad_tiles.sum())} of {bad_tiles.size} tiles; runs {want['runs']}")
    assert 0 < bad_tiles.sum() < bad_tiles.size
    for flags in (0, MEGAKERNEL):
        r = _setup(sc, w, h, bounces, flags)
        info, batches, error = r.render_adaptive(**kw)
        accum = r.read_accum()
        r.close()
        assert (batches[bad_tiles] == 4).all() and (batches[~bad_tiles] <= 4).all() and (batches == 2).any(), flags
        assert np.isnan(error[bad_tiles]).all() and np.isfinite(error[~bad_tiles]).all(), flags
        assert info["tiles_active"][-1] == int(bad_tiles.sum()) and info["batches"] == 4
        assert batches.tobytes() == want["tile_batches"].tobytes() and {k: info[k] for k in RECORDS} == {k: want[k] for k in RECORDS}
        assert np.array_equal(np.isnan(accum), np.isnan(want["accum"]))
        good = np.isfinite(want["accum"])
        assert accum[good].tobytes() == want["accum"][good].tobytes()
        assert np.array_equal(np.isnan(error), np.isnan(want["tile_error"]))
        ok = ~np.isnan(error)
        assert error[ok].tobytes() == want["tile_error"][ok].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the C++ front end

def test_cpp_free_functions_equal_the_python_binding(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    exe = str(tmp_path / "adaptive_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rayzen_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "adaptive_driver.cpp"), "-L", lib, "-lrayzen_host", "-lrayzen_hip",
                           f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"adaptive_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    fp = _lib.FrameParams.from_buffer_copy(raw("frame"))
    q = _lib.AdaptiveParams.from_buffer_copy(raw("params"))
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt))
    r.set_frame(fp)
    info, batches, error = r.render_adaptive(q.batch_spp, q.min_batches, q.max_batches, q.threshold, q.luminance_floor, q.merge_gap, q.max_runs)
    accum = r.read_accum()
    r.close()
    assert accum.tobytes() == raw("accum") and batches.tobytes() == raw("batches") and error.tobytes() == raw("error")
    theirs = _lib.AdaptiveInfo.from_buffer_copy(raw("info"))
    assert {k: info[k] for k in RECORDS} == {k: Renderer._adaptive_info(theirs)[k] for k in RECORDS}
    print(f"driver frame: batches per tile {sorted(set(batches.ravel().tolist()))}, E {np.sort(error.ravel()).tolist()}")
    assert len(set(batches.ravel().tolist())) >= 2
    from rayzen_amd.renderer import adaptive_plan
    mask = np.frombuffer(raw("mask"), np.uint8)
    assert adaptive_plan(mask[:40], mask[40:], 4, 3).tobytes() == raw("plan")
    assert [tuple(x) for x in np.frombuffer(raw("plan"), np.int32).reshape(-1, 2).tolist()] == AR.plan(mask[:40], mask[40:], 4, 3)
    assert AR.plan(mask[:40], mask[40:], 4, 3) == [(0, 2), (5, 17), (39, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# 8. what the meter costs

def _median_ms(hip, stream, call, rounds=15):
    a, b = hip.event(), hip.event()
    times = []
    for k in range(rounds + 2):
        hip.ok(hip.L.hipEventRecord(a, stream))
        call()
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        if k >= 2:
            times.append(float(ms.value))
    for e in (a, b):
        hip.L.hipEventDestroy(e)
    return float(np.median(times))


def test_the_meter_costs_no_more_than_one_atrous_pass():
    """cornell_scene at 1920 x 1080.  The meter of a full batch: rz_adaptive_info.meter_ms of a call in which no tile retires
    (threshold -1, s = 1), over its batches.  One a-trous pass: rz_denoise with K = 2 less rz_denoise with K = 1, device pointers,
    medians of 15 after a warm-up.  Both are measured twice, alternating; the spread is the larger relative difference between the
    two runs of either side.  Measured on an MI355X (profiles/adaptive/README.md): the meter 0.0242 ms per full batch (runs
    0.0241, 0.0242), the pass 0.1452 ms (0.1436, 0.1469), ratio 0.166, spread 0.023.  The bound is set from that measurement: a
    ratio of 0.25 -- one and a half times the measured one, the headroom for another board's clocks and a busier host -- plus the
    spread of the run that is judged.  (What the bytes alone allow is far looser: the meter moves 64 B per pixel in whole
    lines, a pass gathers 25 taps of 48 B.)"""
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 1920, 1080
    r = _setup(sc, w, h, 2)
    stream = L.rz_stream_handle(r._c)
    d32 = hip.alloc(w * h * 12)
    meter, one_pass = [], []
    for _ in range(2):
        per_batch = []
        for k in range(3):
            info = r.render_adaptive(batch_spp=1, min_batches=2, max_batches=8, threshold=-1.0)[0]
            assert info["batches"] == 8 and info["tiles_rendered"] == [info["n_tiles"]] * 8
            if k:
                per_batch.append(info["meter_ms"] / 8)
        meter.append(float(np.median(per_batch)))
        k1 = _median_ms(hip, stream, lambda: r.denoise_device(d32, iterations=1))
        k2 = _median_ms(hip, stream, lambda: r.denoise_device(d32, iterations=2))
        one_pass.append(k2 - k1)
    r.close()
    hip.close()
    spread = max(abs(meter[0] - meter[1]) / min(meter), abs(one_pass[0] - one_pass[1]) / min(one_pass))
    a, b = float(np.mean(meter)), float(np.mean(one_pass))
    bound = 0.25 + spread
    print(f"1920x1080: rz_adaptive_meter {a:.4f} ms per full batch (runs {meter[0]:.4f}, {meter[1]:.4f}); one a-trous pass {b:.4f} ms "
          f"(runs {one_pass[0]:.4f}, {one_pass[1]:.4f}); ratio {a / b:.3f}; spread {spread:.3f}; bound {bound:.3f}")
    assert a <= bound * b

"""rz_coverage and rz_outline on the GPU.  The records and the id image are integers and bit patterns of the t the CPU oracle
computes for the same ray, and the outline is three binary32 operations per channel, so everything is compared for equality
with tests/coverage_ref.py: the oracle's images (rzo.trace on editor_rays) reduced by numpy, and the mask and blend restated.
The two timing tests at the end state their own bounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coverage_cases as CC
import coverage_ref as CR
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, INSTANCE_COVERAGE_DTYPE, RayZenError, Renderer, editor_rays, frame_params
from refit_ref import wobble
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEGAKERNEL = 1                      # RZ_FLAG_MEGAKERNEL
SENTINEL = 0x5A5A5A5A               # what a buffer filled with the byte 0x5A holds as int32
FIELDS = INSTANCE_COVERAGE_DTYPE.names


def _frame(sc, w, h):
    return frame_params(sc.camera, w, h, len(sc.lights), 1, 1)


def _setup(sc, w=None, h=None, flags=0):
    r = Renderer(0, flags)
    r.upload_scene(sc)
    if w:
        r.set_frame(_frame(sc, w, h))
    return r


def _assert_records(got, want, what):
    assert got.dtype == INSTANCE_COVERAGE_DTYPE and got.shape == want.shape, what
    for f in FIELDS:
        a, b = (x[f].view(np.uint32) if f.startswith("t_") else x[f] for x in (got, want))
        bad = np.flatnonzero(a != b)
        assert not len(bad), f"{what}: {f} differs on {len(bad)} records; first {bad[0]}: {got[f][bad[0]]!r} != {want[f][bad[0]]!r}"
    assert got.tobytes() == want.tobytes(), what


def _assert_ids(got, want, what):
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: ids differ on {len(bad)} pixels; first (y, x) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


class _Arrays:
    """A scene as the context holds it now: the eight bindings read back, with the camera of the scene it came from."""

    def __init__(self, r, sc):
        self.arrays = {b: r.read_binding(b) for b in S.BINDING_DTYPES}
        self.camera, self.lights = sc.camera, sc.lights


# ---------------------------------------------------------------------------------------------------------------------
# 1. records and ids are the oracle's, and the ids are the other casts'

@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_records_and_ids_equal_the_restatement_on_the_oracle_images(name):
    sc, w, h, ids, t = CC.case(name)
    n = CC.n_instances(sc)
    r = _setup(sc, w, h)
    rec, got = r.coverage(want_ids=True)
    assert r.n_instances() == n
    _, guides = r.denoise(iterations=0, guides=True)
    rays = editor_rays(sc.camera, w, h)
    traced = r.trace_rays(rays["origin"], rays["dir"])
    r.close()
    _assert_ids(got, ids, name)
    _assert_records(rec, CR.records(ids, t, n), name)
    assert int(rec["pixels"].sum(dtype=np.uint64)) == w * h
    assert guides.dtype == HIT_DTYPE and (guides["instance"] == got).all(), "rz_denoise's guides name other instances"
    assert (traced["instance"].reshape(h, w) == got).all(), "rz_trace_rays names other instances"
    hit = got >= 0
    for k in np.unique(got[hit]):           # t_min / t_max are the guides' t, bit for bit
        tk = guides["t"][got == k]
        assert rec["t_min"][k] == tk.min() and rec["t_max"][k] == tk.max(), k


def test_ties_follow_the_visiting_order():
    import tie_cases as TC
    out = []
    for order in (0, 1):
        sc = TC.scene("stack", order)
        ids, t = CC.images("ties" if order == 0 else "ties-order-1", sc, 64, 48)
        r = _setup(sc)
        rec = r.coverage(_frame(sc, 64, 48))
        r.close()
        _assert_records(rec, CR.records(ids, t, CC.n_instances(sc)), f"order {order}")
        out.append(rec.tobytes())
    assert out[0] != out[1]


@pytest.mark.parametrize("w,h", CC.PARTIAL, ids=lambda v: str(v))
def test_partial_tiles(w, h):
    sc = CC.case("reference")[0]
    ids, t = CC.images("reference", sc, w, h)
    r = _setup(sc)                          # no rz_set_frame: the call is given its frame
    rec, got = r.coverage(_frame(sc, w, h), want_ids=True)
    r.close()
    _assert_ids(got, ids, f"{w}x{h}")
    _assert_records(rec, CR.records(ids, t, CC.n_instances(sc)), f"{w}x{h}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. rectangles

@pytest.mark.parametrize("name,w,h", [("reference", 65, 5), ("lattice", 48, 36)], ids=["65x5", "lattice"])
def test_rectangles(name, w, h):
    hip = Hip()
    sc = CC.case(name)[0]
    ids, t = CC.images(name, sc, w, h)
    n = CC.n_instances(sc)
    fp = _frame(sc, w, h)
    r = _setup(sc)
    d_cov, d_ids = hip.alloc((n + 1) * 32 + 32, 0x5A), hip.alloc(w * h * 4 + 16, 0x5A)
    for what, rect in CC.rectangles(w, h).items():
        want = CR.records(ids, t, n, rect)
        assert int(want["pixels"].sum()) == CR.area(rect, w, h), what
        # the host form: ids outside the rectangle keep what the caller's buffer held
        rec = np.empty(n + 1, INSTANCE_COVERAGE_DTYPE)
        img = np.full((h, w), SENTINEL, np.int32)
        cp = None
        if rect is not None:
            cp = _lib.CoverageParams(*rect)
        rc = r._L.rz_coverage(r._c, C.byref(fp), None if cp is None else C.byref(cp), rec.ctypes.data, rec.nbytes, img.ctypes.data,
                              img.nbytes, _lib.COVERAGE_HOST)
        assert rc == 0, (what, r._L.rz_last_error(r._c))
        _assert_records(rec, want, f"{name} {what} (host)")
        _assert_ids(img, CR.expected_ids(ids, rect, SENTINEL), f"{name} {what} (host)")
        assert int(rec["pixels"].sum(dtype=np.uint64)) == CR.area(rect, w, h)
        # the device form
        hip.ok(hip.L.hipMemset(C.c_void_p(d_cov), 0x5A, (n + 1) * 32 + 32))
        hip.ok(hip.L.hipMemset(C.c_void_p(d_ids), 0x5A, w * h * 4 + 16))
        r.coverage_device(d_cov, (n + 1) * 32, d_ids, fp, rect)
        r.sync()
        dev = hip.download(d_cov, (n + 1) * 32 + 32)
        assert dev[:(n + 1) * 32].tobytes() == want.tobytes() and (dev[(n + 1) * 32:] == 0x5A).all(), what
        dimg = hip.download(d_ids, w * h * 4 + 16)
        assert dimg[:w * h * 4].tobytes() == CR.expected_ids(ids, rect, SENTINEL).tobytes() and (dimg[w * h * 4:] == 0x5A).all(), what
        assert r.select_rect((0, 0, w, h) if rect is None else rect, frame=fp) == CR.select_order(want), what
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. call forms

def test_call_forms_give_the_same_bytes():
    hip = Hip()
    sc, w, h, ids, t = CC.case("instanced")
    n = CC.n_instances(sc)
    r = _setup(sc, w, h)
    rec, img = r.coverage(want_ids=True)                    # frame None: the frame of set_frame
    again, img2 = r.coverage(_frame(sc, w, h), want_ids=True)
    assert again.tobytes() == rec.tobytes() and img2.tobytes() == img.tobytes()
    assert r.coverage().tobytes() == rec.tobytes()          # coverage alone
    d_cov, d_ids = hip.alloc((n + 1) * 32, 0x5A), hip.alloc(w * h * 4, 0x5A)
    r.coverage_device(d_cov, (n + 1) * 32, d_ids)
    r.sync()
    assert hip.download(d_cov, (n + 1) * 32).tobytes() == rec.tobytes() and hip.download(d_ids, w * h * 4).tobytes() == img.tobytes()
    hip.ok(hip.L.hipMemset(C.c_void_p(d_ids), 0x5A, w * h * 4))
    hip.ok(hip.L.hipMemset(C.c_void_p(d_cov), 0x5A, (n + 1) * 32))
    r.coverage_device(None, 0, d_ids)                       # ids alone
    r.sync()
    assert hip.download(d_ids, w * h * 4).tobytes() == img.tobytes() and (hip.download(d_cov, (n + 1) * 32) == 0x5A).all()
    hip.ok(hip.L.hipMemset(C.c_void_p(d_ids), 0x5A, w * h * 4))
    r.coverage_device(d_cov, (n + 1) * 32, None)            # coverage alone
    r.sync()
    assert hip.download(d_cov, (n + 1) * 32).tobytes() == rec.tobytes() and (hip.download(d_ids, w * h * 4) == 0x5A).all()
    r.close()
    hip.close()


def test_a_full_table_and_fewer_sets_give_the_same_bytes(monkeypatch):
    """A wave keeps its groups in a table of 64 entries and sends a group whose key finds it full straight to its private set of
    records.  RZ_COVERAGE_TABLE (a test aid) cuts the table to 1, 2 and 7 entries on the lattice, whose runs hold up to 17 keys,
    and RZ_COVERAGE_SETS the private sets to 1 and 3: the records are the restatement's bytes every time."""
    sc, w, h, ids, t = CC.case("lattice")
    want = CR.records(ids, t, CC.n_instances(sc))
    assert max(len(np.unique(row)) for row in ids) > 7
    r = _setup(sc, w, h)
    for table, sets in ((1, None), (2, 1), (7, 3), (None, 1)):
        for name, v in (("RZ_COVERAGE_TABLE", table), ("RZ_COVERAGE_SETS", sets)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
        _assert_records(r.coverage(), want, f"table {table}, sets {sets}")
        _assert_records(r.coverage(rect=(3, 1, 45, 30)), CR.records(ids, t, CC.n_instances(sc), (3, 1, 45, 30)), f"table {table}, sets {sets}, rect")
    r.close()


@pytest.mark.parametrize("name", ["reference", "instanced", "lattice"])
def test_a_wave_that_casts_many_runs_merges_them_as_the_restatement(name, monkeypatch):
    """A workgroup of the persistent grid casts several runs only when a frame has more runs than the grid has workgroups, about
    4 096: then a group finds its key in the wave's table and is merged into that entry -- pixels added, the box grown across
    rows and columns, the t range widened.  RZ_COVERAGE_GRID (a test aid, same bytes) caps the grid at 1, 3 and 5 workgroups, so
    that the 36 to 48 runs of these frames are cast by waves of 8 to 48 runs each, the table cut to 2 entries as well in one
    round; records and ids are the restatement's on the oracle's images, on the whole frame and on a rectangle."""
    sc, w, h, ids, t = CC.case(name)
    n = CC.n_instances(sc)
    rect = (3, 1, w - 5, h - 4)
    r = _setup(sc, w, h)
    for grid, table in ((1, None), (3, None), (5, 2)):
        monkeypatch.setenv("RZ_COVERAGE_GRID", str(grid))
        if table is None:
            monkeypatch.delenv("RZ_COVERAGE_TABLE", raising=False)
        else:
            monkeypatch.setenv("RZ_COVERAGE_TABLE", str(table))
        rec, got = r.coverage(want_ids=True)
        _assert_ids(got, ids, f"{name}, grid {grid}")
        _assert_records(rec, CR.records(ids, t, n), f"{name}, grid {grid}, table {table}")
        _assert_records(r.coverage(rect=rect), CR.records(ids, t, n, rect), f"{name}, grid {grid}, table {table}, rect")
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the records follow the scene

def test_records_after_update_transforms():
    sc, w, h, ids, t = CC.case("instanced")
    n = CC.n_instances(sc)
    r = _setup(sc, w, h)
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(m, F32).reshape(16) for m in S.instanced_transforms(7, 16)])
    r.update_transforms(xf)
    rec, got = r.coverage(want_ids=True)
    now = _Arrays(r, sc)
    r.close()
    ids2, t2 = CR.oracle_images(now.arrays, sc.camera, w, h)
    _assert_ids(got, ids2, "after update_transforms")
    _assert_records(rec, CR.records(ids2, t2, n), "after update_transforms")
    assert rec.tobytes() != CR.records(ids, t, n).tobytes()


def test_records_after_a_refit():
    sc = S.bunny_scene(n=12, aspect=4 / 3)
    w, h = 24, 18
    r = _setup(sc, w, h)
    before = r.coverage()
    ids, t = CR.oracle_images(sc.arrays, sc.camera, w, h)
    _assert_records(before, CR.records(ids, t, 2), "built")
    r.refit_geometry(wobble(S.make_blob(12, 2.8, 0), 0.5), first=12)
    rec, got = r.coverage(want_ids=True)
    now = _Arrays(r, sc)
    r.close()
    ids2, t2 = CR.oracle_images(now.arrays, sc.camera, w, h)
    _assert_ids(got, ids2, "after the refit")
    _assert_records(rec, CR.records(ids2, t2, 2), "after the refit")
    assert rec.tobytes() != before.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5. isolation

@pytest.mark.parametrize("flags", [0, MEGAKERNEL], ids=["samples", "pixels"])
def test_the_calls_leave_the_render_state_alone(flags):
    sc = S.reference_scene()                                # (its glass carries currentIor from chunk to chunk)
    w, h, spp, bounces = 40, 30, 2, 5
    nl = len(sc.lights)
    ids, t = CC.images("reference", sc, w, h)
    want = CR.records(ids, t, CC.n_instances(sc))

    def run(with_calls):
        r = Renderer(0, flags)
        r.upload_scene(sc)
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, 0))
        r.render()
        first = r.read_accum()
        if with_calls:
            plan, kernel, ms = r.debug_last_plan(), r.last_kernel_name(), r.last_render_ms()
            rec, img = r.coverage(want_ids=True)
            _assert_records(rec, want, "between two chunks")
            r.coverage(_frame(sc, 65, 5), rect=(3, 1, 13, 4))        # another frame: the one of rz_set_frame stays
            r.select_rect((0, 0, 20, 20))
            _, rgba8 = r.present(show_fps=False)
            r.outline(img, [0, 4], rgba8=rgba8, rgb32f=first[..., :3])
            assert r.read_accum().tobytes() == first.tobytes()
            assert (r.debug_last_plan(), r.last_kernel_name(), r.last_render_ms()) == (plan, kernel, ms)
            assert (r.width, r.height) == (w, h)
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
# 6. the backstop

def test_backstop_host_path_reports_and_device_path_leaves_it_to_sync():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 16, 8
    n = CC.n_instances(sc)
    r = _setup(sc, w, h)
    before = r.coverage()
    r.sync()
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    with pytest.raises(RayZenError) as e:
        r.coverage()
    message = str(e.value).split("): ", 1)[1]
    assert e.value.code == -9 and message.startswith("rz_coverage: ") and "0x8" in message, str(e.value)
    r.sync()                                                # reported once, then clear
    assert r.coverage().tobytes() == before.tobytes()
    d_cov = hip.alloc((n + 1) * 32, 0)
    assert L.rz_debug_poke_backstop(r._c, 8) == 0
    r.coverage_device(d_cov, (n + 1) * 32)
    with pytest.raises(RayZenError) as e:
        r.sync()
    assert e.value.code == -9
    r.sync()
    assert hip.download(d_cov, (n + 1) * 32).tobytes() == before.tobytes()
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. rz_outline

def _nan_where_no_outline(rgb, mask):
    free = np.argwhere(~mask)
    if len(free):
        rgb[tuple(free[len(free) // 2])] = (np.nan, np.inf, -np.inf)
    return rgb


@pytest.mark.parametrize("name", sorted(CC.OUTLINE_CASES))
def test_outline_equals_the_restatement(name):
    ids, n, sel = CC.OUTLINE_CASES[name]
    words = CR.bitset(sel, n)
    r = Renderer(0)                                         # no scene, no frame
    for radius in (1, 2, 3, 4):
        mask = CR.outline_mask(ids, words, n, radius)
        for alpha, color in ((1.0, (1.0, 0.6, 0.0)), (0.5, (0.25, 1.5, -0.5)), (0.0, (0.3, 0.3, 0.3))):
            rgb, rgba8 = CC.images_for(ids, seed=radius)
            rgb = _nan_where_no_outline(rgb, mask)
            p = _lib.OutlineParams(ids.shape[1], ids.shape[0], radius, (C.c_float * 3)(*color), alpha, 0)
            got32, got8 = rgb.copy(), rgba8.copy()
            rc = r._L.rz_outline(r._c, C.byref(p), ids.ctypes.data, ids.nbytes, words.ctypes.data if len(words) else None, n,
                                 got8.ctypes.data, got8.nbytes, got32.ctypes.data, got32.nbytes, _lib.OUTLINE_HOST)
            assert rc == 0, r._L.rz_last_error(r._c)
            what = f"{name} radius {radius} alpha {alpha}"
            assert got32.view(np.uint32).tobytes() == CR.outline_rgb32f(rgb, mask, color, alpha).view(np.uint32).tobytes(), what
            assert got8.tobytes() == CR.outline_rgba8(rgba8, mask, color, alpha).tobytes(), what
            assert got32[~mask].view(np.uint32).tobytes() == rgb[~mask].view(np.uint32).tobytes(), what
    r.close()


def test_outline_front_end_each_image_alone_and_the_device_form():
    hip = Hip()
    ids, n, sel = CC.OUTLINE_CASES["257x3"]
    h, w = ids.shape
    rgb, rgba8 = CC.images_for(ids)
    mask = CR.outline_mask(ids, CR.bitset(sel, n), n, 2)
    want32, want8 = CR.outline_rgb32f(rgb, mask, (1.0, 0.6, 0.0), 1.0), CR.outline_rgba8(rgba8, mask, (1.0, 0.6, 0.0), 1.0)
    r = Renderer(0)
    keep32, keep8 = rgb.copy(), rgba8.copy()
    out8, out32 = r.outline(ids, sel, rgba8=rgba8, rgb32f=rgb)
    assert out8.tobytes() == want8.tobytes() and out32.tobytes() == want32.tobytes()
    assert rgb.tobytes() == keep32.tobytes() and rgba8.tobytes() == keep8.tobytes()     # the caller's arrays are not modified
    assert r.outline(ids, sel, rgba8=rgba8)[0].tobytes() == want8.tobytes() and r.outline(ids, sel, rgba8=rgba8)[1] is None
    assert r.outline(ids, sel, rgb32f=rgb)[1].tobytes() == want32.tobytes()
    words, nsel = Renderer.selection_bits(sel)
    assert nsel == max(sel) + 1 and words.tobytes() == CR.bitset(sel, nsel).tobytes()
    d_ids, d_sel, d8, d32 = hip.upload(ids), hip.upload(words), hip.upload(rgba8), hip.upload(rgb)
    r.outline_device(w, h, d_ids, d_sel, nsel, d8, d32)
    r.sync()
    assert hip.download(d8, rgba8.nbytes).tobytes() == want8.tobytes() and hip.download(d32, rgb.nbytes).tobytes() == want32.tobytes()
    r.close()
    hip.close()


def test_outline_on_a_presented_frame():
    sc, w, h, ids, t = CC.case("reference")
    r = _setup(sc, w, h)
    r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), 3, 2))
    r.render()
    rgb, rgba8 = r.present(show_fps=False)
    rec, img = r.coverage(want_ids=True)
    picked = [i for i, _ in r.select_rect((20, 10, 50, 40))]
    out8, out32 = r.outline(img, picked, rgba8=rgba8, rgb32f=rgb, radius=2, color=(1.0, 0.6, 0.0), alpha=0.8)
    r.close()
    assert picked and (img == ids).all()
    n = max(picked) + 1
    mask = CR.outline_mask(ids, CR.bitset(picked, n), n, 2)
    assert mask.any()
    assert out8.tobytes() == CR.outline_rgba8(rgba8, mask, (1.0, 0.6, 0.0), 0.8).tobytes()
    assert out32.tobytes() == CR.outline_rgb32f(rgb, mask, (1.0, 0.6, 0.0), 0.8).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors

def test_coverage_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 16, 8
    n = CC.n_instances(sc)
    r = _setup(sc)
    fp = _frame(sc, w, h)
    bc, bi = (n + 1) * 32, w * h * 4
    d_cov, d_ids = hip.alloc(bc + 16, 0x5A), hip.alloc(bi + 16, 0x5A)

    def cov(ctx, frame=fp, params=None, args=None, flags=0):
        return L.rz_coverage(ctx, None if frame is None else C.byref(frame), params, *(args if args is not None else (d_cov, bc, d_ids, bi)), flags)

    def cp(x0=0, y0=0, x1=w, y1=h, reserved=None):
        p = _lib.CoverageParams(x0, y0, x1, y1)
        if reserved is not None:
            p.reserved[reserved] = 1
        return C.byref(p)

    assert cov(None) == -1 and cov(r._c, frame=None) == -1
    assert cov(r._c, params=cp(5, 0, 4, 8)) == -1 and b"rectangle" in L.rz_last_error(r._c)
    assert cov(r._c, params=cp(0, 3, 4, 2)) == -1
    for k in range(4):
        assert cov(r._c, params=cp(reserved=k)) == -1, k
    assert cov(r._c, args=(None, 0, None, 0)) == -1 and b"neither" in L.rz_last_error(r._c)
    assert cov(r._c, flags=2) == -1 and cov(r._c, flags=0x80000000) == -1
    assert cov(r._c, args=(d_cov + 8, bc, d_ids, bi)) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert cov(r._c, args=(d_cov, bc, d_ids + 2, bi)) == -1
    for bad in ((0, 8), (16, 0), (-1, 8), (1 << 16, 1 << 16)):
        assert cov(r._c, frame=frame_params(sc.camera, bad[0], bad[1], 2, 1, 1)) == -1, bad
    assert cov(r._c, args=(d_cov, bc - 1, d_ids, bi)) == -7 and cov(r._c, args=(d_cov, bc, d_ids, bi - 1)) == -7
    host_cov, host_ids = np.full(bc // 4, SENTINEL, np.int32), np.full(w * h, SENTINEL, np.int32)
    assert L.rz_coverage(r._c, C.byref(fp), None, host_cov.ctypes.data, bc - 1, host_ids.ctypes.data, bi, _lib.COVERAGE_HOST) == -7
    assert L.rz_coverage(r._c, C.byref(fp), cp(3, 3, 2, 4), host_cov.ctypes.data, bc, host_ids.ctypes.data, bi, _lib.COVERAGE_HOST) == -1
    assert (host_cov == SENTINEL).all() and (host_ids == SENTINEL).all()
    # nothing was launched
    r.sync()
    assert (hip.download(d_cov, bc + 16) == 0x5A).all() and (hip.download(d_ids, bi + 16) == 0x5A).all()
    # the context stays usable; nothing is written past the buffers
    assert cov(r._c) == 0
    r.sync()
    assert (hip.download(d_cov, bc + 16)[bc:] == 0x5A).all() and (hip.download(d_ids, bi + 16)[bi:] == 0x5A).all()
    assert hip.download(d_cov, bc).tobytes() == r.coverage(fp).tobytes()
    r.close()
    # no scene
    empty = Renderer(0)
    assert cov(empty._c) == -5 and b"no scene" in L.rz_last_error(empty._c)
    empty.close()
    part = Renderer(0)
    for b in S.BINDING_DTYPES:
        if b != S.BIND_INSTANCES:
            part.upload(b, sc.arrays[b])
    assert cov(part._c) == -5
    part.close()
    hip.close()


def test_outline_error_paths():
    hip = Hip()
    L = _lib.hip()
    w, h, n = 20, 6, 40
    ids = np.zeros((h, w), np.int32)
    ids[2, 3] = 33
    words = CR.bitset([33], n)
    np_ = w * h
    r = Renderer(0)
    d_ids, d_sel = hip.upload(ids), hip.upload(words)
    d8, d32 = hip.alloc(np_ * 4 + 16, 0x5A), hip.alloc(np_ * 12 + 16, 0x5A)

    def params(width=w, height=h, radius=2, color=(1.0, 0.6, 0.0), alpha=1.0, reserved=0):
        return C.byref(_lib.OutlineParams(width, height, radius, (C.c_float * 3)(*color), alpha, reserved))

    def out(ctx, p=None, args=None, flags=0):
        a = args if args is not None else (d_ids, np_ * 4, d_sel, n, d8, np_ * 4, d32, np_ * 12)
        return L.rz_outline(ctx, params() if p is None else p, *a, flags)

    nan, inf = float("nan"), float("inf")
    assert out(None) == -1 and L.rz_outline(r._c, None, d_ids, np_ * 4, d_sel, n, d8, np_ * 4, d32, np_ * 12, 0) == -1
    for bad in (dict(width=0), dict(height=-1), dict(width=1 << 16, height=1 << 16), dict(radius=0), dict(radius=5), dict(radius=-1),
                dict(color=(nan, 0.0, 0.0)), dict(color=(0.0, inf, 0.0)), dict(color=(0.0, 0.0, -inf)), dict(alpha=nan), dict(alpha=-0.01),
                dict(alpha=1.01), dict(alpha=inf), dict(reserved=1)):
        assert out(r._c, params(**bad)) == -1, bad
    assert out(r._c, flags=2) == -1 and out(r._c, flags=0x80000000) == -1
    assert out(r._c, args=(None, np_ * 4, d_sel, n, d8, np_ * 4, d32, np_ * 12)) == -1
    assert out(r._c, args=(d_ids, np_ * 4, None, n, d8, np_ * 4, d32, np_ * 12)) == -1
    assert out(r._c, args=(d_ids, np_ * 4, d_sel, n, None, 0, None, 0)) == -1 and b"neither" in L.rz_last_error(r._c)
    for k in range(4):
        a = [d_ids, np_ * 4, d_sel, n, d8, np_ * 4, d32, np_ * 12]
        a[2 * k] += 2
        assert out(r._c, args=tuple(a)) == -1 and b"aligned" in L.rz_last_error(r._c), k
    assert out(r._c, args=(d_ids, np_ * 4 - 1, d_sel, n, d8, np_ * 4, d32, np_ * 12)) == -7
    assert out(r._c, args=(d_ids, np_ * 4, d_sel, n, d8, np_ * 4 - 1, d32, np_ * 12)) == -7
    assert out(r._c, args=(d_ids, np_ * 4, d_sel, n, d8, np_ * 4, d32, np_ * 12 - 1)) == -7
    host8 = np.full(np_ * 4, 0x5A, np.uint8)
    assert L.rz_outline(r._c, params(), ids.ctypes.data, ids.nbytes, words.ctypes.data, n, host8.ctypes.data, np_ * 4 - 1, None, 0,
                        _lib.OUTLINE_HOST) == -7
    assert (host8 == 0x5A).all()
    r.sync()
    assert (hip.download(d8, np_ * 4 + 16) == 0x5A).all() and (hip.download(d32, np_ * 12 + 16) == 0x5A).all()
    # the context stays usable; n_instances = 0 needs no bit set; nothing is written past the buffers
    assert out(r._c) == 0 and out(r._c, args=(d_ids, np_ * 4, None, 0, d8, np_ * 4, None, 0)) == 0
    r.sync()
    got8 = hip.download(d8, np_ * 4 + 16)
    assert (got8[np_ * 4:] == 0x5A).all() and (hip.download(d32, np_ * 12 + 16)[np_ * 12:] == 0x5A).all()
    mask = CR.outline_mask(ids, words, n, 2)
    want8 = CR.outline_rgba8(np.full((h, w, 4), 0x5A, np.uint8), mask, (1.0, 0.6, 0.0), 1.0)
    assert got8[:np_ * 4].tobytes() == want8.tobytes() and int(mask.sum()) == 24
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the Python and the C++ front end

def test_select_rect_orders_as_the_restatement():
    sc, w, h, ids, t = CC.case("instanced")
    n = CC.n_instances(sc)
    r = _setup(sc, w, h)
    for rect in ((0, 0, w, h), (10, 4, 50, 30), (30, 0, 64, 36), (0, 0, 1, 1)):
        want = CR.records(ids, t, n, rect)
        for min_pixels in (1, 4, 20):
            assert r.select_rect(rect, min_pixels) == CR.select_order(want, min_pixels), (rect, min_pixels)
    whole = r.select_rect((0, 0, w, h))
    r.close()
    px = [p for _, p in whole]
    assert px == sorted(px, reverse=True) and len(whole) == 17 and len(set(px)) < len(px)     # (ties: broken by the lower index)


def test_cpp_free_functions_equal_the_python_binding(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    exe = str(tmp_path / "select_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rayzen_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "select_driver.cpp"), "-L", lib, "-lrayzen_host", "-lrayzen_hip",
                           f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"select_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    fp = _lib.FrameParams.from_buffer_copy(raw("frame"))
    w, h = fp.width, fp.height
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt))
    rec, ids = r.coverage(fp, want_ids=True)
    assert rec.tobytes() == raw("coverage") and len(rec) == 5 and ids.tobytes() == raw("ids") and int(rec["pixels"].sum()) == w * h
    rect = tuple(np.frombuffer(raw("rect"), np.int32).tolist())
    rec2, ids2 = r.coverage(fp, rect, want_ids=True)
    assert rec2.tobytes() == raw("coverage_rect") and ids2.tobytes() == raw("ids_rect")
    picked = r.select_rect(rect, 2, frame=fp)
    assert np.array(picked, np.uint32).reshape(-1, 2).tobytes() == raw("select") and len(picked) >= 2
    in8 = np.frombuffer(raw("in8"), np.uint8).reshape(h, w, 4)
    in32 = np.frombuffer(raw("in32"), F32).reshape(h, w, 3)
    out8, out32 = r.outline(ids, [i for i, _ in picked if i != 0], rgba8=in8, rgb32f=in32, radius=3, color=(0.2, 0.9, 1.0), alpha=0.75)
    r.close()
    assert out8.tobytes() == raw("out8") and out32.tobytes() == raw("out32") and raw("out8") != raw("in8")


# ---------------------------------------------------------------------------------------------------------------------
# 10. what the calls cost

def _alternate(hip, stream, calls, rounds):
    """GPU time (ms, a HIP event pair on the context's stream) of each call of `calls`, alternating them `rounds` times; the
    first round warms them up and is dropped."""
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


# The margins cover the run-to-run spread of the two calls each test compares, (max - min) / median over 12 alternating rounds.
# Both were taken from the first measurement run (the first table of profiles/coverage/README.md and its outline lines), before
# either bound was looked at: rz_coverage 0.2686 (0.2644..0.2763) and the guide cast 0.1623 (0.1605..0.1692), 4.4 % and 5.4 %,
# 1 + 0.044 + 0.054; rz_outline 0.0161 (0.0159..0.0213) and rz_display 0.0147 (0.0129..0.0166), 34 % and 25 %, the larger.
# (Calls of 15 microseconds are mostly launch; later runs had single samples of 0.026 and 0.050 ms among the twelve.  The tests
# compare medians, which those do not move.)
COVERAGE_MARGIN = 1.10
OUTLINE_MARGIN = 1.35


def test_coverage_costs_no_more_than_the_guide_cast():
    """bunny_scene() (69 312 triangles and a floor) at 1920 x 1080: the GPU time of rz_coverage (device form, records and ids)
    against rz_denoise with iterations = 0 and guides on the same frame, which casts the same rays and writes twelve times the
    bytes per pixel.  The two calls alternate for 12 rounds after a warm-up round; medians are compared, and the margin covers the
    run-to-run spread of the two calls.  Measured (profiles/coverage/README.md): rz_coverage 0.155 ms [0.154, 0.157], the guide cast
    0.159 ms [0.158, 0.162], ratio 0.97 against the margin of 1.10.  The cast alone (ids, no records) takes 0.140 ms.  Two earlier
    forms missed this bound: every group's atomics into 256 private sets of records took 0.219 ms, into the caller's records
    2.06 ms."""
    hip = Hip()
    L = _lib.hip()
    sc = S.bunny_scene()
    w, h = 1920, 1080
    r = _setup(sc, w, h)
    n = r.n_instances()
    d_cov, d_ids, d_guides = hip.alloc((n + 1) * 32), hip.alloc(w * h * 4), hip.alloc(w * h * 48)
    stream = L.rz_stream_handle(r._c)
    cov_ms, guide_ms = _alternate(hip, stream, [lambda: r.coverage_device(d_cov, (n + 1) * 32, d_ids),
                                                lambda: r.denoise_device(guides_ptr=d_guides, iterations=0)], 12)
    r.sync()
    rec = np.frombuffer(hip.download(d_cov, (n + 1) * 32).tobytes(), INSTANCE_COVERAGE_DTYPE)
    ids = np.frombuffer(hip.download(d_ids, w * h * 4).tobytes(), np.int32)
    guides = np.frombuffer(hip.download(d_guides, w * h * 48).tobytes(), HIT_DTYPE)
    r.close()
    hip.close()
    assert (guides["instance"] == ids).all() and int(rec["pixels"].sum(dtype=np.uint64)) == w * h
    # every wave casts about eight runs here: the whole records, boxes and t ranges too, against the guides' own instance and t
    _assert_records(rec, CR.records(ids.reshape(h, w), guides["t"].reshape(h, w), n), "1920 x 1080 against the guides")
    c, g = float(np.median(cov_ms)), float(np.median(guide_ms))
    spread = max((max(x) - min(x)) / np.median(x) for x in (cov_ms, guide_ms))
    print(f"1920x1080 bunny 69 312: rz_coverage {c:.3f} ms [{min(cov_ms):.3f}, {max(cov_ms):.3f}], rz_denoise guides {g:.3f} ms "
          f"[{min(guide_ms):.3f}, {max(guide_ms):.3f}]; ratio {c / g:.3f}; worst relative spread {spread:.3f}; margin {COVERAGE_MARGIN}")
    assert c <= COVERAGE_MARGIN * g, (cov_ms, guide_ms)


def test_outline_costs_no_more_than_a_display_call():
    """The same frame: rz_outline (device form, rgba8 in place, the big mesh selected, radius 2) against one rz_display call
    (manual exposure, rgb32f in, rgba8 out): both touch each pixel once.  Alternating, 12 rounds after a warm-up round, medians.
    Measured, as this test printed it in three runs (profiles/coverage/README.md lists them): rz_outline 0.0160, 0.0160 and 0.0163 ms,
    rz_display 0.0131, 0.0131 and 0.0155 ms, ratios 1.22, 1.22 and 1.05 against the margin of 1.35."""
    hip = Hip()
    L = _lib.hip()
    sc = S.bunny_scene()
    w, h = 1920, 1080
    r = _setup(sc, w, h)
    n = r.n_instances()
    d_ids, d8, d32 = hip.alloc(w * h * 4), hip.alloc(w * h * 4, 0x40), hip.alloc(w * h * 12, 0)
    r.coverage_device(None, 0, d_ids)
    words, nsel = Renderer.selection_bits([1])
    d_sel = hip.upload(words)
    stream = L.rz_stream_handle(r._c)
    out_ms, disp_ms = _alternate(hip, stream, [lambda: r.outline_device(w, h, d_ids, d_sel, nsel, rgba8_ptr=d8, alpha=0.5),
                                               lambda: r.display_device(rgb_in_ptr=d32, rgba8_ptr=d8)], 12)
    r.sync()
    r.close()
    hip.close()
    o, d = float(np.median(out_ms)), float(np.median(disp_ms))
    spread = max((max(x) - min(x)) / np.median(x) for x in (out_ms, disp_ms))
    print(f"1920x1080: rz_outline {o:.4f} ms [{min(out_ms):.4f}, {max(out_ms):.4f}], rz_display {d:.4f} ms [{min(disp_ms):.4f}, "
          f"{max(disp_ms):.4f}]; ratio {o / d:.3f}; worst relative spread {spread:.3f}; margin {OUTLINE_MARGIN}")
    assert o <= OUTLINE_MARGIN * d, (out_ms, disp_ms)

"""rz_refit_geometry on the GPU.  Every comparison is of bytes: the refitted context against refit_ref (numpy), against the host
library (Scene.refit_mesh, the byte partner) and against a FRESH context that was given the host library's arrays; frames
also against the oracle on those arrays."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import refit_ref as R
from helpers import oracle_render, mismatch_report
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer, RayZenError, frame_params, HIT_DTYPE
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

HOST_RELAYOUT = 4        # RZ_FLAG_HOST_RELAYOUT
GEOM = (S.BIND_TRIANGLES, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES, S.BIND_BLAS_NODES, S.BIND_BLAS_INDICES, S.BIND_INSTANCES)
MESHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes")


class Case:
    """A scene, the mesh of it that deforms (its id in the host scene, where its triangles start in binding 0, its size)."""

    def __init__(self, sc, mesh_id, first, radius):
        self.sc, self.mesh_id, self.first, self.radius = sc, mesh_id, first, radius
        inst = sc.arrays[S.BIND_INSTANCES]
        nxt = [int(o) for o in inst["globalTriOffset"] if int(o) > first] + [len(sc.arrays[S.BIND_TRIANGLES])]
        self.n = min(nxt) - first
        self.mesh = sc.arrays[S.BIND_TRIANGLES][first:first + self.n].copy()       # the undeformed mesh

    def deformations(self):
        return R.deformations(self.mesh, self.radius)


def _monkey_scene():
    s = S.Scene(camera=S.Camera(position=(0.0, 1.0, 5.0), aspect=16.0 / 9.0))
    floor = s.add_mesh(S.make_cube(4))
    monkey = s.add_mesh(S.load_obj(os.path.join(MESHES, "monkey.obj"), 1))
    s.add_object(floor, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.add_object(monkey, S.rotate(S.identity(), 0.4, (0.0, 1.0, 0.0)))
    return s.build()


CASES = {
    "cube": lambda: Case(S.cornell_scene(), 2, 4, 1.0),
    "monkey": lambda: Case(_monkey_scene(), 1, 12, 1.4),
    "bunny24": lambda: Case(S.bunny_scene(n=24), 1, 12, 2.8),
    "bunny76": lambda: Case(S.bunny_scene(n=76), 1, 12, 2.8),
    "instanced": lambda: Case(S.instanced_scene(n=24), 1, 12, 2.8),
    "hidden_glass": lambda: Case(S.hidden_glass_scene(n=24), 1, 12, 2.8),
    "reference": lambda: Case(S.reference_scene(), 2, 12 + 972, 1.4),
}


@functools.lru_cache(maxsize=1)
def _stress_mesh():
    return S.make_blob(289, 10.0, 0)


@functools.lru_cache(maxsize=1)
def _stress_case():
    return Case(S.stress_scene(), 1, 12, 10.0)


def _upload(arrays, flags=0):
    r = Renderer(0, flags)
    for b in S.BINDING_DTYPES:
        r.upload(b, arrays[b])
    return r


def _state(r):
    """What a caller can observe of the geometry: bindings 0, 5, 6, 7, 8, 9 and both layout arrays, as bytes."""
    out = {b: r.read_binding(b).tobytes() for b in GEOM}
    out["pairs"], out["tris"] = r.debug_read_layout(0).tobytes(), r.debug_read_layout(1).tobytes()
    return out


def _assert_same_state(got, want, what):
    for k in want:
        assert got[k] == want[k], f"{what}: {k} differs"


def _frame(r, sc, W, H, spp, bounces, counted=False):
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), bounces, spp))
    r.clear_accum()
    cnt = r.render_counted() if counted else r.render()
    return r.read_accum(), cnt


def _bits_equal(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)).all()


# ---- 6. the bindings and the layout ------------------------------------------------------------------------------------

def _check_bindings(case, r, flags=0, ref_nodes=True, deformations=None):
    sc = case.sc
    idx_before = sc.arrays[S.BIND_BLAS_INDICES].tobytes()
    for dname, moved in (deformations or case.deformations()):
        before = {b: a.copy() for b, a in sc.arrays.items()}
        r.refit_geometry(moved, case.first)
        sc.refit_mesh(case.mesh_id, moved)                   # the host library, the byte partner
        got = _state(r)
        for b in GEOM:
            assert got[b] == sc.arrays[b].tobytes(), f"{dname}: binding {b} != the host library's"
        assert got[S.BIND_BLAS_INDICES] == idx_before
        if ref_nodes:
            tris = before[S.BIND_TRIANGLES].copy()
            tris[case.first:case.first + case.n] = moved
            assert got[S.BIND_BLAS_NODES] == R.refit_scene_nodes(before, tris).tobytes(), f"{dname}: binding 7 != refit_ref"
        assert got[S.BIND_BLAS_NODES] != before[S.BIND_BLAS_NODES].tobytes(), f"{dname}: nothing moved"
        fresh = _upload(sc.arrays, flags)
        _assert_same_state(got, _state(fresh), dname)
        fresh.close()


@pytest.mark.parametrize("name", ["cube", "monkey", "bunny76", "instanced", "reference"])
def test_bindings_and_layout_after_a_refit(name):
    case = CASES[name]()
    r = _upload(case.sc.arrays)
    _check_bindings(case, r)
    r.close()


@pytest.mark.parametrize("window", [None, "2"])
def test_bindings_and_layout_deep_blas_one_million_triangles(window, monkeypatch):
    if window:
        monkeypatch.setenv("RZ_BLAS_STACK_WINDOW", window)
    case = _stress_case()
    assert case.sc.max_blas_depth >= 21 and case.n > 1000000
    r = _upload(case.sc.arrays)
    amp = 0.2 if window else 0.5
    _check_bindings(case, r, deformations=[(f"wobble{amp}", R.wobble(case.mesh, amp * 10.0 / 2.8))])
    # ... and a frame through the (forced) overflow columns equals the fresh context's
    a, _ = _frame(r, case.sc, 96, 54, 2, 4)
    fresh = _upload(case.sc.arrays)
    b, _ = _frame(fresh, case.sc, 96, 54, 2, 4)
    r.close(); fresh.close()
    assert _bits_equal(a, b)


@pytest.mark.parametrize("name", ["cube", "bunny24", "reference"])
def test_bindings_and_layout_host_relayout_context(name):
    case = CASES[name]()
    r = _upload(case.sc.arrays, HOST_RELAYOUT)
    _check_bindings(case, r, HOST_RELAYOUT)
    r.close()


def test_bindings_and_layout_on_geometry_built_on_the_device():
    cube, blob = S.make_cube(4), S.make_blob(24, 2.8, 0)
    objects = [(0, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0))), (1, S.translate(S.identity(), (0.0, 2.0, 0.0)))]
    host = S.bunny_scene(n=24)                       # the same assembly through the host library
    case = Case(host, 1, 12, 2.8)
    r = Renderer(0)
    r.upload_scene_built_on_device([cube, blob], objects, host.materials, host.lights)
    for b in GEOM:
        assert r.read_binding(b).tobytes() == host.arrays[b].tobytes(), b
    _check_bindings(case, r)
    r.close()


# ---- 7. frames ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bunny24", "instanced", "hidden_glass", "reference"])
def test_frames_after_each_deformation(name, monkeypatch):
    case = CASES[name]()
    sc = case.sc
    W, H = 96, 54
    sc.camera.aspect = W / H
    sc.camera.update()
    r = _upload(sc.arrays)
    first_frame, _ = _frame(r, sc, W, H, 1, 2)
    for dname, moved in case.deformations():
        r.refit_geometry(moved, case.first)
        sc.refit_mesh(case.mesh_id, moved)
        fresh = _upload(sc.arrays)
        for spp, bounces, claims in ((1, 2, False), (4, 4, False), (16, 5, True)):
            if claims:          # small frames take the compacting claims only when told to (tests/test_fuzz_gpu.py)
                monkeypatch.setenv("RZ_GROUPS_PER_CLAIM", "4")
                monkeypatch.setenv("RZ_WPOOL_CHUNK", "64")
            a, ca = _frame(r, sc, W, H, spp, bounces, counted=True)
            b, cb = _frame(fresh, sc, W, H, spp, bounces, counted=True)
            ref, cr = oracle_render(sc, W, H, spp, bounces, want_counters=True, nthreads=16)
            what = f"{name}/{dname}, {spp} spp, {bounces} bounces"
            assert _bits_equal(a, b), f"{what} vs the fresh context: " + mismatch_report(a, b)
            assert _bits_equal(a, ref), f"{what} vs the oracle: " + mismatch_report(a, ref)
            assert ca == cb == cr, what
            assert r.last_kernel_name() == fresh.last_kernel_name()
            if claims:
                plan = r.debug_last_plan()
                assert plan["per_claim"] > 0 and plan["claim_units"] in (8, 16), plan
                assert plan == fresh.debug_last_plan()
                monkeypatch.delenv("RZ_GROUPS_PER_CLAIM")
                monkeypatch.delenv("RZ_WPOOL_CHUNK")
        fresh.close()
    last, _ = _frame(r, sc, W, H, 1, 2)
    r.close()
    assert not _bits_equal(first_frame, last)            # the mesh did move in the frame


def test_a_refit_to_a_transparent_material_switches_to_the_glass_kernels():
    case = CASES["bunny24"]()
    sc = case.sc
    W, H = 96, 54
    sc.camera.aspect = W / H
    sc.camera.update()
    r = _upload(sc.arrays)
    _frame(r, sc, W, H, 2, 4)
    assert "<glass>" not in r.last_kernel_name()
    moved = R.wobble(case.mesh, 0.2)
    moved["materialIndex"] = 3                           # the reference's glass
    r.refit_geometry(moved, case.first)
    sc.refit_mesh(case.mesh_id, moved)
    a, ca = _frame(r, sc, W, H, 2, 4, counted=True)
    assert "<glass>" in r.last_kernel_name(), r.last_kernel_name()
    fresh = _upload(sc.arrays)
    b, cb = _frame(fresh, sc, W, H, 2, 4, counted=True)
    ref, cr = oracle_render(sc, W, H, 2, 4, want_counters=True, nthreads=16)
    assert r.last_kernel_name() == fresh.last_kernel_name()
    assert _bits_equal(a, b) and _bits_equal(a, ref), mismatch_report(a, ref)
    assert ca == cb == cr
    _assert_same_state(_state(r), _state(fresh), "glass")
    # ... and back
    moved["materialIndex"] = 0
    r.refit_geometry(moved, case.first)
    _frame(r, sc, W, H, 2, 4)
    assert "<glass>" not in r.last_kernel_name()
    r.close(); fresh.close()


# ---- 8. refit -> transforms -> render, frame after frame ---------------------------------------------------------------

def test_eight_frames_of_refit_transforms_render():
    case = CASES["instanced"]()
    sc = case.sc
    W, H = 96, 54
    sc.camera.aspect = W / H
    sc.camera.update()
    r = _upload(sc.arrays)
    floor_xf = np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], np.float32)
    for frame in range(8):
        moved = R.wobble(case.mesh, 0.05 + 0.06 * frame)
        xfs = S.instanced_transforms(frame + 1, 16)
        r.refit_geometry(moved, case.first)
        r.update_transforms(np.stack([floor_xf] + [np.asarray(t, np.float32).reshape(16) for t in xfs]))
        a, _ = _frame(r, sc, W, H, 2, 3)
        sc.refit_mesh(case.mesh_id, moved)
        for oid, t in zip(sc.instance_ids, xfs):
            sc.set_transform(oid, t)
        sc.update_dynamic()
        fresh = _upload(sc.arrays)
        b, _ = _frame(fresh, sc, W, H, 2, 3)
        assert _bits_equal(a, b), f"frame {frame}: " + mismatch_report(a, b)
        _assert_same_state(_state(r), _state(fresh), f"frame {frame}")
        fresh.close()
    r.close()


# ---- 9. partial intervals -----------------------------------------------------------------------------------------------

def test_partial_interval_inside_one_mesh():
    case = CASES["bunny24"]()
    sc = case.sc
    r = _upload(sc.arrays)
    moved = R.wobble(case.mesh, 0.5)
    lo, hi = 100, 1500
    r.refit_geometry(moved[lo:hi], case.first + lo)
    mixed = case.mesh.copy()
    mixed[lo:hi] = moved[lo:hi]
    sc.refit_mesh(case.mesh_id, mixed)
    fresh = _upload(sc.arrays)
    _assert_same_state(_state(r), _state(fresh), "inside one mesh")
    a, _ = _frame(r, sc, 96, 54, 2, 3)
    b, _ = _frame(fresh, sc, 96, 54, 2, 3)
    r.close(); fresh.close()
    assert _bits_equal(a, b)


def test_partial_interval_across_two_meshes():
    sc = S.reference_scene()
    r = _upload(sc.arrays)
    tris = sc.arrays[S.BIND_TRIANGLES]
    a_first, b_first = 12, 12 + 972                      # meshes a and b lie back to back
    mesh_a, mesh_b = tris[a_first:a_first + 972].copy(), tris[b_first:b_first + 972].copy()
    moved_a, moved_b = R.wobble(mesh_a, 0.2), R.wobble(mesh_b, 0.2)
    lo, hi = a_first + 500, b_first + 300
    r.refit_geometry(np.concatenate([moved_a[500:], moved_b[:300]]), lo)
    mesh_a[500:] = moved_a[500:]
    mesh_b[:300] = moved_b[:300]
    before_c = sc.arrays[S.BIND_BLAS_NODES].copy()
    sc.refit_mesh(1, mesh_a)
    sc.refit_mesh(2, mesh_b)
    fresh = _upload(sc.arrays)
    _assert_same_state(_state(r), _state(fresh), "across two meshes")
    x, _ = _frame(r, sc, 96, 72, 2, 4)
    y, _ = _frame(fresh, sc, 96, 72, 2, 4)
    r.close(); fresh.close()
    assert _bits_equal(x, y)
    assert (sc.arrays[S.BIND_BLAS_NODES] != before_c).any()


def test_refit_everything_after_rz_update_on_binding_0():
    case = CASES["reference"]()
    sc = case.sc
    r = _upload(sc.arrays)
    _frame(r, sc, 64, 48, 1, 2)
    moved = R.wobble(case.mesh, 0.5)
    tris = sc.arrays[S.BIND_TRIANGLES].copy()
    tris[case.first:case.first + case.n] = moved
    r.update(S.BIND_TRIANGLES, tris)                    # alone: stale boxes
    r.refit_geometry()                                  # n_triangles == 0: every mesh, from binding 0 as it stands
    sc.refit_mesh(case.mesh_id, moved)
    fresh = _upload(sc.arrays)
    _assert_same_state(_state(r), _state(fresh), "after rz_update")
    a, _ = _frame(r, sc, 96, 72, 2, 4)
    b, _ = _frame(fresh, sc, 96, 72, 2, 4)
    r.close(); fresh.close()
    assert _bits_equal(a, b)


def test_refit_after_the_materials_changed_under_the_layout():
    """Materials uploaded after the views were laid out: the per-view transparency hints are stale, and the refit takes the
    host route (patch, refit there, re-layout).  Same bytes, and the frame takes the kernels the new materials ask for."""
    case = CASES["bunny24"]()
    sc = case.sc
    r = _upload(sc.arrays)
    _frame(r, sc, 96, 54, 1, 2)
    mats = sc.materials.copy()
    mats["transparency"][0] = 0.9                       # the mesh's material turns to glass
    r.upload(S.BIND_MATERIALS, mats)
    _frame(r, sc, 96, 54, 1, 2)
    assert "<glass>" in r.last_kernel_name()
    moved = R.wobble(case.mesh, 0.2)
    r.refit_geometry(moved, case.first)
    sc.refit_mesh(case.mesh_id, moved)
    arrays = dict(sc.arrays)
    arrays[S.BIND_MATERIALS] = mats
    fresh = _upload(arrays)
    _assert_same_state(_state(r), _state(fresh), "materials changed")
    a, _ = _frame(r, sc, 96, 54, 2, 4)
    b, _ = _frame(fresh, sc, 96, 54, 2, 4)
    assert _bits_equal(a, b) and r.last_kernel_name() == fresh.last_kernel_name()
    r.close(); fresh.close()


# ---- 10. queries, preview, denoiser; the render state -------------------------------------------------------------------

def test_queries_preview_and_guides_after_a_refit():
    case = CASES["reference"]()
    sc = case.sc
    W, H = 96, 72
    r = _upload(sc.arrays)
    moved = R.wobble(case.mesh, 0.5)
    r.refit_geometry(moved, case.first)
    sc.refit_mesh(case.mesh_id, moved)
    fresh = _upload(sc.arrays)
    rng = np.random.default_rng(9)
    o = rng.uniform(-6, 6, (4000, 3)).astype(np.float32)
    d = (rng.normal(size=(4000, 3))).astype(np.float32)
    for rr in (r, fresh):
        rr.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 2))
        rr.render()
    ha, hb = r.trace_rays(o, d), fresh.trace_rays(o, d)
    for k in ha:
        assert ha[k].tobytes() == hb[k].tobytes(), k
    assert (ha["instance"] >= 0).mean() > 0.1
    (la, va), (lb, vb) = r.shadow_rays(o, d, 20.0), fresh.shadow_rays(o, d, 20.0)
    assert (la == lb).all() and va.tobytes() == vb.tobytes()
    ea, eb = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True), fresh.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
    for x, y in zip(ea, eb):
        assert x.tobytes() == y.tobytes()
    (ca, ga), (cb, gb) = r.denoise(guides=True), fresh.denoise(guides=True)
    assert ga.tobytes() == gb.tobytes() and ca.tobytes() == cb.tobytes()
    pa, pb = r.present(show_bvh=True), fresh.present(show_bvh=True)
    assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes()
    r.close(); fresh.close()


def test_the_call_leaves_the_render_state_alone_and_a_refit_of_nothing_is_a_no_op():
    case = CASES["bunny24"]()
    sc = case.sc
    W, H = 96, 54
    sc.camera.aspect = W / H
    sc.camera.update()
    r, plain = _upload(sc.arrays), _upload(sc.arrays)
    for rr in (r, plain):
        rr.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 2, 0))
        rr.render()
    before_accum, before_plan, before_state = r.read_accum(), r.debug_last_plan(), _state(r)
    r.refit_geometry()                                  # an untouched scene: every byte stays
    assert r.read_accum().tobytes() == before_accum.tobytes()
    assert r.debug_last_plan() == before_plan
    _assert_same_state(_state(r), before_state, "refit of nothing")
    for rr in (r, plain):
        rr.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 2, 2))     # continue the accumulation
        rr.render()
    assert r.read_accum().tobytes() == plain.read_accum().tobytes()
    # a real refit touches neither the accumulation nor the plan
    acc = r.read_accum()
    r.refit_geometry(R.wobble(case.mesh, 0.2), case.first)
    assert r.read_accum().tobytes() == acc.tobytes() and r.debug_last_plan() == before_plan
    r.close(); plain.close()


# ---- 11. host and device pointers; a user stream ------------------------------------------------------------------------

def test_host_and_device_pointer_paths_agree_on_a_user_stream_between_two_renders():
    hip = Hip()
    case = CASES["bunny24"]()
    sc = case.sc
    W, H = 96, 54
    sc.camera.aspect = W / H
    sc.camera.update()
    moved = R.wobble(case.mesh, 0.5)
    via_host = _upload(sc.arrays)
    via_host.refit_geometry(moved, case.first)
    r = _upload(sc.arrays)
    stream = hip.stream()
    r.set_stream(stream)
    d_tris = hip.upload(moved)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 2))
    r.render()                                          # in flight on the stream when the refit is enqueued behind it
    r.refit_geometry_device(d_tris, case.first, len(moved))
    r.clear_accum()
    r.render()
    r.sync()
    a = r.read_accum()
    b, _ = _frame(via_host, sc, W, H, 2, 4)
    assert _bits_equal(a, b)
    _assert_same_state(_state(r), _state(via_host), "device pointer vs host pointer")
    sc.refit_mesh(case.mesh_id, moved)
    assert r.read_binding(S.BIND_TRIANGLES).tobytes() == sc.arrays[S.BIND_TRIANGLES].tobytes()      # the host mirror, fetched on demand
    # a second device-pointer refit, then rz_update on binding 0 patches the fetched mirror, not a stale one
    moved2 = R.wobble(case.mesh, 0.05)
    hip.ok(hip.L.hipMemcpy(d_tris, moved2.ctypes.data, moved2.nbytes, 1))
    r.refit_geometry_device(d_tris, case.first, len(moved2))
    r.update(S.BIND_TRIANGLES, moved[:7], (case.first + 3) * 64)
    r.refit_geometry()
    mixed = moved2.copy()
    mixed[3:10] = moved[:7]
    sc.refit_mesh(case.mesh_id, mixed)
    fresh = _upload(sc.arrays)
    _assert_same_state(_state(r), _state(fresh), "update after a device-pointer refit")
    r.set_stream(0)
    r.close(); via_host.close(); fresh.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()


# ---- 12. errors ---------------------------------------------------------------------------------------------------------

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    case = CASES["bunny24"]()
    sc = case.sc
    r = _upload(sc.arrays)
    _frame(r, sc, 64, 36, 1, 2)
    moved = R.wobble(case.mesh, 0.2)
    d_tris = hip.upload(moved)
    before = _state(r)
    n_all = len(sc.arrays[S.BIND_TRIANGLES])
    call = lambda ctx, ptr, first, n, flags: L.rz_refit_geometry(ctx, C.c_void_p(ptr), first, n, flags)
    assert call(None, d_tris, 0, 1, 0) == -1                                  # null context
    assert call(r._c, None, case.first, 5, 0) == -1                           # NULL triangles with n > 0
    assert call(r._c, None, case.first, 5, _lib.REFIT_HOST) == -1
    assert call(r._c, d_tris + 4, case.first, 5, 0) == -1                     # misaligned device pointer
    assert call(r._c, d_tris, case.first, 5, 0x8) == -1                       # unknown flags
    assert call(r._c, d_tris, n_all - 2, 3, 0) == -4                          # past the end of binding 0
    assert call(r._c, d_tris, n_all + 1, 0, 0) == -4
    assert call(r._c, moved.ctypes.data, n_all, 1, _lib.REFIT_HOST) == -4
    _assert_same_state(_state(r), before, "after the refused calls")
    empty = Renderer(0)
    assert call(empty._c, d_tris, 0, 0, 0) == -5                              # nothing uploaded
    for b in (S.BIND_TRIANGLES, S.BIND_BLAS_NODES, S.BIND_BLAS_INDICES):
        empty.upload(b, sc.arrays[b])
    assert call(empty._c, d_tris, 0, 0, 0) == -5                              # binding 9 (and the rest) missing
    empty.close()
    r.debug_fail_alloc(1)                                                     # out of host memory inside the call
    assert call(r._c, d_tris, case.first, len(moved), 0) == -8
    r.debug_fail_alloc(0)
    # a materialIndex outside the materials: what a fresh upload of the result says, now and later, until it is corrected
    bad = moved.copy()
    bad["materialIndex"][17] = 99
    assert call(r._c, bad.ctypes.data, case.first, len(bad), _lib.REFIT_HOST) == -6
    r.set_frame(frame_params(sc.camera, 64, 36, len(sc.lights), 2, 1))
    with pytest.raises(RayZenError) as e:
        r.render()
    assert e.value.code == -6
    fresh_bad = dict(sc.arrays)
    fresh_bad[S.BIND_TRIANGLES] = sc.arrays[S.BIND_TRIANGLES].copy()
    fresh_bad[S.BIND_TRIANGLES][case.first:case.first + case.n] = bad
    fb = _upload(fresh_bad)
    fb.set_frame(frame_params(sc.camera, 64, 36, len(sc.lights), 2, 1))
    with pytest.raises(RayZenError) as e2:
        fb.render()
    assert e2.value.code == -6
    fb.close()
    # the context is usable: the corrected triangles go in and everything equals the fresh context
    r.refit_geometry(moved, case.first)
    sc.refit_mesh(case.mesh_id, moved)
    fresh = _upload(sc.arrays)
    _assert_same_state(_state(r), _state(fresh), "after the errors")
    a, _ = _frame(r, sc, 64, 36, 2, 3)
    b, _ = _frame(fresh, sc, 64, 36, 2, 3)
    assert _bits_equal(a, b)
    r.close(); fresh.close()
    hip.close()


# ---- 13 / 14. speed -----------------------------------------------------------------------------------------------------

def _median_ms(hip, stream, fn, reps=25):
    a, b = hip.event(), hip.event()
    out = []
    for _ in range(reps):
        hip.ok(hip.L.hipEventRecord(a, stream))
        fn()
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float(0)
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        out.append(ms.value)
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    return float(np.median(out)), float(np.min(out))


@pytest.mark.parametrize("size", ["c2", "c5"])
def test_a_refit_is_faster_than_the_rebuild_it_replaces(size):
    """One rz_refit_geometry (device pointer, whole mesh, TLAS step included) against what the library needed before it for the
    same deformation: rz_build_geometry plus the re-layout the next call triggers (taken here by rz_update_transforms, whose
    own TLAS step both sides then contain).  Device events on a user stream, median of 25.  Only the ordering is asserted; the
    figures go to profiles/refit/README.md."""
    hip = Hip()
    if size == "c2":
        cube, blob, radius = S.make_cube(4), S.make_blob(76, 2.8, 0), 2.8
        objects = [(0, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0))), (1, S.translate(S.identity(), (0.0, 2.0, 0.0)))]
    else:
        cube, blob, radius = S.make_cube(4), _stress_mesh(), 10.0
        objects = [(0, S.translate(S.scale(S.identity(), (40.0, 0.5, 40.0)), (0.0, -28.0, 0.0))), (1, S.identity())]
    mats, lights = S.reference_materials(), S.reference_lights()
    moved = R.wobble(blob, 0.2 * radius / 2.8)
    all_moved = np.concatenate([cube, moved])
    xf = np.stack([np.ascontiguousarray(t, np.float32).reshape(16) for _, t in objects])
    stream = hip.stream()
    r = Renderer(0)
    r.set_stream(stream)
    r.upload_scene_built_on_device([cube, blob], objects, mats, lights)
    r.update_transforms(xf)
    d_tris = hip.upload(moved)
    r.refit_geometry_device(d_tris, 12, len(moved))                # warm-up: the topology is derived here, once
    refit_ms, refit_min = _median_ms(hip, stream, lambda: r.refit_geometry_device(d_tris, 12, len(moved)))

    def rebuild():
        r.build_geometry(all_moved, [(0, 12), (12, len(moved))])
        r.update_transforms(xf)                                    # finalize: the re-layout; then the TLAS step
    rebuild()
    rebuild_ms, rebuild_min = _median_ms(hip, stream, rebuild)
    n = len(moved)
    gbs = 250.0 * n / (refit_ms * 1e-3) / 1e9
    print(f"[refit] {size}: {n} triangles: refit {refit_ms:.3f} ms (min {refit_min:.3f}), rz_build_geometry + re-layout {rebuild_ms:.3f} ms "
          f"(min {rebuild_min:.3f}): x{rebuild_ms / refit_ms:.1f}; ~{gbs:.0f} GB/s of the 250 B/triangle estimate = {gbs / 8000 * 100:.1f} % of 8 TB/s")
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()
    assert refit_ms < rebuild_ms, (refit_ms, rebuild_ms)


def test_what_the_refitted_tree_costs_the_render_recorded():
    """Frame time on the refitted tree / on a rebuilt tree, C2's frame (1920 x 1080, 64 spp, 4 bounces).  Recorded, not asserted
    (the CPU's node counts say about 1.01, 1.03, 1.21); the frames themselves must agree wherever the oracle's did."""
    base = S.bunny_scene(n=76)
    mesh = base.arrays[S.BIND_TRIANGLES][12:].copy()
    W, H, spp, bounces = 1920, 1080, 64, 4
    r = _upload(base.arrays)
    for amp in R.AMPLITUDES:
        moved = R.wobble(mesh, amp)
        r.refit_geometry(moved, 12)
        s = S.Scene(camera=base.camera)
        floor, bunny = s.add_mesh(S.make_cube(4)), s.add_mesh(moved)
        s.add_object(floor, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
        s.add_object(bunny, S.translate(S.identity(), (0.0, 2.0, 0.0)))
        s.build()
        rebuilt = _upload(s.arrays)
        times = []
        for rr in (r, rebuilt):
            rr.set_frame(frame_params(base.camera, W, H, len(base.lights), bounces, spp))
            ms = []
            for _ in range(5):
                rr.clear_accum()
                rr.render()
                rr.sync()
                ms.append(rr.last_render_ms()[0])
            times.append(float(np.median(ms)))
        same = _bits_equal(r.read_accum(), rebuilt.read_accum())
        print(f"[refit] C2 frame, A = {amp}: refitted tree {times[0]:.3f} ms, rebuilt tree {times[1]:.3f} ms: x{times[0] / times[1]:.3f}; "
              f"frames bit-identical: {bool(same)}")
        rebuilt.close()
    r.close()

"""rz_geometry_quality and rz_rebuild_geometry on the GPU.  The metering: the SAH cost of every mesh's tree against quality_ref (numpy, math.fsum) within the 1e-9
relative bound of the definition, on uploaded and device-built geometry, after each deformation of the refit tests, on
host-layout contexts, and on trees large enough for many workgroups; what the call must leave alone; its errors and its price.
The rebuild: every comparison is of bytes -- the rebuilt context against the host library (Scene.rebuild_mesh, the byte partner),
against quality_ref.rebuilt_arrays and against a FRESH context that was given those arrays; frames also against the oracle."""
import ctypes as C

import numpy as np
import pytest

import quality_ref as Q
import refit_ref as R
from rayzen_amd import _lib
from rayzen_amd import scene as S
import skin_ref as K
from helpers import oracle_render, mismatch_report
from rayzen_amd.renderer import Renderer, RayZenError, frame_params
from test_quality_abi import _floor_and_two_blobs
from test_rays_gpu import Hip
from test_refit_gpu import CASES, GEOM, Case, HOST_RELAYOUT, _assert_same_state, _bits_equal, _frame, _median_ms, _state, _stress_case, _upload

pytestmark = pytest.mark.gpu


def _check_records(got, want, what):
    """`got`: the call's records; `want`: quality_ref.scene_quality's dicts."""
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        for f in ("node_offset", "index_offset", "tri_offset", "n_triangles", "n_nodes", "depth"):
            assert int(g[f]) == w[f], f"{what}: {f} of mesh {w['node_offset']}: {int(g[f])} != {w[f]}"
        rel = abs(g["sah_cost"] - w["sah_cost"]) / w["sah_cost"] if w["sah_cost"] else abs(g["sah_cost"])
        print(f"[quality] {what}: mesh at node {w['node_offset']}: cost {g['sah_cost']:.12g}, fsum {w['sah_cost']:.12g}, rel {rel:.2e}")
        assert Q.close(float(g["sah_cost"]), w["sah_cost"]), f"{what}: mesh {w['node_offset']}: {g['sah_cost']!r} vs {w['sah_cost']!r}"
        assert g["node_offset_before"] == g["node_offset"] and g["flags"] == 0 and g["reserved"] == 0.0
        assert g["sah_cost_before"] == g["sah_cost"]


def _check_costs(case, r, deformations=None):
    sc = case.sc
    # render state the call must not touch
    r.set_frame(frame_params(sc.camera, 64, 36, len(sc.lights), 2, 1))
    r.render()
    accum, plan, state = r.read_accum().tobytes(), r.debug_last_plan(), _state(r)
    first = r.geometry_quality()
    built = Q.scene_quality(sc.arrays)
    _check_records(first, built, "as handed over")
    assert (first["sah_cost_built"] == first["sah_cost"]).all()
    assert r.geometry_quality().tobytes() == first.tobytes()              # two calls, identical bytes
    assert r.read_accum().tobytes() == accum and r.debug_last_plan() == plan
    _assert_same_state(_state(r), state, "rz_geometry_quality")
    costs = []
    for dname, moved in (deformations or case.deformations()):
        tris = sc.arrays[S.BIND_TRIANGLES].copy()
        tris[case.first:case.first + case.n] = moved
        want_nodes = R.refit_scene_nodes(sc.arrays, tris)
        r.refit_geometry(moved, case.first)
        got = r.geometry_quality()
        _check_records(got, Q.scene_quality(sc.arrays, want_nodes), dname)
        assert got["sah_cost_built"].tobytes() == first["sah_cost"].tobytes(), f"{dname}: sah_cost_built moved"
        assert r.geometry_quality().tobytes() == got.tobytes()
        k = [int(g["tri_offset"]) for g in got].index(case.first)
        costs.append(float(got["sah_cost"][k] / got["sah_cost_built"][k]))
    return costs


@pytest.mark.parametrize("flags", [0, HOST_RELAYOUT])
@pytest.mark.parametrize("name", ["cube", "monkey", "bunny24", "instanced", "reference"])
def test_cost_against_the_restatement(name, flags):
    case = CASES[name]()
    r = _upload(case.sc.arrays, flags)
    n_meshes = len(Q.meshes(case.sc.arrays))
    assert n_meshes == {"cube": 3, "monkey": 2, "bunny24": 2, "instanced": 2, "reference": 7}[name]      # one record for 16 instances
    ratios = _check_costs(case, r)
    r.close()
    if name != "cube":                                                    # (twelve triangles: the ratios differ in the fourth digit)
        assert ratios[0] < ratios[1] < ratios[2], ratios                  # the three wobbles: the cost follows the deformation


def _built_on_device(sc):
    """A context whose geometry was built on the device from the scene's own meshes and objects (one BLAS per mesh, in the
    scene's node order); its arrays must be the host library's."""
    tris = sc.arrays[S.BIND_TRIANGLES]
    keys = [k for k, _ in Q.meshes(sc.arrays)]
    nodes = sc.arrays[S.BIND_BLAS_NODES]
    meshes = [tris[k[2]:k[2] + Q.tree_shape(nodes[k[0]:end])[2]] for k, end in Q.meshes(sc.arrays)]
    inst = sc.arrays[S.BIND_INSTANCES]
    objects = [(keys.index((int(i["blasNodeOffset"]), int(i["blasTriOffset"]), int(i["globalTriOffset"]))), i["transform"]) for i in inst]
    r = Renderer(0)
    r.upload_scene_built_on_device(meshes, objects, sc.materials, sc.lights)
    for b in GEOM:
        assert r.read_binding(b).tobytes() == sc.arrays[b].tobytes(), b
    return r


@pytest.mark.parametrize("name", ["cube", "monkey", "bunny24", "instanced", "reference"])
def test_cost_on_geometry_built_on_the_device(name):
    case = CASES[name]()
    r = _built_on_device(case.sc)
    _check_costs(case, r)
    r.close()


def test_cost_of_a_tree_of_many_workgroups():
    """bunny_scene(n=76): 41 693 nodes, some 80 workgroups of partial sums for one mesh."""
    case = CASES["bunny76"]()
    r = _upload(case.sc.arrays)
    _check_costs(case, r, deformations=[("wobble0.5", R.wobble(case.mesh, 0.5))])
    r.close()


def test_cost_of_a_deep_blas_of_one_million_triangles():
    case = _stress_case()
    r = _upload(case.sc.arrays)
    got = r.geometry_quality()
    want = Q.scene_quality(case.sc.arrays)
    assert want[1]["n_nodes"] > 600000
    _check_records(got, want, "stress")
    assert r.geometry_quality().tobytes() == got.tobytes()
    r.close()


def test_built_cost_follows_a_new_hand_over():
    """sah_cost_built is measured anew after binding 7 is uploaded or patched, and kept across uploads of other bindings."""
    case = CASES["bunny24"]()
    sc = case.sc
    r = _upload(sc.arrays)
    r.refit_geometry(R.wobble(case.mesh, 0.5), case.first)                 # the first look happens inside the refit
    q = r.geometry_quality()
    assert q["sah_cost"][1] > 1.2 * q["sah_cost_built"][1]
    r.upload(S.BIND_INSTANCES, sc.arrays[S.BIND_INSTANCES])                 # not a hand-over of the tree
    assert r.geometry_quality()["sah_cost_built"].tobytes() == q["sah_cost_built"].tobytes()
    refitted = r.read_binding(S.BIND_BLAS_NODES)
    r.upload(S.BIND_BLAS_NODES, refitted)                                   # the caller hands the refitted tree over: it is "built" now
    q2 = r.geometry_quality()
    assert q2["sah_cost"].tobytes() == q["sah_cost"].tobytes() == q2["sah_cost_built"].tobytes()
    r.close()


def test_errors():
    L = _lib.hip()
    sc = S.cornell_scene()
    n = C.c_size_t(99)
    rec = (_lib.MeshQuality * 8)()
    assert L.rz_geometry_quality(None, rec, 8, C.byref(n)) == -1                 # null context
    empty = Renderer(0)
    assert L.rz_geometry_quality(empty._c, rec, 8, C.byref(n)) == -5             # nothing uploaded
    for b in (S.BIND_TRIANGLES, S.BIND_BLAS_NODES, S.BIND_BLAS_INDICES):
        empty.upload(b, sc.arrays[b])
    assert L.rz_geometry_quality(empty._c, rec, 8, C.byref(n)) == -5             # binding 9 (and the rest) missing
    empty.close()
    r = _upload(sc.arrays)
    before = _state(r)
    assert L.rz_geometry_quality(r._c, None, 0, C.byref(n)) == 0 and n.value == 3        # out == NULL: only the count
    assert L.rz_geometry_quality(r._c, rec, 2, C.byref(n)) == -1                 # a short cap: nothing done
    assert L.rz_geometry_quality(r._c, None, 0, None) == -1
    assert L.rz_geometry_quality(r._c, rec, 8, None) == 0 and rec[2].n_nodes == 9
    r.debug_fail_alloc(1)                                                        # out of host memory inside the call
    assert L.rz_geometry_quality(r._c, rec, 8, C.byref(n)) == -8
    r.debug_fail_alloc(0)
    _assert_same_state(_state(r), before, "after the refused calls")
    r.close()


def test_metering_is_cheaper_than_reading_the_boxes_back():
    """After a refit the boxes live on the device.  The parent commit lets a caller see them only through
    rz_read_binding(BIND_BLAS_NODES); the metering reads them where they are.  Each side runs behind the same refit (so the
    boxes are fresh on the device every time), device events on a user stream, median of 25; only the ordering is asserted."""
    hip = Hip()
    case = CASES["bunny76"]()
    moved = R.wobble(case.mesh, 0.2)
    stream = hip.stream()
    r = _upload(case.sc.arrays)
    r.set_stream(stream)
    d_tris = hip.upload(moved)
    r.refit_geometry_device(d_tris, case.first, len(moved))          # warm-up: topology and the first look
    r.geometry_quality()

    def metered():
        r.refit_geometry_device(d_tris, case.first, len(moved))
        r.geometry_quality()

    def read_back():
        r.refit_geometry_device(d_tris, case.first, len(moved))
        r.read_binding(S.BIND_BLAS_NODES)
    refit_ms, _ = _median_ms(hip, stream, lambda: r.refit_geometry_device(d_tris, case.first, len(moved)))
    meter_ms, meter_min = _median_ms(hip, stream, metered)
    read_ms, read_min = _median_ms(hip, stream, read_back)
    print(f"[quality] C2 mesh ({len(moved)} triangles): refit {refit_ms:.3f} ms; refit + rz_geometry_quality {meter_ms:.3f} ms (min {meter_min:.3f}); "
          f"refit + rz_read_binding(7) {read_ms:.3f} ms (min {read_min:.3f})")
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()
    assert meter_ms < read_ms, (meter_ms, read_ms)


# ---- rz_rebuild_geometry ---------------------------------------------------------------------------------------------------

REBUILT = _lib.QUALITY_REBUILT


def _fresh_like(sc, flags=0):
    """A fresh context given the scene's arrays, then rz_update_transforms with the transforms in force."""
    fresh = _upload(sc.arrays, flags)
    fresh.update_transforms(sc.arrays[S.BIND_INSTANCES]["transform"])
    return fresh


def _rebuild_all_on_host(sc):
    """Scene.rebuild_mesh for every mesh of the scene (an empty mesh rebuilds to the root it had)."""
    n = 0
    while True:
        try:
            sc.rebuild_mesh(n)
        except RuntimeError:
            return n
        n += 1


def _check_rebuilt_everything(case, r, flags=0):
    sc = case.sc
    moved = R.wobble(case.mesh, 0.5 * case.radius / 2.8)
    r.refit_geometry(moved, case.first)
    sc.refit_mesh(case.mesh_id, moved)
    before = r.geometry_quality()
    want = Q.rebuilt_arrays(sc.arrays, {k for k, _ in Q.meshes(sc.arrays)})
    rec = r.rebuild_geometry(0.0)
    assert _rebuild_all_on_host(sc) >= 2
    for b in GEOM:
        assert sc.arrays[b].tobytes() == want[b].tobytes(), f"binding {b}: the host library != quality_ref"
    got = _state(r)
    for b in GEOM:
        assert got[b] == sc.arrays[b].tobytes(), f"binding {b} != the host library's"
    fresh = _fresh_like(sc, flags)
    _assert_same_state(got, _state(fresh), "rebuilt everything vs a fresh context")
    # the records: everything with a cost was rebuilt, and is "built" now
    assert rec["node_offset_before"].tobytes() == before["node_offset"].tobytes()
    assert rec["sah_cost_before"].tobytes() == before["sah_cost"].tobytes()
    assert ((rec["flags"] == REBUILT) == (before["sah_cost"] > 0)).all() and (rec["flags"] == REBUILT).sum() >= 2
    _check_records_after(rec, sc.arrays)
    assert (rec["sah_cost_built"] == rec["sah_cost"]).all()
    k = [int(t) for t in rec["tri_offset"]].index(case.first)
    nodes, idx, _ = S.build_blas(moved)                      # bindings 7 / 8 of the mesh: the builder's, RayZen's bytes
    o, t = int(rec["node_offset"][k]), int(rec["index_offset"][k])
    assert r.read_binding(S.BIND_BLAS_NODES)[o:o + len(nodes)].tobytes() == nodes.tobytes()
    assert r.read_binding(S.BIND_BLAS_INDICES)[t:t + len(idx)].tobytes() == idx.tobytes()
    return fresh


def _check_records_after(rec, arrays):
    want = Q.scene_quality(arrays)
    assert len(rec) == len(want)
    for g, w in zip(rec, want):
        for f in ("node_offset", "index_offset", "tri_offset", "n_triangles", "n_nodes", "depth"):
            assert int(g[f]) == w[f], (f, int(g[f]), w[f])
        assert Q.close(float(g["sah_cost"]), w["sah_cost"]), (g["sah_cost"], w["sah_cost"])
        assert g["reserved"] == 0.0


def _check_frames(r, fresh, sc, what):
    W, H = 96, 54
    sc.camera.aspect = W / H
    sc.camera.update()
    a, _ = _frame(r, sc, W, H, 2, 4)
    b, _ = _frame(fresh, sc, W, H, 2, 4)
    ref = oracle_render(sc, W, H, 2, 4, nthreads=16)
    assert _bits_equal(a, b), f"{what} vs the fresh context: " + mismatch_report(a, b)
    assert _bits_equal(a, ref), f"{what} vs the oracle: " + mismatch_report(a, ref)


@pytest.mark.parametrize("name", ["cube", "monkey", "bunny24", "instanced", "reference"])
def test_rebuild_everything(name):
    case = CASES[name]()
    sc = case.sc
    r = _upload(sc.arrays)
    _frame(r, sc, 64, 36, 1, 2)
    fresh = _check_rebuilt_everything(case, r)
    _check_frames(r, fresh, sc, name)
    if name == "instanced":                                  # ... and the rebuilt trees follow new transforms
        floor_xf = np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], np.float32)
        xfs = S.instanced_transforms(3, 16)
        for rr in (r, fresh):
            rr.update_transforms(np.stack([floor_xf] + [np.asarray(t, np.float32).reshape(16) for t in xfs]))
        for oid, t in zip(sc.instance_ids, xfs):
            sc.set_transform(oid, t)
        sc.update_dynamic()
        got = _state(r)
        _assert_same_state(got, _state(fresh), "after update_transforms")
        for b in GEOM:
            assert got[b] == sc.arrays[b].tobytes(), b
        _check_frames(r, fresh, sc, "instanced after update_transforms")
    r.close(); fresh.close()


def test_rebuild_under_transforms_that_differ_from_the_uploaded_instances():
    """rz_update_transforms BEFORE the rebuild: the transforms in force live on the device only, and the patched instances,
    the world boxes and the TLAS must carry them."""
    case = CASES["instanced"]()
    sc = case.sc
    r = _upload(sc.arrays)
    floor_xf = np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], np.float32)
    xfs = S.instanced_transforms(3, 16)
    r.update_transforms(np.stack([floor_xf] + [np.asarray(t, np.float32).reshape(16) for t in xfs]))
    for oid, t in zip(sc.instance_ids, xfs):
        sc.set_transform(oid, t)
    sc.update_dynamic()
    uploaded = r.read_binding(S.BIND_INSTANCES)
    assert uploaded.tobytes() == sc.arrays[S.BIND_INSTANCES].tobytes()
    fresh = _check_rebuilt_everything(case, r)
    got = r.read_binding(S.BIND_INSTANCES)
    assert got["transform"].tobytes() == uploaded["transform"].tobytes() and got["inverseTransform"].tobytes() == uploaded["inverseTransform"].tobytes()
    _check_frames(r, fresh, sc, "rebuild after update_transforms")
    r.close(); fresh.close()


@pytest.mark.parametrize("route", ["host_relayout", "built_on_device"])
def test_rebuild_everything_on_the_other_routes(route):
    case = CASES["bunny24"]()
    sc = case.sc
    if route == "host_relayout":
        r = _upload(sc.arrays, HOST_RELAYOUT)
        fresh = _check_rebuilt_everything(case, r, HOST_RELAYOUT)
    else:
        cube, blob = S.make_cube(4), S.make_blob(24, 2.8, 0)
        objects = [(0, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0))), (1, S.translate(S.identity(), (0.0, 2.0, 0.0)))]
        r = Renderer(0)
        r.upload_scene_built_on_device([cube, blob], objects, sc.materials, sc.lights)
        fresh = _check_rebuilt_everything(case, r)
    _check_frames(r, fresh, sc, route)
    r.close(); fresh.close()


def test_selective_rebuild():
    sc, blob = _floor_and_two_blobs()
    n = len(blob)
    moved_a, moved_b = R.wobble(blob, 0.5), R.wobble(blob, 0.05)
    # the premises, with the host partner
    built_nodes, built_idx, _ = S.build_blas(blob)
    built = S.sah_cost(built_nodes)
    ratio_a = S.sah_cost(S.refit_blas(moved_a, built_nodes, built_idx)) / built
    ratio_b = S.sah_cost(S.refit_blas(moved_b, built_nodes, built_idx)) / built
    new_a = S.build_blas(moved_a)[0]
    assert ratio_a >= 1.26 and ratio_b <= 1.14 and len(built_nodes) == 443 and len(new_a) != 443, (ratio_a, ratio_b, len(new_a))
    r = _upload(sc.arrays)
    _frame(r, sc, 64, 36, 1, 2)
    r.refit_geometry(np.concatenate([moved_a, moved_b]), 12)
    sc.refit_mesh(1, moved_a)
    sc.refit_mesh(2, moved_b)
    # max_ratio = 2.0: nothing is rebuilt and nothing moves
    state, plan = _state(r), r.debug_last_plan()
    rec = r.rebuild_geometry(2.0)
    assert (rec["flags"] == 0).all() and rec["node_offset"].tolist() == [0, 9, 452] == rec["node_offset_before"].tolist()
    assert abs(rec["sah_cost"][1] / rec["sah_cost_built"][1] - ratio_a) < 1e-8 and abs(rec["sah_cost"][2] / rec["sah_cost_built"][2] - ratio_b) < 1e-8      # (four costs, 1e-9 each)
    _assert_same_state(_state(r), state, "max_ratio = 2.0")
    assert r.debug_last_plan() == plan
    # max_ratio = 1.2: only A
    refitted_b = r.read_binding(S.BIND_BLAS_NODES)[452:].tobytes()
    accum = r.read_accum().tobytes()
    rec = r.rebuild_geometry(1.2)
    assert rec["flags"].tolist() == [0, REBUILT, 0]
    assert rec["node_offset_before"].tolist() == [0, 9, 452] and rec["node_offset"].tolist() == [0, 9, 9 + len(new_a)]
    assert rec["sah_cost_before"][1] > rec["sah_cost"][1] == rec["sah_cost_built"][1]
    assert rec["sah_cost_before"][2] == rec["sah_cost"][2] and abs(rec["sah_cost"][2] / rec["sah_cost_built"][2] - ratio_b) < 1e-8
    got_nodes = r.read_binding(S.BIND_BLAS_NODES)
    assert got_nodes[9:9 + len(new_a)].tobytes() == new_a.tobytes()
    assert got_nodes[9 + len(new_a):].tobytes() == refitted_b                  # B: its refitted bytes, moved
    assert r.read_binding(S.BIND_INSTANCES)["blasNodeOffset"].tolist() == [0, 9, 9 + len(new_a)]
    assert r.read_accum().tobytes() == accum and r.debug_last_plan() == plan   # the render state is untouched
    sc.rebuild_mesh(1)
    got = _state(r)
    for b in GEOM:
        assert got[b] == sc.arrays[b].tobytes(), f"binding {b} != the host library's"
    fresh = _fresh_like(sc)
    _assert_same_state(got, _state(fresh), "selective rebuild vs a fresh context")
    _check_frames(r, fresh, sc, "selective")
    r.close(); fresh.close()


def test_life_after_a_rebuild():
    """A refit after a rebuild equals the host library's; rz_geometry_quality reports the new tree as built; a rig made before
    the rebuild poses the new tree."""
    case = CASES["bunny24"]()
    sc = case.sc
    r = _upload(sc.arrays)
    fresh = _check_rebuilt_everything(case, r)
    fresh.close()
    q = r.geometry_quality()
    assert (q["sah_cost_built"] == q["sah_cost"]).all() and (q["flags"] == 0).all()
    moved = R.wobble(case.mesh, 0.2)
    r.refit_geometry(moved, case.first)
    sc.refit_mesh(case.mesh_id, moved)
    fresh = _fresh_like(sc)
    _assert_same_state(_state(r), _state(fresh), "a refit after a rebuild")
    q2 = r.geometry_quality()
    assert q2["sah_cost_built"].tobytes() == q["sah_cost_built"].tobytes() and q2["sah_cost"][1] != q["sah_cost"][1]
    r.close(); fresh.close()
    # skin_pose -> rebuild -> skin_pose with other bones (the cube of the skinning tests' smallest scene)
    case = CASES["cube"]()
    sc = case.sc
    r = _upload(sc.arrays)
    skin, yr = K.bend_skin(case.mesh)
    rid = r.skin_create(case.first, case.mesh, skin, 2, None)
    for angle in (0.7, -0.4):
        rig = K.Rig(f"bend{angle}", case.mesh, skin, K.bend_bones(yr, angle), None, None)
        r.skin_pose(rid, rig.bones, None)
        sc.refit_mesh(case.mesh_id, S.skin_triangles(rig.rest, rig.skin, rig.bones, None, None))
        if angle == 0.7:
            rec = r.rebuild_geometry(0.0)
            assert (rec["flags"] == REBUILT).all()
            _rebuild_all_on_host(sc)
    fresh = _fresh_like(sc)
    _assert_same_state(_state(r), _state(fresh), "skin_pose -> rebuild -> skin_pose")
    _check_frames(r, fresh, sc, "skin_pose -> rebuild -> skin_pose")
    r.close(); fresh.close()


def test_a_failing_rebuild_leaves_the_context_as_it_was():
    case = CASES["bunny24"]()
    sc = case.sc
    r = _upload(sc.arrays)
    _frame(r, sc, 64, 36, 1, 2)
    r.refit_geometry(R.wobble(case.mesh, 0.5), case.first)
    before = _state(r)
    failures = 0
    for nth in range(1, 200):
        r.debug_fail_alloc(nth)
        try:
            rec = r.rebuild_geometry(0.0)
            break
        except RayZenError as e:
            assert e.code == -8, e
            failures += 1
            r.debug_fail_alloc(0)
            _assert_same_state(_state(r), before, f"after the failure at allocation {nth}")
    else:
        raise AssertionError("the call never succeeded")
    r.debug_fail_alloc(0)
    assert failures >= 5 and (rec["flags"] == REBUILT).all()
    sc.refit_mesh(case.mesh_id, R.wobble(case.mesh, 0.5))
    _rebuild_all_on_host(sc)
    fresh = _fresh_like(sc)
    _assert_same_state(_state(r), _state(fresh), "the call that succeeded")
    r.close(); fresh.close()


def test_rebuild_errors():
    L = _lib.hip()
    sc = S.cornell_scene()
    n = C.c_size_t(0)
    rec = (_lib.MeshQuality * 8)()
    call = lambda ctx, ratio, cap=8, flags=0: L.rz_rebuild_geometry(ctx, C.c_double(ratio), rec, cap, C.byref(n), flags)
    assert call(None, 0.0) == -1
    empty = Renderer(0)
    assert call(empty._c, 0.0) == -5                                          # nothing uploaded
    empty.close()
    r = _upload(sc.arrays)
    before = _state(r)
    assert call(r._c, -0.5) == -1 and call(r._c, float("nan")) == -1          # a negative or NaN ratio
    assert call(r._c, 0.0, flags=1) == -1                                     # unknown flags
    assert call(r._c, 0.0, cap=2) == -1 and n.value == 3                      # a short cap
    _assert_same_state(_state(r), before, "after the refused calls")
    r.close()
    # two distinct triples sharing a node extent: measurable, not rebuildable
    arrays = dict(sc.arrays)
    inst = sc.arrays[S.BIND_INSTANCES].copy()
    tris = np.concatenate([sc.arrays[S.BIND_TRIANGLES], sc.arrays[S.BIND_TRIANGLES][:2]])
    idx = np.concatenate([sc.arrays[S.BIND_BLAS_INDICES], np.arange(2, dtype=np.int32)])
    inst["blasTriOffset"][1], inst["globalTriOffset"][1], inst["blasNodeOffset"][1] = len(idx) - 2, len(tris) - 2, inst["blasNodeOffset"][0]
    arrays[S.BIND_INSTANCES], arrays[S.BIND_TRIANGLES], arrays[S.BIND_BLAS_INDICES] = inst, tris, idx
    r = _upload(arrays)
    assert len(r.geometry_quality()) == 3
    before = _state(r)
    assert call(r._c, 0.0) == -1 and b"share" in L.rz_last_error(r._c)
    _assert_same_state(_state(r), before, "two triples on one node extent")
    assert call(r._c, 1.5) == 0 and all(rec[k].flags == 0 for k in range(3))  # nothing selected: nothing to refuse
    r.close()


def test_a_rebuild_on_the_device_is_faster_than_the_route_through_the_host():
    """rz_rebuild_geometry of the one degraded mesh followed by a render, against what the parent commit offers for triangles
    that were posed on the device: rz_read_binding(BIND_TRIANGLES) + rz_build_geometry + rz_update_transforms + the same
    render.  Each side runs behind the same device-pointer refit, which alternates between two poses so that the tree the
    last round built is degraded again (the posed triangles live on the device only).  Device events on a user stream,
    median of 25; only the ordering is asserted."""
    hip = Hip()
    case = CASES["bunny76"]()
    sc = case.sc
    poses = [R.wobble(case.mesh, 0.5), case.mesh]
    n = len(case.mesh)
    xf = np.ascontiguousarray(sc.arrays[S.BIND_INSTANCES]["transform"], np.float32).reshape(-1, 16)
    stream = hip.stream()
    d_poses = [hip.upload(p) for p in poses]
    ms, rebuilt, turn = {}, [], [0]
    for side in ("device", "host"):
        turn[0] = 1                                          # (the first round refits to the wobbled pose)
        r = _upload(sc.arrays)
        r.set_stream(stream)
        r.set_frame(frame_params(sc.camera, 96, 54, len(sc.lights), 4, 2))

        def device():
            turn[0] += 1
            r.refit_geometry_device(d_poses[turn[0] & 1], case.first, n)
            rebuilt.append(r.rebuild_geometry(1.1)["flags"].tolist())
            r.render()

        def host():
            turn[0] += 1
            r.refit_geometry_device(d_poses[turn[0] & 1], case.first, n)
            tris = r.read_binding(S.BIND_TRIANGLES)
            r.build_geometry(tris, [(0, 12), (12, n)])
            r.update_transforms(xf)
            r.render()
        fn = device if side == "device" else host
        fn()
        ms[side] = _median_ms(hip, stream, fn)
        r.set_stream(0)
        r.close()
    print(f"[quality] C2 mesh ({n} triangles): refit + rz_rebuild_geometry + render {ms['device'][0]:.3f} ms (min {ms['device'][1]:.3f}); "
          f"refit + read_binding(0) + rz_build_geometry + rz_update_transforms + render {ms['host'][0]:.3f} ms (min {ms['host'][1]:.3f})")
    hip.L.hipStreamDestroy(stream)
    hip.close()
    assert all(f == [0, REBUILT] for f in rebuilt), rebuilt      # every round rebuilt the one mesh, and only it
    assert ms["device"][0] < ms["host"][0], ms

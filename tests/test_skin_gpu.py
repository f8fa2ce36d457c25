"""rz_skin_create / rz_skin_pose on the GPU.  Every comparison is of bytes: the posed context against a second context that was
given skin_ref's triangles (numpy) through rz_refit_geometry, and against a FRESH context uploaded with the host library's
arrays after rzh_skin_triangles + Scene.refit_mesh (the byte partners); frames also against the oracle on those arrays."""
import ctypes as C

import numpy as np
import pytest

import skin_ref as K
from helpers import oracle_render, mismatch_report
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer, RayZenError, frame_params
from test_rays_gpu import Hip
from test_refit_gpu import CASES, GEOM, _assert_same_state, _bits_equal, _frame, _state, _upload

pytestmark = pytest.mark.gpu

SIZES = (1, 12, 63, 64, 65, 255, 256, 257, 968)


def _host_pose(rig):
    got = S.skin_triangles(rig.rest, rig.skin, rig.bones, rig.morphs, rig.morph_weights)
    assert got.tobytes() == rig.pose().tobytes(), f"{rig.name}: the host library != skin_ref"
    return got


def _create(r, first, rig):
    return r.skin_create(first, rig.rest, rig.skin, rig.n_bones, rig.morphs)


def _check_pose(case, r, rig_id, rig, what, pose=None):
    """One pose of `rig` on r, whose geometry equals case.sc.arrays when called -- and again on return."""
    sc = case.sc
    before = dict(sc.arrays)
    (pose or (lambda: r.skin_pose(rig_id, rig.bones, rig.morph_weights)))()
    got = _state(r)
    want = rig.pose()
    assert got[S.BIND_TRIANGLES][case.first * 64:(case.first + case.n) * 64] == want.tobytes(), f"{what}: binding 0 != skin_ref"
    other = _upload(before)                              # the same triangles through rz_refit_geometry
    other.refit_geometry(want, case.first)
    _assert_same_state(got, _state(other), f"{what} vs refit_geometry(skin_ref)")
    other.close()
    sc.refit_mesh(case.mesh_id, _host_pose(rig))         # the host library, the byte partner
    for b in GEOM:
        assert got[b] == sc.arrays[b].tobytes(), f"{what}: binding {b} != the host library's"
    fresh = _upload(sc.arrays)
    _assert_same_state(got, _state(fresh), f"{what} vs a fresh context")
    fresh.close()


# ---- bytes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cube", "monkey", "bunny24", "instanced", "reference"])
def test_bytes_after_a_pose_of_every_generator(name):
    case = CASES[name]()
    r = _upload(case.sc.arrays)
    for rig in K.rigs(case.mesh):
        rid = _create(r, case.first, rig)
        _check_pose(case, r, rid, rig, f"{name}/{rig.name}")
        r.skin_destroy(rid)
    r.close()


def test_three_poses_on_one_rig_are_not_cumulative_and_a_pose_follows_update_transforms():
    case = CASES["instanced"]()
    sc = case.sc
    r = _upload(sc.arrays)
    skin, yr = K.bend_skin(case.mesh)
    morphs = K.random_morphs(np.random.default_rng(1), case.mesh, 1, 0.1)
    rid = r.skin_create(case.first, case.mesh, skin, 2, morphs)
    for angle, mw in ((0.3, 0.5), (0.9, 0.0), (-0.4, -1.0)):
        rig = K.Rig(f"bend{angle}", case.mesh, skin, K.bend_bones(yr, angle), morphs, [mw])
        _check_pose(case, r, rid, rig, rig.name)          # from the rest pose every time
    floor_xf = np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], np.float32)
    xfs = S.instanced_transforms(3, 16)
    r.update_transforms(np.stack([floor_xf] + [np.asarray(t, np.float32).reshape(16) for t in xfs]))
    for oid, t in zip(sc.instance_ids, xfs):
        sc.set_transform(oid, t)
    sc.update_dynamic()
    rig = K.Rig("bend after transforms", case.mesh, skin, K.bend_bones(yr, 0.6), morphs, [0.25])
    _check_pose(case, r, rid, rig, rig.name)
    r.close()


# ---- kernel shapes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["skin", "morph", "skin_morph"])
def test_every_tail_of_every_instantiation(kind):
    case = CASES["monkey"]()
    sc = case.sc
    assert case.n == 968
    r = _upload(sc.arrays)
    rng = np.random.default_rng(11)
    full = K.Rig(kind, case.mesh,
                 K.random_skin(rng, 968, 7) if "skin" in kind else None, K.random_bones(rng, 7) if "skin" in kind else None,
                 K.random_morphs(rng, case.mesh, 3, 0.1) if "morph" in kind else None, [0.5, 0.0, -0.75] if "morph" in kind else None)
    cur = sc.arrays[S.BIND_TRIANGLES].copy()
    for n in SIZES:
        off = 0 if n == 968 else 5 + n % 7
        rig = full.sub(off, off + n)
        first = case.first + off
        rid = _create(r, first, rig)
        r.skin_pose(rid, rig.bones, rig.morph_weights)
        r.skin_destroy(rid)
        want = rig.pose()
        assert want.tobytes() != cur[first:first + n].tobytes()
        cur[first:first + n] = want
        got = r.read_binding(S.BIND_TRIANGLES)
        assert got[first:first + n].tobytes() == want.tobytes(), f"{kind}, {n} triangles"
        assert got.tobytes() == cur.tobytes(), f"{kind}, {n} triangles: a triangle outside the range changed"
        sc.refit_mesh(case.mesh_id, cur[case.first:case.first + case.n])
    fresh = _upload(sc.arrays)
    _assert_same_state(_state(r), _state(fresh), kind)
    r.close(); fresh.close()


# ---- device arguments; two rigs ------------------------------------------------------------------------------------------

def test_device_arguments_give_the_bytes_of_host_arguments():
    hip = Hip()
    case = CASES["bunny24"]()
    rig = K.rigs(case.mesh)[-1]
    assert rig.n_bones == 256 and rig.n_morphs == 3
    via_host, r = _upload(case.sc.arrays), _upload(case.sc.arrays)
    via_host.skin_pose(_create(via_host, case.first, rig), rig.bones, rig.morph_weights)
    rid = _create(r, case.first, rig)
    d_bones, d_weights = hip.upload(rig.bones), hip.upload(rig.morph_weights)
    r.skin_pose_device(rid, d_bones, d_weights)
    _assert_same_state(_state(r), _state(via_host), "device arguments vs host arguments")
    assert r.skin_last_kernel_ms() > 0
    # ... and checked against the partners like any other pose (the context is back at the scene's arrays first)
    r.refit_geometry(case.mesh, case.first)
    _check_pose(case, r, rid, rig, "device arguments", pose=lambda: r.skin_pose_device(rid, d_bones, d_weights))
    r.close(); via_host.close()
    hip.close()


def test_two_rigs_on_two_meshes_posed_alternately():
    sc = S.reference_scene()
    r = _upload(sc.arrays)
    tris = sc.arrays[S.BIND_TRIANGLES]
    a_first, b_first, n = 12, 12 + 972, 972
    mesh = {1: tris[a_first:a_first + n].copy(), 2: tris[b_first:b_first + n].copy()}
    first = {1: a_first, 2: b_first}
    rng = np.random.default_rng(4)
    skin = {m: K.random_skin(rng, n, 7) for m in (1, 2)}
    rid = {m: r.skin_create(first[m], mesh[m], skin[m], 7) for m in (1, 2)}
    assert rid[1] != rid[2]
    cur = tris.copy()
    for step, m in enumerate((1, 2, 1, 2)):
        rig = K.Rig(f"step{step}", mesh[m], skin[m], K.random_bones(rng, 7) * np.float32(0.01) + np.tile(S.identity(), (7, 1)))
        r.skin_pose(rid[m], rig.bones)
        cur[first[m]:first[m] + n] = rig.pose()
        assert r.read_binding(S.BIND_TRIANGLES).tobytes() == cur.tobytes(), f"step {step}: the other rig's range changed"
        sc.refit_mesh(m, S.skin_triangles(rig.rest, rig.skin, rig.bones))
        fresh = _upload(sc.arrays)
        _assert_same_state(_state(r), _state(fresh), f"step {step}")
        fresh.close()
    r.close()


# ---- frames and queries --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bunny24", "reference"])
def test_a_frame_after_a_pose_is_the_oracles_frame_on_the_skinned_arrays(name):
    case = CASES[name]()
    sc = case.sc
    W, H = 64, 48
    sc.camera.aspect = W / H
    sc.camera.update()
    r = _upload(sc.arrays)
    first_frame, _ = _frame(r, sc, W, H, 2, 3)
    rig = K.bend(case.mesh, 0.7)
    rid = _create(r, case.first, rig)
    r.skin_pose(rid, rig.bones)
    sc.refit_mesh(case.mesh_id, _host_pose(rig))
    a, _ = _frame(r, sc, W, H, 2, 3)
    ref = oracle_render(sc, W, H, 2, 3, nthreads=16)
    assert _bits_equal(a, ref), f"{name} vs the oracle: " + mismatch_report(a, ref)
    assert not _bits_equal(a, first_frame)               # the mesh did move in the frame
    fresh = _upload(sc.arrays)
    rng = np.random.default_rng(9)
    o = rng.uniform(-6, 6, (2000, 3)).astype(np.float32)
    d = rng.normal(size=(2000, 3)).astype(np.float32)
    fresh.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 3, 2))
    ha, hb = r.trace_rays(o, d), fresh.trace_rays(o, d)
    for k in ha:
        assert ha[k].tobytes() == hb[k].tobytes(), k
    assert (ha["instance"] >= 0).mean() > 0.1
    r.close(); fresh.close()


# ---- rest = NULL ---------------------------------------------------------------------------------------------------------

def test_a_null_rest_pose_captures_binding_0():
    case = CASES["bunny24"]()
    sc = case.sc
    r = _upload(sc.arrays)
    moved = K.bend(case.mesh, 0.4).pose()
    hip = Hip()
    d_tris = hip.upload(moved)
    r.refit_geometry_device(d_tris, case.first, len(moved))      # binding 0 now lives on the device only
    sc.refit_mesh(case.mesh_id, moved)
    skin = np.zeros(case.n, S.SKIN_TRIANGLE)
    skin["weights"][:, :, 0] = 1.0
    rid = r.skin_create(case.first, case.n, skin, 1)             # rest = NULL
    rig = K.Rig("captured", moved, skin, np.stack([S.identity()]))
    _check_pose(case, r, rid, rig, "rest = NULL, identity")
    rig2 = K.Rig("captured, turned", moved, skin, K.random_bones(np.random.default_rng(2), 1) * np.float32(0.001) + S.identity())
    _check_pose(case, r, rid, rig2, "rest = NULL, moved")
    r.close()
    hip.close()


# ---- errors --------------------------------------------------------------------------------------------------------------

def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    case = CASES["bunny24"]()
    sc = case.sc
    r = _upload(sc.arrays)
    _frame(r, sc, 64, 36, 1, 2)
    n, first = case.n, case.first
    n_all = len(sc.arrays[S.BIND_TRIANGLES])
    rng = np.random.default_rng(6)
    rig = K.Rig("errors", case.mesh, K.random_skin(rng, n, 7), K.random_bones(rng, 7) * np.float32(0.01) + np.tile(S.identity(), (7, 1)),
                K.random_morphs(rng, case.mesh, 2, 0.05), [0.5, -0.5])
    rid = _create(r, first, rig)
    before = _state(r)
    out = C.c_int(-77)
    p = lambda a: None if a is None else a.ctypes.data
    morphs = rig.morphs

    def create(ctx, first_, n_, rest, skin, nb, mo, nm, rig_out=out):
        return L.rz_skin_create(ctx, first_, n_, p(rest), p(skin), nb, p(mo), nm, None if rig_out is None else C.byref(rig_out))

    assert create(None, first, n, rig.rest, rig.skin, 7, morphs, 2) == -1                     # null context
    assert create(r._c, first, n, rig.rest, rig.skin, 7, morphs, 2, rig_out=None) == -1       # NULL rig_out
    assert create(r._c, first, 0, rig.rest, rig.skin, 7, morphs, 2) == -1                     # no triangles
    assert create(r._c, first, n, rig.rest, rig.skin, 0, morphs, 2) == -1                     # n_bones outside 1..256
    assert create(r._c, first, n, rig.rest, rig.skin, 257, morphs, 2) == -1
    assert create(r._c, first, n, rig.rest, rig.skin, -1, morphs, 2) == -1
    assert create(r._c, first, n, rig.rest, None, 3, morphs, 2) == -1                         # bones without skin
    assert create(r._c, first, n, rig.rest, None, 0, None, 0) == -1                           # neither skin nor morphs
    assert create(r._c, first, n, rig.rest, None, 0, morphs, 0) == -1
    assert create(r._c, first, n, rig.rest, rig.skin, 7, morphs, -1) == -1                    # negative n_morphs
    assert create(r._c, first, n, rig.rest, rig.skin, 7, None, 2) == -1                       # NULL morphs with n_morphs > 0
    assert create(r._c, n_all - n + 1, n, rig.rest, rig.skin, 7, None, 0) == -4               # past the end of binding 0
    assert create(r._c, n_all + 1, 1, rig.rest, rig.skin, 7, None, 0) == -4
    assert create(r._c, first, n, None, rig.skin, 7, None, 0) == 0                            # (rest = NULL is fine)
    r.skin_destroy(out.value)
    out.value = -77
    assert create(r._c, first, n, rig.rest, rig.skin, 6, None, 0) == -4                       # a kept influence names bone 6 of 6
    bad = rig.skin.copy()
    bad["bones"][n // 2, 1] |= 0xFF << 8
    bad["weights"][n // 2, 1, 1] = np.nan                                                     # NaN is not 0: kept, bone 255 of 7
    assert create(r._c, first, n, rig.rest, bad, 7, None, 0) == -4
    r.debug_fail_alloc(1)
    assert create(r._c, first, n, rig.rest, rig.skin, 7, morphs, 2) == -8                     # out of host memory inside the call
    r.debug_fail_alloc(0)
    assert out.value == -77                                                                   # no failing call wrote an id
    empty = Renderer(0)
    assert create(empty._c, 0, n, rig.rest, rig.skin, 7, None, 0) == -5                       # binding 0 missing
    empty.upload(S.BIND_TRIANGLES, sc.arrays[S.BIND_TRIANGLES])
    assert create(empty._c, first, n, rig.rest, rig.skin, 7, None, 0) == 0
    pose = lambda ctx, rig_, b, w, flags: L.rz_skin_pose(ctx, rig_, C.c_void_p(b), C.c_void_p(w), flags)
    assert pose(empty._c, out.value, p(rig.bones), None, 0) == -5                             # the refit's bindings are missing
    empty.close()

    d_bones, d_weights = hip.upload(rig.bones), hip.upload(rig.morph_weights)
    assert pose(None, rid, p(rig.bones), p(rig.morph_weights), 0) == -1                       # null context
    assert pose(r._c, rid + 100, p(rig.bones), p(rig.morph_weights), 0) == -1                 # unknown rig
    assert pose(r._c, -1, p(rig.bones), p(rig.morph_weights), 0) == -1
    assert pose(r._c, rid, None, p(rig.morph_weights), 0) == -1                               # NULL bones
    assert pose(r._c, rid, p(rig.bones), None, 0) == -1                                       # NULL morph_weights
    assert pose(r._c, rid, d_bones, None, _lib.SKIN_DEVICE_ARGS) == -1
    assert pose(r._c, rid, p(rig.bones), p(rig.morph_weights), 0x8) == -1                     # unknown flags
    assert pose(r._c, rid, d_bones + 4, d_weights, _lib.SKIN_DEVICE_ARGS) == -1               # misaligned device arguments
    assert pose(r._c, rid, d_bones, d_weights + 2, _lib.SKIN_DEVICE_ARGS) == -1
    r.debug_fail_alloc(1)
    assert pose(r._c, rid, p(rig.bones), p(rig.morph_weights), 0) == -8
    r.debug_fail_alloc(0)
    gone = r.skin_create(first, rig.rest, rig.skin, 7)
    r.skin_destroy(gone)
    assert pose(r._c, gone, p(rig.bones), None, 0) == -1                                      # a destroyed rig
    assert L.rz_skin_destroy(r._c, gone) == -1 and L.rz_skin_destroy(None, rid) == -1 and L.rz_skin_destroy(r._c, 12345) == -1
    _assert_same_state(_state(r), before, "after the refused calls")
    # the rig is still usable
    _check_pose(case, r, rid, rig, "after the errors")

    # binding 0 uploaded anew and shorter: the rig's range is past its end until the triangles are back
    r2 = _upload(sc.arrays)
    rid2 = _create(r2, first, rig)
    r2.upload(S.BIND_TRIANGLES, sc.arrays[S.BIND_TRIANGLES][:first + n - 1])
    assert pose(r2._c, rid2, p(rig.bones), p(rig.morph_weights), 0) == -4
    r2.upload(S.BIND_TRIANGLES, sc.arrays[S.BIND_TRIANGLES])
    fresh = _upload(sc.arrays)
    _assert_same_state(_state(r2), _state(fresh), "after the refused pose on a shorter binding 0")
    fresh.close()
    r2.skin_pose(rid2, rig.bones, rig.morph_weights)
    _assert_same_state(_state(r2), _state(r), "the rig after the refused pose")

    # a materialIndex outside the materials in the rest pose: the refit's RZ_ERR_BAD_SCENE
    rest_bad = rig.rest.copy()
    rest_bad["materialIndex"][17] = 99
    rid3 = r2.skin_create(first, rest_bad, rig.skin, 7)
    with pytest.raises(RayZenError) as e:
        r2.skin_pose(rid3, rig.bones)
    assert e.value.code == -6
    r2.set_frame(frame_params(sc.camera, 64, 36, len(sc.lights), 2, 1))
    with pytest.raises(RayZenError) as e2:
        r2.render()
    assert e2.value.code == -6
    r2.skin_pose(rid2, rig.bones, rig.morph_weights)                                          # the good rig corrects it
    _assert_same_state(_state(r2), _state(r), "after the bad rest pose was posed over")
    r.close(); r2.close()
    hip.close()

"""Does the table of tests/scene_edits.py bite?  With the oracle alone (no GPU): every edit that is said to change the frame
moves at least 30 of the 3 072 pixels of the base's oracle frame -- so a context that answers with yesterday's materials,
lights or instances cannot agree with the oracle -- and at most three cases are exempt; every frame rendered between two edits
differs from the one before it as well.  The builders the GPU tests rest on are held to the host library: the TLAS written by
hand to Scene.build's and Scene.update_dynamic's, the array partners of the geometry calls to Scene.refit_mesh's and
Scene.rebuild_mesh's bytes, and the scene with the spare glass mesh to the host library's own build once the mesh is named.

Measured on these inputs (pixels of 3 072 that differ from the frame before the edit): M1 59, M2 317, M3 1 446, M4 59 then 59
(55 against the base), M5 1 466, M6 55, M7b 1 445, L1 1 438, L2 1 401, L3a 1 388, L3b 1 394, L4 1 388 and 1 388 back, I1 339,
I2 241, I3 1 370, I4 1 370 and 1 370 back, M7a 0.  (M6's NaN alone moves nothing: the oracle's `transparency > 0` is false for
it, as the kernels' is; the case also recolours the material, so that a stale record shows.)"""
import numpy as np
import pytest

import refit_ref as R
import scene_edits as E
from helpers import oracle_render
from rayzen_amd import scene as S

FLOOR = 30


def _oracle(b, arrays, nl):
    return oracle_render(b.view(arrays), E.W, E.H, E.SPP, E.BOUNCES, num_lights=nl)


def _changed(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).sum())


def test_at_most_three_cases_leave_the_frame_unchanged():
    unchanged = sorted(n for n, c in E.CASES.items() if not c.changes_frame)
    assert len(unchanged) <= E.MAX_UNCHANGED == 3, unchanged
    assert unchanged == ["I4", "L4", "M7a"]
    assert set(E.IN_PRIOR_STATES) | set(E.BEFORE_GEOMETRY_CALLS) <= set(E.CASES)
    assert {c.base for c in E.CASES.values()} == set(E.BASES)
    assert all(c.why for c in E.CASES.values())
    # which cases patch a binding by rz_update at a non-zero offset (the others upload whole arrays or patch record 0)
    offset = sorted(n for n in E.CASES if any(c.kind == "update" and c.offset > 0 for c in E.case_arrays(n)[1]))
    assert offset == ["I1", "I2", "I3", "I4", "L1", "M1", "M2", "M4", "M5", "M6", "M7a"]


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_the_edit_moves_the_oracle_frame(name):
    case = E.CASES[name]
    b, calls, before, stages = E.case_arrays(name)
    nl_before, nl = len(before[E.LIGHT]), E.num_lights(name, before)
    frames = [_oracle(b, before, nl_before)] + [_oracle(b, a, nl if a is stages[-1] else nl_before) for a in stages]
    moved = [_changed(x, y) for x, y in zip(frames, frames[1:])]
    total = _changed(frames[0], frames[-1])
    print(f"{name}: pixels of {E.W * E.H} that differ from the frame before: {moved}; last against first: {total}")
    assert frames[0].shape == (E.H, E.W, 4)
    if case.changes_frame:
        assert total >= FLOOR, (name, total)
        assert all(m >= FLOOR for m in moved), (name, moved)
    else:
        assert total == 0, (name, total)
        assert all(m >= FLOOR for m in moved[:-1]), (name, moved)          # the frames on the way did change
    # every rz_update is a real edit: the call drops a patch that changes nothing
    cur = before
    for c in calls:
        if c.kind != "frame":
            nxt = E.apply([c], cur)
            assert c.kind == "upload" or nxt[c.binding].tobytes() != cur[c.binding].tobytes(), (name, c.binding)
            cur = nxt


@pytest.mark.parametrize("name", E.IN_PRIOR_STATES)
@pytest.mark.parametrize("state", ["S1", "S3", "S4"])
def test_the_edit_bites_in_the_prior_states_too(state, name):
    """On the arrays the host partners give for the state: moved transforms (S1), a refitted mesh (S3), that mesh rebuilt (S4)."""
    case = E.CASES[name]
    b = E.base(case.base)
    if state == "S1":
        current = E.moved_arrays(b)
    else:
        current = E.refit_arrays(b.arrays, *E.deformed(b))
        if state == "S4":
            current = E.rebuild_arrays(b, current)
    nl0 = len(current[E.LIGHT])
    assert _changed(_oracle(b, current, nl0), _oracle(b, b.arrays, nl0)) >= FLOOR              # the state is not the base's
    final = E.apply(case.edit(current), current)
    moved = _changed(_oracle(b, current, nl0), _oracle(b, final, E.num_lights(name, current)))
    print(f"{name} in {state}: {moved} pixels")
    assert moved >= FLOOR


@pytest.mark.parametrize("name", E.AFTER_A_READ_BACK)
@pytest.mark.parametrize("state", ["S1", "S3"])
def test_a_second_device_call_bites(state, name):
    """What test_a_device_call_after_a_read_back runs with no edit: a second rz_update_transforms with other transforms (S1), a
    second device-pointer refit with another deformation (S3).  The frame moves from the state's to the step's."""
    assert set(E.AFTER_A_READ_BACK) <= set(E.IN_PRIOR_STATES)         # (their edits bite in S1, S3 and S4: the test above)
    b = E.base(E.CASES[name].base)
    if state == "S1":
        current, final = E.moved_arrays(b), E.moved_arrays(b, again=True)
    else:
        current = E.refit_arrays(b.arrays, *E.deformed(b))
        final = E.refit_arrays(current, *E.deformed(b, again=True))
    nl = len(current[E.LIGHT])
    moved = _changed(_oracle(b, current, nl), _oracle(b, final, nl))
    print(f"{name}'s base in {state}, the second call: {moved} pixels")
    assert moved >= FLOOR


def test_the_bases_are_the_scenes_they_name():
    ref = E.base("reference")
    assert len(ref.arrays[S.BIND_TRIANGLES]) == 4872 and len(ref.arrays[E.INST]) == 7
    assert (ref.arrays[E.MAT]["transparency"] > 0).tolist() == [False, False, False, True, False]
    used = set(np.unique(ref.arrays[S.BIND_TRIANGLES]["materialIndex"]).tolist())
    assert used == {0, 1, 2, 3}                                                     # material 4 is the unused one M7b drops
    opaque = E.base("reference_opaque")
    assert not (opaque.arrays[E.MAT]["transparency"] > 0).any()
    for b in (S.BIND_TRIANGLES, S.BIND_BLAS_NODES, E.INST):
        assert opaque.arrays[b].tobytes() == ref.arrays[b].tobytes()
    bunny = E.base("bunny")
    tr = bunny.arrays[E.MAT]["transparency"] > 0
    assert tr.sum() == 1 and tr[3] and 3 in np.unique(bunny.arrays[S.BIND_TRIANGLES]["materialIndex"])     # "the only glass material"
    inst = E.base("instanced").arrays[E.INST]
    assert len(inst) == 17 and len(set(inst["blasNodeOffset"][1:].tolist())) == 1                         # shared views
    for name in E.BASES:
        b = E.base(name)
        assert np.concatenate(b.meshes).tobytes() == b.arrays[S.BIND_TRIANGLES].tobytes()
        assert len(b.objects) == len(b.arrays[E.INST])
        for (m, xf), it in zip(b.objects, b.arrays[E.INST]):
            assert int(it["globalTriOffset"]) == b.ranges[m][0] and np.asarray(xf).tobytes() == it["transform"].tobytes()
        tn, ti = E.tlas_for(b.arrays)                                               # the TLAS by hand is the host library's
        assert tn.tobytes() == b.arrays[S.BIND_TLAS_NODES].tobytes() and ti.tobytes() == b.arrays[S.BIND_TLAS_INDICES].tobytes()


def test_the_spare_glass_mesh_is_held_and_not_named():
    b = E.base("spare_glass")
    tris, inst = b.arrays[S.BIND_TRIANGLES], b.arrays[E.INST]
    n_glass = len(b.meshes[0])
    assert (tris["materialIndex"][:n_glass] == 3).all() and (tris["materialIndex"][n_glass:] != 3).all()
    assert b.arrays[E.MAT]["transparency"][3] > 0
    assert (inst["globalTriOffset"] >= n_glass).all() and (inst["blasNodeOffset"] > 0).all()       # nobody names the glass
    used = np.unique(tris["materialIndex"][n_glass:])
    assert not (b.arrays[E.MAT]["transparency"][used] > 0).any()                                # "an otherwise opaque scene"
    # once instance 2 names it, the arrays are the host library's own build of that scene (instances in another order)
    s = S.Scene(camera=b.camera)
    ids = [s.add_mesh(m) for m in b.meshes]
    s.add_object(ids[0], E.GLASS_T)
    s.add_object(ids[1], b.objects[0][1])
    s.add_object(ids[2], b.objects[1][1])
    s.build(share_meshes=True)
    final = E.case_arrays("I3")[3][-1]
    for k in (S.BIND_TRIANGLES, S.BIND_BLAS_NODES, S.BIND_BLAS_INDICES):
        assert final[k].tobytes() == s.arrays[k].tobytes()
    host = s.arrays[E.INST][[1, 2, 0]].copy()
    host["meshIndex"] = [0, 1, 2]
    assert final[E.INST].tobytes() == host.tobytes()
    a = oracle_render(b.view(final), E.W, E.H, E.SPP, E.BOUNCES)
    c = oracle_render(s, E.W, E.H, E.SPP, E.BOUNCES)
    assert _changed(a, c) == 0                                                                  # the order of the instances does not show
    assert E.case_arrays("I4")[3][-1][E.INST].tobytes() == inst.tobytes()


def test_i1_is_what_update_dynamic_gives():
    sc = S.instanced_scene(n=24, aspect=E.ASPECT)
    sc.set_transform(sc.instance_ids[4], E.I1_T)                 # instance 5: the floor is instance 0
    sc.update_dynamic()
    final = E.case_arrays("I1")[3][-1]
    for k in (E.INST,) + E.TLAS:
        assert final[k].tobytes() == sc.arrays[k].tobytes(), k


def test_the_array_partners_are_the_host_library_s():
    b = E.base("bunny")
    first, n = b.ranges[b.deform]
    moved = R.wobble(b.meshes[b.deform], 0.2)
    sc = S.bunny_scene(n=24, extras=True, aspect=E.ASPECT)
    sc.refit_mesh(1, moved)
    got = E.refit_arrays(b.arrays, first, moved)
    for k in S.GEOMETRY_BINDINGS:
        assert got[k].tobytes() == sc.arrays[k].tobytes(), k
    sc.rebuild_mesh(1)
    got = E.rebuild_arrays(b, got)
    for k in S.GEOMETRY_BINDINGS:
        assert got[k].tobytes() == sc.arrays[k].tobytes(), k
    assert len(got[S.BIND_BLAS_NODES]) != len(b.arrays[S.BIND_BLAS_NODES])                       # later meshes did move
    for name in ("reference_opaque", "spare_glass"):              # an untouched scene rebuilds to itself, empty and spare mesh included
        bb = E.base(name)
        arrays = E.case_arrays("I3")[3][-1] if name == "spare_glass" else bb.arrays
        again = E.rebuild_arrays(bb, arrays)
        for k in S.GEOMETRY_BINDINGS:
            assert again[k].tobytes() == arrays[k].tobytes(), (name, k)

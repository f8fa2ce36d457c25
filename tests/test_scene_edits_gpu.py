"""Material, light and instance edits of a live context (tests/scene_edits.py) on the GPU.  Every comparison is of bytes: the
edited context against a FRESH context that was given the final arrays by eight rz_uploads, and its frames also against the
oracle on those arrays.  A case in a prior state: build the context, bring it to the state, render a frame so that the layout
exists, apply the edit's calls, run one follower, and run the same follower on the fresh context.

Followers -- F1: a frame (bytes, kernel name, rz_debug_last_plan().transparent); F2: the first call after the edit is an
off-frame pass, with no render in between; F3: a geometry call, then the observable state and a frame; F4: rz_read_binding of
all eight bindings.  Prior states -- S0: uploaded; S1: after rz_update_transforms (the device owns instances and TLAS); S2:
geometry built on the device; S3: after a device-pointer refit (binding 0's host copy is stale); S4: after a refit and
rz_rebuild_geometry (bindings 7 and 8 live on the device, the layout read binding 0 where it was); S5: a context that lays
out on the host.  In S1, S3 and S4 the arrays in force are read from a twin context brought to the same state, so that
reading them does not disturb the state under test; on the context under test the frame comes before any rz_read_binding.
The other order has its own tests: in S1 .. S4 every binding is read back (twice) BEFORE the edit, so that both copies of every
array are current when it comes, and in S1 and S3 a second device call follows the read-back with no edit at all -- a look at
the host copies must leave the device's in force.

The row this table found: I3 in S3.  After a device-pointer refit the roots of meshes no instance names are unknown to the
device layout, so the spare glass view sends finalize to the host layout -- which read binding 0's stale host copy and laid
the refitted mesh out undeformed (472 of 3 072 pixels off).  The host fallback of finalize_body now fetches binding 0 first."""
import functools

import numpy as np
import pytest

import scene_edits as E
import skin_ref as K
from helpers import BACKENDS, mismatch_report, oracle_render
from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer, frame_params
from test_rays_gpu import Hip
from test_refit_gpu import HOST_RELAYOUT, _bits_equal, _frame, _state, _upload

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = E.W, E.H, E.SPP, E.BOUNCES
FLOOR = 30                      # pixels an edit must move in the oracle's frame (tests/test_scene_edits_cases.py)


def _render(r, b, arrays, nl):
    return _frame(r, b.view(arrays, nl), W, H, SPP, BOUNCES)[0]


def _oracle(b, arrays, nl):
    return oracle_render(b.view(arrays), W, H, SPP, BOUNCES, num_lights=nl)


@functools.lru_cache(maxsize=None)
def _s0(name):
    """The case on its base scene, with the oracle's frame at every "frame" among its calls and at the end (M6: none)."""
    b, calls, before, stages = E.case_arrays(name)
    nl0, nl = len(before[E.LIGHT]), E.num_lights(name, before)
    frames = [_oracle(b, a, nl if a is stages[-1] else nl0) for a in stages] if E.CASES[name].oracle else [None] * len(stages)
    return b, calls, before, stages, nl0, nl, frames


def _apply(r, calls, on_frame=None):
    for c in calls:
        if c.kind == "upload":
            r.upload(c.binding, c.array)
        elif c.kind == "update":
            r.update(c.binding, c.array, c.offset)
        else:
            on_frame()


def _apply_with_frames(r, b, calls, stages, nl0, frames, what):
    """The edit's calls; a "frame" among them renders one, held to the oracle on the arrays of that moment."""
    at = iter(range(len(stages) - 1))

    def on_frame():
        k = next(at)
        got = _render(r, b, stages[k], nl0)
        if frames[k] is not None:
            assert _bits_equal(got, frames[k]), f"{what}, frame {k} on the way vs the oracle: " + mismatch_report(got, frames[k])
    _apply(r, calls, on_frame)


def _check_frame(name, r, fresh, b, final, nl, oracle, what):
    """F1."""
    case = E.CASES[name]
    a, f = _render(r, b, final, nl), _render(fresh, b, final, nl)
    plan, fresh_plan = r.debug_last_plan()["transparent"], fresh.debug_last_plan()["transparent"]
    print(f"{what}: {r.last_kernel_name()} (fresh: {fresh.last_kernel_name()}), transparent {plan} (fresh: {fresh_plan})")
    assert _bits_equal(a, f), f"{what} vs the fresh context: " + mismatch_report(a, f)
    if oracle is not None:
        assert _bits_equal(a, oracle), f"{what} vs the oracle: " + mismatch_report(a, oracle)
    assert plan >= fresh_plan, what
    if case.transparent != E.AT_LEAST_FRESH:
        assert plan == case.transparent == fresh_plan, what
        assert r.last_kernel_name() == fresh.last_kernel_name(), what
        if r.last_kernel_name().startswith("rz_render_samples"):          # (rz_render_pixels carries no variant in its name)
            assert ("<glass>" in r.last_kernel_name()) == bool(case.transparent), what


def _check_bindings(r, final, what):
    """F4."""
    for k in S.BINDING_DTYPES:
        assert r.read_binding(k).tobytes() == final[k].tobytes(), f"{what}: binding {k}"


def _read_all(r):
    return {k: r.read_binding(k) for k in S.BINDING_DTYPES}


# ---- S0: F1 and F4 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", sorted(BACKENDS))
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_frame_and_bindings_after_the_edit(name, backend):
    b, calls, before, stages, nl0, nl, frames = _s0(name)
    what = f"{name} ({backend})"
    r = _upload(before, BACKENDS[backend])
    _render(r, b, before, nl0)
    _apply_with_frames(r, b, calls, stages, nl0, frames, what)
    fresh = _upload(stages[-1], BACKENDS[backend])
    _check_frame(name, r, fresh, b, stages[-1], nl, frames[-1], what)
    _check_bindings(r, stages[-1], what)
    r.close(); fresh.close()


# ---- S0: F2, the first call after the edit is an off-frame pass ------------------------------------------------------------

def _inputs():
    rng = np.random.default_rng(9)
    o = rng.uniform(-6, 6, (4000, 3)).astype(np.float32)
    d = rng.normal(size=(4000, 3)).astype(np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    rgb = np.stack([0.5 + 0.5 * np.sin(0.37 * x + 0.11 * y), 0.2 + x / W, 0.9 * ((x.astype(np.int32) ^ y.astype(np.int32)) & 3) / 3.0], -1).astype(np.float32)
    rgba = np.concatenate([rgb * SPP, np.full((H, W, 1), SPP, np.float32)], -1)
    return o, d, np.ascontiguousarray(rgb), np.ascontiguousarray(rgba)


RAY_O, RAY_D, RGB, RGBA = _inputs()


def _present(r):
    r.clear_accum()
    return r.present(show_lights=True, show_bvh=True)


FOLLOWERS = {
    "trace_rays": lambda r, cam, nl: list(r.trace_rays(RAY_O, RAY_D).values()),
    "shadow_rays": lambda r, cam, nl: list(r.shadow_rays(RAY_O, RAY_D, 20.0)),
    "render_editor": lambda r, cam, nl: list(r.render_editor(cam, W, H, num_lights=nl, rgb32f=True, hits=True)),
    "denoise": lambda r, cam, nl: list(r.denoise(RGBA, guides=True)),
    "upscale_seethrough": lambda r, cam, nl: list(r.upscale(RGB, factor=2, guides=True, see_through=8, chains=True)),
    "antialias_seethrough": lambda r, cam, nl: list(r.antialias(RGB, factor=2, guides=True, see_through=8, chains=True, edges=True)),
    "present": lambda r, cam, nl: list(_present(r)),
}


def _follow(r, which, cam, nl):
    r.set_frame(frame_params(cam, W, H, nl, BOUNCES, SPP))      # (no render: the frame's size, camera and num_lights only)
    return [np.ascontiguousarray(x).tobytes() for x in FOLLOWERS[which](r, cam, nl)]


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_first_call_after_the_edit_is_an_off_frame_pass(name):
    b, calls, before, stages, nl0, nl, _ = _s0(name)
    final = stages[-1]
    fresh, fresh_before = _upload(final), _upload(before)
    differs = []
    for which in FOLLOWERS:
        r = _upload(before)
        _render(r, b, before, nl0)
        _apply(r, calls, lambda: _render(r, b, before, nl0))
        got = _follow(r, which, b.camera, nl)
        want = _follow(fresh, which, b.camera, nl)
        stale = _follow(fresh_before, which, b.camera, nl0)
        r.close()
        assert len(got) == len(want)
        for k, (x, y) in enumerate(zip(got, want)):
            assert x == y, f"{name}: output {k} of {which} as the first call after the edit differs from the fresh context's"
        if want != stale:
            differs.append(which)
    fresh.close(); fresh_before.close()
    print(f"{name}: the fresh context's answer differs from the one before the edit in {differs or 'nothing'}")
    if E.CASES[name].changes_frame:
        assert differs, f"{name}: no off-frame pass tells the arrays after the edit from those before it"


# ---- S1 .. S5: F4 and F1 --------------------------------------------------------------------------------------------------

def _bring(state, b, hip):
    """A context holding the base scene in the prior state (no frame rendered yet)."""
    if state == "S2":
        r = Renderer(0)
        r.upload_scene_built_on_device(b.meshes, b.objects, b.arrays[E.MAT], b.arrays[E.LIGHT])
        return r
    r = _upload(b.arrays, HOST_RELAYOUT if state == "S5" else 0)
    if state == "S1":
        r.update_transforms(E.moved_transforms(b))
    elif state == "S3":
        _render(r, b, b.arrays, len(b.arrays[E.LIGHT]))          # (the refit patches a layout that exists)
        first, moved = E.deformed(b)
        r.refit_geometry_device(hip.upload(moved), first, len(moved))
    elif state == "S4":
        first, moved = E.deformed(b)
        r.refit_geometry(moved, first)
        rebuilt = r.rebuild_geometry(0.0)
        assert (rebuilt["flags"] & 1).any()
    return r


STATES = ("S1", "S2", "S3", "S4", "S5")


@pytest.mark.parametrize("name", E.IN_PRIOR_STATES)
@pytest.mark.parametrize("state", STATES)
def test_edit_in_a_prior_state(state, name):
    case = E.CASES[name]
    b = E.base(case.base)
    what = f"{name} in {state}"
    hip = Hip()
    r = _bring(state, b, hip)
    if state in ("S1", "S3", "S4"):
        twin = _bring(state, b, hip)
        current = _read_all(twin)
        twin.close()
        moved = [k for k in S.BINDING_DTYPES if current[k].tobytes() != b.arrays[k].tobytes()]
        assert S.BIND_INSTANCES in moved or S.BIND_TRIANGLES in moved, what                        # the state is not the base's
    else:
        current = b.arrays
    nl0 = len(current[E.LIGHT])
    _render(r, b, current, nl0)
    calls = case.edit(current)
    assert not any(c.kind == "frame" for c in calls)
    final = E.apply(calls, current)
    nl = E.num_lights(name, current)
    _apply(r, calls)
    fresh = _upload(final)
    oracle = _oracle(b, final, nl)
    moved = int((oracle.view(np.uint32) != _oracle(b, current, nl0).view(np.uint32)).any(axis=-1).sum())
    assert moved >= FLOOR, f"{what}: the edit moves {moved} pixels of the oracle's frame in this state"
    # F1 first: rz_read_binding brings the host copies up to date (binding 0 after a device-pointer refit, 7 and 8 of geometry
    # on the device), so the finalize that digests the edit must run before anything is read back
    _check_frame(name, r, fresh, b, final, nl, oracle, what)
    _check_bindings(r, final, what)
    r.close(); fresh.close()
    hip.close()


# ---- S1 .. S4 once every host copy has been refreshed: the order the tests above avoid ---------------------------------------

def _bring_and_read_back(state, b, hip, what):
    """The context in the state with a frame rendered and every binding read back twice, and the arrays in force (the twin's)."""
    r = _bring(state, b, hip)
    if state == "S2":
        current = b.arrays
    else:
        twin = _bring(state, b, hip)
        current = _read_all(twin)
        twin.close()
    _render(r, b, current, len(current[E.LIGHT]))
    first, second = _read_all(r), _read_all(r)
    for k in S.BINDING_DTYPES:
        assert first[k].tobytes() == second[k].tobytes(), f"{what}: binding {k}, read twice"
        assert first[k].tobytes() == current[k].tobytes(), f"{what}: binding {k} against the twin's"
    return r, current


def _check_against_fresh(name, r, b, current, final, nl, what):
    """The FLOOR condition on the oracle's frames, then F1 and F4 against a fresh context on `final`."""
    fresh = _upload(final)
    oracle = _oracle(b, final, nl)
    moved = int((oracle.view(np.uint32) != _oracle(b, current, len(current[E.LIGHT])).view(np.uint32)).any(axis=-1).sum())
    assert moved >= FLOOR, f"{what}: the step moves {moved} pixels of the oracle's frame in this state"
    _check_frame(name, r, fresh, b, final, nl, oracle, what)
    _check_bindings(r, final, what)
    fresh.close()


@pytest.mark.parametrize("name", E.AFTER_A_READ_BACK)
@pytest.mark.parametrize("state", ("S1", "S2", "S3", "S4"))
def test_edit_after_a_read_back(state, name):
    """test_edit_in_a_prior_state with the host copies refreshed first: both sides of every group are current when the edit comes."""
    case = E.CASES[name]
    b = E.base(case.base)
    what = f"{name} in {state} after a read-back"
    hip = Hip()
    r, current = _bring_and_read_back(state, b, hip, what)
    calls = case.edit(current)
    _apply(r, calls)
    _check_against_fresh(name, r, b, current, E.apply(calls, current), E.num_lights(name, current), what)
    r.close()
    hip.close()


@pytest.mark.parametrize("name", E.AFTER_A_READ_BACK)
@pytest.mark.parametrize("state", ("S1", "S3"))
def test_a_device_call_after_a_read_back(state, name):
    """A look leaves the device side in force: with no edit, a second rz_update_transforms (S1) or a second device-pointer refit
    (S3) follows the read-back, and the context answers as a fresh one on the arrays the host partners give."""
    b = E.base(E.CASES[name].base)
    what = f"{name}'s base in {state}, a device call after a read-back"
    hip = Hip()
    r, current = _bring_and_read_back(state, b, hip, what)
    if state == "S1":
        r.update_transforms(E.moved_transforms(b, again=True))
        final = E.moved_arrays(b, again=True)
    else:
        first, moved = E.deformed(b, again=True)
        r.refit_geometry_device(hip.upload(moved), first, len(moved))
        final = E.refit_arrays(current, first, moved)
    # (the materials are the base's: the kernel variant and the plan are the fresh context's, whatever the case says of its edit)
    fresh = _upload(final)
    nl = len(final[E.LIGHT])
    oracle = _oracle(b, final, nl)
    moved_px = int((oracle.view(np.uint32) != _oracle(b, current, nl).view(np.uint32)).any(axis=-1).sum())
    assert moved_px >= FLOOR, f"{what}: the call moves {moved_px} pixels of the oracle's frame"
    got, want = _render(r, b, final, nl), _render(fresh, b, final, nl)
    assert _bits_equal(got, want), f"{what} vs the fresh context: " + mismatch_report(got, want)
    assert _bits_equal(got, oracle), f"{what} vs the oracle: " + mismatch_report(got, oracle)
    assert r.last_kernel_name() == fresh.last_kernel_name(), what
    _check_bindings(r, final, what)
    r.close(); fresh.close()
    hip.close()


# ---- S0: F3, a geometry call follows the edit ------------------------------------------------------------------------------

GEOMETRY_CALLS = ("refit_geometry", "skin_pose", "rebuild_geometry", "geometry_quality")


@pytest.mark.parametrize("name", E.BEFORE_GEOMETRY_CALLS)
@pytest.mark.parametrize("call", GEOMETRY_CALLS)
def test_a_geometry_call_after_the_edit(call, name):
    b, calls, before, stages, nl0, nl, frames = _s0(name)
    final = stages[-1]
    what = f"{name}, then {call}"
    first, moved = E.deformed(b)
    r = _upload(before)
    _render(r, b, before, nl0)
    if call == "skin_pose":
        rig = K.bend(b.meshes[b.deform], 0.4)
        rid = r.skin_create(first, rig.rest, rig.skin, rig.n_bones)
    _apply_with_frames(r, b, calls, stages, nl0, frames, what)
    if call == "refit_geometry":
        r.refit_geometry(moved, first)
        want = E.refit_arrays(final, first, moved)
    elif call == "skin_pose":
        r.skin_pose(rid, rig.bones)
        want = E.refit_arrays(final, first, S.skin_triangles(rig.rest, rig.skin, rig.bones))
    elif call == "rebuild_geometry":
        r.rebuild_geometry(0.0)
        want = E.rebuild_arrays(b, final)
    else:
        assert len(r.geometry_quality()) == len(set(tuple(int(i[f]) for f in E.OFFSETS) for i in final[E.INST]))
        want = final
    fresh = _upload(want)
    got, ref = _state(r), _state(fresh)
    for k in S.GEOMETRY_BINDINGS:
        assert ref[k] == want[k].tobytes()
    for k in ref:
        assert got[k] == ref[k], f"{what}: {k} differs from the fresh context's"
    oracle = _oracle(b, want, nl) if E.CASES[name].oracle else None
    _check_frame(name, r, fresh, b, want, nl, oracle, what)
    r.close(); fresh.close()

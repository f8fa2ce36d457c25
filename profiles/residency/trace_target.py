"""The target of a `rocprofv3 --hip-runtime-trace --memory-copy-trace` run that counts, call by call, the device-to-host
copies and the hipStreamSynchronize calls of the entry points that read or write the caller's arrays.  The copies are counted
as hipMemcpy calls of the API trace: every synchronous copy the library makes in these steps is device to host (the fetches
of a host copy among them), and the memory-copy trace does not list copies of a few KB.  Its own device-to-host rows (the
frame and the present read-backs, asynchronous ones) are counted beside them.  One 64 x 48 scene
(tests/scene_edits.py: "bunny") is brought to each of the prior states S1 .. S4 of tests/test_scene_edits_gpu.py with a frame
rendered; then one step runs, then a frame.  Every step gets a context of its own, so each is counted in the state itself.
A step and the frame after it are each bracketed by two hipDeviceSynchronize calls of this driver (the library makes none),
and a line is printed at every bracket.

    rocprofv3 --hip-runtime-trace --memory-copy-trace --output-format csv -d OUT -- python profiles/residency/trace_target.py
    python profiles/residency/trace_target.py --count OUT            # one line per bracket: name, hipMemcpy calls, traced copies, synchronisations
    python profiles/residency/trace_target.py --table OUT_A OUT_B    # both builds side by side, as in README.md
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STATES = ("S1", "S2", "S3", "S4")
STEPS = ("read_binding x 8", "rz_update (material 1)", "rz_update (instance 1)", "rz_upload (materials)", "rz_update_transforms",
         "rz_refit_geometry (device pointer)", "rz_skin_pose", "rz_geometry_quality", "rz_rebuild_geometry",
         "rz_present (path overlay) 1", "rz_present (path overlay) 2", "rz_present (path overlay) 3")


def brackets():
    """The names of the brackets in the order the driver opens them."""
    out = []
    for state in STATES:
        for step in STEPS:
            out.append(f"{state}: {step}")
            if not step.startswith("rz_present"):
                out.append(f"{state}: {step}, then a frame")
    return out


def run():
    import numpy as np
    import scene_edits as E
    import skin_ref as K
    from rayzen_amd import scene as S
    from test_rays_gpu import Hip
    from test_refit_gpu import _frame
    from test_scene_edits_gpu import _bring

    hip = Hip()
    b = E.base("bunny")
    nl = len(b.arrays[E.LIGHT])
    first, moved = E.deformed(b, again=True)
    d_moved = hip.upload(moved)
    rig = K.bend(b.meshes[b.deform], 0.4)
    mats = b.arrays[E.MAT].copy()
    mats["albedo"][1] = (0.2, 0.3, 0.9)

    def frame(r):
        _frame(r, b.view(None, nl), E.W, E.H, E.SPP, E.BOUNCES)

    def bracket(name, fn):
        print(f"[residency] {name}", flush=True)
        hip.ok(hip.L.hipDeviceSynchronize())
        fn()
        hip.ok(hip.L.hipDeviceSynchronize())

    def step(r, name, rid):
        if name.startswith("read_binding"):
            for k in S.BINDING_DTYPES:
                r.read_binding(k)
        elif name == "rz_update (material 1)":
            r.update(E.MAT, mats[1:2], 32)
        elif name == "rz_update (instance 1)":
            rec = r_instances[1:2].copy()
            rec["transform"][0][13] += np.float32(0.25)
            rec["inverseTransform"][0] = S.inverse(rec["transform"][0])
            r.update(E.INST, rec, 144)
        elif name == "rz_upload (materials)":
            r.upload(E.MAT, mats)
        elif name == "rz_update_transforms":
            r.update_transforms(E.moved_transforms(b, again=True))
        elif name.startswith("rz_refit_geometry"):
            r.refit_geometry_device(d_moved, first, len(moved))
        elif name == "rz_skin_pose":
            r.skin_pose(rid, rig.bones)
        elif name == "rz_geometry_quality":
            r.geometry_quality()
        elif name == "rz_rebuild_geometry":
            r.rebuild_geometry(0.0)
        else:
            r.present(show_bvh=True, bvh_mode=1, selected_blas=1, selected_tri=0)

    for state in STATES:
        twin = _bring(state, b, hip)                # the instances in force, read from a twin: the context under test is not looked at
        r_instances = twin.read_binding(E.INST)
        twin.close()
        r = None
        for name in STEPS:
            if r is None or not name.startswith("rz_present (path overlay) ") or name.endswith(" 1"):
                if r is not None:
                    r.close()
                r = _bring(state, b, hip)
                frame(r)
                rid = r.skin_create(first, rig.rest, rig.skin, rig.n_bones) if name == "rz_skin_pose" else None
            bracket(f"{state}: {name}", lambda: step(r, name, rid))
            if not name.startswith("rz_present"):
                bracket(f"{state}: {name}, then a frame", lambda: frame(r))
        r.close()
    hip.close()


def _rows(out, pattern):
    files = sorted(glob.glob(os.path.join(out, "**", pattern), recursive=True))
    assert files, f"no {pattern} under {out}"
    for f in files:
        with open(f, newline="") as fh:
            yield from csv.DictReader(fh)


def count(out):
    """[(bracket, hipMemcpy calls, device-to-host rows of the memory-copy trace, hipStreamSynchronize calls)], by time stamp."""
    api = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"]) for r in _rows(out, "*hip_api_trace.csv")))
    marks = [(s, e) for s, e, f in api if f == "hipDeviceSynchronize"]
    names = brackets()
    assert len(marks) >= 2 * len(names), f"{len(marks)} hipDeviceSynchronize calls for {len(names)} brackets"
    syncs = [s for s, _, f in api if f == "hipStreamSynchronize"]
    copies = [s for s, _, f in api if f == "hipMemcpy"]
    d2h = [int(r["Start_Timestamp"]) for r in _rows(out, "*memory_copy_trace.csv") if "DEVICE_TO_HOST" in r["Direction"].upper()]
    res = []
    for k, name in enumerate(names):
        lo, hi = marks[2 * k][1], marks[2 * k + 1][1]       # (a copy enqueued in the bracket has ended when its closing call returns)
        res.append((name,) + tuple(sum(lo <= t < hi for t in ts) for ts in (copies, d2h, syncs)))
    return res


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--count":
        for name, copies, traced, syncs in count(sys.argv[2]):
            print(f"{name}: {copies} hipMemcpy calls, {traced} traced device-to-host copies, {syncs} synchronisations")
    elif len(sys.argv) > 3 and sys.argv[1] == "--table":
        a, b = count(sys.argv[2]), count(sys.argv[3])
        print("| state: step | hipMemcpy (device to host), A | B | traced device-to-host copies, A | B | hipStreamSynchronize, A | B | |")
        print("|---|---|---|---|---|---|---|---|")
        for (name, ca, ta, sa), (_, cb, tb, sb) in zip(a, b):
            more, fewer = (cb > ca or tb > ta or sb > sa), (cb < ca or tb < ta or sb < sa)
            print(f"| {name} | {ca} | {cb} | {ta} | {tb} | {sa} | {sb} | {'MORE' if more else 'fewer' if fewer else ''} |")
    else:
        run()


if __name__ == "__main__":
    main()

"""The three mutating calls on the scene of profiles/refit/README.md and profiles/skin/README.md -- a floor and `make_blob(76)`,
69 312 triangles, geometry built on the device -- timed with device events on a user stream: rz_refit_geometry with a device
pointer over the whole blob, rz_update_transforms, rz_skin_pose (host bones).  Median of 25 calls after one warm-up call each;
prints one JSON line.  Run once per process, alternating two builds through RAYZEN_HIP_SO.

    python profiles/residency/time_calls.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import refit_ref as R  # noqa: E402
import skin_ref as K  # noqa: E402
from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer  # noqa: E402
from test_rays_gpu import Hip  # noqa: E402
from test_refit_gpu import _median_ms  # noqa: E402


def main():
    hip = Hip()
    cube, blob = S.make_cube(4), S.make_blob(76, 2.8, 0)
    objects = [(0, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0))), (1, S.translate(S.identity(), (0.0, 2.0, 0.0)))]
    xf = np.stack([np.ascontiguousarray(t, np.float32).reshape(16) for _, t in objects])
    moved = R.wobble(blob, 0.2)
    rig = K.bend(blob, 0.4)
    stream = hip.stream()
    r = Renderer(0)
    r.set_stream(stream)
    r.upload_scene_built_on_device([cube, blob], objects, S.reference_materials(), S.reference_lights())
    r.update_transforms(xf)
    d_tris = hip.upload(moved)
    rid = r.skin_create(12, rig.rest, rig.skin, rig.n_bones)
    calls = {"refit_device": lambda: r.refit_geometry_device(d_tris, 12, len(moved)),
             "update_transforms": lambda: r.update_transforms(xf),
             "skin_pose": lambda: r.skin_pose(rid, rig.bones)}
    out = {}
    for name, fn in calls.items():
        fn()                                                        # warm-up (the refit's topology is derived once)
        out[name] = round(_median_ms(hip, stream, fn)[0], 5)
    out["so"] = os.environ.get("RAYZEN_HIP_SO", "")
    print(json.dumps(out), flush=True)
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()


if __name__ == "__main__":
    main()

"""The times of profiles/cost/README.md: rz_render_cost (a HIP event pair on the context's stream) against rz_render_counted and
rz_render on both backends (rz_last_render_ms), and rz_cost_view on both curves; medians of 7 after a warm-up, with the range.

    python profiles/cost/time_calls.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rayzen_amd import _lib, scene as S
from rayzen_amd.renderer import Renderer, frame_params
from test_rays_gpu import Hip

hip = Hip()
L = _lib.hip()
print("source", L.rz_source_hash().decode()[:12])


def timed(r, a, b, fn, reps=7):
    stream = L.rz_stream_handle(r._c)
    out = []
    for k in range(reps + 1):
        hip.ok(hip.L.hipEventRecord(a, stream))
        fn()
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        if k:
            out.append(float(ms.value))
    return float(np.median(out)), min(out), max(out)


for name, make in (("c2 bunny 69 312", lambda: S.bunny_scene(n=76)), ("c2g bunny + glass blob + mirror cube", lambda: S.bunny_scene(n=76, extras=True))):
    sc = make()
    for (w, h, spp) in ((480, 270, 1), (1920, 1080, 1), (1920, 1080, 16)):
        a, b = hip.event(), hip.event()
        res = {}
        for flags, label in ((1, "pixel"), (0, "samples")):
            r = Renderer(0, flags)
            r.upload_scene(sc)
            r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), 4, spp))
            if flags == 1:
                res["cost"] = timed(r, a, b, lambda: r.render_cost_device(None))
                d_rgb = hip.alloc(w * h * 12)
                res["view"] = timed(r, a, b, lambda: r.cost_view_device(d_rgb, None, None))
                res["view_log"] = timed(r, a, b, lambda: r.cost_view_device(d_rgb, None, None, curve="log"))
            ms = []
            for k in range(8):
                r.clear_accum()
                r.render_counted()
                r.sync()
                if k:
                    ms.append(r.last_render_ms()[0])
            res["counted_" + label] = (float(np.median(ms)), min(ms), max(ms))
            ms = []
            for k in range(8):
                r.clear_accum()
                r.render()
                r.sync()
                if k:
                    ms.append(r.last_render_ms()[0])
            res["render_" + label] = (float(np.median(ms)), min(ms), max(ms))
            r.close()
        print(f"{name} {w}x{h} {spp} spp 4 bounces: " + "; ".join(f"{k} {v[0]:.3f} ms ({v[1]:.3f}..{v[2]:.3f})" for k, v in res.items()), flush=True)
hip.close()

"""The times of profiles/coverage/README.md, each a HIP event pair on the context's stream, the calls of a group alternating for
12 rounds after a warm-up round; median and range.

  rz_coverage (device form, records and ids) with the default number of private sets of records (256 at most) and with a set
  per workgroup, 16 sets and 1 set (RZ_COVERAGE_SETS), against rz_denoise with iterations = 0 and guides (the same rays, 80 B per
  pixel written) and against rz_coverage writing ids alone (the cast and 4 B per pixel: what the reduction adds is the difference);
  rz_outline (rgba8 in place, the big mesh selected) against rz_display (manual exposure, rgb32f in, rgba8 out).

    python profiles/coverage/time_calls.py
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
W, H = 1920, 1080


def _alternate(hip, stream, calls, rounds):
    """GPU time (ms) of each call of `calls`, alternating them `rounds` times after a warm-up round."""
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


def show(name, ms):
    print(f"  {name:34s} {np.median(ms):.4f} ms ({min(ms):.4f}..{max(ms):.4f})", flush=True)


for name, make in (("bunny 69 312 + floor", lambda: S.bunny_scene()), ("bunny + glass blob + mirror cube", lambda: S.bunny_scene(extras=True)),
                   ("16 instances + floor", lambda: S.instanced_scene())):
    sc = make()
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 1))
    n = r.n_instances()
    d_cov, d_ids, d_guides = hip.alloc((n + 1) * 32), hip.alloc(W * H * 4), hip.alloc(W * H * 48)
    stream = L.rz_stream_handle(r._c)

    def cov(copies):
        def call():
            if copies:
                os.environ["RZ_COVERAGE_SETS"] = str(copies)
            r.coverage_device(d_cov, (n + 1) * 32, d_ids)
            os.environ.pop("RZ_COVERAGE_SETS", None)
        return call

    labels = ["coverage", "coverage, a set per workgroup", "coverage, 16 sets", "coverage, 1 set (atomics alone)",
              "coverage, ids alone", "denoise guides (iterations 0)"]
    times = _alternate(hip, stream, [cov(0), cov(1 << 20), cov(16), cov(1), lambda: r.coverage_device(None, 0, d_ids),
                                     lambda: r.denoise_device(guides_ptr=d_guides, iterations=0)], 12)
    print(f"{name}, {W}x{H}, {n} instances:")
    for lab, ms in zip(labels, times):
        show(lab, ms)
    d8, d32 = hip.alloc(W * H * 4, 0x40), hip.alloc(W * H * 12, 0)
    words, nsel = Renderer.selection_bits([1])
    d_sel = hip.upload(words)
    times = _alternate(hip, stream, [lambda: r.outline_device(W, H, d_ids, d_sel, nsel, rgba8_ptr=d8, alpha=0.5),
                                     lambda: r.outline_device(W, H, d_ids, d_sel, nsel, rgba8_ptr=d8, rgb32f_ptr=d32, radius=4, alpha=0.5),
                                     lambda: r.display_device(rgb_in_ptr=d32, rgba8_ptr=d8)], 12)
    for lab, ms in zip(["outline, rgba8, radius 2", "outline, rgba8 + rgb32f, radius 4", "display (rgb32f in, rgba8 out)"], times):
        show(lab, ms)
    r.sync()
    r.close()
hip.close()

"""The times of profiles/bloom/README.md, each a HIP event pair on the context's stream around one call in its device form, the
calls alternating for 25 rounds after a warm-up round; median and range.  The frame is the seeded 1920 x 1080 frame of
tests/bloom_ref.py in device memory (about half of its pixels glare at the default threshold).

  rz_bloom with the defaults (6 levels, 12 kernels), rgb32f alone, out of place and in place; with the glare as well; with
  levels = 1 and 8; from the accumulation (rgb_in NULL); with intensity 0 (a copy); against one a-trous pass (rz_denoise,
  iterations = 1) and rz_display (manual, clamp) on the same frame.  Before the times: the bytes the 12 kernels move, from the
  level sizes, and that the timed output equals the restatement's.

    python profiles/bloom/time_calls.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bloom_ref as BR
from rayzen_amd import _lib, scene as S
from rayzen_amd.renderer import Renderer, frame_params
from test_rays_gpu import Hip

hip = Hip()
L = _lib.hip()
print("source", L.rz_source_hash().decode()[:12])
W, H, ROUNDS = 1920, 1080, 25


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


def traffic(levels):
    """Bytes the kernels of one call read and write (rgb32f alone, out of place), each buffer counted once per kernel."""
    sizes = BR.level_sizes(W, H, levels)
    texels = [w * h for w, h in sizes]
    down = W * H * 12 + texels[0] * 16 + sum((a + b) * 16 for a, b in zip(texels, texels[1:]))
    up = sum((2 * a + b) * 16 for a, b in zip(texels, texels[1:]))
    combine = W * H * 24 + texels[0] * 16
    return down + up + combine


sc = S.reference_scene(aspect=W / H)
r = Renderer(0)
r.upload_scene(sc)
r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 1))
r.render()
c = BR.frame(W, H)
d_in, d_out, d_glare, d_8 = hip.upload(c), hip.alloc(c.nbytes), hip.alloc(c.nbytes), hip.alloc(W * H * 4)
d_inplace = hip.upload(c)
stream = L.rz_stream_handle(r._c)
r.bloom_device(d_in, d_out, None)
r.sync()
want = BR.bloom(c)[0]
same = hip.download(d_out, c.nbytes).tobytes() == want.tobytes()
print(f"{W}x{H}: the defaults move {traffic(6) / 1e6:.1f} MB in 12 kernels; output equals the restatement: {same}")
assert same

labels = ["bloom, defaults, rgb32f", "bloom, defaults, in place", "bloom, defaults, rgb32f + glare", "bloom, levels 1", "bloom, levels 8",
          "bloom, from the accumulation", "bloom, intensity 0 (a copy)", "denoise, iterations 1 (one a-trous pass)",
          "display, manual, clamp, rgb32f + rgba8"]
times = _alternate(hip, stream, [lambda: r.bloom_device(d_in, d_out, None), lambda: r.bloom_device(d_inplace, d_inplace, None),
                                 lambda: r.bloom_device(d_in, d_out, d_glare), lambda: r.bloom_device(d_in, d_out, None, levels=1),
                                 lambda: r.bloom_device(d_in, d_out, None, levels=8), lambda: r.bloom_device(None, d_out, None),
                                 lambda: r.bloom_device(d_in, d_out, None, intensity=0.0), lambda: r.denoise_device(d_out, iterations=1),
                                 lambda: r.display_device(d_in, d_out, d_8)], ROUNDS)
r.sync()
for lab, ms in zip(labels, times):
    print(f"  {lab:44s} {np.median(ms):.4f} ms ({min(ms):.4f}..{max(ms):.4f})", flush=True)
med = [float(np.median(t)) for t in times]
print(f"  bloom / a-trous pass: {med[0] / med[7]:.3f}; the defaults at {traffic(6) / med[0] / 1e9:.2f} TB/s of algorithmic traffic")
r.close()
hip.close()

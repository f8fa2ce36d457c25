"""The times of profiles/ao/README.md, each a HIP event pair on the context's stream around one call in its device form, the
calls of a group alternating for 25 rounds after a warm-up round; median and range.  Frames are 1920 x 1080, radius 2.

  rz_ambient_occlusion with smooth = 0 and ao alone (the guide cast and the walks, nothing to resolve) at N = 1, 4, 16; at N = 4
  with the gather (ao alone) and with all three outputs on an rgb32f input -- what the resolve kernel adds is the difference;
  against rz_denoise with iterations = 0 and guides (the same guide cast, 80 B per pixel written instead of 32) and
  rz_shadow_rays on the identical N = 4 rays already in device memory, with either scheduling flag.
  Also printed: which share of the walks ends lit (a miss, or a closest hit beyond the radius) -- what a walk culled at the
  radius could cut short.

    python profiles/ao/time_calls.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ao_ref as AR
from rayzen_amd import _lib, scene as S
from rayzen_amd.renderer import HIT_DTYPE, VISIBILITY_DTYPE, Renderer, frame_params
from test_rays_gpu import Hip

hip = Hip()
L = _lib.hip()
print("source", L.rz_source_hash().decode()[:12])
W, H, RADIUS, ROUNDS = 1920, 1080, 2.0, 25


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
    print(f"  {name:44s} {np.median(ms):.4f} ms ({min(ms):.4f}..{max(ms):.4f})", flush=True)


for name, make in (("reference_scene()", lambda: S.reference_scene()),
                   ("bunny 69 312 + floor + glass blob + mirror cube", lambda: S.bunny_scene(extras=True))):
    sc = make()
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 1))
    d_guides, d_ao, d_in, d_rgb, d_8 = (hip.alloc(W * H * b, 0) for b in (48, 4, 12, 12, 4))
    r.denoise_device(guides_ptr=d_guides, iterations=0)
    r.sync()
    g = AR.guide_of_hits(np.frombuffer(hip.download(d_guides, W * H * 48).tobytes(), HIT_DTYPE), sc.camera, W, H)
    rays, walked = AR.sample_rays(g, 4, RADIUS)
    d_rays, d_vis = hip.upload(rays), hip.alloc(len(rays) * 8)
    stream = L.rz_stream_handle(r._c)

    def ao(**kw):
        return lambda: r.ambient_occlusion_device(radius=RADIUS, **kw)

    labels = ["ao, N = 1, smooth 0, ao alone", "ao, N = 4, smooth 0, ao alone", "ao, N = 16, smooth 0, ao alone",
              "ao, N = 4, smooth 0, ao + rgba8", "ao, N = 4, smooth 1, ao alone", "ao, N = 4, smooth 1, all outputs on an image",
              "denoise guides (iterations 0)", "shadow_rays, the N = 4 rays", "shadow_rays, the N = 4 rays, incoherent"]
    times = _alternate(hip, stream, [ao(ao_ptr=d_ao, samples=1, smooth=False), ao(ao_ptr=d_ao, samples=4, smooth=False),
                                     ao(ao_ptr=d_ao, samples=16, smooth=False), ao(ao_ptr=d_ao, rgba8_ptr=d_8, samples=4, smooth=False),
                                     ao(ao_ptr=d_ao, samples=4), ao(rgb_in_ptr=d_in, ao_ptr=d_ao, rgb32f_ptr=d_rgb, rgba8_ptr=d_8, samples=4),
                                     lambda: r.denoise_device(guides_ptr=d_guides, iterations=0),
                                     lambda: r.shadow_rays_device(d_rays, d_vis, len(rays)),
                                     lambda: r.shadow_rays_device(d_rays, d_vis, len(rays), incoherent=True)], ROUNDS)
    r.sync()
    vis = np.frombuffer(hip.download(d_vis, len(rays) * 8).tobytes(), VISIBILITY_DTYPE)
    print(f"{name}, {W}x{H}: {int(g.hit.sum())} hit pixels of {W * H}, {len(rays)} walks at N = 4")
    for lab, ms in zip(labels, times):
        show(lab, ms)
    med = [float(np.median(t)) for t in times]
    print(f"  the gather adds {med[4] - med[1]:.4f} ms, a resolve without it {med[3] - med[1]:.4f} ms, the walks at N = 4 take "
          f"{med[1] - med[6]:.4f} ms or more (the guide cast of rz_denoise writes 48 B per pixel more)")
    lit = vis["lit"] != 0
    print(f"  walks that end lit: {lit.mean():.3f} of all; lit and unattenuated (a miss or a first hit beyond the radius): "
          f"{(lit & (vis['visibility'] == 1)).mean():.3f}")
    r.close()
hip.close()

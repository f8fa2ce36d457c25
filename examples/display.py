"""Measures the display stage (rz_display): milliseconds per call (device events, median of 25) at 800 x 600 and 1920 x 1080 on
device buffers -- metered exposure + ACES + sRGB (three launches), and a manual exposure with the same curve (one launch) --
beside rz_present_denoised with K = 0, the existing path that moves the same pixels without the stage; then what the meter saw
of a 1-spp frame of reference_scene and how the exposure adapts over a few calls.

    python examples/display.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402
from test_rays_gpu import Hip  # noqa: E402


def timed(r, hip, stream, fn, reps=25):
    a, b = hip.event(), hip.event()
    fn()
    r.sync()
    out = []
    for _ in range(reps):
        hip.ok(hip.L.hipEventRecord(a, stream))
        fn()
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        out.append(ms.value)
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    return float(np.median(out))


def main():
    hip = Hip()
    for W, H in ((800, 600), (1920, 1080)):
        sc = S.reference_scene(aspect=W / H)
        r = Renderer(0)
        r.upload_scene(sc)
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 5, 1, 0))
        r.render()
        n = W * H
        din, d32, d8 = hip.upload(r.denoise(iterations=0)), hip.alloc(n * 12), hip.alloc(n * 4)
        stream = hip.stream()
        r.set_stream(stream)
        auto = timed(r, hip, stream, lambda: r.display_device(din, d32, d8, auto=True, adapt=0.5, curve="aces", transfer="srgb"))
        manual = timed(r, hip, stream, lambda: r.display_device(din, d32, d8, exposure=1.5, curve="aces", transfer="srgb", keep=True))
        accum = timed(r, hip, stream, lambda: r.display_device(None, d32, d8, auto=True, adapt=0.5, curve="aces", transfer="srgb"))
        present = timed(r, hip, stream, lambda: r.present_denoised(iterations=0))
        shown = timed(r, hip, stream, lambda: r.present_display("accum", auto=True, adapt=0.5, curve="aces", transfer="srgb"))
        print(f"{W}x{H}: rz_display auto+ACES+sRGB {auto:.4f} ms (from the accumulation {accum:.4f}), manual+ACES+sRGB {manual:.4f} ms; "
              f"rz_present_denoised K=0 {present:.4f} ms, rz_present_display {shown:.4f} ms")
        r.set_stream(0)
        hip.L.hipStreamDestroy(stream)
        if (W, H) == (800, 600):
            r.display_reset()
            for k in range(4):
                r.display(auto=True, adapt=0.5, low=0.05, high=0.02, curve="aces", transfer="srgb")
                st = r.display_state()
                print(f"  call {k}: exposure {st['exposure']:.4f} target {st['target']:.4f} log2 mean {st['log2_mean']:.3f} "
                      f"counted {st['counted']} below {st['below']} above {st['above']}")
            hist = r.display_state()["histogram"]
            print("  occupied bins:", {int(b): int(hist[b]) for b in np.nonzero(hist)[0]})
        r.close()
    hip.close()


if __name__ == "__main__":
    main()

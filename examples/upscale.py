"""Measures rendering below display size: the C2 frame (bunny_scene, 64 spp, 4 bounces) rendered natively at 1920 x 1080 against
the same frame rendered at 960 x 540 and reconstructed at 1920 x 1080 by rz_upscale (factor 2) -- milliseconds on the device
(events on a user stream, median of 25): the two renders, the upscale on device buffers, its two guide casts alone, and
rz_denoise with K = 1 at 1920 x 1080, the one a-trous pass the stage is meant to cost about as much as.

    python examples/upscale.py
    python examples/upscale.py --see-through [--config c2g]

--see-through times rz_upscale next to rz_upscale_seethrough (max_depth 8: guides that follow glass and perfect mirrors) on one
config at 960 x 540 -> 1920 x 1080, with the share of high pixels whose chain goes past the first hit.
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


def see_through(config):
    """Both variants' times on one config (device events on a user stream, median of 25) and the chain-pixel share."""
    hip = Hip()
    sc, W, H, spp, bounces = S.named_config(config)
    s = 2
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W // s, H // s, len(sc.lights), bounces, 1, 0))
    stream = hip.stream()
    r.set_stream(stream)
    r.render()
    d32, dg, dc = hip.alloc(W * H * 12), hip.alloc(W * H * 48), hip.alloc(W * H * 16)
    t = {"first-hit": timed(r, hip, stream, lambda: r.upscale_device(None, d32, None, factor=s)),
         "first-hit high guide": timed(r, hip, stream, lambda: r.upscale_device(None, None, dg, factor=s))}
    depths = (0, 8) if hasattr(r._L, "rz_upscale_seethrough") else ()      # (an older library: rz_upscale's time alone)
    for md in depths:
        t[f"see-through {md}"] = timed(r, hip, stream, lambda: r.upscale_device(None, d32, None, factor=s, see_through=md))
        t[f"see-through {md} high guide"] = timed(r, hip, stream, lambda: r.upscale_device(None, None, dg, factor=s, see_through=md))
    k = np.zeros(1, np.int32)
    if depths:
        r.upscale_device(None, None, None, factor=s, see_through=8, chains_ptr=dc)
        r.sync()
        k = hip.download(dc, W * H * 16).view(np.int32).reshape(-1, 4)[:, 3] & 0xFF
    r.set_stream(0)
    hip.L.hipStreamDestroy(stream)
    r.close()
    hip.close()
    print(f"{config}: {W // s}x{H // s} -> {W}x{H}; chain pixels {(k > 0).mean():.4f}, mean queries per pixel {1 + k.mean():.4f}, "
          f"deepest chain {int(k.max())}")
    print(f"  rz_upscale:                        {t['first-hit']:.3f} ms (the {W}x{H} guide cast alone: {t['first-hit high guide']:.3f} ms)")
    for md in depths:
        print(f"  rz_upscale_seethrough max_depth {md}: {t[f'see-through {md}']:.3f} ms (the {W}x{H} guide cast alone: "
              f"{t[f'see-through {md} high guide']:.3f} ms) = {t[f'see-through {md}'] / t['first-hit']:.3f} of rz_upscale")


def main():
    if "--see-through" in sys.argv:
        config = sys.argv[sys.argv.index("--config") + 1] if "--config" in sys.argv else "c2"
        return see_through(config)
    hip = Hip()
    sc, W, H, spp, bounces = S.named_config("c2")
    s = 2
    t = {}
    for what, (w, h) in (("native", (W, H)), ("low", (W // s, H // s))):
        r = Renderer(0)
        r.upload_scene(sc)
        r.set_frame(frame_params(sc.camera, w, h, len(sc.lights), bounces, spp, 0))
        stream = hip.stream()
        r.set_stream(stream)
        t[f"render {what}"] = timed(r, hip, stream, r.render)
        d32 = hip.alloc(W * H * 12)
        dg = hip.alloc(W * H * 48)
        if what == "low":
            t["upscale"] = timed(r, hip, stream, lambda: r.upscale_device(None, d32, None, factor=s))
            t["high guide"] = timed(r, hip, stream, lambda: r.upscale_device(None, None, dg, factor=s))
        else:
            t["denoise K=1"] = timed(r, hip, stream, lambda: r.denoise_device(d32, iterations=1))
            t["denoise K=5"] = timed(r, hip, stream, lambda: r.denoise_device(d32))
        r.set_stream(0)
        hip.L.hipStreamDestroy(stream)
        r.close()
    hip.close()
    print(f"C2 {spp} spp, {bounces} bounces")
    print(f"  rz_render {W}x{H}: {t['render native']:.3f} ms")
    print(f"  rz_render {W // s}x{H // s}: {t['render low']:.3f} ms")
    print(f"  rz_upscale {W // s}x{H // s} -> {W}x{H}: {t['upscale']:.3f} ms (the {W}x{H} guide cast alone: {t['high guide']:.3f} ms)")
    print(f"  rz_denoise {W}x{H}: K=1 {t['denoise K=1']:.3f} ms, K=5 {t['denoise K=5']:.3f} ms")
    total = t["render low"] + t["upscale"]
    print(f"  low render + upscale: {total:.3f} ms = {total / t['render native']:.3f} of the native frame "
          f"(saves {t['render native'] - total:.3f} ms; the upscale is {t['upscale'] / (t['render native'] - t['render low']):.3f} of what the smaller render saves)")


if __name__ == "__main__":
    main()

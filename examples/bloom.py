"""Renders reference_scene and presents it twice through the display stage (auto exposure, ACES, sRGB): plain
(rz_present_display) and with glare in front of it (rz_present_bloomed).  Prints which share of the frame glares, how much light
the pass adds, what the metered exposure makes of it, and the time of rz_bloom on device buffers (device events, median of 25)
beside one a-trous pass; writes both frames as PPM files when given a directory.

    python examples/bloom.py [OUTDIR]
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


def write_ppm(path, rgba8):
    h, w = rgba8.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgba8[::-1, :, :3]).tobytes())       # row 0 is the bottom row


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else None
    hip = Hip()
    W, H, spp = 1920, 1080, 8
    sc = S.reference_scene(aspect=W / H)
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, spp, 0))
    r.render()
    display = dict(auto=True, low=0.05, high=0.02, curve="aces", transfer="srgb", show_fps=False)
    bloom = dict(threshold=1.0, knee=0.5, intensity=0.25)
    _, plain = r.present_display(**display)
    e_plain = r.display_state()["exposure"]
    r.display_reset()
    _, bloomed = r.present_bloomed(bloom=bloom, **display)
    e_bloomed = r.display_state()["exposure"]
    out, glare = r.bloom(glare=True, **bloom)
    c = out - np.float32(bloom["intensity"]) * glare
    over = (np.nan_to_num(c).max(axis=-1) > bloom["threshold"]).mean()
    print(f"{W}x{H}, {spp} spp: {over:.2%} of the pixels are over the threshold; the glare's mean is {glare.mean():.4f} and reaches "
          f"{(glare.max(axis=-1) > 1e-3).mean():.2%} of the frame")
    print(f"metered exposure {e_plain:.4f} plain, {e_bloomed:.4f} with glare; {(plain != bloomed).any(axis=-1).mean():.2%} of the "
          f"presented pixels differ")
    n = W * H
    din, d32 = hip.upload(out), hip.alloc(n * 12)
    stream = hip.stream()
    r.set_stream(stream)
    t_bloom = timed(r, hip, stream, lambda: r.bloom_device(din, d32, None, **bloom))
    t_accum = timed(r, hip, stream, lambda: r.bloom_device(None, d32, None, **bloom))
    t_atrous = timed(r, hip, stream, lambda: r.denoise_device(d32, iterations=1))
    print(f"rz_bloom {t_bloom:.4f} ms (from the accumulation {t_accum:.4f}); one a-trous pass {t_atrous:.4f} ms")
    r.set_stream(0)
    hip.L.hipStreamDestroy(stream)
    if outdir:
        os.makedirs(outdir, exist_ok=True)
        write_ppm(os.path.join(outdir, "plain.ppm"), plain)
        write_ppm(os.path.join(outdir, "bloomed.ppm"), bloomed)
        print("wrote", os.path.join(outdir, "plain.ppm"), "and", os.path.join(outdir, "bloomed.ppm"))
    r.close()
    hip.close()


if __name__ == "__main__":
    main()

"""A ray-cast viewport with contact and depth: rz_render_editor's rgb32f fed through rz_ambient_occlusion, all on the device.

    python examples/ambient_occlusion.py [--config reference|bunny|instanced] [--size 1920x1080] [--samples 4] [--radius 2]
                                         [--out ao.ppm]

Prints the time of the two calls (events on the context's stream, median of 25) and the share of pixels the pass darkens; with
--out it writes the darkened frame as a binary PPM (row 0 of the image is the top row).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from rayzen_amd import _lib  # noqa: E402
from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402

CONFIGS = {"reference": lambda: S.reference_scene(aspect=16 / 9), "bunny": lambda: S.bunny_scene(extras=True),
           "instanced": lambda: S.instanced_scene()}


def timed(hip, stream, fn, reps=25):
    a, b = hip.event(), hip.event()
    fn()
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="reference", choices=sorted(CONFIGS))
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    from test_rays_gpu import Hip
    hip = Hip()
    sc = CONFIGS[args.config]()
    r = Renderer(0)
    r.upload_scene(sc)
    fp = frame_params(sc.camera, w, h, len(sc.lights), 1, 1)
    d_rgb, d_ao, d_out8 = hip.alloc(w * h * 12), hip.alloc(w * h * 4), hip.alloc(w * h * 4)
    stream = _lib.hip().rz_stream_handle(r._c)

    def editor():
        r.render_editor_device(sc.camera, w, h, rgb32f_ptr=d_rgb)

    def occlusion():
        r.ambient_occlusion_device(fp, rgb_in_ptr=d_rgb, ao_ptr=d_ao, rgba8_ptr=d_out8, samples=args.samples, radius=args.radius)

    t_editor, t_ao = timed(hip, stream, editor), timed(hip, stream, occlusion)
    r.sync()
    ao = np.frombuffer(hip.download(d_ao, w * h * 4).tobytes(), np.float32)
    print(f"{args.config} {w}x{h}: rz_render_editor {t_editor:.3f} ms + rz_ambient_occlusion (N = {args.samples}, radius {args.radius:g}, "
          f"smoothed) {t_ao:.3f} ms; {float((ao < 1).mean()):.1%} of the pixels darkened, mean ao {float(ao.mean()):.3f}")
    if args.out:
        img = np.frombuffer(hip.download(d_out8, w * h * 4).tobytes(), np.uint8).reshape(h, w, 4)[::-1, :, :3]
        with open(args.out, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
        print("wrote", args.out)
    r.close()
    hip.close()


if __name__ == "__main__":
    main()

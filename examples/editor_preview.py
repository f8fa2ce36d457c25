"""GPU time of one editor-preview frame (rz_render_editor, RGBA8 into device memory) against rz_trace_rays on the same pixel
rays; prints ONE JSON line.

    python3 examples/editor_preview.py [--reps 20] [--warmup 3] [--scenes c2,c2close,c4,c5,ref]

Scenes and sizes: c2, c2close, c4 at 1920 x 1080; c5 (the ~1 M-triangle stress mesh) at 3840 x 2160; ref (RayZen's own
scene) at 800 x 600.  Per scene, medians of `--reps` launches after `--warmup`, device events on a stream of our own:
  * editor_ms:       rz_render_editor, 64 pixels of one row per wave (the default);
  * editor_tiles_ms: the same with RZ_EDITOR_TILES=1 (a wave covers an 8 x 8 tile: the A/B of the wave's shape);
  * trace_tiles_ms:  rz_trace_rays on editor_rays(), reordered tile by tile (64 rays per wave = one 8 x 8 tile);
  * trace_rows_ms:   rz_trace_rays on editor_rays() as returned (pixel order: 64 rays of one row per wave).
The editor frame does the trace of the first and, on top, the clip test and the shading, but loads no ray and stores 4 B
instead of a 48-B hit per pixel."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from rayzen_amd import scene as S                                   # noqa: E402
from rayzen_amd.renderer import Renderer, editor_rays               # noqa: E402
from test_rays_gpu import Hip                                       # noqa: E402

SIZES = {"c2": (1920, 1080), "c2close": (1920, 1080), "c4": (1920, 1080), "c5": (3840, 2160), "ref": (800, 600)}


def tile_order(W, H):
    ty, tx, ly, lx = np.meshgrid(np.arange((H + 7) // 8), np.arange((W + 7) // 8), np.arange(8), np.arange(8), indexing="ij")
    px, py = (tx * 8 + lx).ravel(), (ty * 8 + ly).ravel()
    keep = (px < W) & (py < H)
    return py[keep] * W + px[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="c2,c2close,c4,c5,ref")
    a = ap.parse_args()
    hip = Hip()
    out = {"reps": a.reps, "warmup": a.warmup, "scenes": {}}
    for name in a.scenes.split(","):
        W, H = SIZES[name]
        sc = S.named_config(name)[0] if name != "c5" else S.stress_scene(n=289, aspect=W / H)
        r = Renderer(0)
        r.upload_scene(sc)
        stream = hip.stream()
        r.set_stream(stream)
        n = W * H
        rays = editor_rays(sc.camera, W, H)
        d_rows, d_tiles = hip.upload(rays), hip.upload(rays[tile_order(W, H)])
        d_hits, d8 = hip.alloc(n * 48), hip.alloc(n * 4)
        e0, e1 = hip.event(), hip.event()

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            r.sync()
            ts = []
            for _ in range(a.reps):
                hip.ok(hip.L.hipEventRecord(e0, stream))
                fn()
                hip.ok(hip.L.hipEventRecord(e1, stream))
                hip.ok(hip.L.hipEventSynchronize(e1))
                ms = C.c_float()
                hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), e0, e1))
                ts.append(ms.value)
            return round(float(np.median(ts)), 4)

        res = {"width": W, "height": H, "triangles": int(len(sc.arrays[S.BIND_TRIANGLES]))}
        res["editor_ms"] = timed(lambda: r.render_editor_device(sc.camera, W, H, rgba8_ptr=d8))
        os.environ["RZ_EDITOR_TILES"] = "1"
        res["editor_tiles_ms"] = timed(lambda: r.render_editor_device(sc.camera, W, H, rgba8_ptr=d8))
        del os.environ["RZ_EDITOR_TILES"]
        res["trace_tiles_ms"] = timed(lambda: r.trace_rays_device(d_tiles, d_hits, n))
        res["trace_rows_ms"] = timed(lambda: r.trace_rays_device(d_rows, d_hits, n))
        res["editor_over_trace_rows"] = round(res["editor_ms"] / res["trace_rows_ms"], 3)
        px = hip.download(d8, n * 4).reshape(H, W, 4)
        res["pixels_not_clear"] = round(float((px[..., :3] != np.array([13, 13, 18], np.uint8)).any(-1).mean()), 4)   # rint((0.05, 0.05, 0.07) * 255)
        out["scenes"][name] = res
        r.set_stream(0)
        r.close()
        hip.L.hipEventDestroy(e0)
        hip.L.hipEventDestroy(e1)
        hip.L.hipStreamDestroy(stream)
        hip.close()
        print(name, res, file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Drives rz_denoise_temporal over a sequence: an orbiting camera and moving instances (instanced_scene, rz_update_transforms
every frame), one sample per pixel per frame.  Prints the device time of every call (device events around the call on a user
stream) and the history it reached; where the CPU oracle is importable, also the MSE of the raw last frame and of the temporal
output against a 256-spp render of the last frame, and their ratio.

    python examples/temporal.py [frames] [width] [height]
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


def orbit(base, angle):
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return S.Camera(position=tuple(R @ np.asarray(base.position, np.float64)), target=tuple(R @ np.asarray(base.target, np.float64)),
                    up=tuple(base.up), fov=base.fov, aspect=base.aspect, near=base.near, far=base.far)


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 640
    H = int(sys.argv[3]) if len(sys.argv) > 3 else 360
    hip = Hip()
    sc = S.instanced_scene(n=24, count=16, aspect=W / H)
    base = sc.camera
    floor = np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], np.float32)
    r = Renderer(0)
    r.upload_scene(sc)
    stream = hip.stream()
    r.set_stream(stream)
    d32, dst = hip.alloc(W * H * 12), hip.alloc(W * H * 8)
    a, b = hip.event(), hip.event()
    xf = None
    for fr in range(frames):
        # the per-frame order ("Temporal accumulation")
        moves = S.instanced_transforms(0.25 * fr, 16)
        xf = np.stack([floor] + [np.asarray(t, np.float32).reshape(16) for t in moves])
        r.update_transforms(xf)
        sc.camera = orbit(base, np.radians(0.25) * fr)
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 5, 1, fr))
        r.clear_accum()
        r.render()
        hip.ok(hip.L.hipEventRecord(a, stream))
        r.denoise_temporal_device(d32, None, dst)
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        n = hip.download(dst, W * H * 8).view(np.float32).reshape(H, W, 2)[..., 0]
        print(f"frame {fr:3d}: rz_denoise_temporal {ms.value:.3f} ms, history mean {n.mean():.2f} max {n.max():.0f}, "
              f"restarted {float((n == 1).mean()) * 100:.2f} % of the pixels")
    out = hip.download(d32, W * H * 12).view(np.float32).reshape(H, W, 3)
    raw = r.read_accum()
    r.set_stream(0)
    hip.L.hipStreamDestroy(stream)
    r.close()
    hip.close()
    try:
        import helpers
        from oracle import rzo
    except Exception as e:                  # the oracle is test infrastructure: the example runs without it
        print(f"(no CPU oracle: {e})")
        return
    for oid, t in zip(sc.instance_ids, moves):
        sc.set_transform(oid, t)
    sc.update_dynamic()
    if W * H > 200 * 150:
        print("(the 256-spp reference on the CPU oracle is only rendered for frames of at most 200 x 150)")
        return
    hi = helpers.oracle_render(sc, W, H, 256, 5)
    tgt = hi[..., :3] / hi[..., 3:]
    c1 = raw[..., :3] / np.maximum(raw[..., 3:], 1)
    m_raw, m_out = float(np.mean((c1 - tgt) ** 2)), float(np.mean((out - tgt) ** 2))
    print(f"MSE vs 256 spp: raw last frame {m_raw:.4g}, temporal output {m_out:.4g}, ratio {m_raw / m_out:.2f}")


if __name__ == "__main__":
    main()

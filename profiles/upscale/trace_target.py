"""The target of a `rocprofv3 --kernel-trace --stats` run: 25 rz_upscale calls (960 x 540 -> 1920 x 1080, device buffers, the
accumulation as input) on C2's scene after one untimed call, so the per-kernel averages split the call into its two guide casts
and the gather.

    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/upscale/trace_target.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402
from test_rays_gpu import Hip  # noqa: E402


def main():
    hip = Hip()
    sc, W, H, _, bounces = S.named_config("c2")
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W // 2, H // 2, len(sc.lights), bounces, 1, 0))
    r.render()
    d32 = hip.alloc(W * H * 12)
    for _ in range(26):
        r.upscale_device(None, d32, None, factor=2)
    r.sync()
    r.close()
    hip.close()


if __name__ == "__main__":
    main()

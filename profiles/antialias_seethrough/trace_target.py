"""The target of a `rocprofv3 --kernel-trace --stats` run: 26 rz_antialias calls and 26 rz_antialias_seethrough calls (max_depth 8)
on one config's scene at 1920 x 1080, factor 2 (device buffers, the accumulation as input), so the per-kernel averages split both
calls into their frame-size cast and their edge kernel.

    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/antialias_seethrough/trace_target.py [c2|c2g]
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
    sc, W, H, _, bounces = S.named_config(sys.argv[1] if len(sys.argv) > 1 else "c2g")
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), bounces, 1, 0))
    r.render()
    d32 = hip.alloc(W * H * 12)
    for _ in range(26):
        r.antialias_device(None, d32, None, None, factor=2)
    for _ in range(26):
        r.antialias_device(None, d32, None, None, factor=2, see_through=8)
    r.sync()
    r.close()
    hip.close()


if __name__ == "__main__":
    main()

"""An editor viewport without GL: the ray-cast preview of bunny_scene(extras=True) (Renderer.render_editor), darkened by ambient
occlusion (Renderer.ambient_occlusion), then the editor's own geometry drawn into it with Renderer.draw_lines -- a ground grid,
the selected object's box in its own space, gizmo axes at its origin, all depth-tested against the preview's hits, the hidden
parts of the box and the axes shown faintly -- and last the selection's outline (Renderer.outline).

Prints what each stage changed and writes the frame (H x W x 4 uint8, row 0 = bottom) as gizmos.npy, and as gizmos.ppm (top row
first) for a viewer.

    python examples/gizmos.py [outdir]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from rayzen_amd import lines as LN  # noqa: E402
from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402

W, H = 1920, 1080
SELECTED = 1                                                # the bunny


def main(outdir="."):
    os.makedirs(outdir, exist_ok=True)
    sc = S.bunny_scene(extras=True)
    cam = sc.camera
    r = Renderer(0)
    r.upload_scene(sc)
    fp = frame_params(cam, W, H, len(sc.lights), 1, 1)
    _, rgb, hits = r.render_editor(cam, W, H, rgb32f=True, hits=True)
    shaded = r.ambient_occlusion(fp, rgb=rgb, want=("rgba8",))["rgba8"]
    print(f"preview {W}x{H}: {int((hits['instance'] >= 0).sum())} pixels hit; ambient occlusion darkened "
          f"{int((shaded[..., :3].astype(int).sum(-1) < np.rint(np.clip(rgb, 0, 1) * 255).sum(-1)).sum())} of them")
    # the grid lies in the floor's plane: its depth differs from the floor's by what a pixel's offset from the line is worth,
    # so it is drawn with a bias of its own; hidden_alpha = 0 hides what the objects cover
    floor_y = float(np.median(hits["point"][hits["instance"] == 0][:, 1]))     # where the preview met the floor (instance 0)
    grid = LN.grid(20.0, 1.0, (200, 200, 210, 110), y=floor_y)
    frame, _ = r.draw_lines(grid, rgba8=shaded, hits=hits, frame=fp, width=1.0, depth_bias=1.0 / 64.0, smooth=True)
    print(f"grid: {len(grid)} lines, {int((frame != shaded).any(-1).sum())} pixels")
    # the selection's box is its BLAS root box, given in the instance's own space; the axes stand at its origin
    root = sc.arrays[S.BIND_BLAS_NODES][sc.arrays[S.BIND_INSTANCES]["blasNodeOffset"][SELECTED]]
    gizmo = np.concatenate([LN.box(root["boundsMin"], root["boundsMax"], (255, 160, 0, 255), instance=SELECTED),
                            LN.axes((0.0, 0.0, 0.0), 3.5, instance=SELECTED)])
    before = frame
    frame, _ = r.draw_lines(gizmo, rgba8=frame, hits=hits, frame=fp, width=2.0, hidden_alpha=0.25, smooth=True)
    print(f"box and axes: {len(gizmo)} lines, {int((frame != before).any(-1).sum())} pixels")
    before = frame
    frame, _ = r.outline(hits["instance"], [SELECTED], rgba8=frame, radius=2)
    print(f"outline: {int((frame != before).any(-1).sum())} pixels")
    np.save(os.path.join(outdir, "gizmos.npy"), frame)
    with open(os.path.join(outdir, "gizmos.ppm"), "wb") as f:
        f.write(b"P6 %d %d 255\n" % (W, H) + frame[::-1, :, :3].tobytes())
    r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")

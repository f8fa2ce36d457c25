"""A wobbling bunny_scene: per frame the mesh is displaced (x += A sin(3y + phase), z += A cos(2x)), handed to
rz_refit_geometry and rendered.  Prints, as medians over the frames, the refit (device events, TLAS step included), the frame,
and the same with a rebuild every frame (rz_build_geometry + the re-layout its next render triggers).

    python examples/deform.py [n] [frames]        # n: blob size (76 -> 69 312 triangles), default 76; frames: default 24
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


def wobble(tris, amplitude, phase):
    out = tris.copy()
    a = np.float32(amplitude)
    for f in ("v0", "v1", "v2"):
        v = out[f].copy()
        v[:, 0] = v[:, 0] + a * np.sin(np.float32(3.0) * v[:, 1] + np.float32(phase))
        v[:, 2] = v[:, 2] + a * np.cos(np.float32(2.0) * v[:, 0])
        out[f] = v.astype(np.float32)
    return out


def elapsed(hip, a, b):
    hip.ok(hip.L.hipEventSynchronize(b))
    ms = C.c_float()
    hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
    return ms.value


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 76
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    W, H, spp, bounces = 1920, 1080, 16, 4
    hip = Hip()
    cube, blob = S.make_cube(4), S.make_blob(n, 2.8, 0)
    objects = [(0, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0))), (1, S.translate(S.identity(), (0.0, 2.0, 0.0)))]
    cam = S.Camera(position=(0.0, 2.5, 10.0), aspect=W / H)
    xf = np.stack([np.ascontiguousarray(t, np.float32).reshape(16) for _, t in objects])
    r = Renderer(0)
    stream = hip.stream()
    r.set_stream(stream)
    r.upload_scene_built_on_device([cube, blob], objects, S.reference_materials(), S.reference_lights())
    r.set_frame(frame_params(cam, W, H, 2, bounces, spp))
    r.render()
    r.sync()
    a, b = hip.event(), hip.event()
    d_tris = hip.alloc(blob.nbytes)
    for how in ("refit", "rebuild"):
        step_ms, frame_ms = [], []
        for f in range(frames + 1):             # (frame 0 warms up: the refit derives its topology once per layout)
            moved = wobble(blob, 0.2, 0.26 * f)
            if how == "refit":
                hip.ok(hip.L.hipMemcpy(d_tris, moved.ctypes.data, moved.nbytes, 1))     # (a skinning kernel would write them there)
                hip.ok(hip.L.hipEventRecord(a, stream))
                r.refit_geometry_device(d_tris, len(cube), len(moved))
                hip.ok(hip.L.hipEventRecord(b, stream))
            else:
                hip.ok(hip.L.hipEventRecord(a, stream))
                r.build_geometry(np.concatenate([cube, moved]), [(0, len(cube)), (len(cube), len(moved))])
                r.update_transforms(xf)         # the re-layout happens here
                hip.ok(hip.L.hipEventRecord(b, stream))
            r.clear_accum()
            r.render()
            r.sync()
            if f:
                step_ms.append(elapsed(hip, a, b))
                frame_ms.append(r.last_render_ms()[0])
        print(f"{how:8s} {len(blob)} triangles: {how} {np.median(step_ms):.3f} ms, frame ({W}x{H}, {spp} spp) {np.median(frame_ms):.3f} ms")
    r.set_stream(0)
    r.close()
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    hip.L.hipStreamDestroy(stream)
    hip.close()


if __name__ == "__main__":
    main()

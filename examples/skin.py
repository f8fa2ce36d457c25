"""A bending bunny_scene: the blob hangs on two bones (weights from the corner's height), and per frame the upper bone turns
about the blob's middle.  rz_skin_pose skins the mesh on the device from the rest pose its rig keeps there, refits the BLAS
and rebuilds the TLAS; only the two bones (128 B) cross to the device.  Prints, as medians over the frames: the pose call
(device events, refit and TLAS included), the skinning kernel alone, a device-to-device copy of 96 B per triangle on the same
stream (the yardstick: it moves the 192 B per triangle the skin-only kernel moves), the frame, and the same through the host
route the call replaces: skinning in numpy, hipMemcpy of the triangles, rz_refit_geometry on them.

    python examples/skin.py [n] [frames] [spp]    # n: blob size (76 -> 69 312 triangles), default 76; frames: default 24
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import skin_ref as K  # noqa: E402
from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402
from test_rays_gpu import Hip  # noqa: E402


def elapsed(hip, a, b):
    hip.ok(hip.L.hipEventSynchronize(b))
    ms = C.c_float()
    hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
    return ms.value


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 76
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    spp = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    W, H, bounces = 1920, 1080, 4
    hip = Hip()
    hip.L.hipMemcpyAsync.restype, hip.L.hipMemcpyAsync.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    cube, blob = S.make_cube(4), S.make_blob(n, 2.8, 0)
    objects = [(0, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0))), (1, S.translate(S.identity(), (0.0, 2.0, 0.0)))]
    cam = S.Camera(position=(0.0, 2.5, 10.0), aspect=W / H)
    r = Renderer(0)
    stream = hip.stream()
    r.set_stream(stream)
    r.upload_scene_built_on_device([cube, blob], objects, S.reference_materials(), S.reference_lights())
    r.set_frame(frame_params(cam, W, H, 2, bounces, spp))
    r.render()
    r.sync()
    skin, y_range = K.bend_skin(blob)
    rig = r.skin_create(len(cube), blob, skin, 2)
    a, b = hip.event(), hip.event()
    d_tris = hip.alloc(blob.nbytes)
    d_copy = hip.alloc(2 * 96 * len(blob))
    angle = lambda f: 0.6 * np.sin(0.26 * f)
    lds = " (bone table staged in LDS)" if os.environ.get("RZ_SKIN_LDS") == "1" else ""

    pose_ms, kernel_ms, copy_ms, frame_ms = [], [], [], []
    for f in range(frames + 1):                 # (frame 0 warms up: the refit derives its topology once per layout)
        bones = K.bend_bones(y_range, angle(f))
        hip.ok(hip.L.hipEventRecord(a, stream))
        r.skin_pose(rig, bones)
        hip.ok(hip.L.hipEventRecord(b, stream))
        r.clear_accum()
        r.render()
        r.sync()
        if f:
            pose_ms.append(elapsed(hip, a, b))
            kernel_ms.append(r.skin_last_kernel_ms())
            frame_ms.append(r.last_render_ms()[0])
        hip.ok(hip.L.hipEventRecord(a, stream))
        hip.ok(hip.L.hipMemcpyAsync(d_copy + 96 * len(blob), d_copy, 96 * len(blob), 3, stream))
        hip.ok(hip.L.hipEventRecord(b, stream))
        if f:
            copy_ms.append(elapsed(hip, a, b))
    med = lambda v: float(np.median(v))
    print(f"device   {len(blob)} triangles{lds}: pose {med(pose_ms):.3f} ms, skinning kernel {med(kernel_ms):.4f} ms "
          f"(copy of 96 B/triangle {med(copy_ms):.4f} ms: x{med(kernel_ms) / med(copy_ms):.2f}), "
          f"frame ({W}x{H}, {spp} spp) {med(frame_ms):.3f} ms")

    host_ms, numpy_ms, frame_ms = [], [], []
    for f in range(frames + 1):
        bones = K.bend_bones(y_range, angle(f))
        t0 = time.perf_counter()
        moved = K.pose(blob, skin, bones)
        t1 = time.perf_counter()
        hip.ok(hip.L.hipMemcpy(d_tris, moved.ctypes.data, moved.nbytes, 1))
        r.refit_geometry_device(d_tris, len(cube), len(moved))         # (synchronises: the TLAS depth comes back)
        t2 = time.perf_counter()
        r.clear_accum()
        r.render()
        r.sync()
        if f:
            host_ms.append((t2 - t0) * 1e3)
            numpy_ms.append((t1 - t0) * 1e3)
            frame_ms.append(r.last_render_ms()[0])
    print(f"host     {len(blob)} triangles: numpy skin + hipMemcpy + refit {med(host_ms):.3f} ms (numpy {med(numpy_ms):.3f} ms, "
          f"copy + refit {med(host_ms) - med(numpy_ms):.3f} ms), frame {med(frame_ms):.3f} ms")
    r.skin_destroy(rig)
    r.set_stream(0)
    r.close()
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    hip.L.hipStreamDestroy(stream)
    hip.close()


if __name__ == "__main__":
    main()

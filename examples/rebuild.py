"""The loop of examples/deform.py with the exit it lacked: per frame the mesh is displaced with a growing amplitude and refitted
(rz_refit_geometry), its tree is metered (rz_geometry_quality), and once the SAH cost has reached max_ratio times the cost the
tree was built with, rz_rebuild_geometry rebuilds that mesh on the device, from the triangles where they are.  Prints per frame:
the cost ratio, the frame's milliseconds, and whether it rebuilt.

    python examples/rebuild.py [n] [frames] [max_ratio]   # n: blob size (76 -> 69 312 triangles); defaults 76, 24, 1.2
    python examples/rebuild.py --table [n] [A ...]        # per amplitude: cost ratio, frame ms refitted / rebuilt, the calls' ms
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from rayzen_amd import _lib  # noqa: E402
from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402
from deform import elapsed, wobble  # noqa: E402
from test_rays_gpu import Hip  # noqa: E402

W, H, BOUNCES = 1920, 1080, 4


def setup(hip, n, spp, radius=2.8, floor=(8.0, 0.5, 8.0), floor_y=-3.0, lift=2.0, camera=(0.0, 2.5, 10.0)):
    cube, blob = S.make_cube(4), S.make_blob(n, radius, 0)
    objects = [(0, S.translate(S.scale(S.identity(), floor), (0.0, floor_y, 0.0))), (1, S.translate(S.identity(), (0.0, lift, 0.0)))]
    cam = S.Camera(position=camera, aspect=W / H)
    r = Renderer(0)
    stream = hip.stream()
    r.set_stream(stream)
    r.upload_scene_built_on_device([cube, blob], objects, S.reference_materials(), S.reference_lights())
    r.set_frame(frame_params(cam, W, H, 2, BOUNCES, spp))
    r.render()
    r.sync()
    return r, stream, cube, blob


def timed(hip, stream, a, b, fn):
    """(device ms between two events around fn, wall ms of fn)."""
    hip.ok(hip.L.hipEventRecord(a, stream))
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    hip.ok(hip.L.hipEventRecord(b, stream))
    return elapsed(hip, a, b), wall, out


def frame_ms(r, reps=5):
    ms = []
    for _ in range(reps):
        r.clear_accum()
        r.render()
        r.sync()
        ms.append(r.last_render_ms()[0])
    return float(np.median(ms))


def animate(n, frames, max_ratio):
    hip = Hip()
    r, stream, cube, blob = setup(hip, n, 16)
    a, b = hip.event(), hip.event()
    d_tris = hip.alloc(blob.nbytes)
    for f in range(frames):
        moved = wobble(blob, 0.04 * f, 0.26 * f)                # the deformation grows: the tree built for the rest shape degrades
        hip.ok(hip.L.hipMemcpy(d_tris, moved.ctypes.data, moved.nbytes, 1))     # (a skinning kernel would write them there)
        r.refit_geometry_device(d_tris, len(cube), len(moved))
        q = r.geometry_quality()[1]
        ratio = q["sah_cost"] / q["sah_cost_built"]
        rebuilt, step = "", 0.0
        if ratio > max_ratio:
            step, _, rec = timed(hip, stream, a, b, lambda: r.rebuild_geometry(max_ratio))
            rebuilt = f"  rebuilt in {step:.3f} ms: cost {rec[1]['sah_cost_before']:.2f} -> {rec[1]['sah_cost']:.2f}, {rec[1]['n_nodes']} nodes"
        r.clear_accum()
        r.render()
        r.sync()
        print(f"frame {f:3d}  A = {0.04 * f:.2f}  cost ratio {ratio:.3f}  frame {r.last_render_ms()[0]:.3f} ms{rebuilt}")
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()


def table(n, amplitudes=(0.05, 0.2, 0.5, 1.0)):
    """What justifies the feature, per amplitude: sah_cost / sah_cost_built, the frame on the refitted tree, the frame after the
    rebuild, and what the calls cost (device ms between events on the context's stream / wall ms)."""
    hip = Hip()
    a, b = hip.event(), hip.event()
    print(f"source {_lib.hip().rz_source_hash().decode()[:12]}, blob n = {n}, frame {W}x{H}, 64 spp, {BOUNCES} bounces")
    for amp in amplitudes:
        r, stream, cube, blob = setup(hip, n, 64)
        moved = wobble(blob, amp, 0.0)
        d_tris = hip.upload(moved)
        r.refit_geometry_device(d_tris, len(cube), len(moved))          # (derives the topology, takes the first look)
        refit = [timed(hip, stream, a, b, lambda: r.refit_geometry_device(d_tris, len(cube), len(moved)))[:2] for _ in range(25)]
        meter = [timed(hip, stream, a, b, r.geometry_quality)[:2] for _ in range(25)]
        q = r.geometry_quality()[1]
        before = frame_ms(r)
        dev, wall, rec = timed(hip, stream, a, b, lambda: r.rebuild_geometry(1.0))      # the deformed mesh alone: the floor's ratio is 1
        assert rec["flags"].tolist() == [0, _lib.QUALITY_REBUILT], rec["flags"]
        after = frame_ms(r)
        # ... and once more with everything allocated: back to the rest pose, which the tree just built does not fit
        d_rest = hip.upload(blob)
        r.refit_geometry_device(d_rest, len(cube), len(blob))
        dev2, wall2, rec2 = timed(hip, stream, a, b, lambda: r.rebuild_geometry(1.0))
        assert rec2["flags"].tolist() == [0, _lib.QUALITY_REBUILT], rec2["flags"]
        med = lambda xs: (float(np.median([x[0] for x in xs])), float(np.median([x[1] for x in xs])))
        print(f"A = {amp:4.2f}: {len(blob)} triangles, {q['n_nodes']} -> {rec[1]['n_nodes']} nodes; cost ratio {q['sah_cost'] / q['sah_cost_built']:.3f} "
              f"(rebuilt / built {rec[1]['sah_cost'] / q['sah_cost_built']:.3f}); frame {before:.3f} ms refitted, {after:.3f} ms rebuilt (x{before / after:.3f}); "
              f"refit {med(refit)[0]:.3f} / {med(refit)[1]:.3f} ms, rz_geometry_quality {med(meter)[0]:.3f} / {med(meter)[1]:.3f} ms, "
              f"rz_rebuild_geometry (the one mesh, re-layout and TLAS) {dev:.3f} / {wall:.3f} ms, the context's second {dev2:.3f} / {wall2:.3f} ms")
        r.set_stream(0)
        r.close()
        hip.L.hipStreamDestroy(stream)
    hip.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        table(int(sys.argv[2]) if len(sys.argv) > 2 else 76, tuple(float(x) for x in sys.argv[3:]) or (0.05, 0.2, 0.5, 1.0))
    else:
        animate(int(sys.argv[1]) if len(sys.argv) > 1 else 76, int(sys.argv[2]) if len(sys.argv) > 2 else 24,
                float(sys.argv[3]) if len(sys.argv) > 3 else 1.2)

"""The times of profiles/lines/README.md, each a HIP event pair on the context's stream, the calls of a group alternating for
12 rounds after a warm-up round; median and range.  bunny_scene() (69 312 triangles and a floor) at 1920 x 1080.

  rz_draw_lines (device form, rgba8 in place) for three sets of lines, each with rz_denoise's guides as hits and without hits:
    editor      about 300: a ground grid, the big mesh's box in its own space, axes (tests/test_lines_gpu.py: editor_set)
    boxes       12 000: the boxes of 1 000 objects scattered over the floor, world space
    mesh edges  the unique edges of the big mesh, about 104 000, in its instance's space
  and for the two larger sets the same call without lists (RZ_LINES_UNBINNED=1): every tile walks every line behind the
  rectangle test.  The yardstick is rz_denoise with iterations = 0 and guides: the cast that makes the depth image.

    python profiles/lines/time_calls.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rayzen_amd import _lib, lines as LN, scene as S
from rayzen_amd.renderer import Renderer, frame_params
from test_lines_gpu import editor_set
from test_rays_gpu import Hip

hip = Hip()
L = _lib.hip()
print("source", L.rz_source_hash().decode()[:12])
W, H = 1920, 1080
ROUNDS = 12


def _alternate(stream, calls, rounds):
    """GPU time (ms) of each call of `calls`, alternating them `rounds` times after a warm-up round."""
    a, b = hip.event(), hip.event()
    times = [[] for _ in calls]
    for k in range(rounds + 1):
        for i, call in enumerate(calls):
            hip.ok(hip.L.hipEventRecord(a, stream))
            call()
            hip.ok(hip.L.hipEventRecord(b, stream))
            hip.ok(hip.L.hipEventSynchronize(b))
            ms = C.c_float()
            hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
            if k:
                times[i].append(float(ms.value))
    for e in (a, b):
        hip.L.hipEventDestroy(e)
    return times


def show(name, ms):
    print(f"  {name:44s} {np.median(ms):.4f} ms ({min(ms):.4f}..{max(ms):.4f})", flush=True)


sc = S.bunny_scene()
r = Renderer(0)
r.upload_scene(sc)
fp = frame_params(sc.camera, W, H, len(sc.lights), 1, 1)
r.set_frame(fp)
inst, tris = sc.arrays[S.BIND_INSTANCES], sc.arrays[S.BIND_TRIANGLES]
rng = np.random.default_rng(1)
centres = rng.uniform((-12.0, -2.5, -14.0), (12.0, 2.0, 6.0), (1000, 3))
sets = {"editor": editor_set(sc),
        "boxes": np.concatenate([LN.box(c - 0.4, c + 0.4, (255, 160, 0, 255)) for c in centres]),
        "mesh edges": LN.mesh_edges(tris[int(inst["globalTriOffset"][1]):], (20, 20, 20, 160), instance=1)}
d8, d_guides = hip.alloc(W * H * 4, 0x40), hip.alloc(W * H * 48)
r.denoise_device(guides_ptr=d_guides, iterations=0)
stream = L.rz_stream_handle(r._c)


def draw(d_lines, n, hits, unbinned=False):
    def call():
        if unbinned:
            os.environ["RZ_LINES_UNBINNED"] = "1"
        r.draw_lines_device(d_lines, n, d8, None, d_guides if hits else None, frame=fp)
        os.environ.pop("RZ_LINES_UNBINNED", None)
    return call


print(f"bunny 69 312 + floor, {W}x{H}:")
for name, lines in sets.items():
    d_lines, n = hip.upload(lines), len(lines)
    calls = [draw(d_lines, n, True), draw(d_lines, n, False), lambda: r.denoise_device(guides_ptr=d_guides, iterations=0)]
    labels = [f"{name} ({n}), hits", f"{name} ({n}), no hits", "denoise guides (iterations 0)"]
    for lab, ms in zip(labels, _alternate(stream, calls, ROUNDS)):
        show(lab, ms)
    if name != "editor":
        rounds = 3 if n > 50000 else 6
        calls = [draw(d_lines, n, True, True), draw(d_lines, n, False, True)]
        for lab, ms in zip([f"{name} ({n}), hits, unbinned", f"{name} ({n}), no hits, unbinned"], _alternate(stream, calls, rounds)):
            show(lab, ms)
    hip.ok(hip.L.hipMemset(d8, 0x40, W * H * 4))
r.sync()
r.close()
hip.close()

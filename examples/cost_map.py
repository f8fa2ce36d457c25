"""Where a frame is expensive, and whether a rebuild helped where it matters: the per-pixel traversal cost map
(Renderer.render_cost / cost_view) on bunny_scene, three times --

  built      the mesh on the tree it was built with
  refitted   the mesh displaced by examples/deform.py's wobble and refitted (rz_refit_geometry): the topology is kept, the boxes
             grow and overlap, and the same camera pays more bytes for the same pixels
  rebuilt    after rz_rebuild_geometry: a fresh tree for the displaced triangles, and the sum comes back down

Prints per stage the frame's cost sum (the reference algorithm's bytes), the hottest pixel, the SAH cost ratio of the mesh and the
time of the call, and how much of the frame changed; writes the three maps (H x W uint64 byte values) and their false colours.

    python examples/cost_map.py [n] [amplitude] [outdir]      # n: blob size (76 -> 69 312 triangles); defaults 76, 0.5, .
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "examples")]

from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402
from deform import wobble  # noqa: E402

W, H, SPP, BOUNCES = 480, 270, 1, 4
WEIGHTS = dict(tlas_nodes=32, tlas_leaf_indices=4, instances=144, blas_nodes=32, triangles=68, materials=32, light_fetches=32)


def bytes_of(rec):
    """The value rz_cost_view's metric 0 gives a pixel (include/rayzen_hip.h)."""
    return sum(np.uint64(k) * rec[f].astype(np.uint64) for f, k in WEIGHTS.items()) + np.uint64(16)


def stage(r, name, outdir):
    t0 = time.perf_counter()
    rec = r.render_cost()
    ms = (time.perf_counter() - t0) * 1e3
    rgb, st = r.cost_view(stats=True)
    q = r.geometry_quality()[1]
    v = bytes_of(rec)
    assert int(v.sum()) == st["sum_value"] and int(v[st["max_y"], st["max_x"]]) == st["max_value"]
    print(f"{name:9s} sum {st['sum_value']:>12d} B  hottest pixel ({st['max_x']}, {st['max_y']}) with {st['max_value']} B  "
          f"SAH cost ratio {q['sah_cost'] / q['sah_cost_built']:.3f}  render_cost {ms:.2f} ms (host path, with the copy)")
    np.save(os.path.join(outdir, f"cost_{name}.npy"), v)
    np.save(os.path.join(outdir, f"cost_{name}_rgb.npy"), rgb)
    return v


def main(n=76, amplitude=0.5, outdir="."):
    os.makedirs(outdir, exist_ok=True)
    sc = S.bunny_scene(n=n)
    floor, blob = S.make_cube(4), S.make_blob(n, 2.8, 0)
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), BOUNCES, SPP))
    built = stage(r, "built", outdir)
    r.refit_geometry(wobble(blob, amplitude, 0.0), first=len(floor))
    refitted = stage(r, "refitted", outdir)
    r.rebuild_geometry(1.0)
    rebuilt = stage(r, "rebuilt", outdir)
    r.close()
    more = refitted > built
    print(f"refit:   {int(more.sum())} of {W * H} pixels pay more, x{refitted.sum() / built.sum():.3f} over the frame, "
          f"x{(refitted[more] / built[more]).max():.1f} at worst")
    less = rebuilt < refitted
    print(f"rebuild: {int(less.sum())} pixels pay less, x{rebuilt.sum() / refitted.sum():.3f} over the frame "
          f"(x{rebuilt.sum() / built.sum():.3f} of the built frame: the displaced mesh is another shape)")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 76, float(sys.argv[2]) if len(sys.argv) > 2 else 0.5,
         sys.argv[3] if len(sys.argv) > 3 else ".")

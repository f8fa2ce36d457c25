"""Spending samples where the noise is: Renderer.render_adaptive next to Renderer.render on the same frame, twice --

  far     bunny_scene at the benchmark camera: two thirds of the frame are sky, the noise sits on the glass and the mirror
  close   the camera 0.9 units outside the mesh: the mesh fills the frame and most of it is converged after a few batches

Prints per view the time of the uniform frame (one launch, and in batches), the time of the adaptive frame, the share of the
samples it traced, the tiles still active after every batch and how many tiles ended at which sample count; checks that a pixel
of the adaptive frame that went to the end equals the uniform frame's bit for bit; writes the per-tile batch counts and errors.

    python examples/adaptive.py [n] [threshold] [outdir]      # n: blob size (76 -> 69 312 triangles); defaults 76, 0.02, .
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402

W, H, BOUNCES = 1920, 1080, 4
BATCH, MIN_BATCHES, MAX_BATCHES = 8, 4, 8


def timed(call, rounds=5):
    call()
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), out


def view(name, sc, threshold, outdir):
    r = Renderer(0)
    r.upload_scene(sc)
    nl, spp = len(sc.lights), BATCH * MAX_BATCHES

    def uniform():
        r.set_frame(frame_params(sc.camera, W, H, nl, BOUNCES, spp))
        r.render()
        r.sync()

    def batched():
        r.render_scene(sc, W, H, spp, BOUNCES, chunk=BATCH)
        r.sync()

    def adaptive():
        r.set_frame(frame_params(sc.camera, W, H, nl, BOUNCES, 1))
        return r.render_adaptive(batch_spp=BATCH, min_batches=MIN_BATCHES, max_batches=MAX_BATCHES, threshold=threshold)

    ms_uniform, _ = timed(uniform)
    full = r.read_accum()
    ms_batched, _ = timed(batched)
    ms_adaptive, (info, batches, error) = timed(adaptive)
    accum = r.read_accum()
    r.close()
    done = accum[..., 3] == spp
    assert accum[done].tobytes() == full[done].tobytes()        # the pixels that took every batch are the uniform frame's
    counts = {int(k) * BATCH: int(v) for k, v in zip(*np.unique(batches, return_counts=True))}
    print(f"{name:6s} uniform {spp} spp {ms_uniform:.2f} ms (in batches of {BATCH}: {ms_batched:.2f} ms); adaptive {ms_adaptive:.2f} ms "
          f"({ms_adaptive / ms_uniform:.2f} x), {info['samples_traced'] / info['samples_uniform']:.3f} of the samples")
    print(f"       tiles active after each batch {info['tiles_active']}; tiles by final spp {counts}; "
          f"render {info['render_ms']:.2f} ms, meter {info['meter_ms']:.3f} ms")
    np.save(os.path.join(outdir, f"adaptive_{name}_batches.npy"), batches)
    np.save(os.path.join(outdir, f"adaptive_{name}_error.npy"), error)


def main(n=76, threshold=0.02, outdir="."):
    os.makedirs(outdir, exist_ok=True)
    view("far", S.bunny_scene(n=n, extras=True), threshold, outdir)
    view("close", S.bunny_scene(n=n, camera_position=S.CLOSE_CAMERA), threshold, outdir)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 76, float(a[1]) if len(a) > 1 else 0.02, a[2] if len(a) > 2 else ".")

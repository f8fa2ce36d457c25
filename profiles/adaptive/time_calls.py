"""The figures of profiles/adaptive/README.md.  Times are host clocks around a call that ends in a synchronise (rz_render_adaptive
synchronises itself; rz_render is followed by rz_sync), medians of ROUNDS after a warm-up call, the variants of a configuration
alternating.  Frames are 1920 x 1080, s = 8, min_batches = 4, max_batches = 8, so a uniform frame has 64 spp; --batches=16,2,4
measures another split of the same 64.  merge_gap and max_runs are the defaults except in the sweeps.

  python profiles/adaptive/time_calls.py [config ...]        c2 c2close c2g c4 (rayzen_amd.scene.NAMED_CONFIGS' scenes)
  python profiles/adaptive/time_calls.py --render-only ...   rz_render at 64 spp alone: what a library without the call can run
                                                             (RAYZEN_HIP_SO=<the parent commit's library>)
  python profiles/adaptive/time_calls.py --sweep c2          the merge_gap / max_runs sweeps

Per configuration: rz_render at 64 spp in one launch and chunked at s; rz_render_adaptive with threshold -1 (no tile retires: the
scheme's own overhead over the chunked render -- launches per batch, read-backs, the meter); thresholds 0.01, 0.02, 0.05 with the
share of samples traced, the runs per batch and the RMSE of the resolved frame against a 1024-spp frame of the same build, next
to the uniform 64-spp frame's."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]
from rayzen_amd import _lib, scene as S
from rayzen_amd.renderer import Renderer, frame_params

ROUNDS = 7
S_BATCH, MIN_B, MAX_B = 8, 4, 8          # --batches=S,MIN,MAX overrides them
for _a in sys.argv[1:]:
    if _a.startswith("--batches="):
        S_BATCH, MIN_B, MAX_B = (int(x) for x in _a.split("=")[1].split(","))
SPP = S_BATCH * MAX_B


def resolved(accum):
    return (accum[..., :3] / np.maximum(accum[..., 3:4], 1.0)).astype(np.float64)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.clip(a, 0, 1) - np.clip(b, 0, 1)) ** 2)))


def alternate(calls, rounds=ROUNDS):
    """Median wall ms of each call, alternating; one warm-up round."""
    times = [[] for _ in calls]
    for k in range(rounds + 1):
        for i, call in enumerate(calls):
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if k:
                times[i].append(dt)
    return [(float(np.median(t)), min(t), max(t)) for t in times]


def main():
    args = sys.argv[1:]
    render_only, sweep = "--render-only" in args, "--sweep" in args
    names = [a for a in args if not a.startswith("--")] or ["c2", "c2close", "c2g", "c4"]
    print("source", _lib.hip().rz_source_hash().decode()[:12], flush=True)
    for name in names:
        sc, W, H, _, bounces = S.named_config(name)
        r = Renderer(0)
        r.upload_scene(sc)
        nl = len(sc.lights)

        def frame(spp, base=0):
            r.set_frame(frame_params(sc.camera, W, H, nl, bounces, spp, base))

        def one_shot():
            frame(SPP)
            r.render()
            r.sync()

        def chunked():
            for k in range(MAX_B):
                frame(S_BATCH, k * S_BATCH)
                r.render()
            r.sync()

        if render_only:
            (ms, lo, hi), = alternate([one_shot])
            print(f"{name}: rz_render at {SPP} spp {ms:.3f} ms ({lo:.3f}..{hi:.3f}); kernel {r.last_render_ms()[0]:.3f} ms", flush=True)
            r.close()
            continue

        last = {}

        def adaptive(key, **kw):
            def call():
                frame(1)
                last[key] = r.render_adaptive(batch_spp=S_BATCH, min_batches=MIN_B, max_batches=MAX_B, **kw)[0]
            return call

        if sweep:
            cases = [(0.02, g, m) for g in (0, 8, 32, 240) for m in (16, 64, 256, 1 << 20)]
            cases += [(t, 8, m) for t in (0.02, 0.05) for m in (1, 2, 3, 4, 6, 8, 12)]
            res = alternate([adaptive(c, threshold=c[0], merge_gap=c[1], max_runs=c[2]) for c in cases], 5)
            print(f"{name}: threshold, merge_gap, max_runs -> ms (share of samples; most runs in a batch)")
            for (t, g, m), (ms, lo, hi) in zip(cases, res):
                i = last[(t, g, m)]
                print(f"  threshold {t} gap {g:4d} runs {m:8d}: {ms:7.3f} ms ({lo:.3f}..{hi:.3f})  share {i['samples_traced'] / i['samples_uniform']:.3f}  "
                      f"max runs {max(i['runs'])}  render {i['render_ms']:.3f} meter {i['meter_ms']:.3f}", flush=True)
            r.close()
            continue

        # the reference: 1024 spp in chunks of 64
        for k in range(16):
            frame(64, 64 * k)
            r.render()
        r.sync()
        ref = resolved(r.read_accum())
        one_shot()
        uniform = resolved(r.read_accum())
        print(f"{name}: {W}x{H}, {bounces} bounces; RMSE of the uniform {SPP}-spp frame against 1024 spp: {rmse(uniform, ref):.5f}", flush=True)
        thresholds = (0.01, 0.02, 0.05)
        res = alternate([one_shot, chunked, adaptive("none", threshold=-1.0)] + [adaptive(t, threshold=t) for t in thresholds])
        for lab, (ms, lo, hi) in zip(["rz_render, one launch", f"rz_render, {MAX_B} chunks of {S_BATCH}", "adaptive, threshold -1"], res):
            print(f"  {lab:34s} {ms:8.3f} ms ({lo:.3f}..{hi:.3f})", flush=True)
        i = last["none"]
        print(f"    threshold -1: render launches {i['render_ms']:.3f} ms, meter {i['meter_ms']:.3f} ms in {i['batches']} batches; "
              f"overhead over the chunked render {res[2][0] - res[1][0]:+.3f} ms ({res[2][0] / res[1][0]:.3f} x)")
        for t, (ms, lo, hi) in zip(thresholds, res[3:]):
            adaptive(t, threshold=t)()
            img = resolved(r.read_accum())
            i = last[t]
            print(f"  adaptive, threshold {t:<5}              {ms:8.3f} ms ({lo:.3f}..{hi:.3f})  {ms / res[0][0]:.3f} x one launch, "
                  f"{ms / res[1][0]:.3f} x chunked; share of samples {i['samples_traced'] / i['samples_uniform']:.3f}; batches {i['batches']}; "
                  f"active {i['tiles_active']}; runs {i['runs']}; render {i['render_ms']:.3f} meter {i['meter_ms']:.3f} ms; "
                  f"RMSE {rmse(img, ref):.5f}", flush=True)
        r.close()


if __name__ == "__main__":
    main()

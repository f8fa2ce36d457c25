"""Selecting what is on screen: a marquee dragged over bunny_scene(extras=True) (Renderer.select_rect: rz_coverage on a rectangle),
the selection outlined on the presented frame (Renderer.outline: rz_outline after rz_present), and what the two calls cost at
1080p beside the host route an editor would otherwise take -- rz_denoise's guides (48 B per pixel) read back and histogrammed
with numpy.

Prints the selection and the per-instance coverage of the whole frame, writes the outlined frame (H x W x 4 uint8, row 0 =
bottom) as select_outlined.npy, and as select_outlined.ppm (top row first) for a viewer.

    python examples/select.py [outdir]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402

W, H, SPP, BOUNCES = 1920, 1080, 1, 4
NAMES = ["floor", "bunny", "glass blob", "mirror cube"]


def best_of(fn, reps=5):
    """Wall-clock milliseconds of fn(), which returns when its result is on the host: the best of `reps` after a warm-up."""
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out)


def host_route(r, rect):
    """The marquee without rz_coverage: the guide records of every pixel read back, the rectangle histogrammed on the host."""
    _, guides = r.denoise(iterations=0, guides=True)
    x0, y0, x1, y1 = rect
    inst = guides["instance"][y0:y1, x0:x1]
    n = r.n_instances()
    return np.bincount(np.where(inst < 0, n, inst).ravel(), minlength=n + 1)


def main(outdir="."):
    os.makedirs(outdir, exist_ok=True)
    sc = S.bunny_scene(extras=True)
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), BOUNCES, SPP))
    r.render()
    rec = r.coverage()
    for i, c in enumerate(rec):
        who = NAMES[i] if i < len(NAMES) else "(misses)"
        box = f"x {c['x_min']}..{c['x_max']}, y {c['y_min']}..{c['y_max']}" if c["pixels"] else "not on screen"
        depth = f", t {c['t_min']:.2f}..{c['t_max']:.2f}" if c["pixels"] and i < len(rec) - 1 else ""
        print(f"  {who:12s} {int(c['pixels']):8d} pixels  {box}{depth}")
    rect = (W // 3, H // 4, W - 100, H - 200)               # the drag: from the bunny's left flank to the glass blob
    picked = r.select_rect(rect, min_pixels=16)
    print(f"marquee {rect}: " + ", ".join(f"{NAMES[i]} ({p} px)" for i, p in picked))
    selected = [i for i, _ in picked if NAMES[i] != "floor"]
    _, ids = r.coverage(want_ids=True)
    _, rgba8 = r.present(show_fps=False)
    outlined, _ = r.outline(ids, selected, rgba8=rgba8, radius=2)
    changed = int((outlined != rgba8).any(axis=-1).sum())
    print(f"outline of {[NAMES[i] for i in selected]}: {changed} pixels changed")
    np.save(os.path.join(outdir, "select_outlined.npy"), outlined)
    with open(os.path.join(outdir, "select_outlined.ppm"), "wb") as f:
        f.write(b"P6 %d %d 255\n" % (W, H) + outlined[::-1, :, :3].tobytes())
    # what it costs, the host seeing the answer: a dozen integers against 100 MB of hits
    want = host_route(r, rect)
    assert r.coverage(rect=rect)["pixels"].tolist() == want.tolist()
    t_cov = best_of(lambda: r.select_rect(rect, min_pixels=16))
    t_host = best_of(lambda: host_route(r, rect))
    t_out = best_of(lambda: r.outline(ids, selected, rgba8=rgba8, radius=2))
    print(f"{W}x{H}, wall clock with the copies: select_rect {t_cov:.2f} ms; guides read back and histogrammed {t_host:.2f} ms; "
          f"outline (host images staged both ways) {t_out:.2f} ms")
    r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")

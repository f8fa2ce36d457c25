"""How many first-hit shadow queries of a workload have their light behind the surface (dot(n, l) <= 0), counted on the CPU
with the oracle's ray queries at the pixel centres of a reduced frame (tests/backface_ref.py: census):

    python profiles/r06_backface/cpu_count.py [c2 | c2close | ...] [width height]      (default: c2 384 216)

Prints the hit fraction, the occluded share of the shadow queries, the share behind per light and per instance, and the share
of the time spent in rzo.shadow that the queries with the light behind took."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rayzen_amd import scene as S      # noqa: E402
from backface_ref import census        # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "c2"
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (384, 216)
sc = S.named_config(name)[0]
c = census(sc, W, H, shadows=True)
hits, q = c["hits"], c["queries"]
nb = sum(c["behind"])
print(f"{name} at {W}x{H} pixel centres: {hits} of {c['pixels']} pixels hit = {hits / c['pixels']:.3f}")
print(f"shadow queries {q}: occluded {c['occluded']} = {100 * c['occluded'] / q:.2f} %; light behind {nb} = {100 * nb / q:.2f} %")
for li, b in enumerate(c["behind"]):
    print(f"  light {li}: dot(n, l) <= 0 for {b} hit pixels = {100 * b / hits:.1f} %")
for inst, (n, b) in sorted(c["by_instance"].items()):
    print(f"  instance {inst}: {n} shadow queries, {b} with the light behind = {100 * b / max(n, 1):.1f} %")
print(f"hit pixels with a light behind {c['any_behind']}, with every light in front {c['all_front']}")
mean_all, mean_b = c["seconds"] / q, c["seconds_behind"] / max(nb, 1)
print(f"time in rzo.shadow: {c['seconds']:.2f} s, of it {c['seconds_behind']:.2f} s = {100 * c['seconds_behind'] / c['seconds']:.1f} % in the queries "
      f"with the light behind ({mean_b / mean_all:.2f} x the mean query; the call's Python overhead is in both)")

"""Are the inputs of tests/tie_cases.py sharp?  With the oracle alone (no GPU): on these scenes and rays the ORDER in which a
closest-hit query visits instances, nodes and triangles decides its answer -- so a kernel that visits them in another order, or
breaks a tie the other way, cannot agree with the oracle by accident (tests/test_ties_gpu.py holds the kernels to it).

Per scene, over all its ray families (measured on these inputs; the per-family figures are printed):

                rays   hits   winner changes with the instance   winner differs, SAH BLAS   hit flag differs, SAH BLAS
                              order while t keeps its bits       against a one-leaf BLAS    against a one-leaf BLAS
  stack         4667   1980   1924                               299                        289
  glass-stack   4667   1980   1924                               299                        289
  facing        4667   2300   2244                               568                        418
  deep          3488   3183   3171                               391                        190

(the hit flag differs where a ray lies in a plane of an inner box: 0 * inf = NaN in the slab test, which the one-leaf BLAS never
evaluates below its root; the winner differs where two triangles of ONE mesh are met at the same t -- a shared edge or vertex,
or the doubled sheet of "facing".)

Rendered at 64 x 48, 16 spp, 6 bounces, "facing": 39 581 of 49 152 camera paths start a third segment and 11 097 third and later
segments hit something -- every one of them a tie; the two instance orders give frames that differ in 100 % of the pixels of "stack",
"glass-stack" and "facing"."""
import numpy as np
import pytest

import tie_cases as T
from helpers import oracle_render

W, H = 64, 48


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_ties_decide_the_winner(name):
    s0, s1 = T.scene(name, 0), T.scene(name, 1)
    o0, o1, leaf = T.oracle_scene(s0), T.oracle_scene(s1), T.one_leaf_oracle_scene(s0)
    total = np.zeros(5, np.int64)
    for fam, (o, d) in T.families(name).items():
        a, b, c = T.oracle_trace(o0, o, d), T.oracle_trace(o1, o, d), T.oracle_trace(leaf, o, d)
        assert (a["hit"] == b["hit"]).all()                 # the instance order moves no ray between hit and miss
        both = a["hit"] & b["hit"]
        by_order = both & (a["material"] != b["material"]) & (_bits(a["t"]) == _bits(b["t"]))
        by_blas = a["hit"] & c["hit"] & (a["material"] != c["material"])
        flag = a["hit"] != c["hit"]
        row = np.array([len(o), a["hit"].sum(), by_order.sum(), by_blas.sum(), flag.sum()])
        total += row
        print(f"{name:12s} {fam:8s} rays {row[0]:5d}  hits {row[1]:5d}  winner by instance order {row[2]:5d}  "
              f"winner by BLAS shape {row[3]:5d}  hit flag by BLAS shape {row[4]:5d}")
    print(f"{name:12s} total    rays {total[0]:5d}  hits {total[1]:5d}  winner by instance order {total[2]:5d}  "
          f"winner by BLAS shape {total[3]:5d}  hit flag by BLAS shape {total[4]:5d}")
    assert total[2] >= 1000, total          # nearly every hit is a tie between instances
    assert total[3] >= 100, total
    assert total[4] >= 100, total


def test_the_doubled_sheet_wins_in_both_stacks_of_the_render_variant():
    """"facing", instance order 0: the instance visited first among the coincident ones -- the winner -- is the doubled sheet, in
    the near stack and in the far one, so the tie INSIDE its BLAS decides what is seen (measured: 2 099 of 2 300 hits)."""
    sc = T.scene("facing", 0)
    inst = sc.arrays[T.S.BIND_INSTANCES]
    tris = sc.arrays[T.S.BIND_TRIANGLES]
    doubled = [k for k in range(len(inst)) if _tri_count(sc, k) == 256]
    assert len(doubled) == 2
    osc = T.oracle_scene(sc)
    won = {k: 0 for k in doubled}
    hits = 0
    for fam, (o, d) in T.families("facing").items():
        a = T.oracle_trace(osc, o, d)
        hits += int(a["hit"].sum())
        for k in doubled:
            won[k] += int((a["hit"] & (a["instance"] == k)).sum())
    print(f"facing: hits won by the doubled sheets {won} of {hits}")
    assert all(v >= 100 for v in won.values()), won
    assert len(tris) == 1408


def _tri_count(sc, k):
    inst = sc.arrays[T.S.BIND_INSTANCES]
    starts = sorted(set(int(g) for g in inst["globalTriOffset"])) + [len(sc.arrays[T.S.BIND_TRIANGLES])]
    g = int(inst["globalTriOffset"][k])
    return starts[starts.index(g) + 1] - g


def test_deep_is_deeper_than_a_stack_window_of_two():
    assert T.scene("deep").max_blas_depth > 2 + 2, T.scene("deep").max_blas_depth


def test_shadow_families_are_sharp():
    """`restart` holds first hits at t < 0.001: from 2^-11 above a sheet the walk starts again below it and ends lit at full
    visibility (measured: all 722 such rays, in both scenes).  In `reach` the answer turns on one ulp of max_dist: of the 1 761
    rays that meet the sheets all are lit at max_dist and an ulp below it, and an ulp above it none in "stack" and 1 760 in
    "glass-stack", where the glass wins the tie in instance order 0 and the walk goes on at 0.94 -- in order 1 an opaque sheet
    wins and the two orders disagree on those 1 760 rays."""
    for name in ("stack", "glass-stack"):
        osc, osc1 = T.oracle_scene(T.scene(name, 0)), T.oracle_scene(T.scene(name, 1))
        fam = T.shadow_families(osc)
        o, d, md = fam["restart"]
        lit, vis = T.oracle_shadow(osc, o, d, md)
        above = (o[:, 2] > T.SHEET_Z) & (d[:, 2] < 0)
        restarted = above & lit & (vis == 1.0)
        print(f"{name}: restart: {int(above.sum())} rays from 2^-11 above a sheet, {int(restarted.sum())} of them lit at visibility 1")
        assert restarted.sum() >= 100 and (restarted == above).all()
        o, d, md = fam["reach"]
        n = len(o) // 3
        lit, vis = T.oracle_shadow(osc, o, d, md)
        lit1, vis1 = T.oracle_shadow(osc1, o, d, md)
        meets = T.oracle_trace(osc, o[:n], d[:n])["hit"]
        at, below, over = lit[:n] & meets, lit[n:2 * n] & meets, lit[2 * n:] & meets
        differ = (lit != lit1) | (_bits(vis) != _bits(vis1))
        print(f"{name}: reach: {int(meets.sum())} rays that meet the sheets; lit at max_dist {int(at.sum())}, an ulp below "
              f"{int(below.sum())}, an ulp above {int(over.sum())}; the instance orders disagree on {int(differ.sum())}")
        assert at.sum() >= 1000 and (at == below).all()
        if name == "stack":
            assert over.sum() == 0 and differ.sum() == 0
        else:
            assert differ.sum() >= 1000


_frames = {}


def _frame(name, order, spp, bounces):
    k = (name, order, spp, bounces)
    if k not in _frames:
        _frames[k] = oracle_render(T.scene(name, order), W, H, spp, bounces, nthreads=8, want_counters=True)
    return _frames[k]


@pytest.mark.parametrize("name", ["stack", "glass-stack", "facing"])
def test_the_instance_order_shows_in_the_frame(name):
    a, _ = _frame(name, 0, 16, 6)
    b, _ = _frame(name, 1, 16, 6)
    differ = (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).mean()
    print(f"{name}: the two instance orders differ in {differ * 100:.1f} % of {W * H} pixels")
    assert differ > 0.9


def test_the_render_variant_has_later_segments():
    """A path's prefix does not depend on the bounce budget (its seeds are a function of pixel, sample and bounce), and `scatters`
    counts the hits of all its segments: scatters(budget n) - scatters(budget n - 1) is the number of n-th segments that hit."""
    sc = {b: _frame("facing", 0, 16, b)[1]["scatters"] for b in (1, 2, 6)}
    third_started = sc[2] - sc[1]          # second segments that hit: each starts a third
    later_hits = sc[6] - sc[2]             # hits of third and later segments
    print(f"facing, 16 spp: {W * H * 16} camera paths, {third_started} start a third segment, "
          f"{later_hits} third and later segments hit something")
    assert third_started >= 10000 and later_hits >= 10000

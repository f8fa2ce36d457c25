"""The large adversarial cases of tests/cppref_cases.py (LARGE_ADVERSARIAL) bite (no GPU: the host library and numpy only).
Each is there for one thing the device builder's large-node path (rz_blas_device.hip, nodes of more than 4096 triangles:
bbL_setup ... bbL_scatter) decides: where the root splits, that no SAH cost is finite, which sign a zero in a large node's
box has, how deep the tree gets, how many large nodes stand on one level.  This module asserts, on the host's nodes -- which
tests/test_cppref.py holds to RayZen's own BVH.cpp -- that every case really is what it is there for.  The device builder
on the same cases: tests/test_cppref_gpu.py, tests/test_blas_device_gpu.py."""
import numpy as np
import pytest

import cppref_cases as K

LARGE_NODE = 4096            # BB_LARGE of rz_blas_device.hip
CHUNK = 2048                 # BB_CHUNK
CASES = dict((n, c) for n, c, _ in K.LARGE_ADVERSARIAL)
QUICK = [n for n, _, slow in K.LARGE_ADVERSARIAL if not slow]

_BUILT = {}


def built(name):
    """(triangles, nodes, indices, depth, triangles below each node, level of each node), the host's build."""
    if name not in _BUILT:
        tris = CASES[name]()
        nodes, idx, depth = K.host_build(name, tris)
        _BUILT[name] = (tris, nodes, idx, depth) + K.node_counts_and_levels(nodes)
    return _BUILT[name]


def root_split(name):
    _, nodes, _, _, count, _ = built(name)
    L = int(nodes[0]["leftFirst"])
    return int(count[L]), int(count[L + 1])


def large_nodes(name):
    _, nodes, _, _, count, _ = built(name)
    return np.flatnonzero(count > LARGE_NODE)


def test_the_constants_are_the_kernels():
    import os
    import re
    src = open(os.path.join(os.path.dirname(K.GOLDEN), "..", "rayzen_amd", "csrc", "hip", "rz_blas_device.hip")).read()
    assert int(re.search(r"constexpr int BB_LARGE = (\d+);", src).group(1)) == LARGE_NODE
    assert [int(re.search(rf"constexpr int {k} = (\d+);", src).group(1)) for k in ("BB_THREADS", "BB_E")] == [256, 8]
    assert re.search(r"constexpr int BB_CHUNK = BB_THREADS \* BB_E;", src) and 256 * 8 == CHUNK


@pytest.mark.parametrize("name", QUICK)
def test_every_case_has_a_large_node_and_a_valid_tree(name):
    tris, nodes, idx, depth, count, level = built(name)
    assert len(tris) > LARGE_NODE and count[0] == len(tris) and len(large_nodes(name)) >= 1
    assert sorted(idx.tolist()) == list(range(len(tris)))
    assert depth == int(level.max())


# the root's split: (left, right).  A chunk boundary (2048, 4096, 6144), one triangle from either end, a chunk that goes
# wholly to one side, and the two sides of the midpoint fallback.
ROOT_SPLITS = {
    "adv_huge_6000": (3025, 2975), "adv_huge_widest_z_6000": (3015, 2985), "adv_huge_widest_x_6000": (2996, 3004),
    "adv_clusters_4096_2000": (4096, 2000),
    "adv_clusters_2048_4049": (2048, 4049), "adv_three_clusters": (6144, 4097), "adv_outlier_first": (1, 6000),
    "adv_outlier_last": (6000, 1), "adv_zero_4200": (1, 4199),
}


@pytest.mark.parametrize("name", sorted(ROOT_SPLITS))
def test_the_root_splits_where_the_case_says(name):
    assert root_split(name) == ROOT_SPLITS[name]


def _area32(lo, hi):
    e = (hi - lo).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(2.0) * ((e[0] * e[1] + e[1] * e[2]) + e[2] * e[0])


@pytest.mark.parametrize("name,axis", [("adv_huge_6000", 1), ("adv_huge_widest_z_6000", 2), ("adv_huge_widest_x_6000", 0)])
def test_the_huge_roots_have_no_finite_cost_and_split_at_the_midpoint(name, axis):
    """The root's area is inf in binary32, so every cost is inf or NaN, findSAHSplit returns no split and BVH.cpp:135-149
    partitions by the centroid against the middle of the widest extent (x: the `axis == -1` read) -- swapping in input
    order, which the sorted order of a SAH split is not.  One case per axis."""
    tris, nodes, idx, _, count, _ = built(name)
    lo, hi = nodes[0]["boundsMin"], nodes[0]["boundsMax"]
    assert np.isinf(_area32(lo, hi))
    e = hi - lo
    assert (1 if e[1] > e[0] and e[1] > e[2] else 2 if e[2] > e[0] else 0) == axis        # BVH.cpp:138-139
    cen = ((tris["v0"] + tris["v1"]) + tris["v2"]) / np.float32(3.0)
    below = cen[:, axis] < np.float32(0.5) * (lo[axis] + hi[axis])
    nl = root_split(name)[0]
    assert nl == int(below.sum())
    assert sorted(idx[:nl].tolist()) == np.flatnonzero(below).tolist()


def test_the_clusters_put_whole_chunks_on_one_side():
    """adv_clusters_2048_4049: the left child is the LAST 2048 triangles of the input, the right one the first 4049;
    adv_three_clusters: the root's 6144 | 4097 leaves two large children on one level."""
    _, _, idx, _, _, _ = built("adv_clusters_2048_4049")
    assert sorted(idx[:2048].tolist()) == list(range(4049, 6097))
    _, nodes, idx, _, count, level = built("adv_three_clusters")
    assert sorted(idx[:6144].tolist()) == list(range(6144))
    big = large_nodes("adv_three_clusters")
    assert len(big) == 3 and np.bincount(level[big]).max() == 2


@pytest.mark.parametrize("name,first", [("adv_outlier_first", True), ("adv_outlier_last", False)])
def test_the_outlier_is_split_off_alone(name, first):
    _, nodes, idx, _, count, _ = built(name)
    assert int(idx[0 if first else 6000]) == (0 if first else 6000)
    assert len(large_nodes(name)) == 2                 # the root and the 6000 that remain


def test_the_lattices_are_deep_and_hold_many_large_nodes():
    """Integer lattices: equal costs and equal centroids in droves, a long tail of large nodes (one per level)."""
    for name, depth, large in [("adv_lattice_20000", 337, 53), ("adv_lattice_tight_9000", 1042, 7)]:
        assert built(name)[3] == depth and len(large_nodes(name)) == large, name
    assert built("adv_lattice_tight_9000")[3] > 1000


def test_the_duplicates_split_one_off_a_large_node():
    _, nodes, _, depth, count, _ = built("adv_dup_4200")
    big = large_nodes("adv_dup_4200")
    left = count[nodes["leftFirst"][big]]
    assert depth == 294 and len(big) == 32
    assert int(((left == 1) | (left == count[big] - 1)).sum()) >= 1


def test_the_zero_triangles_make_a_chain_deeper_than_4096():
    """Parent area 0: every cost is 0 / 1e-6f = 0, the first candidate wins, every node splits 1 | N - 1 down to 4 triangles."""
    _, nodes, _, depth, count, level = built("adv_zero_4200")
    assert depth == 4197 > 4096 and len(nodes) == 2 * 4196 + 1
    big = large_nodes("adv_zero_4200")
    assert len(big) == 104 and (count[nodes["leftFirst"][big]] == 1).all()
    assert np.bincount(level)[1:].max() == 2


# ---- signed zeros ---------------------------------------------------------------------------------------------------------------

def _first_in_node(tris, nodes, idx, count, node, parent):
    """The triangles that can stand first in `node`'s range when computeBounds reads it: the range then has the order its parent's
    split left it in -- sorted by (centroid[axis], id) along the parent's split axis (BVH.cpp:128-133), so the first is the least
    of the node's set.  The axis is not stored; every axis whose order separates the parent's two children is taken."""
    cen = ((tris["v0"] + tris["v1"]) + tris["v2"]) / np.float32(3.0)

    def triangles(i):
        out, stack = [], [i]
        while stack:
            k = stack.pop()
            if nodes[k]["count"] >= 0:
                out += idx[nodes[k]["leftFirst"]:nodes[k]["leftFirst"] + nodes[k]["count"]].tolist()
            else:
                stack += [int(nodes[k]["leftFirst"]), int(nodes[k]["leftFirst"]) + 1]
        return np.array(sorted(out))

    L = int(nodes[parent]["leftFirst"])
    a, b = triangles(L), triangles(L + 1)
    mine = a if node == L else b
    firsts = set()
    for axis in range(3):
        key = lambda ids: sorted(zip((cen[ids, axis] + np.float32(0.0)).tolist(), ids.tolist()))
        if key(a)[-1] < key(b)[0]:
            firsts.add(key(mine)[0][1])
    assert firsts
    return firsts


@pytest.mark.parametrize("name,planted,everywhere", [("adv_floor_one_minus_zero_last", 9999, False),
                                                    ("adv_floor_plus_zero_first", 0, True)])
def test_the_planted_zero_decides_the_sign_of_the_large_boxes(name, planted, everywhere):
    """computeBounds keeps the FIRST of equal values, and -0 == +0: a node's y bounds carry the sign of the first triangle of its
    range.  One triangle has the other sign (`everywhere`: signbit of all the others).  The root's range is the input order:
    triangle 0 decides.  The two large children read their ranges in the parent's sorted order, where the planted triangle
    does not stand first: they carry the sign of all the others."""
    tris, nodes, idx, _, count, level = built(name)
    y = np.stack([tris[k][:, 1] for k in ("v0", "v1", "v2")], 1)
    assert (y == 0).all() and (np.signbit(y[planted]) != everywhere).all()
    assert (np.signbit(np.delete(y, planted, 0)) == everywhere).all()
    big = large_nodes(name)
    assert big.tolist() == [0, 1, 2] and level[big].tolist() == [1, 2, 2]
    expected = {0: bool(np.signbit(y[0, 0]))}
    for node in (1, 2):
        assert planted not in _first_in_node(tris, nodes, idx, count, node, 0)
        expected[node] = everywhere
    for node, sign in expected.items():
        lo, hi = nodes[node]["boundsMin"][1], nodes[node]["boundsMax"][1]
        assert lo == 0 and hi == 0 and bool(np.signbit(lo)) == sign and bool(np.signbit(hi)) == sign, (node, lo, hi)
    assert expected[0] is False and (expected[1] is True) == everywhere


def test_the_mixed_floor_has_both_signs_in_its_large_boxes():
    tris, nodes, _, _, count, level = built("adv_floor_pm0_10000")
    big = large_nodes("adv_floor_pm0_10000")
    assert len(big) == 3 and np.bincount(level[big]).max() == 2
    signs = {bool(np.signbit(nodes[i][k][1])) for i in big for k in ("boundsMin", "boundsMax")}
    assert signs == {False, True}
    assert all(nodes[i]["boundsMin"][1] == 0 and nodes[i]["boundsMax"][1] == 0 for i in big)


# ---- the two soups of millions ---------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_the_2_3_million_soup_has_more_than_256_large_nodes_on_one_level():
    """bbL_setup numbers the chunks of a level's large nodes 256 nodes at a time."""
    _, nodes, _, depth, count, level = built("adv_soup_2300000")
    per_level = np.bincount(level[count > LARGE_NODE])
    assert per_level.max() > 256, per_level.tolist()
    assert depth < 64


@pytest.mark.slow
def test_the_4_2_million_soup_has_a_root_of_more_than_2048_chunks():
    """bbL_node scans a node's chunk totals 2048 chunks at a time.  (From the fixture's record: the mesh itself is built in
    tests/test_cppref.py.)"""
    n = int(K.load_large()["adv_soup_4200000__digest"][3])
    assert n == 4200000 and n > CHUNK * 2048 and -(-n // CHUNK) > 2048

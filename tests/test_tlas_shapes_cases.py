"""The table of tests/tlas_shapes.py bites (no GPU: the host library and the oracle only): RayZen's builder really makes
chains deeper than the shader's stack[64] of instances spread over many octaves, the cut is visible to rays and in frames,
every pattern partitions the root as its mask says, and the restatement of the pop order in tlas_shapes.py tells the
device kernel's hand-down of `below` (rz_tlas_device.hip: left child `below`, right child `below + 1`) from its mirror image.
RayZen's own BVH.cpp on every shape: tests/test_cppref.py, through tests/cppref_cases.py::tlas_cases."""
import os
import re

import numpy as np
import pytest

import cppref_cases as K
import tlas_shapes as T
from helpers import oracle_render, oracle_scene
from oracle import rzo
from rayzen_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (depth, the most stack entries below a node when it is popped, internal nodes whose push does not fit stack[64]): a chain
# of n instances has n levels and a right-leaning one cuts n - 64 links; the others as computed here once
EXPECTED = {
    "chain_right_70": (70, 69, 6), "chain_right_100": (100, 99, 36), "chain_left_100": (100, 1, 0),
    "chain_y_right_100": (100, 99, 36), "identical_130": (9, 8, 0), "identical_64": (7, 6, 0), "identical_65": (8, 7, 0),
    "pattern_64_b_then_one_o": (9, 7, 0), "pattern_64_one_o_then_b": (9, 7, 0), "pattern_64_one_b_last": (9, 7, 0),
    "pattern_64_alternate": (8, 6, 0), "pattern_64_alternate_o_first": (8, 6, 0), "pattern_64_blocks_of_64": (7, 6, 0),
    "pattern_64_first_o_at_64": (7, 6, 0), "pattern_64_first_o_at_63": (9, 7, 0), "pattern_64_random_b_0.9": (9, 7, 0),
    "pattern_64_random_b_0.1": (9, 7, 0), "pattern_65_b_then_one_o": (9, 7, 0), "pattern_65_one_o_then_b": (9, 7, 0),
    "pattern_65_one_b_last": (9, 7, 0), "pattern_65_alternate": (8, 6, 0), "pattern_65_alternate_o_first": (8, 6, 0),
    "pattern_65_blocks_of_64": (9, 7, 0), "pattern_65_first_o_at_64": (9, 7, 0), "pattern_65_first_o_at_63": (9, 7, 0),
    "pattern_65_random_b_0.9": (9, 7, 0), "pattern_65_random_b_0.1": (9, 7, 0), "pattern_127_b_then_one_o": (10, 8, 0),
    "pattern_127_one_o_then_b": (10, 8, 0), "pattern_127_one_b_last": (10, 8, 0), "pattern_127_alternate": (9, 7, 0),
    "pattern_127_alternate_o_first": (9, 7, 0), "pattern_127_blocks_of_64": (9, 7, 0),
    "pattern_127_first_o_at_64": (10, 8, 0), "pattern_127_first_o_at_63": (10, 8, 0),
    "pattern_127_random_b_0.9": (10, 8, 0), "pattern_127_random_b_0.1": (10, 8, 0), "pattern_128_b_then_one_o": (10, 8, 0),
    "pattern_128_one_o_then_b": (10, 8, 0), "pattern_128_one_b_last": (10, 8, 0), "pattern_128_alternate": (9, 7, 0),
    "pattern_128_alternate_o_first": (9, 7, 0), "pattern_128_blocks_of_64": (9, 7, 0),
    "pattern_128_first_o_at_64": (10, 8, 0), "pattern_128_first_o_at_63": (10, 8, 0),
    "pattern_128_random_b_0.9": (10, 8, 0), "pattern_128_random_b_0.1": (10, 7, 0), "pattern_129_b_then_one_o": (10, 8, 0),
    "pattern_129_one_o_then_b": (10, 8, 0), "pattern_129_one_b_last": (10, 8, 0), "pattern_129_alternate": (9, 7, 0),
    "pattern_129_alternate_o_first": (9, 7, 0), "pattern_129_blocks_of_64": (10, 8, 0),
    "pattern_129_first_o_at_64": (10, 8, 0), "pattern_129_first_o_at_63": (10, 8, 0),
    "pattern_129_random_b_0.9": (10, 8, 0), "pattern_129_random_b_0.1": (10, 7, 0), "pattern_200_b_then_one_o": (11, 9, 0),
    "pattern_200_one_o_then_b": (11, 9, 0), "pattern_200_one_b_last": (11, 9, 0), "pattern_200_alternate": (10, 8, 0),
    "pattern_200_alternate_o_first": (10, 8, 0), "pattern_200_blocks_of_64": (10, 8, 0),
    "pattern_200_first_o_at_64": (11, 9, 0), "pattern_200_first_o_at_63": (11, 9, 0),
    "pattern_200_random_b_0.9": (11, 9, 0), "pattern_200_random_b_0.1": (11, 9, 0),
    "pattern_1000_b_then_one_o": (13, 11, 0), "pattern_1000_one_o_then_b": (13, 11, 0),
    "pattern_1000_one_b_last": (13, 11, 0), "pattern_1000_alternate": (12, 10, 0),
    "pattern_1000_alternate_o_first": (12, 10, 0), "pattern_1000_blocks_of_64": (12, 10, 0),
    "pattern_1000_first_o_at_64": (13, 11, 0), "pattern_1000_first_o_at_63": (13, 11, 0),
    "pattern_1000_random_b_0.9": (13, 11, 0), "pattern_1000_random_b_0.1": (13, 11, 0), "grid_ties_700": (14, 13, 0),
    "signed_zero_boxes_130": (9, 7, 0), "random_3000": (16, 12, 0),
}

_HOST = {}


def host(name):
    """The shape with its transforms in force on the host, built once."""
    if name not in _HOST:
        _HOST[name] = T.get(name).host_scene()[0]
    return _HOST[name]


def _tlas(name):
    sc = host(name)
    return sc.arrays[S.BIND_TLAS_NODES], sc.arrays[S.BIND_TLAS_INDICES]


def test_the_record_dtype_is_the_struct():
    """TlasDfs of rz_scene_dev.h: 64 B, and the offsets the header static_asserts (tests/test_abi_layout.py parses only
    include/, so the header states them and this reads the statement)."""
    assert T.TLAS_DFS.itemsize == 64
    assert {f: T.TLAS_DFS.fields[f][1] for f in T.TLAS_DFS.names} == T.TLAS_DFS_OFFSETS
    src = open(os.path.join(ROOT, "rayzen_amd", "csrc", "hip", "rz_scene_dev.h")).read()
    stated = dict((f, int(o)) for f, o in re.findall(r"offsetof\(TlasDfs, (\w+)\) == (\d+)", src))
    assert stated == T.TLAS_DFS_OFFSETS
    assert re.search(r"static_assert\(sizeof\(TlasDfs\) == 64", src)
    body = re.search(r"struct alignas\(64\) TlasDfs \{(.*?)\n\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*;", body) == list(T.TLAS_DFS.names)         # the members, in order


def test_the_table_is_the_one_the_expectations_were_computed_for():
    assert sorted(EXPECTED) == sorted(T.NAMES)
    assert len(T.NAMES) == 7 + len(T.PATTERN_SIZES) * len(T.PATTERN_KINDS) + 3
    for name in T.NAMES:
        sh = T.get(name)
        assert np.isfinite(sh.transforms).all() and np.isfinite(sh.dirs).all(), name
        assert len(sh.dirs) == sh.n + T.N_BETWEEN + T.N_RANDOM
        det = np.linalg.det(sh.transforms.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64))
        assert np.isfinite(det).all() and (det != 0.0).all(), name              # invertible, every one (in binary64)


@pytest.mark.parametrize("name", T.NAMES)
def test_depth_and_cut(name):
    nodes, idx = _tlas(name)
    assert len(nodes) == 2 * T.get(name).n - 1
    assert T.tree_stats(nodes) == EXPECTED[name]
    # the rule the device kernel applies (`below + 2 <= 64`, below handed down) lets the nodes expand that the shader's loop
    # with its real stack expands
    assert T.cut_by_rule(nodes) == T.shader_walk(nodes)[1]
    dfs = T.pop_order(nodes, idx)
    assert int((dfs["count"] == 0).sum()) == EXPECTED[name][2]
    assert dfs["skip"][0] == len(nodes) and (dfs["skip"] > np.arange(len(dfs))).all()
    assert sorted(dfs["inst0"][dfs["count"] > 0].tolist()) == list(range(T.get(name).n))


def test_the_swapped_hand_down_is_told_apart():
    """rz_tlas_device.hip hands `below` to the left child and `below + 1` to the right one.  Swapped, a right-leaning chain
    would look as harmless as a left-leaning one: nothing cut on chain_right_70, where the shader's loop cuts 6 links --
    and a left-leaning chain would lose links it walks to the bottom."""
    nodes, idx = _tlas("chain_right_70")
    real = T.shader_walk(nodes)[1]
    assert T.cut_by_rule(nodes, 0, 1) == real
    swapped = T.cut_by_rule(nodes, 1, 0)
    assert swapped != real and len(swapped) == 69 and len(real) == 63
    assert T.tree_stats(nodes, 1, 0) == (70, 1, 0)
    want = T.pop_order(nodes, idx)
    mutant = want.copy()
    order = T.complete_order(nodes, 1, 0)
    mutant["count"] = [nodes[i]["count"] if nodes[i]["count"] > 0 else (-1 if below + 2 <= T.STACK else 0)
                       for i, level, below, skip in order]
    assert mutant.tobytes() != want.tobytes() and int((mutant["count"] != want["count"]).sum()) == 6
    nodes, idx = _tlas("chain_left_100")
    assert T.cut_by_rule(nodes, 0, 1) == T.shader_walk(nodes)[1] and len(T.cut_by_rule(nodes, 1, 0)) == 63


def _missing(name):
    sh, osc = T.get(name), oracle_scene(host(name))
    return [i for i in range(sh.n) if not rzo.trace(osc, sh.origins[i], sh.dirs[i])["hit"]]


def test_the_cut_is_visible_to_rays():
    """The rays at the instances' centres: a right-leaning chain hangs its n - 63 nearest instances out of reach, and from
    beside the chain nothing lies behind them."""
    assert _missing("chain_right_70") == list(range(7))
    missing = _missing("chain_right_100")
    assert len(missing) >= 20
    assert missing == list(range(37))                   # the 36 cut links hang the 37 nearest instances out of reach
    assert _missing("chain_y_right_100") == list(range(37))
    assert _missing("chain_left_100") == []              # all 100 found


def _frame_and_balanced(name):
    sc = host(name)
    frame = oracle_render(sc, 64, 36, 1, 2)
    boxes = K.leaf_boxes(sc.arrays[S.BIND_TLAS_NODES], sc.arrays[S.BIND_TLAS_INDICES], T.get(name).n)
    saved = sc.arrays[S.BIND_TLAS_NODES], sc.arrays[S.BIND_TLAS_INDICES]
    sc.arrays[S.BIND_TLAS_NODES], sc.arrays[S.BIND_TLAS_INDICES] = T.balanced_tlas(boxes)
    try:
        assert T.tree_stats(sc.arrays[S.BIND_TLAS_NODES])[0] <= 8
        balanced = oracle_render(sc, 64, 36, 1, 2)
    finally:
        sc.arrays[S.BIND_TLAS_NODES], sc.arrays[S.BIND_TLAS_INDICES] = saved
    assert np.isfinite(frame).all() and np.isfinite(balanced).all()
    return int((frame.view(np.uint32) != balanced.view(np.uint32)).any(-1).sum())


@pytest.mark.parametrize("name,pixels", [("chain_right_70", 42), ("chain_right_100", 454), ("chain_y_right_100", 454)])
def test_the_cut_is_visible_in_a_frame(name, pixels):
    """64 x 36, 1 spp, 2 bounces: the same instances under a hand-built balanced TLAS show the cubes the chain cannot reach."""
    differ = _frame_and_balanced(name)
    assert differ >= 30
    assert differ == pixels


def test_no_cut_no_difference():
    assert _frame_and_balanced("chain_left_100") == 0


@pytest.mark.parametrize("n", T.PATTERN_SIZES)
@pytest.mark.parametrize("kind", T.PATTERN_KINDS)
def test_pattern_partitions_the_root_as_its_mask_says(n, kind):
    """From the host's own leaf boxes and root node: the centres below the root's split (BVH.cpp:214-222, in binary32) are
    the mask's B positions, the first `other` stands where the mask has its first O, and the root's left subtree holds
    nT instances -- count / 2 where the mask is one-sided (BVH.cpp:223)."""
    name = T.pattern_name(n, kind)
    mask = T.pattern_mask(n, kind)
    nodes, idx = _tlas(name)
    boxes = K.leaf_boxes(nodes, idx, n)
    root = nodes[0]
    extent = root["boundsMax"] - root["boundsMin"]
    axis = 1 if extent[1] > extent[0] and extent[1] > extent[2] else 2 if extent[2] > extent[0] else 0      # BVH.cpp:197-199
    split = np.float32(0.5) * (root["boundsMin"][axis] + root["boundsMax"][axis])
    centre = (boxes["boundsMin"][:, axis] + boxes["boundsMax"][:, axis]) * np.float32(0.5)
    below = centre < split
    one_sided = mask.all() or not mask.any()
    assert axis == (2 if one_sided else 0)      # (equal centres: the cube's one 1.000001 makes z the longest extent)
    leaves = lambda i: 1 if nodes[i]["count"] > 0 else leaves(int(nodes[i]["leftFirst"])) + leaves(int(nodes[i]["leftFirst"]) + 1)
    mid = leaves(int(root["leftFirst"]))
    if one_sided:
        assert not below.any() or below.all()
        assert mid == n // 2
        return
    assert split == 0.0
    assert (below == mask).all()
    assert int(below.sum()) == int(mask.sum()) and int(np.flatnonzero(~below)[0]) == int(np.flatnonzero(~mask)[0])
    assert mid == int(mask.sum())
    # the left subtree holds the B instances, the right one the others (every leaf holds one instance, numbered left first)
    assert sorted(idx[:mid].tolist()) == np.flatnonzero(mask).tolist()
    assert sorted(idx[mid:].tolist()) == np.flatnonzero(~mask).tolist()


def test_the_patterns_reach_both_partition_paths_and_the_positions_named():
    one_sided = [(n, k) for n in T.PATTERN_SIZES for k in T.PATTERN_KINDS if T.pattern_mask(n, k).all() or not T.pattern_mask(n, k).any()]
    assert one_sided == [(64, "blocks_of_64"), (64, "first_o_at_64")]
    for n in T.PATTERN_SIZES[1:]:
        assert int(np.flatnonzero(~T.pattern_mask(n, "first_o_at_64"))[0]) == 64
        assert int(np.flatnonzero(~T.pattern_mask(n, "first_o_at_63"))[0]) == 63
    for n in T.PATTERN_SIZES:
        assert abs(T.pattern_mask(n, "random_b_0.9").mean() - 0.9) < 0.1 and abs(T.pattern_mask(n, "random_b_0.1").mean() - 0.1) < 0.1


def test_signed_zero_corners_are_there():
    nodes, idx = _tlas("signed_zero_boxes_130")
    boxes = K.leaf_boxes(nodes, idx, 130)
    corners = np.concatenate([boxes["boundsMin"], boxes["boundsMax"]])
    assert (corners == 0.0).sum() >= 130
    inst = host("signed_zero_boxes_130").arrays[S.BIND_INSTANCES]
    assert np.signbit(inst["inverseTransform"][inst["inverseTransform"] == 0.0]).any()      # -0 in what the kernel must copy


def test_every_shape_is_in_rayzens_fixture():
    with np.load(K.fixture("tlas")) as z:
        whole, digests = K.tlas_names(z)
    assert all(K.shape_case(n) in whole + digests for n in T.NAMES)

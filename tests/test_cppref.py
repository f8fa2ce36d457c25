"""The host builders, the oracle's restatement and the OBJ readers against RayZen's OWN BVH.cpp / Mesh.cpp (oracle/cppref: the
two sources compiled as they stand against a stand-in for the GLM operations they use).  Everything is exact: bytes or digests.

Group 1 (never skips): the recorded outputs of the reference, tests/golden/cppref_*.npz (written by tests/golden/make_cppref.py).
Group 2 (`live`; skips only where oracle/_ref/cppref is not built): the reference re-run here -- the fixtures are current, and a
few hundred seeded random soups go through all three builders.
"""
import os
import tempfile

import numpy as np
import pytest

import cppref_cases as K
from oracle import rzo
from oracle.cppref import cppref
from rayzen_amd import scene as S

BLAS = K.blas_fixture_cases()
LARGE = K.load_large()
with np.load(K.fixture("tlas")) as _z:
    TLAS = {k: _z[k] for k in _z.files}
with np.load(K.fixture("obj")) as _z:
    OBJ = {k: _z[k] for k in _z.files}
TLAS_NAMES, TLAS_DIGESTS = K.tlas_names(TLAS)
OBJ_TEXTS = sorted(k[len("text__"):-len("__bytes")] for k in OBJ if k.endswith("__bytes"))

live = pytest.mark.skipif(not cppref.built(), reason="oracle/_ref/cppref is not built (the reference's sources are not here)")


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape[0]} records, RayZen's has {want.shape[0]}"
    if got.tobytes() != want.tobytes():
        a, b = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
        first = int(np.flatnonzero((a != b).any(1))[0])
        raise AssertionError(f"{what}: first difference at record {first}: {got[first]} != RayZen's {want[first]}")


# ---- group 1: fixtures ------------------------------------------------------------------------------------------------------

def test_the_fixture_holds_every_case_of_the_list():
    want = [(g, n) for g, make in K.BLAS_GROUPS.items() for n, _ in make()]
    assert sorted(BLAS) == sorted(want)
    assert sorted(TLAS_NAMES + TLAS_DIGESTS) == sorted(n for n, _ in K.tlas_cases())
    assert TLAS_DIGESTS == sorted(K.TLAS_BY_DIGEST)
    assert sorted(OBJ_TEXTS) == sorted(K.obj_texts())
    assert sorted(k[:-len("__digest")] for k in LARGE if k.endswith("__digest")) == sorted(n for n, _, _ in K.LARGE)


@pytest.mark.parametrize("group,name", BLAS, ids=[f"{g}-{n}" for g, n in BLAS])
def test_blas_host_and_oracle_equal_rayzens_build(group, name):
    tris, nodes, idx, oob = K.load_blas(group, name)
    hn, hi, depth = S.build_blas(tris)
    _same(hn, nodes, "host nodes")
    _same(hi, idx, "host indices")
    assert depth == K.depth_of(nodes)
    on, oi = rzo.build_blas(tris)
    _same(on.view(S.BVH_NODE), nodes, "oracle nodes")
    _same(oi, idx, "oracle indices")


def test_a_refit_of_unmoved_vertices_is_the_identity_on_rayzens_nodes():
    """BVH::refit (librayzen_host.so) and its numpy statement (tests/refit_ref.py) leave RayZen's own nodes as they are when no
    vertex moved -- signs of zero included, which the union of two children alone does not reproduce: buildBLAS folds a node's
    box in the order its triangles had before the range was sorted (dev_signed_zeros300, node 21, was the first to show it)."""
    import refit_ref
    for g, name in BLAS:
        tris, nodes, idx, _ = K.load_blas(g, name)
        _same(S.refit_blas(tris, nodes, idx), nodes, f"{g}/{name}: host refit")
        _same(refit_ref.refit(tris, nodes, idx), nodes, f"{g}/{name}: numpy refit")


def test_the_inputs_are_what_the_constructors_build_today():
    """A drifted generator (or an edited soup() in the suites the cases are borrowed from) shows here, not as a mismatch."""
    for g, make in K.BLAS_GROUPS.items():
        for name, ctor in make():
            assert np.ascontiguousarray(ctor()).tobytes() == K.load_blas(g, name)[0].tobytes(), (g, name)
    for name, ctor in K.tlas_cases():
        roots = np.ascontiguousarray(ctor())
        if name in TLAS_DIGESTS:
            assert [K.sha(roots), str(len(roots))] == [str(x) for x in TLAS[f"{name}__digest"][[0, 3]]], name
        else:
            assert roots.tobytes() == TLAS[f"{name}__roots"].tobytes(), name
    for name, (text, asserted) in K.obj_texts().items():
        assert text == OBJ[f"text__{name}__bytes"].tobytes(), name
        assert (K.obj_asserted_mask(text, asserted) == OBJ[f"text__{name}__mask"]).all(), name


def test_the_axis_minus_one_cases_are_there():
    """BVH.cpp:137-144 with axis == -1 (no SAH split and x the widest extent) is exercised by flagged fixtures, in small
    and large meshes, and not by ordinary ones."""
    flagged = [n for g, n in BLAS if K.load_blas(g, n)[3] > 0]
    assert len(flagged) >= 30 and "dev_big50" in flagged and "huge_widest_x_120" in flagged
    assert not [n for n in flagged if n.startswith(("size_", "bvh_", "lattice", "denormal", "zeros"))]


def _large(name, ctor, builders):
    tin, tnodes, tidx, n, nn, depth = [str(x) for x in LARGE[f"{name}__digest"]]
    tris = ctor()
    assert (len(tris), K.sha(tris)) == (int(n), tin), f"{name}: the generator no longer makes the mesh the fixture was recorded for"
    for what, build in builders:
        out = build(tris)
        assert len(out[0]) == int(nn), (what, len(out[0]), nn)
        assert (K.sha(out[0]), K.sha(out[1])) == (tnodes, tidx), f"{what} differs from RayZen's build of {name}"
        if len(out) > 2:
            assert out[2] == int(depth), what


@pytest.mark.parametrize("name", [n for n, _, slow in K.LARGE if not slow])
def test_large_blas_by_digest(name):
    ctor = dict((n, c) for n, c, _ in K.LARGE)[name]
    builders = [("host", lambda tris: K.host_build(name, tris))]     # (shared with tests/test_blas_large_cases.py)
    if int(LARGE[f"{name}__digest"][3]) <= 20000:           # the oracle's O(N log^2 N) restatement: the bigger ones are slow
        builders.append(("oracle", rzo.build_blas))
    _large(name, ctor, builders)


SLOW_ADVERSARIAL = [n for n, _, slow in K.LARGE_ADVERSARIAL if slow]


@pytest.mark.slow
@pytest.mark.parametrize("name", SLOW_ADVERSARIAL)
def test_large_adversarial_soups_by_digest_host(name):
    """2.3 M and 4.2 M triangles: 9 s and 19 s of host build on the build machine (the oracle's restatement would take minutes)."""
    _large(name, dict((n, c) for n, c, _ in K.LARGE)[name], [("host", lambda tris: K.host_build(name, tris))])


@pytest.mark.slow
@pytest.mark.parametrize("name", ["blob76_r2.8", "blob150_r1", "blob289_r10"])
def test_large_blas_by_digest_host_and_oracle(name):
    _large(name, dict((n, c) for n, c, _ in K.LARGE)[name], [("host", S.build_blas), ("oracle", rzo.build_blas)])


@pytest.mark.parametrize("name", TLAS_NAMES)
def test_tlas_host_and_oracle_equal_rayzens_build(name):
    roots = TLAS[f"{name}__roots"].view(S.BVH_NODE).reshape(-1)
    nodes, idx = TLAS[f"{name}__nodes"].view(S.BVH_NODE).reshape(-1), TLAS[f"{name}__idx"]
    assert len(nodes) == 2 * len(roots) - 1
    hn, hi = S.build_tlas(roots)
    _same(hn, nodes, "host TLAS nodes")
    _same(hi, idx, "host TLAS indices")
    on, oi = rzo.build_tlas(roots)
    _same(on.view(S.BVH_NODE), nodes, "oracle TLAS nodes")
    _same(oi, idx, "oracle TLAS indices")


@pytest.mark.parametrize("name", TLAS_DIGESTS)
def test_tlas_by_digest_host_and_oracle_equal_rayzens_build(name):
    roots = dict(K.tlas_cases())[name]()
    assert K.tlas_matches(TLAS, name, *S.build_tlas(roots), roots=roots) is None
    on, oi = rzo.build_tlas(roots)
    assert K.tlas_matches(TLAS, name, on.view(S.BVH_NODE), oi) is None


@pytest.mark.parametrize("mesh", K.OBJ_MESHES)
@pytest.mark.parametrize("reader", ["host", "oracle"])
def test_obj_meshes_equal_rayzens_reader(mesh, reader):
    """v0 / v1 / v2 / materialIndex field by field (pads and tail zero on both sides: the reference leaves its tail padding
    uninitialised, the harness copies the fields into zeroed records)."""
    digest, n = [str(x) for x in OBJ[f"mesh__{mesh}__sha"]]
    load = S.load_obj if reader == "host" else rzo.load_obj
    t = load(os.path.join(K.MESHES, mesh), 1)
    assert len(t) == int(n) and K.sha(t) == digest


def _fields(t):
    t = np.ascontiguousarray(t).view(S.TRIANGLE).reshape(-1)
    return np.stack([t["v0"], t["v1"], t["v2"]], 1).view(np.uint32), t["materialIndex"]


def _check_obj_text(name, load):
    text = OBJ[f"text__{name}__bytes"].tobytes()
    want, wmat = _fields(OBJ[f"text__{name}__tris"])
    mask = OBJ[f"text__{name}__mask"]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "case.obj")
        with open(path, "wb") as f:
            f.write(text)
        got, gmat = _fields(load(path, 2))
    assert got.shape == want.shape, f"{name}: {len(got)} triangles, RayZen's reader makes {len(want)}"
    bad = (got != want) & mask
    assert not bad.any(), (f"{name}: triangle / vertex / component {np.argwhere(bad)[0].tolist()}: "
                           f"{got.view(np.float32)[bad][0]!r} != RayZen's {want.view(np.float32)[bad][0]!r}")
    assert (gmat == wmat).all() and (gmat == 2).all()


@pytest.mark.parametrize("name", OBJ_TEXTS)
def test_obj_text_host_reader_equals_rayzens(name):
    _check_obj_text(name, S.load_obj)


@pytest.mark.parametrize("name", OBJ_TEXTS)
def test_obj_text_oracle_reader_equals_rayzens(name):
    _check_obj_text(name, rzo.load_obj)


def test_obj_fixture_records_what_rayzen_does_with_out_of_range_and_non_decimal_tokens():
    """The behaviour the readers were corrected to, as the compiled reference showed it (istringstream >> float of libstdc++):
    overflow stores +-FLT_MAX and fails the stream, underflow stores the denormal or zero and goes on, `nan` / `inf` store 0 and
    fail, a hexadecimal token stores its leading 0 and fails at the x."""
    f = lambda name: np.ascontiguousarray(OBJ[f"text__{name}__tris"]).view(S.TRIANGLE).reshape(-1)
    t = f("out_of_range")
    assert t["v0"][0][0] == K.FLT_MAX                                          # v 1e40 ...
    assert t["v1"][0].tolist() == [1.0, 0.0, 2.0] and t["v2"][0].tolist() == [1.0, -0.0, 2.0]      # 1e-50 -> 0, and the line goes on
    assert np.signbit(t["v2"][0][1])
    assert t["v0"][1].tolist() == [1.0, 2.0, float(K.FLT_MAX)] and t["v1"][1][0] == -K.FLT_MAX
    assert t["v0"][2].view(np.uint32).tolist() == [71362, 0x80000001, 0]       # denormals kept; 7e-46 is below half the least one
    t = f("nan_inf_hex")
    assert t["v0"][0][0] == 0.0 and t["v1"][0].tolist()[:2] == [1.0, 0.0] and t["v2"][0].tolist() == [1.0, 2.0, 0.0]
    assert t["v0"][1].tolist()[:2] == [0.0, 0.0]                               # 0x1p3: 0, then the x fails


# ---- group 2: the reference, live ----------------------------------------------------------------------------------------------

@live
def test_live_fixtures_are_current():
    for g, name in BLAS:
        tris, nodes, idx, oob = K.load_blas(g, name)
        rn, ri, roob = cppref.build_blas(tris, want_axis_minus_one=True)
        _same(rn.view(S.BVH_NODE), nodes, f"{g}/{name} nodes")
        _same(ri, idx, f"{g}/{name} indices")
        assert roob == oob, (g, name)
    for name in TLAS_NAMES:
        rn, ri = cppref.build_tlas(TLAS[f"{name}__roots"].view(S.BVH_NODE).reshape(-1))
        assert rn.tobytes() == TLAS[f"{name}__nodes"].tobytes() and ri.tobytes() == TLAS[f"{name}__idx"].tobytes(), name
    for name in TLAS_DIGESTS:
        roots = dict(K.tlas_cases())[name]()
        assert K.tlas_matches(TLAS, name, *cppref.build_tlas(roots), roots=roots) is None, name
    for name in OBJ_TEXTS:
        t = cppref.load_obj_text(OBJ[f"text__{name}__bytes"].tobytes(), 2)
        assert t.tobytes() == OBJ[f"text__{name}__tris"].tobytes(), name
    for mesh in K.OBJ_MESHES:
        t = cppref.load_obj(os.path.join(K.MESHES, mesh), 1)
        assert [K.sha(t), str(len(t))] == [str(x) for x in OBJ[f"mesh__{mesh}__sha"]]


@live
@pytest.mark.parametrize("name", [n for n, _, slow in K.LARGE if not slow])
def test_live_large_fixtures_are_current(name):
    _large(name, dict((n, c) for n, c, _ in K.LARGE)[name], [("RayZen's BVH.cpp", cppref.build_blas)])


@live
@pytest.mark.slow
def test_live_one_million_triangles():
    """The reference's buildBLAS takes 7.3 s on 1 002 252 triangles on the build machine (the fixture records the time)."""
    _large("blob289_r10", dict((n, c) for n, c, _ in K.LARGE)["blob289_r10"], [("RayZen's BVH.cpp", cppref.build_blas)])


@live
@pytest.mark.slow
@pytest.mark.parametrize("name", SLOW_ADVERSARIAL)
def test_live_large_adversarial_soups(name):
    """The reference's buildBLAS takes 26 s on the 2.3 M soup and 41 s on the 4.2 M one on the build machine."""
    _large(name, dict((n, c) for n, c, _ in K.LARGE)[name], [("RayZen's BVH.cpp", cppref.build_blas)])


def _random_soup(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    kind = seed % 5
    if kind == 0:                                     # ordinary
        return K._rand(n, seed, 5.0, float(rng.uniform(0.01, 2.0)))
    if kind == 1:                                     # lattice: ties
        return K._lattice(n, seed, extent=int(rng.integers(1, 6)))
    if kind == 2:                                     # magnitudes 1e10 ... 3e38
        mag = 10.0 ** rng.uniform(10, 38.4)
        return K._rand(n, seed, mag, mag / float(rng.uniform(2, 50)))
    if kind == 3:                                     # signed zeros and a few small values
        pool = np.array([0.0, -0.0, 0.5, -0.5, 1.0], np.float32)
        return K.tri(*[pool[rng.integers(0, len(pool), (n, 3))] for _ in range(3)])
    t = K._rand(n, seed, 3.0, 0.5)                    # flat in one plane, with duplicates
    for k in ("v0", "v1", "v2"):
        v = t[k]
        v[:, seed % 3] = np.float32(1.25)
        t[k] = v
    t[n // 2:] = t[:n - n // 2]
    return t


@live
@pytest.mark.parametrize("block", range(6))
def test_live_random_soups_through_all_three_builders(block):
    reached = 0
    for seed in range(50 * block, 50 * block + 50):
        tris = _random_soup(seed)
        rn, ri, oob = cppref.build_blas(tris, want_axis_minus_one=True)
        reached += oob > 0
        hn, hi, _ = S.build_blas(tris)
        on, oi = rzo.build_blas(tris)
        _same(hn, rn.view(S.BVH_NODE), f"seed {seed}: host nodes")
        _same(hi, ri, f"seed {seed}: host indices")
        _same(on.view(S.BVH_NODE), rn.view(S.BVH_NODE), f"seed {seed}: oracle nodes")
        _same(oi, ri, f"seed {seed}: oracle indices")
    assert reached >= 3                               # every block has its share of axis == -1 builds


@live
def test_live_random_tlas():
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(1, 80))
        roots = np.zeros(n, S.BVH_NODE)
        if seed % 2:
            lo = rng.integers(-4, 5, (n, 3)).astype(np.float32)
            roots["boundsMin"], roots["boundsMax"] = lo, lo + rng.integers(0, 3, (n, 3)).astype(np.float32)
        else:
            lo = rng.uniform(-30, 30, (n, 3)).astype(np.float32)
            roots["boundsMin"], roots["boundsMax"] = lo, lo + rng.uniform(0, 6, (n, 3)).astype(np.float32)
        rn, ri = cppref.build_tlas(roots)
        hn, hi = S.build_tlas(roots)
        on, oi = rzo.build_tlas(roots)
        assert hn.tobytes() == rn.tobytes() and hi.tobytes() == ri.tobytes(), seed
        assert on.tobytes() == rn.tobytes() and oi.tobytes() == ri.tobytes(), seed


@live
def test_live_midpoint_method_and_cache_round_trip():
    """The reference's other split method builds a valid tree over the same triangles, and BVH::saveToFile / loadFromFile give
    back the arrays in the layout the product's BLAS cache writes: u64 count, nodes, u64 count, indices."""
    tris = K._rand(300, 77, 4.0, 0.3)
    mn, mi = cppref.build_blas(tris, method=cppref.MIDPOINT)
    assert sorted(mi.tolist()) == list(range(300)) and len(mn) % 2 == 1
    (bn, bi), (ln, li), raw = cppref.save_load_round_trip(tris)
    assert bn.tobytes() == ln.tobytes() and bi.tobytes() == li.tobytes()
    hn, hi, _ = S.build_blas(tris)
    want = np.uint64(len(hn)).tobytes() + hn.tobytes() + np.uint64(len(hi)).tobytes() + hi.tobytes()
    assert raw == want

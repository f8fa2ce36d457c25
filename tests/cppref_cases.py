"""The inputs of the comparison with RayZen's own BVH.cpp / Mesh.cpp (oracle/cppref): one list, used by the fixture writer
(tests/golden/make_cppref.py), by the CPU tests (tests/test_cppref.py) and by the GPU tests (tests/test_cppref_gpu.py).

Every BLAS case is (name, constructor).  The inputs tests/test_bvh.py and tests/test_blas_device_gpu.py build are made with
THOSE modules' constructors (imported, not restated); the adversarial ones are defined here.  Only finite vertices: a NaN
centroid breaks std::sort's ordering contract inside the reference, whose output is then undefined.
Fixture files (tests/golden/cppref_<group>.npz) hold, per case, `<case>__tris / __nodes / __idx / __oob` (whole cases) or
`<case>__digest` (large cases: SHA-256 of the input, then SHA-256 / length of the reference's nodes and indices, and the depth;
in cppref_tlas.npz `<case>__roots / __nodes / __idx`, or `<case>__digest` for the cases of TLAS_BY_DIGEST).
"""
import hashlib
import os

import numpy as np

from rayzen_amd import scene as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MESHES = os.path.join(GOLDEN, "meshes")
F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def fixture(group):
    return os.path.join(GOLDEN, f"cppref_{group}.npz")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def depth_of(nodes):
    """Levels of the tree (a lone root: 1), the `depth` S.build_blas and Renderer.build_blas report."""
    best, stack = 0, [(0, 1)]
    while stack:
        i, d = stack.pop()
        best = max(best, d)
        if nodes[i]["count"] < 0:
            L = int(nodes[i]["leftFirst"])
            stack += [(L, d + 1), (L + 1, d + 1)]
    return best


def tri(v0, v1, v2, material=0):
    """(n, 3) float32 vertex arrays -> TRIANGLE records."""
    v0 = np.asarray(v0, F32)
    t = np.zeros(len(v0), S.TRIANGLE)
    t["v0"], t["v1"], t["v2"], t["materialIndex"] = v0, np.asarray(v1, F32), np.asarray(v2, F32), material
    return t


# ---- the inputs of the existing suites ------------------------------------------------------------------------------------

def suite_cases():
    import test_blas_device_gpu as G
    import test_bvh as B
    monkey = lambda: S.load_obj(os.path.join(MESHES, "monkey.obj"), 1)
    cases = [
        # tests/test_bvh.py
        ("bvh_cube", lambda: S.make_cube(0)), ("bvh_blob6", lambda: S.make_blob(6, 2.8, 0)),
        ("bvh_blob20", lambda: S.make_blob(20, 2.8, 1)),
        ("bvh_soup1", lambda: B._soup(1, 0)), ("bvh_soup4", lambda: B._soup(4, 1)), ("bvh_soup5", lambda: B._soup(5, 2)),
        ("bvh_soup777", lambda: B._soup(777, 3)), ("bvh_soup3000", lambda: B._soup(3000, 4, scale=0.05)),
        ("bvh_soup600dup", lambda: B._soup(600, 5, dup=True)), ("bvh_identical37", lambda: np.repeat(B._soup(1, 6), 37)),
        ("bvh_monkey", monkey), ("bvh_cube_obj", lambda: S.load_obj(os.path.join(MESHES, "cube.obj"), 3)),
        ("bvh_empty", lambda: np.zeros(0, S.TRIANGLE)),
    ]
    # tests/test_blas_device_gpu.py
    cases += [(f"dev_soup{n}", lambda n=n: G.soup(n, n)) for n in (1, 2, 4, 5, 7, 33, 257, 2049, 5000)]
    cases += [("dev_blob12", lambda: S.make_blob(12, 1.0, 0))]

    def dup():
        t = G.soup(600, 5)
        t[200:400] = t[0:200]
        return t

    def grid():
        g = G.soup(64, 6)
        for k in ("v0", "v1", "v2"):
            g[k] = np.round(g[k] * 2) / 2
        return np.concatenate([g] * 5)

    def signed_zeros():
        t = G.soup(300, 7, spread=1.0, size=0.5)
        rng = np.random.default_rng(8)
        for k in ("v0", "v1", "v2"):
            v = t[k]
            m = rng.random(v.shape) < 0.3
            v[m] = np.where(rng.random(m.sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
            v[:, 1] = np.where(v[:, 1] < 0, np.float32(-0.0), v[:, 1])
            t[k] = v
        return t

    big = lambda: G.soup(50, 9, spread=1e19, size=1e18)
    cases += [("dev_dup600", dup), ("dev_grid320", grid), ("dev_signed_zeros300", signed_zeros),
              ("dev_zeros37", lambda: np.zeros(37, S.TRIANGLE)), ("dev_big50", big),
              ("dev_mixed250", lambda: np.concatenate([G.soup(200, 10), big()])),
              ("dev_soup100", lambda: G.soup(100, 1)),
              # the meshes of S.bunny_scene(n=20, extras=True) that are not above already
              ("dev_glass_blob5", lambda: S.make_blob(5, 1.2, 3, seed=7)), ("dev_mirror_cube", lambda: S.make_cube(2))]
    return cases


# ---- finite adversarial meshes ---------------------------------------------------------------------------------------------

def _rand(n, seed, centre, size):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-centre, centre, (n, 3))
    return tri(*[(c + rng.uniform(-size, size, (n, 3))).astype(F32) for _ in range(3)])


def _lattice(n, seed, extent=4):
    """Integer-lattice vertices: centroids and costs tie in droves."""
    rng = np.random.default_rng(seed)
    return tri(*[rng.integers(-extent, extent + 1, (n, 3)).astype(F32) for _ in range(3)])


def adversarial_cases():
    cases = []

    def zeros(n, seed):                              # every coordinate +0 or -0, or one of a few small values
        rng = np.random.default_rng(seed)
        pool = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], F32)
        return tri(*[pool[rng.integers(0, len(pool), (n, 3))] for _ in range(3)])

    def zero_planes(n, seed):                        # a random soup whose negative side is clamped to -0, axis by axis
        t = _rand(n, seed, 1.0, 0.5)
        for k in ("v0", "v1", "v2"):
            v = t[k]
            t[k] = np.where(v < 0, F32(-0.0), np.where(v < 0.2, F32(0.0), v))
        return t

    cases += [("zeros_pm_40", lambda: zeros(40, 1)), ("zeros_pm_513", lambda: zeros(513, 2)),
              ("zero_planes_200", lambda: zero_planes(200, 3))]

    def denormal(n, seed, top):
        rng = np.random.default_rng(seed)
        return tri(*[(rng.integers(-top, top + 1, (n, 3)).astype(np.float64) * 2.0 ** -149).astype(F32) for _ in range(3)])

    cases += [("denormal_small_64", lambda: denormal(64, 4, 40)), ("denormal_wide_300", lambda: denormal(300, 5, 8000000)),
              ("denormal_and_normal_128", lambda: np.concatenate([denormal(64, 6, 1000), _rand(64, 7, 1e-37, 1e-38)]))]

    cases += [("lattice_100", lambda: _lattice(100, 8)), ("lattice_tight_700", lambda: _lattice(700, 9, extent=1)),
              ("lattice_1500", lambda: _lattice(1500, 10, extent=9))]

    def points(n, seed, lattice):
        rng = np.random.default_rng(seed)
        p = rng.integers(-3, 4, (n, 3)).astype(F32) if lattice else rng.uniform(-5, 5, (n, 3)).astype(F32)
        return tri(p, p, p)

    def lines(n, seed):
        rng = np.random.default_rng(seed)
        a, b = rng.uniform(-5, 5, (n, 3)).astype(F32), rng.uniform(-5, 5, (n, 3)).astype(F32)
        return tri(a, b, a)

    cases += [("points_random_90", lambda: points(90, 11, False)), ("points_lattice_400", lambda: points(400, 12, True)),
              ("lines_150", lambda: lines(150, 13)),
              ("points_lines_and_triangles_300", lambda: np.concatenate([points(100, 14, True), lines(100, 15), _lattice(100, 16)]))]

    # magnitudes 1e10 ... 3e38: box areas overflow near 1e18-1e19 (an extent of ~1e19 squared is past FLT_MAX), every cost is
    # then inf or NaN, findSAHSplit returns no split and the midpoint fallback runs -- with axis == -1 where x is widest
    for k, mag in enumerate((1e10, 1e15, 1e17, 1e18, 3e18, 1e19, 3e19, 1e20, 1e25, 1e30, 1e35, 1e38)):
        for n in (9, 70, 300):
            cases.append((f"huge_{mag:.0e}_{n}".replace("+", ""), lambda mag=mag, n=n, k=k: _rand(n, 100 + 3 * k + n, mag, mag / 10)))

    def near_flt_max(n, seed):                       # coordinates up to 3e38: sums of three overflow to inf in the centroid
        rng = np.random.default_rng(seed)
        return tri(*[rng.uniform(-3e38, 3e38, (n, 3)).astype(F32) for _ in range(3)])

    def widest(n, seed, axis):                       # overflowing boxes whose widest extent is `axis`
        t = _rand(n, seed, 1e19, 1e18)
        for k in ("v0", "v1", "v2"):
            v = t[k]
            v[:, axis] *= F32(8.0)
            t[k] = v
        return t

    cases += [("huge_3e38_5", lambda: near_flt_max(5, 17)), ("huge_3e38_33", lambda: near_flt_max(33, 18)),
              ("huge_3e38_260", lambda: near_flt_max(260, 19))]
    cases += [(f"huge_widest_{'xyz'[a]}_120", lambda a=a: widest(120, 20 + a, a)) for a in range(3)]
    cases += [("huge_beside_small_400", lambda: np.concatenate([_rand(200, 23, 4.0, 0.3), _rand(200, 24, 1e19, 1e18)]))]

    def flat(n, seed, axis, value, extent):
        t = _rand(n, seed, extent, extent / 20)
        for k in ("v0", "v1", "v2"):
            v = t[k]
            v[:, axis] = value
            t[k] = v
        return t

    for a in range(3):
        cases += [(f"flat_{'xyz'[a]}_250", lambda a=a: flat(250, 30 + a, a, 0.75, 5.0)),
                  (f"flat_{'xyz'[a]}_huge_extent_90", lambda a=a: flat(90, 40 + a, a, -2.0, 1e19)),
                  (f"flat_{'xyz'[a]}_minus_zero_60", lambda a=a: flat(60, 50 + a, a, -0.0, 3.0))]
    return cases


def size_cases():
    """Sizes 1..9 and around every power of two up to 4097: random soups below 600, integer lattices above."""
    sizes = list(range(1, 10))
    for p in range(4, 13):
        sizes += [2 ** p - 1, 2 ** p, 2 ** p + 1]
    sizes = sorted(set(sizes))
    return [(f"size_{n}", (lambda n=n: _rand(n, 1000 + n, 4.0, 0.3)) if n < 600 else (lambda n=n: _lattice(n, 1000 + n, extent=12)))
            for n in sizes]


LARGE = [("blob76_r2.8", lambda: S.make_blob(76, 2.8, 0), False),           # tests/test_bvh.py: 69 312 triangles
         ("blob40_seed3", lambda: S.make_blob(40, 1.0, 0, seed=3), False),   # tests/test_blas_device_gpu.py: 19 200
         ("blob76_r1", lambda: S.make_blob(76, 1.0, 0), False),              # C2's mesh
         ("blob24_r2.8", lambda: S.make_blob(24, 2.8, 0), False),            # the instanced scenes' mesh here: 6 912
         ("blob150_r1", lambda: S.make_blob(150, 1.0, 0), False),            # 270 000
         ("blob289_r10", lambda: S.make_blob(289, 10.0, 0), True)]           # 1 002 252 (slow)

# ---- adversarial meshes of more than 4096 triangles: the device builder's large-node path (rz_blas_device.hip, bbL_*) -------
# What each is for is asserted, on the host's nodes, by tests/test_blas_large_cases.py.

def _cluster(n, seed, x):
    """A soup of extent ~2 whose every vertex is moved by x along the x axis."""
    t = _rand(n, seed, 1.0, 0.05)
    for k in ("v0", "v1", "v2"):
        v = t[k]
        v[:, 0] += F32(x)
        t[k] = v
    return t


def _huge(n, seed, widest=None):
    """Boxes whose area overflows binary32: no SAH cost is finite, the midpoint fallback splits (along `widest`, stretched 8 x)."""
    t = _rand(n, seed, 1e19, 1e18)
    for k in ("v0", "v1", "v2"):
        v = t[k]
        if widest is not None:
            v[:, widest] *= F32(8.0)
        t[k] = v
    return t


def _floor(n, y_of):
    """A soup flattened into the plane y = 0; y_of(n) gives each vertex' zero, (n, 3 vertices) float32 of +0 / -0."""
    t = _rand(n, 5, 4.0, 0.3)
    y = np.asarray(y_of(n), F32)
    for j, k in enumerate(("v0", "v1", "v2")):
        v = t[k]
        v[:, 1] = y[:, j]
        t[k] = v
    return t


def _floor_pm0(n):
    return np.where(np.random.default_rng(6).random((n, 3)) < 0.5, F32(0.0), F32(-0.0))


def _floor_planted(n, everywhere, planted, at):
    y = np.full((n, 3), everywhere, F32)
    y[at] = planted
    return y


LARGE_ADVERSARIAL = [
    ("adv_lattice_20000", lambda: _lattice(20000, 1, 12), False),             # cost ties in droves, across chunks and axes
    ("adv_lattice_tight_9000", lambda: _lattice(9000, 2, 2), False),          # 125 distinct vertices: a tree ~1000 levels deep
    ("adv_huge_6000", lambda: _huge(6000, 3), False),                         # the fallback on a large node (y the widest)
    ("adv_huge_widest_z_6000", lambda: _huge(6000, 3, 2), False),             # the fallback along z
    ("adv_huge_widest_x_6000", lambda: _huge(6000, 3, 0), False),             # ... and with axis == -1
    ("adv_clusters_4096_2000", lambda: np.concatenate([_cluster(4096, 1, -100), _cluster(2000, 2, 100)]), False),
    ("adv_clusters_2048_4049", lambda: np.concatenate([_cluster(4049, 3, 100), _cluster(2048, 4, -100)]), False),
    ("adv_three_clusters", lambda: np.concatenate([_cluster(2048, 5, -300), _cluster(4096, 6, 0), _cluster(4097, 7, 300)]), False),
    ("adv_outlier_first", lambda: np.concatenate([_cluster(1, 8, -1e4), _cluster(6000, 9, 0)]), False),      # a split at i == 1
    ("adv_outlier_last", lambda: np.concatenate([_cluster(6000, 9, 0), _cluster(1, 8, 1e4)]), False),        # at i == N - 1
    ("adv_floor_pm0_10000", lambda: _floor(10000, _floor_pm0), False),        # the sign of a zero in a large node's box
    ("adv_floor_one_minus_zero_last", lambda: _floor(10000, lambda n: _floor_planted(n, 0.0, -0.0, n - 1)), False),
    ("adv_floor_plus_zero_first", lambda: _floor(10000, lambda n: _floor_planted(n, -0.0, 0.0, 0)), False),
    ("adv_dup_4200", lambda: np.repeat(_rand(1, 7, 1.0, 0.3), 4200), False),  # one triangle 4200 times
    ("adv_zero_4200", lambda: np.zeros(4200, S.TRIANGLE), False),             # a chain 4197 levels deep: every node splits 1 | N-1
    ("adv_soup_2300000", lambda: _rand(2300000, 8, 4.0, 0.05), True),         # more than 256 large nodes on one level (slow)
    ("adv_soup_4200000", lambda: _rand(4200000, 8, 4.0, 0.05), True),         # a root of more than 2048 chunks (slow)
]
LARGE += LARGE_ADVERSARIAL

_HOST_BUILDS = {}


def host_build(name, tris):
    """S.build_blas of a LARGE case, built once per session for the modules that share it (up to 2.3 M triangles are kept)."""
    if name in _HOST_BUILDS:
        return _HOST_BUILDS[name]
    out = S.build_blas(tris)
    if len(tris) <= 2300000:
        _HOST_BUILDS[name] = out
    return out


def node_counts_and_levels(nodes):
    """Per node: the triangles below it and its level (the root: 1)."""
    left = nodes["leftFirst"].astype(np.int64)
    count, level = nodes["count"].astype(np.int64), np.zeros(len(nodes), np.int64)
    internal_by_level, front = [], np.zeros(1, np.int64)
    while len(front):                                # level by level: a deep chain is thousands of short steps, not of nodes
        level[front] = len(internal_by_level) + 1
        internal = front[count[front] < 0]
        internal_by_level.append(internal)
        front = np.concatenate([left[internal], left[internal] + 1])
    for internal in internal_by_level[::-1]:
        count[internal] = count[left[internal]] + count[left[internal] + 1]
    assert (level > 0).all()
    return count, level


BLAS_GROUPS = {"suite": suite_cases, "adversarial": adversarial_cases, "sizes": size_cases}


def blas_fixture_cases():
    """[(group, name)] of every whole BLAS case, from the fixture files alone."""
    out = []
    for g in BLAS_GROUPS:
        with np.load(fixture(g)) as z:
            out += [(g, k[:-len("__tris")]) for k in z.files if k.endswith("__tris")]
    return out


def load_blas(group, name):
    with np.load(fixture(group)) as z:
        return (z[f"{name}__tris"].view(S.TRIANGLE).reshape(-1), z[f"{name}__nodes"].view(S.BVH_NODE).reshape(-1),
                z[f"{name}__idx"], int(z[f"{name}__oob"]))


def load_large():
    with np.load(fixture("large")) as z:
        return {k: z[k] for k in z.files}


# ---- TLAS ---------------------------------------------------------------------------------------------------------------------

INSTANCED = [("inst16", 24, 16, (0, 3, 7, 11)), ("inst9", 6, 9, (0, 5))]      # name, blob n, count, frames


def instanced_frame_transforms(sc, frame, count):
    """Object 0 (the floor) keeps its transform; the `count` instances take S.instanced_transforms(frame, count)."""
    return np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                    [np.asarray(t, F32).reshape(16) for t in S.instanced_transforms(frame, count)])


def leaf_boxes(nodes, idx, n):
    """instance -> its world box, read off the one-instance leaves of a TLAS (BVH.cpp:204-208): BVH_NODE records, only
    boundsMin / boundsMax set."""
    roots = np.zeros(n, S.BVH_NODE)
    seen = np.zeros(n, bool)
    for nd in nodes:
        if nd["count"] == 1:
            i = int(idx[nd["leftFirst"]])
            roots[i]["boundsMin"], roots[i]["boundsMax"] = nd["boundsMin"], nd["boundsMax"]
            seen[i] = True
    assert seen.all()
    return roots


def tlas_cases():
    cases = []
    for n, seed in [(1, 0), (2, 1), (3, 2), (16, 3), (50, 4)]:               # tests/test_bvh.py::test_tlas_builder_matches
        def make(n=n, seed=seed):
            rng = np.random.default_rng(seed)
            roots = np.zeros(n, S.BVH_NODE)
            lo = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
            roots["boundsMin"], roots["boundsMax"] = lo, lo + rng.uniform(0.1, 4, (n, 3)).astype(np.float32)
            return roots
        cases.append((f"random_{n}", make))

    def identical(n):
        roots = np.zeros(n, S.BVH_NODE)
        roots["boundsMin"], roots["boundsMax"] = (-1, -1, -1), (1, 1, 1)
        return roots

    cases += [("identical_6", lambda: identical(6)), ("identical_2", lambda: identical(2)), ("identical_33", lambda: identical(33))]

    def lattice(n, seed):                            # box corners on a coarse lattice: centroids equal the split plane often
        rng = np.random.default_rng(seed)
        roots = np.zeros(n, S.BVH_NODE)
        lo = rng.integers(-3, 4, (n, 3)).astype(F32)
        roots["boundsMin"], roots["boundsMax"] = lo, lo + rng.integers(0, 3, (n, 3)).astype(F32)
        return roots

    def signed_zeros(n, seed):                       # corners that are +0 or -0: the sign glm::min / glm::max keep shows in the boxes
        rng = np.random.default_rng(seed)
        roots = np.zeros(n, S.BVH_NODE)
        roots["boundsMin"] = np.array([-0.0, 0.0, -1.0, -2.0], F32)[rng.integers(0, 4, (n, 3))]
        roots["boundsMax"] = np.array([-0.0, 0.0, 1.0, 2.0], F32)[rng.integers(0, 4, (n, 3))]
        return roots

    cases += [("lattice_40", lambda: lattice(40, 5)), ("lattice_257", lambda: lattice(257, 6)),
              ("signed_zeros_24", lambda: signed_zeros(24, 7)), ("signed_zeros_130", lambda: signed_zeros(130, 8))]

    for name, n, count, frames in INSTANCED:
        for fr in frames:
            def make(n=n, count=count, fr=fr):
                sc = S.instanced_scene(n=n, count=count)
                for oid, t in zip(sc.instance_ids, S.instanced_transforms(fr, count)):
                    sc.set_transform(oid, t)
                sc.update_dynamic()
                return leaf_boxes(sc.arrays[S.BIND_TLAS_NODES], sc.arrays[S.BIND_TLAS_INDICES], count + 1)
            cases.append((f"{name}_frame{fr}", make))

    def rayzen_main():
        sc = S.reference_scene(monkey_obj=os.path.join(MESHES, "monkey.obj"))
        return leaf_boxes(sc.arrays[S.BIND_TLAS_NODES], sc.arrays[S.BIND_TLAS_INDICES], 7)

    cases.append(("rayzen_main_scene", rayzen_main))

    # tests/tlas_shapes.py: the world boxes SceneBuffers::updateDynamic gives every shape of the table (chains deeper than the
    # shader's stack, equal centres, chosen partitions, lattices, signed zeros)
    import tlas_shapes
    for name in tlas_shapes.NAMES:
        def make(name=name):
            sh = tlas_shapes.get(name)
            sc, _ = sh.host_scene()
            return leaf_boxes(sc.arrays[S.BIND_TLAS_NODES], sc.arrays[S.BIND_TLAS_INDICES], sh.n)
        cases.append((shape_case(name), make))
    return cases


def shape_case(name):
    return f"shape_{name}"


TLAS_BY_DIGEST = ("shape_random_3000",)         # 3 000 x (32 + 64 + 4) B: recorded as the large BLAS cases are


def tlas_digest(roots, nodes, idx):
    return np.array([sha(roots), sha(nodes), sha(idx), str(len(roots)), str(len(nodes))])


def tlas_names(fix):
    """(whole cases, cases by digest) of a loaded cppref_tlas.npz."""
    return (sorted(k[:-len("__roots")] for k in fix if k.endswith("__roots")),
            sorted(k[:-len("__digest")] for k in fix if k.endswith("__digest")))


def tlas_matches(fix, name, nodes, idx, roots=None):
    """None, or what differs between a TLAS (and optionally its input boxes) and the fixture's record of RayZen's build."""
    nodes, idx = np.ascontiguousarray(nodes), np.ascontiguousarray(idx)
    if f"{name}__digest" in fix:
        want = [str(x) for x in fix[f"{name}__digest"]]
        if roots is not None and (sha(roots), str(len(roots))) != (want[0], want[3]):
            return "root boxes"
        if str(len(nodes)) != want[4] or sha(nodes) != want[1]:
            return "nodes"
        return None if sha(idx) == want[2] else "indices"
    if roots is not None and np.ascontiguousarray(roots).tobytes() != fix[f"{name}__roots"].tobytes():
        return "root boxes"
    if nodes.tobytes() != fix[f"{name}__nodes"].tobytes():
        return "nodes"
    return None if idx.tobytes() == fix[f"{name}__idx"].tobytes() else "indices"


# ---- OBJ ------------------------------------------------------------------------------------------------------------------------
# Each text is a list of lines: ("v", text, asserted) -- a vertex line and how many of its components may be asserted (3 unless
# an extraction fails: with real GLM the reference's `glm::vec3 v;` is uninitialised, so what follows the failing component is
# RayZen's stack, and a component the stream never reached -- a short line -- is not written at all); ("f", text) -- a face line
# with in-range numeric indices only (anything else is an out-of-bounds read or an uncaught throw in the reference);
# ("x", text) -- any other line.  `eol` joins them; `final` says whether the last line ends with it.

def _obj(lines, eol="\n", final=True):
    text = eol.join(t for _, t, *_ in lines) + (eol if final else "")
    return text.encode("ascii"), [a[2] for a in lines if a[0] == "v"]


_TRI = [("v", "v 0 0 0", 3), ("v", "v 1 0 0", 3), ("v", "v 0 1 0", 3), ("v", "v 1 1 0.5", 3), ("v", "v -1 2 3.25", 3)]


def obj_texts():
    """name -> (bytes, asserted components per vertex line)."""
    T = {}
    T["crlf"] = _obj(_TRI + [("x", "vn 0 0 1"), ("f", "f 1 2 3"), ("f", "f 2 4 3 5")], eol="\r\n")
    T["slashes"] = _obj(_TRI + [("x", "vt 0.5 0.5"), ("x", "vn 0 0 1"), ("f", "f 1/1/1 2/1/1 3/1/1"), ("f", "f 2//1 4//1 3//1"),
                                ("f", "f 5/1 4/1 1/1")])
    T["polygons"] = _obj(_TRI + [("x", "# a pentagon, a quad, a two-gon and a lone index"), ("f", "f 1 2 4 5 3"), ("f", "f 5 4 3 2"),
                                 ("f", "f 1 2"), ("f", "f 3"), ("x", "f"), ("x", "g group"), ("x", "usemtl m"), ("x", "s off")])
    T["no_final_newline"] = _obj(_TRI + [("f", "f 1 2 3"), ("f", "f 3 4 5")], final=False)
    T["no_final_newline_crlf"] = _obj(_TRI + [("f", "f 1 2 3"), ("f", "f 3 4 5")], eol="\r\n", final=False)
    T["spacing"] = _obj([("v", "v   1.5\t 2.5   -3.5   ", 3), ("v", "v 4 5 6 1.0", 3), ("x", "v\t7 8 9"), ("x", " v 1 1 1"),
                         ("x", "vv 1 1 1"), ("v", "v 10 11 12 # colour", 3), ("v", "v 1 2 3", 3),
                         ("f", "f  1   2\t3  "), ("f", "f 2 3 4"), ("x", "f\t1 2 3"), ("x", " f 1 2 3"), ("x", "")])
    T["plus_and_exponents"] = _obj([("v", "v +1 +2.5 +.5", 3), ("v", "v 1e2 1E2 1e+2", 3), ("v", "v 1.e-2 -1.5E-3 +2.e+1", 3),
                                    ("v", "v 000.5 -00 0010", 3), ("v", "v 1. .5 -.25", 3), ("v", "v 123456789 0.1234567891234 16777217", 3),
                                    ("v", "v 3.4028235e38 -3.4028235e38 1.17549435e-38", 3), ("f", "f 1 2 3"), ("f", "f 4 5 6"),
                                    ("f", "f 7 1 2"), ("f", "f +1 +2 +3"), ("f", "f 01 002 3")])
    T["out_of_range"] = _obj([("v", "v 1e40 1e-50 0", 1), ("v", "v 1 1e-50 2", 3), ("v", "v 1 -1e-50 2", 3), ("v", "v 1 2 1e39", 3),
                              ("v", "v -1e40 5 6", 1), ("v", "v 7 -3.5e38 8", 2), ("v", "v 1e-40 -1e-45 7e-46", 3),
                              ("v", "v 3.4028236e38 1 1", 3), ("v", "v 3.4028235678e38 1 1", 1), ("v", "v 1e-46 2 3", 3),
                              ("v", "v 1e99999 1 1", 1), ("v", "v 1e-99999 1 1", 3),
                              ("f", "f 1 2 3"), ("f", "f 4 5 6"), ("f", "f 7 8 9"), ("f", "f 10 11 12")])
    T["nan_inf_hex"] = _obj([("v", "v nan 0 0", 1), ("v", "v 1 inf 0", 2), ("v", "v 1 2 -inf", 3), ("v", "v 0x1p3 1 0", 2),
                             ("v", "v NAN 1 1", 1), ("v", "v infinity 1 1", 1), ("v", "v 1 2 0x10", 3), ("v", "v -nan 1 1", 1),
                             ("v", "v 5 6 7", 3), ("f", "f 1 2 3"), ("f", "f 4 5 6"), ("f", "f 7 8 9")])
    T["malformed_numbers"] = _obj([("v", "v 1.5abc 2 3", 2), ("v", "v 1e 2 3", 1), ("v", "v 1e+ 2 3", 1), ("v", "v . 2 3", 1),
                                   ("v", "v 1..2 3 4", 3), ("v", "v 1 2", 2), ("v", "v 1", 1), ("v", "v ", 0), ("v", "v - 1 2", 1),
                                   ("v", "v 1,5 2 3", 2), ("v", "v 1e5e2 2 3", 2), ("v", "v 1f 2 3", 2), ("v", "v 1.0.0 2 3", 3),
                                   ("v", "v +-1 2 3", 1), ("v", "v 1e2.5 7 8", 3),
                                   ("f", "f 1 2 3"), ("f", "f 4 5 6"), ("f", "f 7 8 9"), ("f", "f 10 11 12"), ("f", "f 13 14 15")])
    T["odd_whitespace"] = _obj([("v", "v 1\v2\f3", 3), ("v", "v 4 5 6", 3), ("v", "v 7 8 9", 3), ("f", "f 1\v2\f3"),
                                ("f", "f 1 2\r3")])
    T["face_tokens"] = _obj(_TRI + [("f", "f 1abc 2 3"), ("f", "f 2.9 3.1 4"), ("f", "f 1/ 2/ 3/"), ("f", "f 3/x/y 4/-1 5/")])
    return T


OBJ_MESHES = ("monkey.obj", "cube.obj")


def obj_asserted_mask(text, asserted):
    """(n_triangles, 3 vertices, 3 components) bool: which components of the reference's output may be asserted, from the
    per-vertex-line counts and this module's own reading of its own face lines (cut at '/', leading integer, fan)."""
    import re
    faces = []
    for line in re.split(rb"\n", text):
        if line[:2] == b"f ":
            ids = [int(re.match(rb"[+-]?\d+", tok.split(b"/")[0]).group()) for tok in line[2:].split()]
            faces += [(ids[0], ids[i], ids[i + 1]) for i in range(1, len(ids) - 1)] if len(ids) >= 3 else []
    mask = np.zeros((len(faces), 3, 3), bool)
    for t, f in enumerate(faces):
        for k, v in enumerate(f):
            mask[t, k, :asserted[v - 1]] = True
    return mask

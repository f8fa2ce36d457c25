"""A table of TLAS shapes for the device rebuild (rz_tlas_device.hip) and the list it writes in the shader's pop order
(TlasDfs, rz_scene_dev.h): what RayZen's own builder (BVH.cpp:178-240) makes of instances spread over many octaves (chains
deeper than the shader's stack[64]), of equal centres (the count / 2 fallback at every level), of chosen below / other
sequences at the root (the Lomuto partition the kernel emulates with a queue) and of lattices and signed zeros (ties).

One list, used by tests/cppref_cases.py (the fixture of RayZen's own build of every shape), tests/test_tlas_shapes_cases.py
(CPU: the table has the depths, cuts and partitions it says) and tests/test_tlas_shapes_gpu.py.  Every shape is cubes
(S.make_cube: Blender's, +-1; two materials, shared meshes) uploaded at identity and moved by the transforms alone, a camera, and a batch of
rays: one per instance aimed at its centre, 256 aimed between neighbours, 256 seeded random directions.

Also here, because all three users need them: the numpy dtype of a TlasDfs record, a restatement of the shader's TLAS loop
(FS:464-501) that lists the nodes in pop order, and a hand-built balanced TLAS over the same leaf boxes.
"""
import numpy as np

from rayzen_amd import scene as S

F32 = np.float32
I32 = np.int32

# rz_scene_dev.h: struct TlasDfs (the header static_asserts these offsets)
TLAS_DFS = np.dtype({"names": ["bmin", "first", "bmax", "count", "skip", "inst0", "pad"],
                     "formats": [(F32, 3), I32, (F32, 3), I32, I32, I32, (I32, 6)],
                     "offsets": [0, 12, 16, 28, 32, 36, 40], "itemsize": 64})
TLAS_DFS_OFFSETS = dict(bmin=0, first=12, bmax=16, count=28, skip=32, inst0=36, pad=40)

STACK = 64                      # the shader's `int stack[64]` (FS:460)
N_BETWEEN = N_RANDOM = 256


class Shape:
    def __init__(self, name, transforms, camera, seed, ray_eye=None):
        self.name = name
        self.transforms = np.ascontiguousarray(transforms, F32).reshape(-1, 16)
        self.n = len(self.transforms)
        self.camera = camera
        eye = camera.position if ray_eye is None else ray_eye
        self.origins, self.dirs = _rays(self.transforms[:, 12:15].astype(np.float64), np.asarray(eye, np.float64), seed)

    def scene(self):
        """The scene as uploaded: every instance at identity.  Returns (scene, object ids)."""
        sc = S.Scene(camera=self.camera)
        cube, mirror = sc.add_mesh(S.make_cube(0)), sc.add_mesh(S.make_cube(2))
        ids = [sc.add_object(mirror if i % 3 == 0 else cube) for i in range(self.n)]
        sc.build(share_meshes=True)
        return sc, ids

    def host_scene(self, transforms=None):
        """... and with the transforms in force on the host (SceneBuffers::updateDynamic): the expected bindings 9 / 10 / 11."""
        sc, ids = self.scene()
        set_transforms(sc, ids, self.transforms if transforms is None else transforms)
        return sc, ids


def set_transforms(sc, ids, transforms):
    for oid, t in zip(ids, np.ascontiguousarray(transforms, F32).reshape(-1, 16)):
        sc.set_transform(oid, t)
    sc.update_dynamic()


def _rays(centres, eye, seed):
    """(origins, unit directions), float32: n rays at the instances' centres (a cube's world-box centre is its translation),
    N_BETWEEN at points between instance i and i + 1, N_RANDOM seeded directions; all from `eye`.  Directions are
    normalised in binary64 (a chain's far end lies 2^99 away: nothing here may square a distance in binary32)."""
    rng = np.random.default_rng(seed)
    n = len(centres)
    k = np.arange(N_BETWEEN) % n
    u = rng.uniform(0.25, 0.75, (N_BETWEEN, 1))
    between = centres[k] * (1.0 - u) + centres[(k + 1) % n] * u
    d = np.concatenate([centres - eye, between - eye, rng.normal(size=(N_RANDOM, 3))])
    norm = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(norm > 0, d / np.where(norm > 0, norm, 1.0), np.array([0.0, 0.0, -1.0]))
    return np.tile(eye, (len(d), 1)).astype(F32), d.astype(F32)


def _trs(pos, scale):
    """translate(identity, pos) * scale(scale), column-major, as glm builds it (every entry one exact value)."""
    pos, scale = np.asarray(pos, np.float64).reshape(-1, 3), np.asarray(scale, np.float64)
    scale = np.broadcast_to(scale[:, None] if scale.ndim == 1 else scale, pos.shape)        # (n,): uniform per instance
    m = np.zeros((len(pos), 16), F32)
    m[:, 0], m[:, 5], m[:, 10], m[:, 15] = scale[:, 0], scale[:, 1], scale[:, 2], 1.0
    m[:, 12:15] = pos
    return m


# ---- chains: one instance per octave ------------------------------------------------------------------------------------------

def chain(n, sign, long_axis=0, side=None, ray_side=None):
    """Instance i at (sign 2^i, 0.3 2^i sin i, 0.3 2^i cos i), scaled by 0.2 2^i: the midpoint split peels the farthest
    instance off at every level.  sign = -1: the peeled one is the LEFT child (its centre is below the split) and the
    chain goes on in the right child, which the shader pops first while the left leaf waits on the stack -- from level 63
    on the stack is full and the n - 63 NEAREST instances hang out of reach.  sign = +1: the chain goes on in the left
    child and one entry waits at most.  long_axis = 1 permutes the axes (x -> y -> z -> x).

    The camera: seen from the origin every direction of the spiral is covered by some farther cube (S.make_cube spans
    +-1, so a cube fills 0.2 rad around its centre on a ring of 0.3 rad), and a ray at an unreachable cube would only
    find the one behind it.  `side` = k puts the camera beside the chain instead, 1.4 2^k away from the axis at
    x = -2^(k - 1), looking across it: rays at the near instances leave the spiral's cone behind them, and instances
    k - 3 .. k - 1 fill a good part of a 64 x 36 frame.  A frame needs k small (the shader builds a pixel's direction as
    (camera + offset) - camera in binary32), rays that leave 37 instances behind need the eye 2^35 out: `ray_side` puts
    the eye of the ray batch there, and it is the one place where the batch is not cast from the camera.
    (glm::inverse of a scale of 0.2 2^i overflows binary32 in its determinant from i = 45 on: those instances' inverse
    matrices are NaN in RayZen as here, no ray ever enters them, and they are in the table as what a front end gets that
    spreads objects this far, not as something to aim at.)"""
    i = np.arange(n, dtype=np.float64)
    p = np.stack([sign * 2.0 ** i, 0.3 * 2.0 ** i * np.sin(i), 0.3 * 2.0 ** i * np.cos(i)], 1)
    p = np.roll(p, long_axis, axis=1)
    beside = lambda k: np.roll(np.array([sign * 2.0 ** (k - 1), 0.0, 1.4 * 2.0 ** k]), long_axis)
    if side is None:
        eye, look = np.zeros(3), np.array([float(sign), 0.0, 0.0])
    else:
        eye, look = beside(side), np.array([0.0, 0.0, -1.0])
    up = np.roll(np.array([0.0, 1.0, 0.0]), long_axis)
    cam = S.Camera(position=tuple(eye), target=tuple(np.roll(look, long_axis)), up=tuple(up), fov=70.0, aspect=16.0 / 9.0)
    return _trs(p, 0.2 * 2.0 ** i), cam, (None if ray_side is None else beside(ray_side))


# ---- equal centres ---------------------------------------------------------------------------------------------------------------

def identical(n):
    cam = S.Camera(position=(0.0, 0.0, 3.0), aspect=16.0 / 9.0)
    return _trs(np.tile([0.0, 0.0, -2.0], (n, 1)), np.ones(n)), cam


# ---- chosen below / other sequences at the root ------------------------------------------------------------------------------------

PATTERN_SIZES = (64, 65, 127, 128, 129, 200, 1000)
PATTERN_KINDS = ("b_then_one_o", "one_o_then_b", "one_b_last", "alternate", "alternate_o_first", "blocks_of_64",
                 "first_o_at_64", "first_o_at_63", "random_b_0.9", "random_b_0.1")


def pattern_mask(n, kind):
    """True: the instance at that position is `below` the root's split (B); False: `other` (O)."""
    i = np.arange(n)
    rng = np.random.default_rng(1000 * n + PATTERN_KINDS.index(kind))
    if kind == "b_then_one_o":
        return i < n - 1
    if kind == "one_o_then_b":
        return i > 0
    if kind == "one_b_last":
        return i == n - 1
    if kind == "alternate":
        return i % 2 == 0
    if kind == "alternate_o_first":
        return i % 2 == 1
    if kind == "blocks_of_64":
        return (i // 64) % 2 == 0
    if kind in ("first_o_at_64", "first_o_at_63"):
        f = int(kind[-2:])
        return (i < f) | ((i > f) & (rng.random(n) < 0.5))          # (n = 64 has no position 64: all B)
    return rng.random(n) < float(kind[-3:])


def pattern(n, kind):
    """Centres at x = -1 - i 2^-10 (B) or +1 + i 2^-10 (O), cubes of edge 0.5.  Two of the n instances are anchors that fix
    the root's bounds, so that its split is x = 0 whatever the mask: the first B stands at x = -4 and the first O at x = +4
    (each on its own side, so the sequence is the mask's).  A one-sided mask cannot be laid out with a split at all -- the
    builder takes its count / 2 fallback only where every centre equals the split -- so there every instance stands at
    x = -1."""
    mask = pattern_mask(n, kind)
    i = np.arange(n, dtype=np.float64)
    x = np.where(mask, -1.0 - i / 1024.0, 1.0 + i / 1024.0)
    if mask.all() or not mask.any():
        x[:] = -1.0
    else:
        x[np.flatnonzero(mask)[0]], x[np.flatnonzero(~mask)[0]] = -4.0, 4.0
    p = np.stack([x, np.zeros(n), np.zeros(n)], 1)
    cam = S.Camera(position=(0.0, 1.5, 9.0), target=(0.0, -0.15, -1.0), fov=60.0, aspect=16.0 / 9.0)
    return _trs(p, np.full(n, 0.5)), cam


# ---- lattices, signed zeros, random ---------------------------------------------------------------------------------------------------

def scattered(n, seed, snapped):
    """The generator of tests/test_gpu_cases.py::test_device_tlas_matches_host_for_random_transforms, statement for statement
    (there n % 3 == 0 chooses the snapped branch and the seed is n)."""
    rng = np.random.default_rng(seed)
    xf = []
    for _ in range(n):
        pos = np.round(rng.uniform(-20, 20, 3) / 8.0) * 8.0 if snapped else rng.uniform(-20, 20, 3)
        t = S.translate(S.identity(), pos)
        t = S.rotate(t, 0.0 if snapped else float(rng.uniform(0, 6.28)), rng.normal(size=3))
        t = S.scale(t, (1.0, 1.0, 1.0) if snapped else rng.uniform(0.3, 3.0, 3))
        xf.append(np.asarray(t, F32).reshape(16))
    cam = S.Camera(position=(0.0, 0.0, 60.0), fov=45.0, aspect=16.0 / 9.0)
    return np.stack(xf), cam


def signed_zero_boxes(n, seed=130):
    """Scales of +-1 (half of them negative) and translations of +-1 that cancel one face of the cube's +-1 exactly (on z
    the face at -1: the other one is Blender's 1.000001): every world box is [0, 2] or [-2, 0] per axis up to that last
    place, and the zero corner is the sum (-+1 + +-0) + (+-0 + +-1) of mat4 * vec4, whose zero products carry the signs of
    the scales.  Eight distinct boxes: ties in every bound and equal centres at every level."""
    rng = np.random.default_rng(seed)
    s = np.where(rng.random((n, 3)) < 0.5, 1.0, -1.0)
    t = np.where(rng.random((n, 3)) < 0.5, 1.0, -1.0)
    t[:, 2] = s[:, 2]
    cam = S.Camera(position=(0.7, 0.5, 7.0), fov=50.0, aspect=16.0 / 9.0)
    return _trs(t, s), cam


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

def _table():
    T = {
        "chain_right_70": lambda: chain(70, -1, side=7), "chain_right_100": lambda: chain(100, -1, side=7, ray_side=35),
        "chain_left_100": lambda: chain(100, +1), "chain_y_right_100": lambda: chain(100, -1, long_axis=1, side=7, ray_side=35),
        "identical_130": lambda: identical(130), "identical_64": lambda: identical(64), "identical_65": lambda: identical(65),
    }
    for n in PATTERN_SIZES:
        for kind in PATTERN_KINDS:
            T[pattern_name(n, kind)] = lambda n=n, kind=kind: pattern(n, kind)
    T["grid_ties_700"] = lambda: scattered(700, 700, True)
    T["signed_zero_boxes_130"] = lambda: signed_zero_boxes(130)
    # (the random branch of the generator: its own n % 3 rule would snap 3 000 to the lattice, which grid_ties_700 has)
    T["random_3000"] = lambda: scattered(3000, 3000, False)
    return T


def pattern_name(n, kind):
    return f"pattern_{n}_{kind}"


_TABLE = _table()
NAMES = list(_TABLE)
CHAINS = [n for n in NAMES if n.startswith("chain_")]
_made = {}


def get(name):
    if name not in _made:
        xf, cam, *eye = _TABLE[name]()
        _made[name] = Shape(name, xf, cam, seed=NAMES.index(name), ray_eye=eye[0] if eye else None)
    return _made[name]


# ---- the shader's TLAS loop, restated ---------------------------------------------------------------------------------------------------

def shader_walk(nodes):
    """FS:464-501 with every box test passing: `int stack[64]; sp = 0; stack[sp++] = 0;` pop, and for an internal node push
    left then right (so right is popped first) -- when both fit; the oracle (rz_oracle.c) drops a push that does not.
    Returns (nodes in the order they are popped, the set of internal nodes that expanded)."""
    stack = np.zeros(STACK, np.int64)
    sp = 0
    stack[sp] = 0
    sp += 1
    popped, expanded = [], set()
    while sp > 0:
        sp -= 1
        i = int(stack[sp])
        popped.append(i)
        if nodes[i]["count"] < 0 and sp + 2 <= STACK:
            expanded.add(i)
            stack[sp], stack[sp + 1] = nodes[i]["leftFirst"], nodes[i]["leftFirst"] + 1
            sp += 2
    return popped, expanded


def complete_order(nodes, left_add=0, right_add=1):
    """The whole tree in pop order (right child first) whether a push fits or not, as the list holds it.  Per position:
    (node, level, stack entries below it when popped, position after its subtree).  The entries below a child are its
    parent's plus `left_add` / `right_add`: the left child waits under the right one."""
    order, todo = [], [(0, 1, 0, -1)]
    parent = []
    while todo:
        i, level, below, par = todo.pop()
        pos = len(order)
        order.append([i, level, below, 0])
        parent.append(par)
        if nodes[i]["count"] < 0:
            L = int(nodes[i]["leftFirst"])
            todo.append((L, level + 1, below + left_add, pos))
            todo.append((L + 1, level + 1, below + right_add, pos))
    size = [1] * len(order)
    for p in range(len(order) - 1, 0, -1):
        size[parent[p]] += size[p]
    for p, rec in enumerate(order):
        rec[3] = p + size[p]
    return order


def pop_order(nodes, idx):
    """TlasDfs[] of a TLAS, independent of rz_context.hip's tlas_pop_order: positions and skips from the complete walk's
    subtree sizes, and `count` of an internal node -1 where the shader's loop with its real stack of 64 expanded it, 0 where
    its push was dropped (or it lies under such a node and is never popped at all)."""
    nodes = np.ascontiguousarray(nodes).view(S.BVH_NODE).reshape(-1)
    out = np.zeros(len(nodes), TLAS_DFS)
    if not len(nodes):
        return out
    popped, expanded = shader_walk(nodes)
    order = complete_order(nodes)
    assert len(order) == len(nodes)
    # what the loop pops is the list with the subtrees of dropped pushes left out, in the same order
    listed = [rec[0] for rec in order]
    it = iter(listed)
    assert all(any(i == j for j in it) for i in popped), "the loop's pops are not a subsequence of the list"
    for p, (i, level, below, skip) in enumerate(order):
        nd = nodes[i]
        out[p]["bmin"], out[p]["bmax"], out[p]["first"], out[p]["skip"] = nd["boundsMin"], nd["boundsMax"], nd["leftFirst"], skip
        if nd["count"] > 0:
            out[p]["count"], out[p]["inst0"] = nd["count"], idx[nd["leftFirst"]]
        else:
            out[p]["count"] = -1 if i in expanded else 0
    return out


def tree_stats(nodes, left_add=0, right_add=1):
    """(depth, the most stack entries below any node, internal nodes that cannot push: below + 2 > 64)."""
    order = complete_order(nodes, left_add, right_add)
    cut = sum(1 for i, level, below, skip in order if nodes[i]["count"] < 0 and below + 2 > STACK)
    return max(r[1] for r in order), max(r[2] for r in order), cut


def cut_by_rule(nodes, left_add=0, right_add=1):
    """The internal nodes the `below + 2 <= 64` rule of rz_tlas_device.hip lets expand, with the given hand-down."""
    return {i for i, level, below, skip in complete_order(nodes, left_add, right_add) if nodes[i]["count"] < 0 and below + 2 <= STACK}


def balanced_tlas(boxes):
    """A hand-built TLAS over the same one-instance leaves (BVH_NODE records: boundsMin / boundsMax of instance i), halved by
    index whatever the geometry: depth ceil(log2 n) + 1, children adjacent as RayZen allocates them."""
    n = len(boxes)
    nodes, idx = np.zeros(2 * n - 1, S.BVH_NODE), np.zeros(n, I32)
    used, leaves = [1], [0]

    def fill(at, lo, hi):
        nodes[at]["boundsMin"] = boxes["boundsMin"][lo:hi].min(0)
        nodes[at]["boundsMax"] = boxes["boundsMax"][lo:hi].max(0)
        if hi - lo == 1:
            nodes[at]["leftFirst"], nodes[at]["count"] = leaves[0], 1
            idx[leaves[0]] = lo
            leaves[0] += 1
            return
        L = used[0]
        used[0] += 2
        nodes[at]["leftFirst"], nodes[at]["count"] = L, -1
        mid = (lo + hi) // 2
        fill(L, lo, mid)
        fill(L + 1, mid, hi)

    fill(0, 0, n)
    return nodes, idx

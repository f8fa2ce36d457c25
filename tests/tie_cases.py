"""Scenes and rays on which the ORDER of a closest-hit query decides its answer: coincident geometry, so that two or more
triangles are met at the same t and the strict `t < tHit` rule keeps whichever was visited first; rays through shared vertices
and edges; rays lying in box planes (0 * inf = NaN in the slab test); zero-thickness boxes.  Shared by tests/test_tie_cases.py
(the oracle alone: are the inputs sharp?) and tests/test_ties_gpu.py (the kernels against the oracle, bit for bit).

Winner tags: every triangle of every mesh carries its own materialIndex, and the material array has one entry per triangle --
the reference's material 0 (or its glass, or its mirror) with an albedo of its own.  The `material` of a hit and the colour of a
pixel then name the winning triangle.

All coordinates are dyadic, so that the ties are exact."""
import numpy as np

from oracle import rzo
from rayzen_amd import scene as S

F32 = np.float32
SHEET_Z = -1.0            # where the coincident sheets of "stack" lie
FACING_Z = 3.0            # the second stack of the render variant
GRID = np.arange(-4.5, 4.5 + 1e-9, 0.25)       # 37 values: every lattice line of the sheets, the lines between, a margin outside
OBLIQUE = np.array([-0.5, 0.25, -1.0])


# ---------------------------------------------------------------------------------------------------------------------
# meshes and tags

def sheet(lo, hi, z, other_diagonal=False, reverse=False, n=8):
    """An n x n lattice of S.make_quad cells over [lo, hi]^2 at height z (row by row, two triangles per cell)."""
    xs = np.linspace(lo, hi, n + 1)
    quads = []
    for j in range(n):
        for i in range(n):
            p = [(xs[i], xs[j], z), (xs[i + 1], xs[j], z), (xs[i + 1], xs[j + 1], z), (xs[i], xs[j + 1], z)]
            if other_diagonal:
                p = p[1:] + p[:1]
            quads.append(S.make_quad(p[0], p[1], p[2], p[3], 0))
    t = np.concatenate(quads)
    return t[::-1].copy() if reverse else t


def doubled_sheet(lo, hi, z, n=8):
    """The same lattice with every triangle present twice, next to its twin: ties INSIDE one BLAS for every ray that hits, not
    only for those through an edge."""
    t = sheet(lo, hi, z, n=n)
    return np.repeat(t, 2)


class Tags:
    """Hands out one material per triangle.  kind: 'matte' (the reference's material 0), 'glass' (its material 3) or 'mirror'
    (its material 2); a callable maps the tag to a kind."""

    def __init__(self):
        self.kinds = []

    def tag(self, tris, kind="matte"):
        t = tris.copy()
        first = len(self.kinds)
        t["materialIndex"] = np.arange(first, first + len(t), dtype=np.int32)
        self.kinds += [kind(first + k) if callable(kind) else kind for k in range(len(t))]
        return t

    def materials(self):
        ref = S.reference_materials()
        row = {"matte": ref[0], "glass": ref[3], "mirror": ref[2]}
        m = np.zeros(len(self.kinds), S.MATERIAL)
        i = np.arange(len(m), dtype=np.float64)
        albedo = np.stack([0.15 + 0.8 * ((i * c) % 1.0) for c in (0.6180339887, 0.4142135624, 0.7320508076)], 1).astype(F32)
        for k, kind in enumerate(self.kinds):
            m[k] = row[kind]
        m["albedo"] = albedo
        assert len(np.unique(albedo, axis=0)) == len(m)          # the colour names the triangle
        return m


def _translate(v):
    return S.translate(S.identity(), v)


def stack_scene(order=0, glass=False, facing=False, width=64, height=48):
    """Scene "stack": four coincident sheets at z = -1.
      mesh A  [-4, 4]^2 at z = 0             instanced twice with the same translation to z = -1
      mesh B  the same sheet baked at z = -1, the other diagonal, triangles in reverse order; identity
      mesh C  [-2, 2]^2 at z = 0             scaled (2, 2, 1), then translated to z = -1
    order 1 lists the instances the other way round (the meshes, and so the tags, stay).  glass: mesh C carries the reference's
    glass fields -- its instance is the one visited first in order 0, so there the glass wins the ties, and in order 1 an opaque
    sheet does.  facing (the render variant): a second stack at z = +3 facing the first with the camera between them, a
    doubled sheet (ties inside one BLAS) in both stacks, and every third tag a mirror, so that paths live on to a third and
    later segment -- which tie like the first."""
    tags = Tags()
    kind = (lambda k: "mirror" if k % 3 == 0 else "matte") if facing else "matte"
    A = tags.tag(sheet(-4.0, 4.0, 0.0), kind)
    B = tags.tag(sheet(-4.0, 4.0, SHEET_Z, other_diagonal=True, reverse=True), kind)
    C = tags.tag(sheet(-2.0, 2.0, 0.0), "glass" if glass else kind)
    D = tags.tag(doubled_sheet(-4.0, 4.0, 0.0), kind) if facing else None
    cam = S.Camera(position=(0.0, 0.0, 2.5 if facing else 3.0), aspect=width / height)
    sc = S.Scene(materials=tags.materials(), camera=cam)
    mA, mB, mC = sc.add_mesh(A), sc.add_mesh(B), sc.add_mesh(C)
    scaled = S.scale(S.identity(), (2.0, 2.0, 1.0))
    objects = [(mA, _translate((0.0, 0.0, SHEET_Z))), (mA, _translate((0.0, 0.0, SHEET_Z))), (mB, S.identity()),
               (mC, S.translate(scaled, (0.0, 0.0, SHEET_Z)))]
    if facing:
        mD = sc.add_mesh(D)
        objects += [(mD, _translate((0.0, 0.0, SHEET_Z))),
                    (mA, _translate((0.0, 0.0, FACING_Z))), (mB, _translate((0.0, 0.0, FACING_Z - SHEET_Z))),
                    (mC, S.translate(scaled, (0.0, 0.0, FACING_Z))), (mD, _translate((0.0, 0.0, FACING_Z)))]
    for mesh, xf in (objects[::-1] if order else objects):
        sc.add_object(mesh, xf)
    return sc.build()


def deep_scene(order=0):
    """Scene "deep": two coincident instances of one organic mesh; the second is a mesh of its own, the same triangles in
    reverse order under their own tags.  Every hit is a tie between the two, inside BLASes ten levels deep."""
    tags = Tags()
    blob = S.make_blob(8, 2.0, 0, seed=5)
    for f in ("v0", "v1", "v2"):                # vertices on a 1/64 lattice: a ray from a dyadic eye AT a vertex meets it exactly
        blob[f] = np.round(blob[f] * 64.0) / 64.0
    m1, m2 = tags.tag(blob), tags.tag(blob[::-1].copy())
    sc = S.Scene(materials=tags.materials(), camera=S.Camera(position=(0.0, 0.0, 6.0), aspect=4 / 3))
    a, b = sc.add_mesh(m1), sc.add_mesh(m2)
    for mesh in ((b, a) if order else (a, b)):
        sc.add_object(mesh)
    return sc.build()


SCENES = {
    "stack": lambda order=0: stack_scene(order),
    "glass-stack": lambda order=0: stack_scene(order, glass=True),
    "facing": lambda order=0: stack_scene(order, facing=True),
    "deep": deep_scene,
}

_scenes = {}


def scene(name, order=0):
    """The built scene (cached: the tests share it and leave it unchanged)."""
    if (name, order) not in _scenes:
        _scenes[name, order] = SCENES[name](order)
    return _scenes[name, order]


def oracle_scene(sc):
    a = sc.arrays
    return rzo.Scene(a[S.BIND_TRIANGLES], a[S.BIND_MATERIALS], a[S.BIND_LIGHTS], a[S.BIND_TLAS_NODES], a[S.BIND_TLAS_INDICES],
                     a[S.BIND_BLAS_NODES], a[S.BIND_BLAS_INDICES], a[S.BIND_INSTANCES])


def one_leaf_oracle_scene(sc):
    """The same scene with every BLAS replaced by ONE leaf that holds all its triangles in mesh order (as
    test_oracle_trace.py::test_bvh_traversal_equals_brute_force builds its flat node): the same triangles at the same t, another
    visiting order, and no inner boxes for a ray to miss."""
    a = sc.arrays
    inst = a[S.BIND_INSTANCES].copy()
    nodes, idx = a[S.BIND_BLAS_NODES], a[S.BIND_BLAS_INDICES].copy()
    starts = sorted(set(int(g) for g in inst["globalTriOffset"])) + [len(a[S.BIND_TRIANGLES])]
    roots = sorted(set(int(o) for o in inst["blasNodeOffset"]))
    flat = np.zeros(len(roots), S.BVH_NODE)
    for k in range(len(inst)):
        g, off = int(inst["globalTriOffset"][k]), int(inst["blasNodeOffset"][k])
        n = starts[starts.index(g) + 1] - g
        root = nodes[off]
        flat[roots.index(off)] = (root["boundsMin"], 0, root["boundsMax"], n)
        t0 = int(inst["blasTriOffset"][k])
        idx[t0:t0 + n] = np.arange(n, dtype=np.int32)
        inst["blasNodeOffset"][k] = roots.index(off)
    return rzo.Scene(a[S.BIND_TRIANGLES], a[S.BIND_MATERIALS], a[S.BIND_LIGHTS], a[S.BIND_TLAS_NODES], a[S.BIND_TLAS_INDICES],
                     flat, idx, inst)


# ---------------------------------------------------------------------------------------------------------------------
# closest-hit ray families: name -> (origins, directions), float32 (n, 3)

def _grid_points(step=0.25, z=SHEET_Z):
    g = GRID[::int(round(step / 0.25))]
    gx, gy = np.meshgrid(g, g)
    return np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], 1)


def _rays(o, d):
    o, d = np.broadcast_arrays(np.asarray(o, np.float64), np.asarray(d, np.float64))
    return np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)


def stack_families():
    """down     along -z from every point of the 0.25 grid: through vertices, edges and interiors; with x or y on a lattice line the
                ray lies in box planes
       oblique  the direction (-0.5, 0.25, -1), not normalised, aimed at the same grid points
       inplane  rays lying in the plane of the sheets (|a| < 1e-4 rejects every triangle; the boxes have no thickness)
       onsheet  origins exactly on a sheet, leaving to either side
       random   the control: rays with nothing special about them"""
    fam = {}
    tgt = _grid_points()
    fam["down"] = _rays(tgt + (0.0, 0.0, 2.0), (0.0, 0.0, -1.0))
    fam["oblique"] = _rays(tgt - 2.0 * OBLIQUE, OBLIQUE)
    g = GRID
    lines = [(np.stack([np.full(len(g), -5.0), g, np.full(len(g), SHEET_Z)], 1), d) for d in ((1.0, 0.0, 0.0), (1.0, 0.5, 0.0))]
    lines += [(np.stack([g, np.full(len(g), -5.0), np.full(len(g), SHEET_Z)], 1), d) for d in ((0.0, 1.0, 0.0), (1.0, 1.0, 0.0))]
    lines += [(np.stack([np.full(len(g), 5.0), g, np.full(len(g), SHEET_Z)], 1), (-1.0, -1.0, 0.0))]
    fam["inplane"] = _rays(np.concatenate([o for o, _ in lines]), np.concatenate([np.broadcast_to(d, o.shape) for o, d in lines]))
    on = _grid_points(0.5)
    dirs = ((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), tuple(OBLIQUE), tuple(-OBLIQUE))
    fam["onsheet"] = _rays(np.concatenate([on] * len(dirs)), np.concatenate([np.broadcast_to(d, on.shape) for d in dirs]))
    rng = np.random.default_rng(20)
    o = np.concatenate([rng.uniform(-5.0, 5.0, (300, 2)), rng.uniform(-0.5, 2.5, (300, 1))], 1)
    t = np.concatenate([rng.uniform(-4.5, 4.5, (300, 2)), np.full((300, 1), SHEET_Z)], 1)
    fam["random"] = _rays(o, t - o)
    return fam


def deep_families(sc):
    """vertex  rays aimed at the vertices of the mesh, from six sides
       axis    axis-parallel rays through the vertices: they lie in the planes of every box that ends at that vertex
       random  the control"""
    tris = sc.arrays[S.BIND_TRIANGLES]
    v = np.unique(np.concatenate([tris["v0"], tris["v1"], tris["v2"]]).astype(np.float64), axis=0)
    fam = {}
    eyes = ((0.0, 0.0, 8.0), (8.0, -4.0, 2.0), (-8.0, 1.0, -3.0), (2.0, 8.0, -1.0), (-3.0, -8.0, 4.0), (1.0, 2.0, -8.0))
    o = np.concatenate([np.broadcast_to(e, v.shape) for e in eyes])
    fam["vertex"] = _rays(o, np.concatenate([v] * len(eyes)) - o)
    down, along = v.copy(), v.copy()
    down[:, 2], along[:, 0] = 8.0, -8.0
    fam["axis"] = _rays(np.concatenate([down, along]), np.concatenate([np.broadcast_to((0.0, 0.0, -1.0), v.shape),
                                                                         np.broadcast_to((1.0, 0.0, 0.0), v.shape)]))
    rng = np.random.default_rng(21)
    o = rng.normal(size=(400, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * 8.0
    fam["random"] = _rays(o, -o + rng.normal(size=(400, 3)) * 1.2)
    return fam


_families = {}


def families(name):
    if name not in _families:
        _families[name] = deep_families(scene("deep")) if name == "deep" else stack_families()
    return _families[name]


# ---------------------------------------------------------------------------------------------------------------------
# shadow-ray families: name -> (origins, directions, max_dist)

def shadow_families(osc):
    """restart  origins on a sheet and 2^-11 above it: the first hit lies at t < 0.001 and the walk starts again 0.001 further on
       reach    max_dist exactly the distance to the sheets (2 along -z: `traveled >= maxDist` holds with equality), and one ulp to
                either side of it; for the oblique direction the distance is the oracle's own t of that ray"""
    fam = {}
    on = _grid_points(0.5)
    parts = []
    for lift in (0.0, 2.0 ** -11):
        for d in ((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), tuple(OBLIQUE)):
            parts.append(_rays(on + (0.0, 0.0, lift), d))
    o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    fam["restart"] = (o, d, np.full(len(o), 1e30, F32))
    tgt = _grid_points()
    o1, d1 = _rays(tgt + (0.0, 0.0, 2.0), (0.0, 0.0, -1.0))
    dist1 = np.full(len(o1), 2.0, F32)
    o2, d2 = _rays(tgt - 2.0 * OBLIQUE, OBLIQUE)
    dist2 = np.array([rzo.trace(osc, o2[i], d2[i])["t"] for i in range(len(o2))], F32)       # (1e30 on a miss: its neighbours are finite)
    o, d, dist = np.concatenate([o1, o2]), np.concatenate([d1, d2]), np.concatenate([dist1, dist2])
    below, above = np.nextafter(dist, F32(0.0)), np.nextafter(dist, F32(np.inf))
    fam["reach"] = (np.concatenate([o, o, o]), np.concatenate([d, d, d]), np.concatenate([dist, below, above]).astype(F32))
    return fam


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's answers, as arrays

def oracle_trace(osc, o, d):
    """rzo.trace for every ray: dict of arrays hit, t, point, normal, material, instance."""
    n = len(o)
    out = dict(hit=np.zeros(n, bool), t=np.zeros(n, F32), point=np.zeros((n, 3), F32), normal=np.zeros((n, 3), F32),
               material=np.zeros(n, np.int32), instance=np.zeros(n, np.int32))
    for i in range(n):
        w = rzo.trace(osc, o[i], d[i])
        for k in out:
            out[k][i] = w[k]
    return out


def oracle_shadow(osc, o, d, max_dist):
    lit, vis = np.zeros(len(o), bool), np.zeros(len(o), F32)
    for i in range(len(o)):
        lit[i], vis[i] = rzo.shadow(osc, o[i], d[i], float(max_dist[i]))
    return lit, vis


def submissions(n, seed=0):
    """The three ways a family is submitted, as index arrays into it: in order; every ray 64 times in a row (a wave holds ONE
    ray: the scalar fetches, the uniform leaf and the hand-written loop); randomly permuted (the general step)."""
    return {"in_order": np.arange(n), "wave_per_ray": np.repeat(np.arange(n), 64),
            "permuted": np.random.default_rng(seed).permutation(n)}

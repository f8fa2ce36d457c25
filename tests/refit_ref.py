"""The definition of rz_refit_geometry (include/rayzen_hip.h) restated in numpy: the third statement beside the host library
(BVH::refit) and the device kernels (rz_refit.hip).  Plus the deformations the refit tests share.

A refit keeps every leftFirst, count and the index array, and recomputes only the boxes:
  * a leaf (count > 0): computeBounds (RayZen/src/BVH.cpp:11-19) over its own slots, in order, from +-FLT_MAX:
    bmin = glm::min(bmin, glm::min(v0, glm::min(v1, v2))), bmax likewise;
  * an internal node: glm::min(left.min, right.min), glm::max(left.max, right.max) -- except that a bound which compares
    equal to the one the node holds keeps the node's bits (the sign of a zero: the builder folded the node's box in an order
    a refit cannot know, so only this makes a refit of unmoved vertices the identity on RayZen's own nodes);
  * a leaf with count == 0 is left as it is.
glm::min(a, b) = (b < a) ? b : a and glm::max(a, b) = (a < b) ? b : a -- NOT numpy's minimum / maximum, which differ on NaN
and on the sign of a zero."""
import numpy as np

FLT_MAX = np.float32(3.402823466e+38)


def gmin(a, b):
    return np.where(b < a, b, a)


def gmax(a, b):
    return np.where(a < b, b, a)


def levels(nodes):
    """Depth of every node of one BLAS (child indices relative to `nodes`), root = 0; -1 for nodes the root does not reach."""
    depth = np.full(len(nodes), -1, np.int32)
    depth[0] = 0
    frontier = np.array([0], np.int64)
    d = 0
    while frontier.size:
        inner = frontier[nodes["count"][frontier] < 0]
        left = nodes["leftFirst"][inner].astype(np.int64)
        frontier = np.concatenate([left, left + 1])
        d += 1
        depth[frontier] = d
    return depth


def refit(tris, nodes, idx):
    """The refitted copy of `nodes` for the mesh's moved triangles `tris` (original order) and its index array `idx`."""
    out = nodes.copy()
    if len(nodes) == 0:
        return out
    count, left = nodes["count"], nodes["leftFirst"].astype(np.int64)
    bmin, bmax = out["boundsMin"], out["boundsMax"]       # views into out
    leaves = np.nonzero(count > 0)[0]
    if leaves.size:
        lmin = np.full((leaves.size, 3), FLT_MAX, np.float32)
        lmax = np.full((leaves.size, 3), -FLT_MAX, np.float32)
        for s in range(int(count[leaves].max())):
            on = count[leaves] > s
            t = tris[idx[left[leaves[on]] + s]]
            lmin[on] = gmin(lmin[on], gmin(t["v0"], gmin(t["v1"], t["v2"])))
            lmax[on] = gmax(lmax[on], gmax(t["v0"], gmax(t["v1"], t["v2"])))
        bmin[leaves], bmax[leaves] = lmin, lmax
    depth = levels(nodes)
    for d in range(int(depth.max()), -1, -1):
        inner = np.nonzero((depth == d) & (count < 0))[0]
        if inner.size:
            a, b = left[inner], left[inner] + 1
            mn, mx = gmin(bmin[a], bmin[b]), gmax(bmax[a], bmax[b])
            bmin[inner] = np.where(mn == bmin[inner], bmin[inner], mn)        # equal to what the node holds: its bits stay
            bmax[inner] = np.where(mx == bmax[inner], bmax[inner], mx)
    return out


def refit_scene_nodes(arrays, tris=None):
    """Binding 7 of a scene refitted mesh by mesh (a mesh: a distinct (blasNodeOffset, blasTriOffset, globalTriOffset) among the
    instances) from `tris` (binding 0; default: the scene's own)."""
    from rayzen_amd import scene as S
    tris = arrays[S.BIND_TRIANGLES] if tris is None else tris
    nodes = arrays[S.BIND_BLAS_NODES].copy()
    idx = arrays[S.BIND_BLAS_INDICES]
    inst = arrays[S.BIND_INSTANCES]
    starts = sorted(set(int(o) for o in inst["blasNodeOffset"])) + [len(nodes)]
    seen = set()
    for i in inst:
        key = (int(i["blasNodeOffset"]), int(i["blasTriOffset"]), int(i["globalTriOffset"]))
        if key in seen:
            continue
        seen.add(key)
        end = starts[starts.index(key[0]) + 1]
        nodes[key[0]:end] = refit(tris[key[2]:], nodes[key[0]:end], idx[key[1]:])
    return nodes


# ---- the deformations -------------------------------------------------------------------------------------------------

AMPLITUDES = (0.05, 0.2, 0.5)


def wobble(tris, amplitude):
    """x += A sin(3 y), then z += A cos(2 x) with the displaced x: a pure function of the vertex, so shared vertices stay shared."""
    out = tris.copy()
    a = np.float32(amplitude)
    for f in ("v0", "v1", "v2"):
        v = out[f].copy()
        v[:, 0] = v[:, 0] + a * np.sin(np.float32(3.0) * v[:, 1])
        v[:, 2] = v[:, 2] + a * np.cos(np.float32(2.0) * v[:, 0])
        out[f] = v.astype(np.float32)
    return out


def jitter(tris, scale, seed=1234):
    """A seeded random displacement per DISTINCT vertex (shared vertices stay shared)."""
    out = tris.copy()
    v = np.concatenate([out["v0"], out["v1"], out["v2"]]).astype(np.float32)
    uniq, inv = np.unique(v.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    d = np.random.default_rng(seed).uniform(-scale, scale, (len(uniq), 3)).astype(np.float32)
    moved = (v + d[inv.reshape(-1)]).astype(np.float32)
    n = len(out)
    out["v0"], out["v1"], out["v2"] = moved[:n], moved[n:2 * n], moved[2 * n:]
    return out


def deformations(tris, radius=2.8):
    """(name, deformed triangles) for the cases every refit test uses: the three amplitudes (absolute for a mesh of radius 2.8,
    scaled with the radius of others) and one jitter."""
    k = radius / 2.8
    return [(f"wobble{a}", wobble(tris, a * k)) for a in AMPLITUDES] + [("jitter", jitter(tris, 0.05 * k))]

"""The definitions of rz_geometry_quality and rz_rebuild_geometry (include/rayzen_hip.h) restated in numpy: the third statement
beside the host library (BVH::sahCost, SceneBuffers::rebuildMesh) and the device (rz_quality.hip, the device builder).

The cost of one BLAS, over the nodes its root reaches, areas in binary64 from the binary32 bounds:
    A(n) = 2 (dx dy + dy dz + dz dx),  d = (double)max - (double)min,  A = 0 when any d fails d >= 0;
    cost = (sum of A over internal nodes + sum of A * count over leaves) / A(root),  0 when A(root) == 0.
The sum here is math.fsum's: exactly rounded, the value the other two statements are held to within 1e-9 relative."""
import math

import numpy as np

import refit_ref as R
from rayzen_amd import scene as S

REL_TOL = 1e-9      # the issue's bound: <= 2^21 non-negative terms x 2^-53 (2.3e-10) for any order, plus the roundings per term


def areas(nodes):
    d = nodes["boundsMax"].astype(np.float64) - nodes["boundsMin"].astype(np.float64)
    a = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
    return np.where((d >= 0.0).all(axis=1), a, 0.0)


def sah_cost(nodes):
    """The cost of one BLAS (child indices relative to `nodes`, root = node 0)."""
    if len(nodes) == 0:
        return 0.0
    reach = R.levels(nodes) >= 0
    a = areas(nodes)
    count = nodes["count"].astype(np.float64)
    terms = np.where(nodes["count"] < 0, a, a * count)[reach]
    return 0.0 if a[0] == 0.0 else math.fsum(terms.tolist()) / float(a[0])


def tree_shape(nodes):
    """(reachable nodes, depth in nodes, slots the leaves name) of one BLAS."""
    lv = R.levels(nodes)
    reach = lv >= 0
    leaves = reach & (nodes["count"] >= 0)
    slots = int((nodes["leftFirst"][leaves] + nodes["count"][leaves]).max()) if leaves.any() else 0
    return int(reach.sum()), int(lv.max()) + 1, slots


def meshes(arrays):
    """The meshes of a scene -- distinct (blasNodeOffset, blasTriOffset, globalTriOffset) among the instances, ascending -- each
    with its node extent [node offset, the next larger distinct node offset or the end of binding 7)."""
    inst = arrays[S.BIND_INSTANCES]
    keys = sorted(set((int(i["blasNodeOffset"]), int(i["blasTriOffset"]), int(i["globalTriOffset"])) for i in inst))
    starts = sorted(set(k[0] for k in keys)) + [len(arrays[S.BIND_BLAS_NODES])]
    return [(k, starts[starts.index(k[0]) + 1]) for k in keys]


def scene_quality(arrays, nodes=None):
    """What rz_geometry_quality reports for a scene's arrays (binding 7 = `nodes` if given), without sah_cost_built: a list of
    dicts in the call's order."""
    nodes = arrays[S.BIND_BLAS_NODES] if nodes is None else nodes
    out = []
    for key, end in meshes(arrays):
        sub = nodes[key[0]:end]
        n_nodes, depth, slots = tree_shape(sub)
        out.append(dict(node_offset=key[0], index_offset=key[1], tri_offset=key[2], n_triangles=slots, n_nodes=n_nodes, depth=depth,
                        sah_cost=sah_cost(sub)))
    return out


def close(got, want):
    """Within the bound of the definition (both zero counts)."""
    return got == want or abs(got - want) <= REL_TOL * abs(want)


def rebuilt_arrays(arrays, selected):
    """rz_rebuild_geometry's result on a scene's arrays: `selected` holds the triples (as `meshes` lists them) to rebuild.
    Meshes in ascending blasNodeOffset; a selected one contributes S.build_blas of its triangles of binding 0 (and its
    indices go to its slots of binding 8), the others their node extent verbatim, shifted; nodes in front of the first mesh
    stay; every instance's blasNodeOffset is patched; world boxes and the TLAS follow with the instances' transforms.
    Returns a new dict of arrays (bindings 0 and 8's size unchanged)."""
    from rayzen_amd import _lib
    out = {b: a.copy() for b, a in arrays.items()}
    nodes, idx, tris = arrays[S.BIND_BLAS_NODES], out[S.BIND_BLAS_INDICES], arrays[S.BIND_TRIANGLES]
    ms = meshes(arrays)
    parts = [nodes[:ms[0][0][0]]] if ms else [nodes]
    at = len(parts[0])
    moved = {}
    for key, end in ms:
        assert key[0] not in moved, "two meshes share a node extent"
        moved[key[0]] = at
        if key in selected:
            n = tree_shape(nodes[key[0]:end])[2]
            new_nodes, new_idx, _ = S.build_blas(tris[key[2]:key[2] + n])
            idx[key[1]:key[1] + n] = new_idx
            parts.append(new_nodes)
        else:
            parts.append(nodes[key[0]:end])
        at += len(parts[-1])
    out[S.BIND_BLAS_NODES] = np.concatenate(parts)
    inst = out[S.BIND_INSTANCES]
    inst["blasNodeOffset"] = [moved[int(o)] for o in inst["blasNodeOffset"]]
    roots = out[S.BIND_BLAS_NODES][inst["blasNodeOffset"]].copy()
    for i in range(len(inst)):
        xf = np.ascontiguousarray(inst["transform"][i], np.float32).reshape(16)
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        r1 = roots[i:i + 1].copy()
        _lib.host().rzh_world_bounds(r1.ctypes.data, xf.ctypes.data, mn.ctypes.data, mx.ctypes.data)
        roots[i]["boundsMin"], roots[i]["boundsMax"] = mn, mx
    out[S.BIND_TLAS_NODES], out[S.BIND_TLAS_INDICES] = S.build_tlas(roots)
    return out

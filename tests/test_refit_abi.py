"""rz_refit_geometry without a GPU: the exported symbols, the three statements of the definition against one another (the
builder, BVH::refit of the host library, refit_ref's numpy), the scene-level host partner, the oracle's frame on a refitted
tree against its frame on a rebuilt one, and the code-object metadata of the rz_refit_* kernels.  Bytes everywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import refit_ref as R
from helpers import oracle_render
from rayzen_amd import _lib
from rayzen_amd import scene as S
from test_rays_abi import _kernel_metadata

MESHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes")


def _meshes():
    return [("cube.obj", S.load_obj(os.path.join(MESHES, "cube.obj"), 0), 1.0),
            ("monkey.obj", S.load_obj(os.path.join(MESHES, "monkey.obj"), 1), 1.4),
            ("blob", S.make_blob(24, 2.8, 0), 2.8),
            ("empty", np.zeros(0, S.TRIANGLE), 1.0)]


def test_symbols_and_abi_revision():
    assert "rz_refit_geometry" in _lib.HIP_SYMBOLS and {"rzh_refit_blas", "rzh_scene_refit_mesh"} <= set(_lib.HOST_SYMBOLS)
    hip = C.CDLL(_lib.HIP_SO)          # (loading needs no GPU)
    assert hasattr(hip, "rz_refit_geometry")
    hip.rz_abi_version.restype = C.c_int
    assert hip.rz_abi_version() == 5 == _lib.ABI_VERSION
    host = _lib.host()
    assert hasattr(host, "rzh_refit_blas") and hasattr(host, "rzh_scene_refit_mesh")
    header = open(os.path.join(os.path.dirname(MESHES), "..", "..", "include", "rayzen_hip.h")).read()
    assert "#define RZ_REFIT_HOST 1u" in header and "#define RZ_ABI_VERSION 5" in header.replace("  ", " ")
    assert _lib.REFIT_HOST == 1


@pytest.mark.parametrize("which", range(4), ids=["cube", "monkey", "blob", "empty"])
def test_refit_of_an_unmodified_mesh_is_the_builders_tree(which):
    name, tris, _ = _meshes()[which]
    nodes, idx, _ = S.build_blas(tris)
    assert R.refit(tris, nodes, idx).tobytes() == nodes.tobytes(), f"{name}: refit_ref != builder"
    assert S.refit_blas(tris, nodes, idx).tobytes() == nodes.tobytes(), f"{name}: rzh_refit_blas != builder"


def _subtree_vertex_bounds(tris, nodes, idx):
    """Per node, the numpy min / max over every vertex of its subtree (an independent statement: no glm::min order)."""
    lo = np.full((len(nodes), 3), np.inf)
    hi = np.full((len(nodes), 3), -np.inf)
    for n in range(len(nodes) - 1, -1, -1):            # children are numbered after their parent
        c, l = int(nodes["count"][n]), int(nodes["leftFirst"][n])
        if c > 0:
            t = tris[idx[l:l + c]]
            v = np.concatenate([t["v0"], t["v1"], t["v2"]]).astype(np.float64)
            lo[n], hi[n] = v.min(0), v.max(0)
        elif c < 0:
            lo[n], hi[n] = np.minimum(lo[l], lo[l + 1]), np.maximum(hi[l], hi[l + 1])
    return lo, hi


@pytest.mark.parametrize("which", range(3), ids=["cube", "monkey", "blob"])
def test_refit_after_each_deformation(which):
    name, tris, radius = _meshes()[which]
    nodes, idx, _ = S.build_blas(tris)
    idx_before = idx.copy()
    for dname, moved in R.deformations(tris, radius):
        ref = R.refit(moved, nodes, idx)
        host = S.refit_blas(moved, nodes, idx)
        assert host.tobytes() == ref.tobytes(), f"{name}/{dname}: rzh_refit_blas != refit_ref"
        assert (host["leftFirst"] == nodes["leftFirst"]).all() and (host["count"] == nodes["count"]).all()
        assert (idx == idx_before).all()
        assert host.tobytes() != nodes.tobytes(), f"{name}/{dname}: the deformation moved nothing"
        lo, hi = _subtree_vertex_bounds(moved, host, idx)
        assert (host["boundsMin"] <= lo).all() and (host["boundsMax"] >= hi).all(), f"{name}/{dname}: a vertex outside its node's box"
        assert (host["boundsMin"] == lo.astype(np.float32)).all() and (host["boundsMax"] == hi.astype(np.float32)).all()   # ... and tight


def test_refit_blas_refuses_inconsistent_arrays():
    tris = S.make_cube(0)
    nodes, idx, _ = S.build_blas(tris)
    bad = nodes.copy()
    bad["leftFirst"][0] = len(nodes)            # a child outside the array
    with pytest.raises(RuntimeError):
        S.refit_blas(tris, bad, idx)
    bad_idx = idx.copy()
    bad_idx[3] = 99
    with pytest.raises(RuntimeError):
        S.refit_blas(tris, nodes, bad_idx)


def _expected_scene_arrays(before, first, moved):
    """Bindings 0, 5, 6, 7, 9 of a scene assembled from the deformed triangles and refit_ref's nodes: instances unchanged,
    world boxes of the refitted roots (main.cpp:974-993), the TLAS built over them."""
    tris = before[S.BIND_TRIANGLES].copy()
    tris[first:first + len(moved)] = moved
    nodes = R.refit_scene_nodes(before, tris)
    inst = before[S.BIND_INSTANCES]
    roots = np.zeros(len(inst), S.BVH_NODE)
    for i, it in enumerate(inst):
        r1 = nodes[int(it["blasNodeOffset"]):int(it["blasNodeOffset"]) + 1].copy()
        xf = np.ascontiguousarray(it["transform"], np.float32)
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        _lib.host().rzh_world_bounds(r1.ctypes.data, xf.ctypes.data, mn.ctypes.data, mx.ctypes.data)
        roots[i] = r1[0]
        roots[i]["boundsMin"], roots[i]["boundsMax"] = mn, mx
    tn, ti = S.build_tlas(roots)
    return {S.BIND_TRIANGLES: tris, S.BIND_BLAS_NODES: nodes, S.BIND_INSTANCES: inst.copy(), S.BIND_TLAS_NODES: tn, S.BIND_TLAS_INDICES: ti}


@pytest.mark.parametrize("name", ["instanced", "reference"])
def test_scene_refit_mesh_matches_a_scene_assembled_from_the_parts(name):
    if name == "instanced":
        sc, mesh_id, radius = S.instanced_scene(n=12), 1, 2.8        # 16 instances, one shared BLAS
        assert len(set(sc.arrays[S.BIND_INSTANCES]["blasNodeOffset"].tolist())) == 2
    else:
        sc, mesh_id, radius = S.reference_scene(), 2, 1.4            # the mirror mesh; every object its own mesh
    for case in range(4):
        before = {b: a.copy() for b, a in sc.arrays.items()}
        # the mesh's triangles where the scene keeps them: the one instance range that starts where the mesh was placed
        firsts = sorted(set(before[S.BIND_INSTANCES]["globalTriOffset"].tolist()))
        first = firsts[1] if name == "instanced" else 12 + 972       # floor (12), mesh a (972), then mesh b
        n = 12 * 12 * 12 if name == "instanced" else 972
        dname, moved = R.deformations(before[S.BIND_TRIANGLES][first:first + n], radius)[case]
        want = _expected_scene_arrays(before, first, moved)
        sc.refit_mesh(mesh_id, moved)
        for b in (S.BIND_TRIANGLES, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES, S.BIND_BLAS_NODES, S.BIND_INSTANCES):
            assert sc.arrays[b].tobytes() == want[b].tobytes(), f"{name}/{dname}: binding {b} differs"
        assert sc.arrays[S.BIND_BLAS_INDICES].tobytes() == before[S.BIND_BLAS_INDICES].tobytes()
        assert sc.arrays[S.BIND_BLAS_NODES].tobytes() != before[S.BIND_BLAS_NODES].tobytes()
        assert sc.arrays[S.BIND_TLAS_NODES].tobytes() != before[S.BIND_TLAS_NODES].tobytes()


def test_scene_refit_mesh_refuses_a_changed_count():
    sc = S.cornell_scene()
    with pytest.raises(RuntimeError):
        sc.refit_mesh(2, S.make_cube(0)[:5])
    with pytest.raises(RuntimeError):
        sc.refit_mesh(7, S.make_cube(0))


def _bunny_like(mesh, n_for_name=24):
    """bunny_scene's assembly (floor + mesh) around a given mesh."""
    s = S.Scene(camera=S.Camera(position=(0.0, 2.5, 10.0), aspect=16.0 / 9.0))
    floor = s.add_mesh(S.make_cube(4))
    bunny = s.add_mesh(mesh)
    s.add_object(floor, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.add_object(bunny, S.translate(S.identity(), (0.0, 2.0, 0.0)))
    return s.build()


@pytest.mark.parametrize("amplitude", R.AMPLITUDES)
def test_oracle_frame_on_the_refitted_tree_is_the_frame_on_a_rebuilt_tree(amplitude):
    """The experiment the feature rests on, on exactly its inputs: bunny_scene(n=24), 192 x 108, 4 spp, 4 bounces, the mesh
    displaced by x += A sin(3y), z += A cos(2x).  0 of 20 736 pixels differ.  (Closest hits are tree-independent only up to
    exact ties and box-edge rounding: asserted on these inputs, claimed for no others.)"""
    mesh = S.make_blob(24, 2.8, 0)
    base = S.bunny_scene(n=24)
    refitted = _bunny_like(mesh)
    for b in S.BINDING_DTYPES:
        assert refitted.arrays[b].tobytes() == base.arrays[b].tobytes()      # the assembly above IS bunny_scene's
    moved = R.wobble(mesh, amplitude)
    refitted.refit_mesh(1, moved)
    rebuilt = _bunny_like(moved)
    assert refitted.arrays[S.BIND_TRIANGLES].tobytes() == rebuilt.arrays[S.BIND_TRIANGLES].tobytes()
    assert refitted.arrays[S.BIND_BLAS_NODES].tobytes() != rebuilt.arrays[S.BIND_BLAS_NODES].tobytes()      # another tree ...
    a = oracle_render(refitted, 192, 108, 4, 4)
    b = oracle_render(rebuilt, 192, 108, 4, 4)
    differing = int((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).sum())
    print(f"A = {amplitude}: {differing} of {a.shape[0] * a.shape[1]} pixels differ")
    assert differing == 0                                                                                    # ... the same frame
    assert (a.view(np.uint32) != oracle_render(base, 192, 108, 4, 4).view(np.uint32)).any()                 # (and it did move)


def test_refit_kernels_spill_nothing():
    meta = _kernel_metadata(_lib.HIP_SO)
    refit = {k: v for k, v in meta.items() if "rz_refit_" in k}
    for want in ("rz_refit_tris", "rz_refit_level", "rz_refit_leaf_root", "rz_refit_roots"):
        assert any(want in k for k in refit), (want, sorted(refit))
    for name, (spill, priv) in refit.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"
    for name in meta:       # (tests/test_denoise_abi.py counts kernels by these substrings)
        if "rz_refit_" in name:
            assert not any(s in name for s in ("rz_denoise_atrous", "rz_denoise_guides", "rz_editor_kernel"))

"""BLAS quality metering and rebuild (rz_geometry_quality, rz_rebuild_geometry): the C-ABI struct and symbols, the kernels'
register budget, and the host partners rzh_blas_sah_cost and rzh_scene_rebuild_mesh against the numpy restatement of the
definitions (quality_ref.py) -- everything that can be checked without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import quality_ref as Q
import refit_ref as R
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import MESH_QUALITY
from test_rays_abi import _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = os.path.join(ROOT, "tests", "golden", "meshes")
QUALITY_HIP_SYMBOLS = ("rz_geometry_quality", "rz_rebuild_geometry")
QUALITY_HOST_SYMBOLS = ("rzh_blas_sah_cost", "rzh_scene_rebuild_mesh")


def test_quality_struct_and_symbols():
    L = _lib.hip()
    assert L.rz_sizeof(_lib.SIZEOF_MESH_QUALITY) == 64 == C.sizeof(_lib.MeshQuality) == MESH_QUALITY.itemsize
    assert _lib.SIZEOF_MESH_QUALITY == 20 and L.rz_sizeof(19) == 0                  # 19 stays unassigned (test_skin_abi.py probes it)
    want = {"node_offset": 0, "index_offset": 4, "tri_offset": 8, "node_offset_before": 12, "n_triangles": 16, "n_nodes": 20,
            "depth": 24, "flags": 28, "sah_cost": 32, "sah_cost_built": 40, "sah_cost_before": 48, "reserved": 56}
    assert [f for f, _ in _lib.MeshQuality._fields_] == list(want) == list(MESH_QUALITY.names)
    for f, off in want.items():
        assert getattr(_lib.MeshQuality, f).offset == off == MESH_QUALITY.fields[f][1], f
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5           # additive: the revision stays
    lib, host = C.CDLL(_lib.HIP_SO), C.CDLL(_lib.HOST_SO)
    for name in QUALITY_HIP_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name
    for name in QUALITY_HOST_SYMBOLS:
        assert hasattr(host, name) and name in _lib.HOST_SYMBOLS, name
    assert not any(n.startswith("rz_group_") and ("quality" in n or "rebuild" in n) for n in _lib.HIP_SYMBOLS)


def test_the_header_states_the_struct_as_the_library_compiled_it():
    text = open(os.path.join(ROOT, "include", "rayzen_hip.h")).read()
    rec = text[text.index("typedef struct rz_mesh_quality"):text.index("} rz_mesh_quality;")]
    order = ["node_offset, index_offset, tri_offset;", "node_offset_before;", "n_triangles;", "n_nodes;", "depth;", "uint32_t flags;",
             "double   sah_cost;", "double   sah_cost_built;", "double   sah_cost_before;", "double   reserved;"]
    at = [rec.index(s) for s in order]
    assert at == sorted(at)
    assert "#define RZ_QUALITY_REBUILT 1u" in text and "#define RZ_ABI_VERSION 5" in text and _lib.QUALITY_REBUILT == 1
    assert "int rz_geometry_quality(rz_ctx* ctx, rz_mesh_quality* out, size_t cap, size_t* n_meshes);" in text
    assert "int rz_rebuild_geometry(rz_ctx* ctx, double max_ratio, rz_mesh_quality* out, size_t cap, size_t* n_meshes, unsigned flags" in text


def test_quality_kernels_use_no_scratch():
    meta = _kernel_metadata(_lib.HIP_SO)
    found = {k: v for k, v in meta.items() if "rz_quality_" in k}
    assert len(found) == 2, sorted(meta)            # the partial sums, the per-view finish
    for name, (spill, priv) in found.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


def _monkey():
    return S.load_obj(os.path.join(MESHES, "monkey.obj"), 1)


BUILT = {"cube": (lambda: S.make_cube(0), 10.667), "monkey": (_monkey, 19.951), "blob8": (lambda: S.make_blob(8, 2.8, 0), 23.337),
         "blob24": (lambda: S.make_blob(24, 2.8, 0), 30.974)}


@pytest.mark.parametrize("name", sorted(BUILT))
def test_host_cost_against_the_restatement(name):
    make, built_cost = BUILT[name]
    tris = make()
    nodes, idx, depth = S.build_blas(tris)
    want = Q.sah_cost(nodes)
    assert abs(want - built_cost) < 1e-3                         # the figure the feature was argued with
    assert Q.close(S.sah_cost(nodes), want), (S.sah_cost(nodes), want)
    assert Q.tree_shape(nodes) == (len(nodes), depth, len(tris))
    last = want
    radius = 1.4 if name == "monkey" else 2.8
    for amp in R.AMPLITUDES:                                     # the cost grows with the deformation of a refitted tree
        moved = R.wobble(tris, amp * radius / 2.8) if name != "cube" else R.wobble(tris, amp)
        refitted = S.refit_blas(moved, nodes, idx)
        want = Q.sah_cost(refitted)
        assert Q.close(S.sah_cost(refitted), want), (name, amp, S.sah_cost(refitted), want)
        assert want > last, (name, amp)
        last = want


def test_host_cost_of_a_root_that_is_a_leaf_and_of_an_empty_mesh():
    quad = S.make_quad((0, 0, 0), (1, 0, 0), (1, 1, 0.5), (0, 1, 0.5), 0)
    nodes, _, depth = S.build_blas(quad)
    assert len(nodes) == 1 and nodes["count"][0] == 2 and depth == 1
    assert S.sah_cost(nodes) == 2.0 == Q.sah_cost(nodes)        # A * 2 / A, exactly
    flat = S.make_quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), 0)       # a box without volume still has an area
    nodes, _, _ = S.build_blas(flat)
    assert S.sah_cost(nodes) == 2.0 == Q.sah_cost(nodes)
    nodes, _, _ = S.build_blas(np.zeros(0, S.TRIANGLE))         # one root with an inverted box and no triangles
    assert len(nodes) == 1 and nodes["count"][0] == 0
    assert S.sah_cost(nodes) == 0.0 == Q.sah_cost(nodes)


@pytest.mark.parametrize("corner", ["nan", "1e30"])
def test_host_cost_with_a_non_finite_or_huge_corner(corner):
    tris = S.make_blob(8, 2.8, 0)
    nodes, idx, _ = S.build_blas(tris)
    moved = tris.copy()
    moved["v1"][37, 1] = np.nan if corner == "nan" else np.float32(1e30)
    refitted = S.refit_blas(moved, nodes, idx)
    got, want = S.sah_cost(refitted), Q.sah_cost(refitted)
    assert np.isfinite(want) and want >= 0.0
    assert Q.close(got, want), (got, want)


def test_host_cost_refuses_what_is_not_a_tree():
    nodes, _, _ = S.build_blas(S.make_blob(8, 2.8, 0))
    bad = nodes.copy()
    bad["leftFirst"][0] = len(nodes)                            # children outside the array
    with pytest.raises(RuntimeError):
        S.sah_cost(bad)
    loop = nodes.copy()
    loop["leftFirst"][1 if nodes["count"][1] < 0 else 2] = 0    # a child that is its own ancestor
    with pytest.raises(RuntimeError):
        S.sah_cost(loop)


# ---- Scene.rebuild_mesh, the host partner of rz_rebuild_geometry --------------------------------------------------------

GEOM = (S.BIND_TRIANGLES, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES, S.BIND_BLAS_NODES, S.BIND_BLAS_INDICES, S.BIND_INSTANCES)


def _floor_and_two_blobs():
    """Floor cube, then blob A, then blob B -- separate meshes in that node order."""
    s = S.Scene(camera=S.Camera(position=(0.0, 2.5, 12.0), aspect=16.0 / 9.0))
    blob = S.make_blob(8, 2.8, 0)
    floor, a, b = s.add_mesh(S.make_cube(4)), s.add_mesh(blob), s.add_mesh(blob.copy())
    s.add_object(floor, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.add_object(a, S.translate(S.identity(), (-3.2, 2.0, 0.0)))
    s.add_object(b, S.translate(S.identity(), (3.2, 2.0, 0.0)))
    return s.build(), blob


def test_rebuild_mesh_against_the_restatement_and_a_scene_built_from_scratch():
    sc, blob = _floor_and_two_blobs()
    moved_a, moved_b = R.wobble(blob, 0.5), R.wobble(blob, 0.05)
    sc.refit_mesh(1, moved_a)
    sc.refit_mesh(2, moved_b)
    (floor, _), (a, end_a), (b, end_b) = Q.meshes(sc.arrays)
    assert (a[0], b[0], end_a - a[0]) == (9, 9 + 443, 443)
    ratio_a = S.sah_cost(sc.arrays[S.BIND_BLAS_NODES][a[0]:end_a]) / S.sah_cost(S.build_blas(blob)[0])
    ratio_b = S.sah_cost(sc.arrays[S.BIND_BLAS_NODES][b[0]:end_b]) / S.sah_cost(S.build_blas(blob)[0])
    assert ratio_a >= 1.26 and ratio_b <= 1.14, (ratio_a, ratio_b)          # computed when the feature was argued: 1.322, 1.010
    want = Q.rebuilt_arrays(sc.arrays, {a})
    refitted_b = sc.arrays[S.BIND_BLAS_NODES][b[0]:end_b].tobytes()
    sc.rebuild_mesh(1)
    for bnd in GEOM:
        assert sc.arrays[bnd].tobytes() == want[bnd].tobytes(), bnd
    new_a, new_idx, _ = S.build_blas(moved_a)
    assert len(new_a) != 443                                                 # (489: every later mesh moves)
    got = sc.arrays[S.BIND_BLAS_NODES]
    assert got[9:9 + len(new_a)].tobytes() == new_a.tobytes()
    assert sc.arrays[S.BIND_BLAS_INDICES][12:12 + len(blob)].tobytes() == new_idx.tobytes()
    assert got[9 + len(new_a):].tobytes() == refitted_b                      # B: its refitted bytes, moved
    assert sc.arrays[S.BIND_INSTANCES]["blasNodeOffset"].tolist() == [0, 9, 9 + len(new_a)]
    # ... and with B rebuilt too, the scene is the one built from scratch on the moved triangles
    sc.rebuild_mesh(2)
    sc.rebuild_mesh(0)
    s = S.Scene(camera=sc.camera)
    floor, ma, mb = s.add_mesh(S.make_cube(4)), s.add_mesh(moved_a), s.add_mesh(moved_b)
    s.add_object(floor, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.add_object(ma, S.translate(S.identity(), (-3.2, 2.0, 0.0)))
    s.add_object(mb, S.translate(S.identity(), (3.2, 2.0, 0.0)))
    s.build()
    for bnd in GEOM:
        assert sc.arrays[bnd].tobytes() == s.arrays[bnd].tobytes(), bnd
    assert (sc.max_blas_depth, sc.tlas_depth) == (s.max_blas_depth, s.tlas_depth)
    with pytest.raises(RuntimeError):
        sc.rebuild_mesh(3)


def test_rebuild_mesh_of_a_shared_mesh_and_of_an_empty_one():
    sc = S.instanced_scene(n=8)
    blob = sc.arrays[S.BIND_TRIANGLES][12:].copy()
    sc.refit_mesh(1, R.wobble(blob, 0.5))
    want = Q.rebuilt_arrays(sc.arrays, {(9, 12, 12)})
    sc.rebuild_mesh(1)
    for bnd in GEOM:
        assert sc.arrays[bnd].tobytes() == want[bnd].tobytes(), bnd
    ref = S.reference_scene()
    before = {b: ref.arrays[b].tobytes() for b in GEOM}
    empty = [k for k, end in Q.meshes(ref.arrays) if Q.tree_shape(ref.arrays[S.BIND_BLAS_NODES][k[0]:end])[2] == 0]
    assert len(empty) == 1
    want = Q.rebuilt_arrays(ref.arrays, set(empty))
    for bnd in GEOM:                                                         # an empty mesh rebuilds to the root it had
        assert want[bnd].tobytes() == before[bnd], bnd

"""The device builders against RayZen's OWN BVH.cpp: rz_build_blas, rz_build_geometry, the TLAS rebuild of
rz_update_transforms and rz_refit_geometry's starting point equal what the reference's compiled sources computed (oracle/cppref),
byte for byte or by digest.  Reads only the fixtures tests/golden/cppref_*.npz (tests/golden/make_cppref.py wrote them where
the reference is); nothing of the reference is needed on the GPU machine."""
import os

import numpy as np
import pytest

import cppref_cases as K
from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

BLAS = K.blas_fixture_cases()
LARGE = K.load_large()
with np.load(K.fixture("tlas")) as _z:
    TLAS = {k: _z[k] for k in _z.files}


@pytest.fixture(scope="module")
def r():
    rr = Renderer(0)
    yield rr
    rr.close()


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape[0]} records, RayZen's has {want.shape[0]}"
    if got.tobytes() != want.tobytes():
        a, b = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
        first = int(np.flatnonzero((a != b).any(1))[0])
        raise AssertionError(f"{what}: first difference at record {first}: {got[first]} != RayZen's {want[first]}")


@pytest.mark.parametrize("group,name", BLAS, ids=[f"{g}-{n}" for g, n in BLAS])
def test_build_blas_equals_rayzens_build(r, group, name):
    tris, nodes, idx, oob = K.load_blas(group, name)
    dn, di, depth, ms = r.build_blas(tris)
    _same(dn, nodes, "device nodes")
    _same(di, idx, "device indices")
    assert depth == K.depth_of(nodes)


@pytest.mark.parametrize("name", [n for n, _, _ in K.LARGE])
def test_build_blas_large_by_digest(r, name):
    tin, tnodes, tidx, n, nn, depth = [str(x) for x in LARGE[f"{name}__digest"]]
    tris = dict((k, c) for k, c, _ in K.LARGE)[name]()
    assert (len(tris), K.sha(tris)) == (int(n), tin), f"{name}: the generator no longer makes the mesh the fixture was recorded for"
    dn, di, ddepth, ms = r.build_blas(tris)
    assert (len(dn), ddepth) == (int(nn), int(depth))
    assert K.sha(dn) == tnodes, f"device nodes differ from RayZen's build of {name}"
    assert K.sha(di) == tidx, f"device indices differ from RayZen's build of {name}"


GEOMETRY_SETS = [
    ["bvh_monkey", "bvh_empty", "dev_signed_zeros300", "dev_big50", "size_5", "lattice_tight_700", "bvh_cube"],
    ["huge_widest_x_120", "dev_soup2049", "zeros_pm_513", "size_1", "huge_3e38_260", "denormal_wide_300", "bvh_empty",
     "points_lines_and_triangles_300", "flat_y_huge_extent_90", "size_4097", "dev_mixed250"],
]


def _by_name(name):
    group = [g for g, n in BLAS if n == name][0]
    return K.load_blas(group, name)


@pytest.mark.parametrize("names", GEOMETRY_SETS, ids=["seven_meshes", "eleven_meshes"])
def test_build_geometry_slices_equal_rayzens_per_mesh_builds(r, names):
    """Bindings 7 / 8 hold the meshes' BLAS back to back, unmodified (main.cpp:1030-1035): mesh i is nodes[node_offset ..
    + n_nodes) and indices[index_offset .. + n_triangles)."""
    cases = [_by_name(n) for n in names]
    ranges, first = [], 0
    for tris, _, _, _ in cases:
        ranges.append((first, len(tris)))
        first += len(tris)
    built = r.build_geometry(np.concatenate([c[0] for c in cases]), ranges)
    all_nodes, all_idx = r.read_binding(S.BIND_BLAS_NODES), r.read_binding(S.BIND_BLAS_INDICES)
    assert len(all_nodes) == sum(len(c[1]) for c in cases) and len(all_idx) == first
    for name, (tris, nodes, idx, _), b in zip(names, cases, built):
        assert b["n_nodes"] == len(nodes) and b["depth"] == K.depth_of(nodes), name
        _same(all_nodes[b["node_offset"]:b["node_offset"] + b["n_nodes"]], nodes, f"{name}: nodes")
        _same(all_idx[b["index_offset"]:b["index_offset"] + len(tris)], idx, f"{name}: indices")
        assert np.asarray(b["root"]).tobytes() == nodes[0].tobytes(), name


def _check_tlas(r, name, n):
    tn, ti = r.read_binding(S.BIND_TLAS_NODES), r.read_binding(S.BIND_TLAS_INDICES)
    boxes = K.leaf_boxes(tn, ti, n)
    if f"{name}__digest" in TLAS:                        # (a case recorded by digest: cppref_cases.TLAS_BY_DIGEST)
        differs = K.tlas_matches(TLAS, name, tn, ti, roots=boxes)
        assert differs is None, f"{name}: the device's {differs} differ from RayZen's build"
        return
    roots = TLAS[f"{name}__roots"].view(S.BVH_NODE).reshape(-1)
    # first the world boxes: a difference here is a difference in the transform arithmetic, not in the TLAS builder
    diff = [i for i in range(n) if boxes[i].tobytes() != roots[i].tobytes()]
    assert not diff, (f"{name}: world boxes of instances {diff} differ from the fixture's: device "
                      f"{[(boxes[i]['boundsMin'].tolist(), boxes[i]['boundsMax'].tolist()) for i in diff[:3]]}, fixture "
                      f"{[(roots[i]['boundsMin'].tolist(), roots[i]['boundsMax'].tolist()) for i in diff[:3]]}")
    _same(tn, TLAS[f"{name}__nodes"].view(S.BVH_NODE).reshape(-1), f"{name}: TLAS nodes")
    _same(ti, TLAS[f"{name}__idx"], f"{name}: TLAS indices")


@pytest.mark.parametrize("name,n,count,frames", K.INSTANCED, ids=[c[0] for c in K.INSTANCED])
def test_update_transforms_rebuilds_rayzens_tlas(name, n, count, frames):
    sc = S.instanced_scene(n=n, count=count)
    rr = Renderer(0)
    rr.upload_scene(sc)
    for fr in frames[::-1] + frames:                     # every frame twice, the second time after another one
        rr.update_transforms(K.instanced_frame_transforms(sc, fr, count))
        _check_tlas(rr, f"{name}_frame{fr}", count + 1)
    rr.close()


def test_update_transforms_on_rayzens_own_scene():
    """RayZen's seven objects (main.cpp:360-384) with the real monkey.obj, the empty `car` mesh included."""
    sc = S.reference_scene(monkey_obj=os.path.join(K.MESHES, "monkey.obj"))
    rr = Renderer(0)
    rr.upload_scene(sc)
    rr.update_transforms(np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"], np.float32).reshape(-1, 16))
    _check_tlas(rr, "rayzen_main_scene", 7)
    rr.close()


REFIT_MESHES = ["bvh_monkey", "dev_signed_zeros300", "lattice_tight_700", "bvh_empty", "dev_mixed250", "points_lattice_400"]


def _refit_parts():
    cases = [_by_name(n) for n in REFIT_MESHES]
    objects = [(i, S.translate(S.identity(), (3.0 * i - 6.0, 0.0, -4.0))) for i in range(len(cases))]
    objects.append((0, S.rotate(S.translate(S.identity(), (0.0, 2.5, -6.0)), 0.8, (0.0, 1.0, 0.0))))      # the monkey twice
    return cases, objects


def _check_refit(rr, cases, offsets):
    all_nodes, all_idx = rr.read_binding(S.BIND_BLAS_NODES), rr.read_binding(S.BIND_BLAS_INDICES)
    for name, (tris, nodes, idx, _), (no, io) in zip(REFIT_MESHES, cases, offsets):
        _same(all_nodes[no:no + len(nodes)], nodes, f"{name}: nodes after the refit")
        _same(all_idx[io:io + len(idx)], idx, f"{name}: indices after the refit")


def test_refit_with_unchanged_vertices_keeps_rayzens_build_host_assembled_scene():
    """rz_refit_geometry's `topology kept` is RayZen's topology, and its recomputed boxes are RayZen's boxes."""
    cases, objects = _refit_parts()
    sc = S.Scene()
    ids = [sc.add_mesh(c[0]) for c in cases]
    for mi, xf in objects:
        sc.add_object(ids[mi], xf)
    sc.build(share_meshes=True)
    inst = sc.arrays[S.BIND_INSTANCES]
    offsets = [(int(inst[i]["blasNodeOffset"]), int(inst[i]["blasTriOffset"])) for i in range(len(cases))]
    rr = Renderer(0)
    rr.upload_scene(sc)
    _check_refit(rr, cases, offsets)                     # what the host assembled is RayZen's already
    rr.refit_geometry()
    _check_refit(rr, cases, offsets)
    first = int(inst[2]["globalTriOffset"])              # and a partial refit: one mesh's own triangles handed over again
    rr.refit_geometry(cases[2][0], first=first)
    _check_refit(rr, cases, offsets)
    assert rr.read_binding(S.BIND_TRIANGLES).tobytes() == sc.arrays[S.BIND_TRIANGLES].tobytes()
    rr.close()


def test_refit_with_unchanged_vertices_keeps_rayzens_build_device_built_scene():
    cases, objects = _refit_parts()
    rr = Renderer(0)
    up = rr.upload_scene_built_on_device([c[0] for c in cases], objects, S.reference_materials(), S.reference_lights())
    inst = up[S.BIND_INSTANCES]
    offsets = [(int(inst[i]["blasNodeOffset"]), int(inst[i]["blasTriOffset"])) for i in range(len(cases))]
    _check_refit(rr, cases, offsets)
    rr.refit_geometry()
    _check_refit(rr, cases, offsets)
    rr.close()

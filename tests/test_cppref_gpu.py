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
from test_blas_device_gpu import check

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
    """The blobs, and the adversarial meshes of the large-node path (cppref_cases.LARGE_ADVERSARIAL; what each is there for:
    tests/test_blas_large_cases.py).  Only where a digest differs is the host library asked for its build, to name the first
    record that differs: 9 s and 19 s of host build for the two soups of millions are not on the passing path.
    Measured on an MI355X, generator and hashing included (device time of the build alone in brackets): adv_soup_2300000
    0.43 s (34 ms), adv_soup_4200000 0.76 s (48 ms), adv_zero_4200 -- 4197 levels, one round trip each, and 8394 launches of
    the two numbering kernels -- 0.46 s (462 ms); adv_lattice_tight_9000, 1042 levels, 0.11 s."""
    tin, tnodes, tidx, n, nn, depth = [str(x) for x in LARGE[f"{name}__digest"]]
    tris = dict((k, c) for k, c, _ in K.LARGE)[name]()
    assert (len(tris), K.sha(tris)) == (int(n), tin), f"{name}: the generator no longer makes the mesh the fixture was recorded for"
    dn, di, ddepth, ms = r.build_blas(tris)
    print(f"[cppref] {name}: {len(tris)} triangles, {len(dn)} nodes, depth {ddepth}, device {ms:.1f} ms")
    same = (len(dn), K.sha(dn), K.sha(di)) == (int(nn), tnodes, tidx)
    if not same and name in [k for k, _, _ in K.LARGE_ADVERSARIAL]:
        hn, hi, _ = S.build_blas(tris)
        assert (K.sha(hn), K.sha(hi)) == (tnodes, tidx), f"{name}: the HOST library differs from RayZen's build"
        _same(dn, hn, f"{name}: device nodes")
        _same(di, hi, f"{name}: device indices")
    assert (len(dn), ddepth) == (int(nn), int(depth))
    assert K.sha(dn) == tnodes, f"device nodes differ from RayZen's build of {name}"
    assert K.sha(di) == tidx, f"device indices differ from RayZen's build of {name}"


@pytest.mark.parametrize("name", [n for n, _, slow in K.LARGE_ADVERSARIAL if not slow])
def test_build_blas_large_adversarial_equals_the_host_library(r, name):
    """Byte for byte, so that a failure names the record (the digests above only say that one differs)."""
    check(r, dict((k, c) for k, c, _ in K.LARGE_ADVERSARIAL)[name](), oracle=False)


def test_a_tree_deeper_than_4096_levels_leaves_the_context_usable(r):
    """adv_zero_4200 builds (4197 levels: the builder has no depth bound), and the build workspace serves the next mesh."""
    cases = dict((k, c) for k, c, _ in K.LARGE_ADVERSARIAL)
    nodes, idx, depth, _ = r.build_blas(cases["adv_zero_4200"]())
    assert depth == 4197 and len(nodes) == 8393
    tris, want, widx, _ = _by_name("size_4097")
    dn, di, _, _ = r.build_blas(tris)
    _same(dn, want, "size_4097 after the deep chain: nodes")
    _same(di, widx, "size_4097 after the deep chain: indices")


GEOMETRY_SETS = [
    ["bvh_monkey", "bvh_empty", "dev_signed_zeros300", "dev_big50", "size_5", "lattice_tight_700", "bvh_cube"],
    ["huge_widest_x_120", "dev_soup2049", "zeros_pm_513", "size_1", "huge_3e38_260", "denormal_wide_300", "bvh_empty",
     "points_lines_and_triangles_300", "flat_y_huge_extent_90", "size_4097", "dev_mixed250"],
    # large, small, large: the context's build workspace is used again after a bigger build
    ["adv_lattice_20000", "size_5", "adv_huge_6000", "adv_floor_pm0_10000", "bvh_empty", "adv_clusters_4096_2000", "adv_outlier_last"],
]


def _by_name(name):
    """(triangles, nodes, indices, ...): RayZen's build from the whole fixtures; of a large adversarial case the host library's,
    which test_build_blas_large_by_digest's digests and tests/test_cppref.py hold to RayZen's."""
    large = dict((k, c) for k, c, _ in K.LARGE_ADVERSARIAL)
    if name in large:
        tris = large[name]()
        nodes, idx, _ = K.host_build(name, tris)
        assert (K.sha(nodes), K.sha(idx)) == tuple(str(x) for x in LARGE[f"{name}__digest"][1:3]), name
        return tris, nodes, idx, 0
    group = [g for g, n in BLAS if n == name][0]
    return K.load_blas(group, name)


@pytest.mark.parametrize("names", GEOMETRY_SETS, ids=["seven_meshes", "eleven_meshes", "large_small_large"])
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


def test_rebuild_geometry_builds_a_large_node_from_the_device_triangles():
    """rz_rebuild_geometry hands the builder binding 0 where it is current -- on the device, after a refit -- and the mesh is
    adv_floor_pm0_10000, moved in x only (every y stays the +0 or -0 it was): three nodes of more than 4096 triangles whose y
    bounds carry the sign of a zero.  Bindings 0 and 5 to 9 equal the host partner's (Scene.refit_mesh, Scene.rebuild_mesh),
    and the mesh's slice is the host builder's BLAS of the moved triangles."""
    mesh = dict((k, c) for k, c, _ in K.LARGE_ADVERSARIAL)["adv_floor_pm0_10000"]()
    s = S.Scene()
    floor, big = s.add_mesh(S.make_cube(4)), s.add_mesh(mesh)
    s.add_object(floor, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.add_object(big, S.identity())
    sc = s.build()
    inst = sc.arrays[S.BIND_INSTANCES]
    first = int(inst[1]["globalTriOffset"])
    assert first == 12 and len(sc.arrays[S.BIND_TRIANGLES]) == 12 + len(mesh)
    moved = mesh.copy()
    for k in ("v0", "v1", "v2"):
        v = moved[k]
        v[:, 0] += np.float32(0.5) * np.sin(np.float32(2.0) * v[:, 2]).astype(np.float32)
        moved[k] = v
    y = np.stack([moved[k][:, 1] for k in ("v0", "v1", "v2")])
    assert (y == 0).all() and np.signbit(y).any() and not np.signbit(y).all()
    rr = Renderer(0)
    rr.upload_scene(sc)
    rr.refit_geometry(moved, first)
    sc.refit_mesh(big, moved)
    rec = rr.rebuild_geometry(0.0)
    assert (rec["flags"] == 1).all() and len(rec) == 2          # RZ_QUALITY_REBUILT, both meshes
    sc.rebuild_mesh(floor)
    sc.rebuild_mesh(big)
    for b in (S.BIND_BLAS_NODES, S.BIND_BLAS_INDICES, S.BIND_TRIANGLES, S.BIND_INSTANCES, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES):
        _same(rr.read_binding(b), sc.arrays[b], f"binding {b} after the rebuild")
    nodes, idx, _ = S.build_blas(moved)
    count, _ = K.node_counts_and_levels(nodes)
    assert int((count > 4096).sum()) >= 2
    o, t = int(rec["node_offset"][1]), int(rec["index_offset"][1])
    _same(rr.read_binding(S.BIND_BLAS_NODES)[o:o + len(nodes)], nodes, "the mesh's nodes")
    _same(rr.read_binding(S.BIND_BLAS_INDICES)[t:t + len(idx)], idx, "the mesh's indices")
    rr.close()

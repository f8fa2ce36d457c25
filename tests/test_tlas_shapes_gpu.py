"""The device TLAS rebuild (rz_tlas_device.hip: rz_tlas_refit) on the shapes of tests/tlas_shapes.py: chains deeper than
the shader's stack[64], equal centres, chosen root partitions on both partition paths, lattices, signed zeros, 3 000 random.

What it writes is read back whole -- bindings 9 / 10 / 11 and, through rz_debug_read_layout's view 2, the TlasDfs list every
traversal walks -- and held, byte for byte, to the host's SceneBuffers::updateDynamic, to RayZen's own BVH.cpp (the fixture),
to a FRESH context that was handed the read-back bindings (its list comes from the host routine tlas_pop_order) and to the
restatement of the shader's loop in tlas_shapes.py (a real stack of 64).  Rays and a counted frame then go through the list
and equal the oracle bit for bit, tallies included.  The same after the calls that rebuild the TLAS from the transforms the
device kept (refit, rebuild, pose), and going from a deep tree to a shallow one and back.

All 64 bytes of a record are compared: both routes zero the six pad words.
"""
import numpy as np
import pytest

import cppref_cases as K
import tlas_shapes as T
from helpers import oracle_frame, oracle_scene
from oracle import rzo
from rayzen_amd import scene as S
from rayzen_amd.renderer import RayZenError, Renderer, frame_params
from test_cppref_gpu import _check_tlas
from test_rays_gpu import _assert_trace_matches_oracle, _bits

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 64, 36, 2, 3
TLAS_BINDINGS = (S.BIND_INSTANCES, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES)
ALL_BINDINGS = tuple(S.BINDING_DTYPES)
GEOM = (S.BIND_TRIANGLES, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES, S.BIND_BLAS_NODES, S.BIND_BLAS_INDICES, S.BIND_INSTANCES)


class Arrays:
    """What helpers.oracle_scene / oracle_frame need of a scene: the eight arrays, a camera, the lights."""

    def __init__(self, arrays, camera):
        self.arrays, self.camera, self.lights = arrays, camera, arrays[S.BIND_LIGHTS]


def read_all(r):
    return {b: r.read_binding(b) for b in ALL_BINDINGS}


def fresh_context(arrays):
    f = Renderer(0)
    for b in ALL_BINDINGS:
        f.upload(b, arrays[b])
    return f


def same_binding(b, got, want, what):
    """Byte for byte.  One allowance, in binding 9 alone: where the host's inverseTransform holds a NaN the device's must hold
    a NaN, whichever -- glm::inverse of a chain's scales of 0.2 2^45 and more multiplies 0 by an overflowed cofactor, and the
    sign of a NaN that an operation makes or hands on is the processor's (measured on chain_right_100: 880 NaN words on either
    side, 0x7fc00000 and 0xffc00000 on both, not in the same places; every other word equal); every other word of the
    record, and every record without a NaN, is compared as bytes."""
    assert got.shape == want.shape, (what, b)
    if b == S.BIND_INSTANCES:
        hn = np.isnan(want["inverseTransform"])
        if hn.any():
            assert (np.isnan(got["inverseTransform"]) == hn).all(), f"{what}: binding 9: NaNs of inverseTransform in other places"
            got, want = got.copy(), want.copy()
            got["inverseTransform"][hn] = want["inverseTransform"][hn] = 0.0
    assert got.tobytes() == want.tobytes(), f"{what}: binding {b} differs from the host library's"


def dfs_of(r):
    return r.debug_read_layout(2).view(T.TLAS_DFS)


def same_records(got, want, what):
    assert got.shape == want.shape, f"{what}: {len(got)} records, expected {len(want)}"
    if got.tobytes() != want.tobytes():
        a, b = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
        first = int(np.flatnonzero((a != b).any(1))[0])
        raise AssertionError(f"{what}: first difference at position {first}: {got[first]} != {want[first]}")


def max_dist(n):
    """Shadow-ray ranges: unbounded for the even rays, 0.75 2^(i mod 40) for the odd ones."""
    i = np.arange(n)
    return np.where(i % 2 == 0, np.float32(1e30), (0.75 * 2.0 ** (i % 40)).astype(np.float32)).astype(np.float32)


def check_list(r, arrays, fresh, what):
    got = dfs_of(r)
    same_records(got, dfs_of(fresh), f"{what}: device-built list vs the fresh context's (tlas_pop_order)")
    same_records(got, T.pop_order(arrays[S.BIND_TLAS_NODES], arrays[S.BIND_TLAS_INDICES]), f"{what}: device-built list vs the restatement")


def check_rays(r, arrays, camera, sh, fresh, what):
    osc = oracle_scene(Arrays(arrays, camera))
    o, d = sh.origins, sh.dirs
    h = r.trace_rays(o, d)
    _assert_trace_matches_oracle(osc, o, d, h)
    hf = fresh.trace_rays(o, d)
    for k in h:
        assert h[k].tobytes() == hf[k].tobytes(), f"{what}: rz_trace_rays `{k}` differs from the fresh context's"
    md = max_dist(len(o))
    lit, vis = r.shadow_rays(o, d, md)
    bad = []
    for i in range(len(o)):
        wl, wv = rzo.shadow(osc, o[i], d[i], float(md[i]))
        if wl != bool(lit[i]) or _bits([wv])[0] != _bits(vis[i:i + 1])[0]:
            bad.append((i, wl, wv, lit[i], vis[i]))
    assert not bad, f"{what}: {len(bad)} of {len(o)} shadow rays differ from rzo.shadow; first: {bad[0]}"
    lf, vf = fresh.shadow_rays(o, d, md)
    assert lit.tobytes() == lf.tobytes() and vis.tobytes() == vf.tobytes(), f"{what}: rz_shadow_rays differs from the fresh context's"
    return h


def counted_frame(r, camera, n_lights):
    r.set_frame(frame_params(camera, W, H, n_lights, BOUNCES, SPP))
    counters = r.render_counted()
    return r.read_accum(), counters


# ---- test A: rz_update_transforms --------------------------------------------------------------------------------------------------

class Updated:
    def __init__(self, name):
        self.name, self.sh = name, T.get(name)
        self.host, ids = self.sh.scene()
        self.r = Renderer(0)
        self.r.upload_scene(self.host)                           # every instance at identity
        self.r.update_transforms(self.sh.transforms)
        T.set_transforms(self.host, ids, self.sh.transforms)     # the host's updateDynamic: the expected arrays
        self.arrays = read_all(self.r)
        self.fresh = fresh_context(self.arrays)

    def close(self):
        self.r.close()
        self.fresh.close()


@pytest.fixture(scope="module", params=T.NAMES)
def up(request):
    u = Updated(request.param)
    yield u
    u.close()


def test_update_transforms_bindings_equal_the_hosts_and_rayzens(up):
    for b in TLAS_BINDINGS:
        same_binding(b, up.arrays[b], up.host.arrays[b], up.name)
    assert np.isnan(up.host.arrays[S.BIND_INSTANCES]["inverseTransform"]).any() == (up.name in T.CHAINS)
    _check_tlas(up.r, K.shape_case(up.name), up.sh.n)


def test_update_transforms_list_equals_the_host_routines_and_the_restatement(up):
    check_list(up.r, up.arrays, up.fresh, up.name)
    assert len(dfs_of(up.r)) == 2 * up.sh.n - 1


def test_update_transforms_rays_equal_the_oracle_and_the_fresh_context(up):
    h = check_rays(up.r, up.arrays, up.sh.camera, up.sh, up.fresh, up.name)
    assert (h["instance"][:up.sh.n] >= 0).any()


def test_update_transforms_frame_and_tallies_equal_the_oracle(up):
    """A wrong `skip` that costs visits but no hit shows only in the tallies."""
    g, gc = counted_frame(up.r, up.sh.camera, len(up.host.lights))
    o, oc = rzo.render(oracle_scene(up.host), oracle_frame(up.host, W, H, SPP, BOUNCES), nthreads=8, want_counters=True)
    assert g.shape == o.shape and (g.view(np.uint32) == o.view(np.uint32)).all(), up.name
    for k in ("tlas_nodes", "tlas_leaf_indices", "instances", "blas_nodes", "triangles"):
        assert gc[k] == oc[k], (up.name, k)
    f, fc = counted_frame(up.fresh, up.sh.camera, len(up.host.lights))
    assert g.tobytes() == f.tobytes() and gc == fc, up.name


@pytest.mark.parametrize("name", T.CHAINS)
def test_present_with_the_depth_of_a_chain(name):
    """rz_present's box overlays walk the node array with a stack the context sizes by the depth the device kernel reported."""
    u = Updated(name)
    try:
        for r in (u.r, u.fresh):
            r.render_scene(u.host, W, H, 1, 2)
        for kw in (dict(show_bvh=True, bvh_mode=0), dict(show_bvh=True, bvh_mode=1, selected_blas=1, selected_tri=3)):
            rgb, rgba8 = u.r.present(**kw)
            frgb, frgba8 = u.fresh.present(**kw)
            assert rgb.tobytes() == frgb.tobytes() and rgba8.tobytes() == frgba8.tobytes(), (name, kw)
    finally:
        u.close()


def test_the_hook_reports_sizes_and_errors():
    u = Updated("identical_65")
    try:
        L, c = u.r._L, u.r._c
        import ctypes as C
        need = C.c_size_t(0)
        assert L.rz_debug_read_layout(c, 2, None, 0, C.byref(need)) == 0 and need.value == 64 * (2 * 65 - 1)
        buf = np.zeros(need.value, np.uint8)
        assert L.rz_debug_read_layout(c, 2, buf.ctypes.data, need.value - 1, C.byref(need)) == -7       # RZ_ERR_BUFFER_SIZE
        assert not buf.any()
        assert L.rz_debug_read_layout(c, 3, None, 0, C.byref(need)) == -1 and L.rz_debug_read_layout(c, -1, None, 0, C.byref(need)) == -1
        assert L.rz_debug_read_layout(c, 2, buf.ctypes.data, buf.nbytes, None) == 0 and buf.tobytes() == dfs_of(u.r).tobytes()
        with pytest.raises(RayZenError):
            u.r.debug_read_layout(3)
    finally:
        u.close()


# ---- test B: the calls that rebuild from the transforms the device kept ---------------------------------------------------------------

NULLPTR_SHAPES = ("chain_right_100", T.pattern_name(200, "alternate"), "identical_130", "random_3000")


def _cube_range(arrays):
    """(first triangle, count) of the matte cube's mesh: instance 1 uses it (tlas_shapes.Shape.scene)."""
    first = int(arrays[S.BIND_INSTANCES]["globalTriOffset"][1])
    return first, 12


def _refit_unchanged(u):
    u.r.refit_geometry()


def _refit_scaled(u):
    first, n = _cube_range(u.arrays)
    moved = u.arrays[S.BIND_TRIANGLES][first:first + n].copy()
    for k in ("v0", "v1", "v2"):
        moved[k] = moved[k] * np.float32(1.5)                    # about the cube's centre, the origin
    u.r.refit_geometry(moved, first=first)
    u.host.refit_mesh(0, moved)                                  # the host partner, transforms in force
    got = read_all(u.r)
    for b in GEOM:
        same_binding(b, got[b], u.host.arrays[b], f"{u.name} after the scaled refit")
    assert got[S.BIND_TLAS_NODES].tobytes() != u.arrays[S.BIND_TLAS_NODES].tobytes()        # world boxes changed


def _rebuild(u):
    q = u.r.rebuild_geometry(max_ratio=0.0)
    assert len(q) == 2


def _pose(u):
    first, n = _cube_range(u.arrays)
    skin = np.zeros(n, S.SKIN_TRIANGLE)
    skin["weights"][:, :, 0] = 1.0
    rig = u.r.skin_create(first, n, skin, 1)                     # rest pose: binding 0 as it stands
    u.r.skin_pose(rig, np.stack([S.identity()]))


@pytest.mark.parametrize("op", [_refit_unchanged, _refit_scaled, _rebuild, _pose], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("name", NULLPTR_SHAPES)
def test_rebuilds_from_the_kept_transforms(name, op):
    u = Updated(name)
    after = None
    try:
        op(u)
        arrays = read_all(u.r)
        after = fresh_context(arrays)
        what = f"{name} after {op.__name__.strip('_')}"
        if op is not _refit_scaled:                              # nothing moved: the TLAS is the one rz_update_transforms built
            for b in TLAS_BINDINGS:
                assert arrays[b].tobytes() == u.arrays[b].tobytes(), f"{what}: binding {b} changed"
        for b in ALL_BINDINGS:
            assert after.read_binding(b).tobytes() == arrays[b].tobytes(), (what, b)
        check_list(u.r, arrays, after, what)
        check_rays(u.r, arrays, u.sh.camera, u.sh, after, what)
    finally:
        u.close()
        if after is not None:
            after.close()


# ---- test C: a deep tree, a shallow one, the deep one again ------------------------------------------------------------------------------

def test_back_and_forth_between_a_chain_and_a_shallow_tree():
    """Level lists and scratch of a 100-level build must not leak into the 10-level build that follows, nor the other way."""
    chain, rnd = T.get("chain_right_100"), T.get("random_3000")
    sc, ids = chain.scene()
    r = Renderer(0)
    r.upload_scene(sc)
    lists = []
    try:
        for step, xf in enumerate((chain.transforms, rnd.transforms[:100], chain.transforms)):
            r.update_transforms(xf)
            T.set_transforms(sc, ids, xf)
            arrays = read_all(r)
            for b in TLAS_BINDINGS:
                same_binding(b, arrays[b], sc.arrays[b], f"step {step}")
            f = fresh_context(arrays)
            try:
                check_list(r, arrays, f, f"step {step}")
            finally:
                f.close()
            lists.append(dfs_of(r).copy())
        assert lists[0].tobytes() == lists[2].tobytes() and int((lists[0]["count"] == 0).sum()) == 36
        assert int((lists[1]["count"] == 0).sum()) == 0
    finally:
        r.close()

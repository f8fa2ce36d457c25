"""Closest-hit tie-breaking on the GPU, on coincident geometry (tests/tie_cases.py; tests/test_tie_cases.py shows with the oracle
alone that on these inputs the visiting order decides the answer).  rz_trace.h restates the reference's strict `t < tHit` rule and
its `tmin > tHit` cull once per walk -- the general leaf loop, the uniform-leaf scalar path, the take-right / take-left decisions
of the general step, of the uniform step and of the hand-written loop, pop_entry, the TLAS walks of trace_closest and
trace_spread, and all of it again in pool_trace.  Here every one of them meets ties: rz_trace_rays and rz_shadow_rays against
the oracle's one-ray functions and rendered frames and tallies against the oracle's, bit for bit, no ray and no pixel left out.
A walk cut short at its backstop fails the call that made it (rz_trace_rays / rz_shadow_rays) or the rz_sync after the frame."""
import numpy as np
import pytest

import tie_cases as T
from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer
from helpers import BACKENDS, hip_render, mismatch_report, oracle_render

pytestmark = pytest.mark.gpu

RZ_FLAG_HOST_RELAYOUT = 4
F32 = np.float32
W, H, BOUNCES = 64, 48, 6


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# references: computed once, shared, never written to

_refs = {}


def _frozen(d):
    for a in d.values() if isinstance(d, dict) else d:
        a.setflags(write=False)
    return d


def trace_reference(name, order, fam):
    k = ("trace", name, order, fam)
    if k not in _refs:
        o, d = T.families(name)[fam]
        _refs[k] = _frozen(T.oracle_trace(T.oracle_scene(T.scene(name, order)), o, d))
    return _refs[k]


def shadow_case(name, order, fam):
    """(origins, directions, max_dist, the oracle's lit, the oracle's visibility)"""
    k = ("shadow", name, order, fam)
    if k not in _refs:
        osc = T.oracle_scene(T.scene(name, order))
        o, d, md = T.shadow_families(osc)[fam]
        _refs[k] = _frozen((o, d, md) + T.oracle_shadow(osc, o, d, md))
    return _refs[k]


def frame_reference(name, order, spp, width=W, height=H):
    k = ("frame", name, order, spp, width, height)
    if k not in _refs:
        img, cnt = oracle_render(_sized(name, order, width, height), width, height, spp, BOUNCES, nthreads=16, want_counters=True)
        img.setflags(write=False)
        _refs[k] = (img, cnt)
    return _refs[k]


def _sized(name, order, width, height):
    sc = T.scene(name, order)
    assert abs(sc.camera.aspect - width / height) < 1e-6
    return sc


@pytest.fixture(scope="module")
def renderers():
    """One context per (scene, instance order, flags), shared by the ray tests of this module."""
    made = {}

    def get(name, order, flags=0):
        if (name, order, flags) not in made:
            r = Renderer(0, flags)
            r.upload_scene(T.scene(name, order))
            made[name, order, flags] = r
        return made[name, order, flags]

    yield get
    for r in made.values():
        r.close()


# ---------------------------------------------------------------------------------------------------------------------
# rz_trace_rays

def assert_hits_match(sc, ref, sel, h, what):
    """Every field of every ray against rzo.trace (the rays of the family at `sel`), and the returned ids against the scene's
    arrays: prim is a triangle of binding 0 that carries the winning tag, triangle its index inside the instance's mesh."""
    hit = ref["hit"][sel]
    tris, inst = sc.arrays[S.BIND_TRIANGLES], sc.arrays[S.BIND_INSTANCES]
    ok = np.where(hit, h["instance"] == ref["instance"][sel], h["instance"] == -1)
    ok &= np.where(hit, h["material"] == ref["material"][sel], h["material"] == -1)
    ok &= _bits(h["t"]) == np.where(hit, _bits(ref["t"][sel]), _bits(F32(1e30)))
    ok &= (_bits(h["point"]) == np.where(hit[:, None], _bits(ref["point"][sel]), 0)).all(axis=1)
    ok &= (_bits(h["normal"]) == np.where(hit[:, None], _bits(ref["normal"][sel]), 0)).all(axis=1)
    prim = h["prim"]
    inside = (prim >= 0) & (prim < len(tris))
    tag = np.where(inside, tris["materialIndex"][np.clip(prim, 0, len(tris) - 1)], -2)
    local = prim - inst["globalTriOffset"][np.clip(h["instance"], 0, len(inst) - 1)]
    ok &= np.where(hit, inside & (tag == h["material"]) & (local == h["triangle"]), (prim == -1) & (h["triangle"] == -1))
    bad = np.nonzero(~ok)[0]
    if len(bad):
        i = int(bad[0])
        j = int(sel[i])
        pytest.fail(f"{what}: {len(bad)} of {len(sel)} rays differ from rzo.trace; first: ray {j} of the family (position {i}): "
                    f"oracle {({k: ref[k][j] for k in ref})}, HIP {({k: h[k][i] for k in h})}")


def _trace_all_ways(r, sc, name, order, fam, what=""):
    o, d = T.families(name)[fam]
    ref = trace_reference(name, order, fam)
    for how, sel in T.submissions(len(o), seed=len(fam)).items():
        for incoherent in (False, True):
            h = r.trace_rays(o[sel], d[sel], incoherent=incoherent)       # (raises if a walk was cut short at its backstop)
            assert_hits_match(sc, ref, sel, h, f"{name} order {order}, {fam}, {how}, incoherent={incoherent}{what}")


STACK_LIKE = [("stack", 0), ("stack", 1), ("glass-stack", 0), ("facing", 0), ("facing", 1)]
STACK_FAMILIES = ["down", "oblique", "inplane", "onsheet", "random"]
DEEP_FAMILIES = ["vertex", "axis", "random"]


@pytest.mark.parametrize("fam", STACK_FAMILIES)
@pytest.mark.parametrize("name,order", STACK_LIKE)
def test_trace_rays_on_coincident_sheets(name, order, fam, renderers):
    _trace_all_ways(renderers(name, order), T.scene(name, order), name, order, fam)


@pytest.mark.parametrize("fam", DEEP_FAMILIES)
@pytest.mark.parametrize("order", [0, 1])
def test_trace_rays_on_coincident_deep_meshes(order, fam, renderers):
    _trace_all_ways(renderers("deep", order), T.scene("deep", order), "deep", order, fam)


@pytest.mark.parametrize("fam", DEEP_FAMILIES)
def test_trace_rays_deep_through_the_overflow_columns(fam, monkeypatch):
    """RZ_BLAS_STACK_WINDOW=2: all but two entries of every stack live in the overflow columns, culled at pop time all the same."""
    monkeypatch.setenv("RZ_BLAS_STACK_WINDOW", "2")
    sc = T.scene("deep", 0)
    assert sc.max_blas_depth > 4
    r = Renderer(0)
    r.upload_scene(sc)
    try:
        _trace_all_ways(r, sc, "deep", 0, fam, ", stack window 2")
    finally:
        r.close()


@pytest.mark.parametrize("name", ["stack", "deep"])
def test_trace_rays_with_the_host_relayout(name, renderers):
    r = renderers(name, 0, RZ_FLAG_HOST_RELAYOUT)
    for fam in T.families(name):
        _trace_all_ways(r, T.scene(name, 0), name, 0, fam, ", host re-layout")


# ---------------------------------------------------------------------------------------------------------------------
# rz_shadow_rays

@pytest.mark.parametrize("fam", ["restart", "reach"])
@pytest.mark.parametrize("name,order", [("stack", 0), ("stack", 1), ("glass-stack", 0), ("glass-stack", 1)])
def test_shadow_rays_on_coincident_sheets(name, order, fam, renderers):
    """glass-stack: in order 0 the tie goes to the glass (the walk multiplies by 0.94 and goes on), in order 1 to an opaque sheet."""
    r = renderers(name, order)
    o, d, md, want_lit, want_vis = shadow_case(name, order, fam)
    for how, sel in T.submissions(len(o), seed=7).items():
        for incoherent in (False, True):
            lit, vis = r.shadow_rays(o[sel], d[sel], md[sel], incoherent=incoherent)
            bad = np.nonzero((lit != want_lit[sel]) | (_bits(vis) != _bits(want_vis[sel])))[0]
            if len(bad):
                i = int(bad[0])
                j = int(sel[i])
                pytest.fail(f"{name} order {order}, {fam}, {how}, incoherent={incoherent}: {len(bad)} of {len(sel)} shadow rays "
                            f"differ from rzo.shadow; first: ray {j} (origin {o[j]}, direction {d[j]}, max_dist {md[j]!r}): "
                            f"oracle {want_lit[j], want_vis[j]}, HIP {lit[i], vis[i]}")


# ---------------------------------------------------------------------------------------------------------------------
# rendered frames

def _render(sc, spp, backend=None, counted=False, width=W, height=H):
    """(image, tallies or None, kernel name); the rz_sync at the end reports a walk that was cut short at its backstop."""
    r = Renderer(0, BACKENDS[backend] if backend else 0)
    try:
        out = hip_render(sc, width, height, spp, BOUNCES, counted=counted, renderer=r)
        name = r.last_kernel_name()
        r.sync()
    finally:
        r.close()
    return (out[0], out[1], name) if counted else (out, None, name)


def assert_same_bits(gpu, ref, what):
    assert (gpu.view(np.uint32) == ref.view(np.uint32)).all(), f"{what}: " + mismatch_report(gpu, ref)


@pytest.mark.parametrize("backend", ["auto", "pixel"])
@pytest.mark.parametrize("spp", [1, 16, 64, 130])      # the group code | several pixels per wave | one batch | several batches, not a divisor
@pytest.mark.parametrize("name", ["stack", "facing", "glass-stack"])
def test_frames(name, spp, backend):
    gpu, _, _ = _render(T.scene(name), spp, backend)
    assert_same_bits(gpu, frame_reference(name, 0, spp)[0], f"{name}, {spp} spp, backend {backend}")


@pytest.mark.parametrize("name", ["stack", "facing", "glass-stack"])
def test_frames_in_the_other_instance_order(name):
    gpu, _, _ = _render(T.scene(name, 1), 16)
    assert_same_bits(gpu, frame_reference(name, 1, 16)[0], f"{name}, instance order 1, 16 spp")


def _claims(monkeypatch):
    monkeypatch.setenv("RZ_GROUPS_PER_CLAIM", "4")
    monkeypatch.setenv("RZ_CROSS_CLAIM_POOL", "1")
    monkeypatch.setenv("RZ_WPOOL_CHUNK", "64")


@pytest.mark.parametrize("spp", [16, 64])
def test_through_claims_and_pools(spp, monkeypatch):
    """The third and later segments of "facing" -- ties inside the doubled sheet's BLAS and between the instances -- traced by
    pool_trace's own copy of the walk."""
    _claims(monkeypatch)
    gpu, _, kernel = _render(T.scene("facing"), spp)
    assert kernel == "rz_render_samples+pool", kernel
    assert_same_bits(gpu, frame_reference("facing", 0, spp)[0], f"facing, {spp} spp, claims of 4 with cross-claim pools")


@pytest.mark.parametrize("claims", [True, False])
def test_glass_stack_on_claims_and_on_the_group_code(claims, monkeypatch):
    _claims(monkeypatch)
    monkeypatch.setenv("RZ_GLASS_CLAIMS", "1" if claims else "0")
    gpu, _, kernel = _render(T.scene("glass-stack"), 64)
    assert kernel == ("rz_render_samples<glass>+pool" if claims else "rz_render_samples<glass>"), kernel
    assert_same_bits(gpu, frame_reference("glass-stack", 0, 64)[0], f"glass-stack, 64 spp, RZ_GLASS_CLAIMS={int(claims)}")


# ---------------------------------------------------------------------------------------------------------------------
# counted launches: a node culled at tmin == tHit, or a leaf entered that the reference skips, moves a tally and no pixel

@pytest.mark.parametrize("spp", [16, 64])
@pytest.mark.parametrize("name", ["stack", "facing"])
def test_tallies(name, spp):
    img, cnt, _ = _render(T.scene(name), spp, counted=True)
    ref, rc = frame_reference(name, 0, spp)
    assert_same_bits(img, ref, f"{name}, counted, {spp} spp")
    assert set(cnt) == set(rc), (sorted(cnt), sorted(rc))
    for field in sorted(rc):
        assert cnt[field] == rc[field], f"{name}, {spp} spp: {field}: HIP {cnt[field]}, oracle {rc[field]}"

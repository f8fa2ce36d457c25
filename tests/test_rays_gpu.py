"""Batched ray queries (rz_trace_rays / rz_shadow_rays, rz_rays.hip) against the oracle's one-ray functions, bit for bit, and
the triangle ids they return against the scene arrays, RayZen's brute-force pick (main.cpp:515-547) and rz_present."""
import ctypes as C

import numpy as np
import pytest

from oracle import rzo
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, RAY_DTYPE, VISIBILITY_DTYPE, Renderer, frame_params, make_rays, pick_ray
from helpers import oracle_scene

pytestmark = pytest.mark.gpu

RZ_FLAG_HOST_RELAYOUT = 4
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# rays

def _instance_boxes(sc):
    """World box of every instance's BLAS root (None for an empty mesh's inverted root)."""
    inst, nodes = sc.arrays[S.BIND_INSTANCES], sc.arrays[S.BIND_BLAS_NODES]
    out = []
    for it in inst:
        root = nodes[int(it["blasNodeOffset"])]
        lo, hi = np.asarray(root["boundsMin"], np.float64), np.asarray(root["boundsMax"], np.float64)
        if np.any(lo > hi):
            out.append(None)
            continue
        m = np.asarray(it["transform"], np.float64).reshape(4, 4).T
        c = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]) @ m.T
        out.append((c[:, :3].min(0), c[:, :3].max(0)))
    return out


def _world_box(sc):
    boxes = [b for b in _instance_boxes(sc) if b is not None]
    lo, hi = np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)
    pad = 0.2 * (hi - lo) + 0.1
    return lo - pad, hi + pad


def _instance_centres(sc, with_empty=False):
    c = [None if b is None else (b[0] + b[1]) / 2 for b in _instance_boxes(sc)]
    return c if with_empty else np.array([x for x in c if x is not None])


def _random_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * rng.choice([1.0, 0.05, 7.5], size=(n, 1))         # unit and non-unit


def _axis_dirs(rng, n):
    d = np.zeros((n, 3))
    for k in range(n):
        nz = rng.integers(1, 3)                                     # one or two nonzero components: zeros elsewhere
        ax = rng.choice(3, nz, replace=False)
        d[k, ax] = rng.choice([-1.0, 1.0, -2.5, 0.3], nz)
    return d


def _random_rays(sc, r, seed, n=3000):
    """Seeded rays from outside, inside meshes, on surfaces and from the camera; axis-parallel and non-unit directions."""
    rng = np.random.default_rng(seed)
    lo, hi = _world_box(sc)
    k = n // 6
    o1 = rng.uniform(lo, hi, size=(2 * k, 3))
    d1 = np.concatenate([_random_dirs(rng, k), _axis_dirs(rng, k)])
    cam = np.asarray(sc.camera.position, np.float64)
    o2 = np.repeat(cam[None], k, axis=0)
    d2 = _random_dirs(rng, k)
    cen = _instance_centres(sc)
    o3 = cen[rng.integers(0, len(cen), k)] + rng.normal(scale=1e-3, size=(k, 3))      # starting inside a mesh
    d3 = np.concatenate([_random_dirs(rng, k - k // 4), _axis_dirs(rng, k // 4)])
    # on surfaces: where earlier rays hit, leaving in any direction (into the surface as well)
    seed_o, seed_d = np.concatenate([o1, o2]).astype(F32), np.concatenate([d1, d2]).astype(F32)
    h = r.trace_rays(seed_o, seed_d)
    pts = h["point"][h["instance"] >= 0]
    m = n - 4 * k
    o4 = pts[rng.integers(0, len(pts), m)] if len(pts) else rng.uniform(lo, hi, size=(m, 3))
    d4 = np.concatenate([_random_dirs(rng, m - m // 4), _axis_dirs(rng, m // 4)])
    o = np.concatenate([o1, o2, o3, o4]).astype(F32)
    d = np.concatenate([d1, d2, d3, d4]).astype(F32)
    return o, d


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_trace_matches_oracle(osc, o, d, h):
    bad = []
    for i in range(len(o)):
        w = rzo.trace(osc, o[i], d[i])
        if not w["hit"]:
            ok = (h["instance"][i] == -1 and h["material"][i] == -1 and h["triangle"][i] == -1 and h["prim"][i] == -1
                  and _bits(h["t"][i:i + 1])[0] == _bits([1e30])[0] and not h["point"][i].any() and not h["normal"][i].any())
        else:
            ok = (h["instance"][i] == w["instance"] and h["material"][i] == w["material"]
                  and _bits(h["t"][i:i + 1])[0] == _bits([w["t"]])[0]
                  and (_bits(h["point"][i]) == _bits(w["point"])).all() and (_bits(h["normal"][i]) == _bits(w["normal"])).all())
        if not ok:
            bad.append((i, o[i], d[i], w, {k: h[k][i] for k in h}))
    assert not bad, f"{len(bad)} of {len(o)} rays differ from rzo.trace; first: {bad[0]}"


def _normalize32(v):
    l2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    return (v / np.sqrt(l2)[..., None]).astype(F32)


def _assert_triangle_ids(sc, o, d, h, instances=None):
    """For every hit the returned triangle (binding 0, index prim) reproduces it: FS:411's normal transformed as
    trace_closest does (within 2 ulp), the ray meets that triangle where the hit point is (barycentric tolerance 1e-5), and
    prim - globalTriOffset == triangle."""
    tris = sc.arrays[S.BIND_TRIANGLES]
    inst = sc.arrays[S.BIND_INSTANCES] if instances is None else instances
    sel = np.nonzero(h["instance"] >= 0)[0]
    assert len(sel) > 0
    ii, prim = h["instance"][sel], h["prim"][sel]
    assert (prim - inst["globalTriOffset"][ii] == h["triangle"][sel]).all()
    assert ((prim >= 0) & (prim < len(tris))).all()
    t = tris[prim]
    v0, v1, v2 = (np.asarray(t[f], F32) for f in ("v0", "v1", "v2"))
    e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(F32)
    ln = _normalize32(n)
    it = np.asarray(inst["inverseTransform"][ii], F32)               # column-major: element (row r, col c) at 4c + r
    wn = np.stack([(it[:, 4 * k + 0] * ln[:, 0] + it[:, 4 * k + 1] * ln[:, 1]) + it[:, 4 * k + 2] * ln[:, 2] for k in range(3)],
                  axis=1).astype(F32)
    wn = _normalize32(wn)
    got = h["normal"][sel]
    assert (np.abs(got - wn) <= 2 * np.spacing(np.abs(wn))).all(), float(np.abs(got - wn).max())
    # the hit point lies on that triangle: the ray, taken to object space in binary64, meets it at barycentrics within 1e-5
    # of the triangle, at the returned point
    inv64 = np.asarray(inst["inverseTransform"][ii], np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    fwd64 = np.asarray(inst["transform"][ii], np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    lo = np.einsum("nij,nj->ni", inv64[:, :3, :3], o[sel].astype(np.float64)) + inv64[:, :3, 3]
    ld = np.einsum("nij,nj->ni", inv64[:, :3, :3], d[sel].astype(np.float64))
    a0, a1, a2 = v0.astype(np.float64), v1.astype(np.float64), v2.astype(np.float64)
    E1, E2 = a1 - a0, a2 - a0
    P = np.cross(ld, E2)
    det = (E1 * P).sum(1)
    s = lo - a0
    u = (s * P).sum(1) / det
    Q = np.cross(s, E1)
    v = (ld * Q).sum(1) / det
    tl = (E2 * Q).sum(1) / det
    tol = 1e-5
    assert ((u >= -tol) & (v >= -tol) & (u + v <= 1 + tol)).all(), (u.min(), v.min(), (u + v).max())
    wp = np.einsum("nij,nj->ni", fwd64[:, :3, :3], lo + ld * tl[:, None]) + fwd64[:, :3, 3]
    scale = 1.0 + np.abs(wp).max(1)
    assert (np.abs(wp - h["point"][sel]).max(1) <= 1e-4 * scale).all()


def _renderer(sc, flags=0):
    r = Renderer(0, flags)
    r.upload_scene(sc)
    return r


SCENES = {
    "cornell": lambda: S.cornell_scene(),
    "c2": lambda: S.bunny_scene(n=76, aspect=16 / 9),
    "bunny_extras": lambda: S.bunny_scene(aspect=16 / 9, extras=True),
    "instanced_shared": lambda: S.instanced_scene(n=24, count=16, share_meshes=True),
    "instanced_own": lambda: S.instanced_scene(n=24, count=16, share_meshes=False),
    "ref": lambda: S.reference_scene(include_empty=True),
    "hidden_glass": lambda: S.hidden_glass_scene(),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_trace_rays_matches_oracle_and_triangle_ids(name):
    sc = SCENES[name]()
    osc = oracle_scene(sc)
    r = _renderer(sc)
    o, d = _random_rays(sc, r, seed=sum(name.encode()))
    h = r.trace_rays(o, d)
    _assert_trace_matches_oracle(osc, o, d, h)
    _assert_triangle_ids(sc, o, d, h)
    # the lane-by-lane walk gives the same bytes
    h2 = r.trace_rays(o, d, incoherent=True)
    for k in h:
        assert (h[k].view(np.uint8) == h2[k].view(np.uint8)).all(), k
    r.close()
    # and so does the host re-layout
    r2 = _renderer(sc, RZ_FLAG_HOST_RELAYOUT)
    h3 = r2.trace_rays(o, d)
    r2.close()
    for k in h:
        assert (h[k].view(np.uint8) == h3[k].view(np.uint8)).all(), k


def test_trace_rays_after_update_transforms_c4():
    sc = S.instanced_scene(n=76, count=16)
    r = _renderer(sc)
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(t, F32).reshape(16) for t in S.instanced_transforms(7, 16)])
    r.update_transforms(xf)
    arrays = dict(sc.arrays)
    for b in (S.BIND_INSTANCES, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES):
        arrays[b] = r.read_binding(b)
    osc = rzo.Scene(arrays[S.BIND_TRIANGLES], arrays[S.BIND_MATERIALS], arrays[S.BIND_LIGHTS], arrays[S.BIND_TLAS_NODES],
                    arrays[S.BIND_TLAS_INDICES], arrays[S.BIND_BLAS_NODES], arrays[S.BIND_BLAS_INDICES], arrays[S.BIND_INSTANCES])
    o, d = _random_rays(sc, r, seed=44)
    h = r.trace_rays(o, d)
    h2 = r.trace_rays(o, d, incoherent=True)
    r.close()
    _assert_trace_matches_oracle(osc, o, d, h)
    _assert_triangle_ids(sc, o, d, h, instances=arrays[S.BIND_INSTANCES])
    for k in h:
        assert (h[k].view(np.uint8) == h2[k].view(np.uint8)).all(), k


@pytest.mark.parametrize("window", [None, "2"])
def test_trace_rays_deep_blas_with_and_without_overflow(window, monkeypatch):
    """stress_scene: a depth-21 BLAS; RZ_BLAS_STACK_WINDOW=2 sends most of every stack through the overflow columns."""
    if window:
        monkeypatch.setenv("RZ_BLAS_STACK_WINDOW", window)
    sc = _stress()
    assert sc.max_blas_depth >= 21
    r = _renderer(sc)
    o, d = _random_rays(sc, r, seed=21, n=2400)
    h = r.trace_rays(o, d)
    h2 = r.trace_rays(o, d, incoherent=True)
    r.close()
    _assert_trace_matches_oracle(oracle_scene(sc), o, d, h)
    _assert_triangle_ids(sc, o, d, h)
    for k in h:
        assert (h[k].view(np.uint8) == h2[k].view(np.uint8)).all(), k


_STRESS = []


def _stress():
    if not _STRESS:
        _STRESS.append(S.stress_scene())
    return _STRESS[0]


# ---------------------------------------------------------------------------------------------------------------------
# shadow rays

def _glass_centres(sc):
    tris, mats, inst = sc.arrays[S.BIND_TRIANGLES], sc.arrays[S.BIND_MATERIALS], sc.arrays[S.BIND_INSTANCES]
    cen = _instance_centres(sc, with_empty=True)
    out = []
    for k, it in enumerate(inst):
        g = int(it["globalTriOffset"])
        if cen[k] is not None and g < len(tris) and mats[int(tris[g]["materialIndex"])]["transparency"] > 0:
            out.append(cen[k])
    return np.array(out)


@pytest.mark.parametrize("name", ["c2g", "ref"])
def test_shadow_rays_through_glass_match_oracle(name):
    sc = S.bunny_scene(n=24, aspect=16 / 9, extras=True) if name == "c2g" else S.reference_scene(include_empty=True)
    osc = oracle_scene(sc)
    r = _renderer(sc)
    rng = np.random.default_rng(7)
    o, d = _random_rays(sc, r, seed=8, n=1800)
    glass = _glass_centres(sc)
    assert len(glass)
    lo, hi = _world_box(sc)
    og = rng.uniform(lo, hi, size=(900, 3))
    dg = glass[rng.integers(0, len(glass), 900)] + rng.normal(scale=0.3, size=(900, 3)) - og
    o = np.concatenate([o, og]).astype(F32)
    d = np.concatenate([d, dg]).astype(F32)
    finite = (np.linalg.norm(d.astype(np.float64), axis=1) * rng.uniform(0.3, 3.0, len(d))).astype(F32)
    passed_glass = 0
    for md in (finite, np.full(len(d), 1e30, F32), np.full(len(d), np.inf, F32)):
        lit, vis = r.shadow_rays(o, d, md)
        lit2, vis2 = r.shadow_rays(o, d, md, incoherent=True)
        assert (lit == lit2).all() and (_bits(vis) == _bits(vis2)).all()
        bad = []
        for i in range(len(o)):
            wl, wv = rzo.shadow(osc, o[i], d[i], float(md[i]))
            if wl != bool(lit[i]) or _bits([wv])[0] != _bits(vis[i:i + 1])[0]:
                bad.append((i, wl, wv, lit[i], vis[i]))
        assert not bad, f"{len(bad)} of {len(o)} shadow rays differ; first: {bad[0]}"
        passed_glass += int(((vis > 0) & (vis < 1)).sum())
    r.close()
    assert passed_glass > 0          # some rays went through glass


# ---------------------------------------------------------------------------------------------------------------------
# picking

def _brute_pick(sc, o, d):
    """main.cpp:515-547 in float32 numpy: every triangle of every object, object-local t, |a| < 1e-6.  Returns
    (instance, triangle, t, runner-up t, |a| of the winner) or None."""
    tris, inst, nodes = sc.arrays[S.BIND_TRIANGLES], sc.arrays[S.BIND_INSTANCES], sc.arrays[S.BIND_BLAS_NODES]
    starts = sorted(set(int(g) for g in inst["globalTriOffset"])) + [len(tris)]
    best = []
    for k, it in enumerate(inst):
        if int(nodes[int(it["blasNodeOffset"])]["count"]) == 0:
            continue                    # an empty mesh: no triangle to test (and its offset is its successor's)
        g = int(it["globalTriOffset"])
        end = starts[starts.index(g) + 1]
        T = tris[g:end]
        if len(T) == 0:
            continue
        m = np.asarray(it["inverseTransform"], F32)
        lo = np.array([(m[r] * o[0] + m[4 + r] * o[1]) + (m[8 + r] * o[2] + m[12 + r] * F32(1)) for r in range(3)], F32)
        ldv = np.array([(m[r] * d[0] + m[4 + r] * d[1]) + (m[8 + r] * d[2] + m[12 + r] * F32(0)) for r in range(3)], F32)
        ld = _normalize32(ldv[None])[0]
        v0, v1, v2 = (np.asarray(T[f], F32) for f in ("v0", "v1", "v2"))
        e1, e2 = v1 - v0, v2 - v0
        hh = np.cross(np.broadcast_to(ld, e2.shape), e2).astype(F32)
        a = (e1 * hh).sum(1, dtype=F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = F32(1) / a
            s = (lo - v0).astype(F32)
            u = f * (s * hh).sum(1, dtype=F32)
            q = np.cross(s, e1).astype(F32)
            v = f * (q * ld).sum(1, dtype=F32)
            t = f * (e2 * q).sum(1, dtype=F32)
        ok = (np.abs(a) >= 1e-6) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 1e-4)
        for j in np.nonzero(ok)[0]:
            best.append((float(t[j]), k, int(j), float(abs(a[j]))))
    if not best:
        return None
    best.sort()
    runner = best[1][0] if len(best) > 1 else np.inf
    return best[0][1], best[0][2], best[0][0], runner, best[0][3]


def _ref_scene_unscaled():
    """reference_scene with the floor's and the glass's scale replaced by identity: every transform a pure translation."""
    s = S.Scene(camera=S.Camera(position=(0.0, 0.0, 3.0), target=(0.0, 0.0, -1.0), aspect=800 / 600))
    I = S.identity()
    floor = s.add_mesh(S.make_cube(0))
    blob = lambda mat, seed: s.add_mesh(S.fit_to_box(S.make_blob(9, 1.0, mat, seed=seed), S.SUZANNE_HALF_EXTENTS))
    a, b = blob(1, 1), blob(2, 2)
    car = s.add_mesh(np.zeros(0, S.TRIANGLE))
    c, d, glass = blob(0, 3), blob(0, 4), blob(3, 5)
    s.add_object(floor, S.translate(I, (0.0, -3.0, 0.0)))
    s.add_object(a, S.translate(I, (-4.0, 0.0, 0.0)))
    s.add_object(b, S.translate(I, (4.0, 0.0, 0.0)))
    s.add_object(car, S.translate(I, (0.0, 0.0, 0.0)))
    s.add_object(c, S.translate(I, (0.0, 0.0, -4.0)))
    s.add_object(d, S.translate(I, (0.0, 0.0, 4.0)))
    s.add_object(glass, S.translate(I, (2.5, 0.8, 2.5)))
    return s.build()


@pytest.mark.parametrize("name", ["cornell", "ref_unscaled"])
def test_pick_equals_brute_force_pick(name):
    sc = S.cornell_scene() if name == "cornell" else _ref_scene_unscaled()
    r = _renderer(sc)
    W, H = 800, 600
    compared = hits = 0
    # (a grid off the screen's centre lines: a ray in the plane of a face -- the cornell camera is level with the cube's top --
    #  meets the brute-force loop's triangles on their edges, where a BVH's box test and a bare triangle loop may differ)
    for mx in np.linspace(3.3, W - 2.9, 23):
        for my in np.linspace(2.7, H - 3.1, 17):
            got = r.pick(mx, my, W, H, sc.camera)
            o, d = pick_ray(mx, my, W, H, sc.camera)
            want = _brute_pick(sc, o, d)
            if want is None:
                assert got is None, (mx, my, got)
                continue
            inst, tri, t, runner, a = want
            if runner - t <= 1e-4 or a < 1e-4:
                continue
            compared += 1
            hits += 1
            assert got == (inst, tri), (mx, my, got, want)
    r.close()
    assert compared >= 40


def test_pick_feeds_present():
    sc = S.reference_scene(include_empty=True)
    W, H = 160, 120
    r = _renderer(sc)
    r.render_scene(sc, W, H, 1, 2)
    acc = r.read_accum()
    picked = None
    for mx, my in ((400, 200), (150, 300), (650, 300), (400, 450)):
        picked = r.pick(mx, my, 800, 600, sc.camera)
        if picked is not None:
            break
    assert picked is not None
    inst, tri = picked
    kw = dict(show_bvh=True, bvh_mode=1, selected_blas=inst, selected_tri=tri)
    rgb, rgba8 = r.present(**kw)
    want_rgb, want_rgba8 = rzo.present(oracle_scene(sc), acc, sc.camera.view, sc.camera.proj, len(sc.lights), **kw)
    assert (rgb.view(np.uint32) == want_rgb.view(np.uint32)).all()
    assert (rgba8 == want_rgba8).all()
    # the selection draws a branch: the overlay differs from the frame without one
    plain, _ = r.present(show_bvh=True, bvh_mode=1, selected_blas=inst, selected_tri=-12345)
    r.close()
    assert (plain != rgb).any()


# ---------------------------------------------------------------------------------------------------------------------
# the device path, batch sizes, streams, render state, errors, speed

class Hip:
    """Device memory, streams and events through the HIP runtime librayzen_hip.so itself is linked against (ctypes), for the
    tests of the device-pointer path."""

    def __init__(self):
        _lib.hip()
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
        L = self.L = C.CDLL(path)
        vp, sz, pvp = C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)
        for name, args in (("hipMalloc", [pvp, sz]), ("hipFree", [vp]), ("hipMemcpy", [vp, vp, sz, C.c_int]),
                           ("hipMemset", [vp, C.c_int, sz]), ("hipDeviceSynchronize", []), ("hipStreamCreate", [pvp]),
                           ("hipStreamDestroy", [vp]), ("hipStreamSynchronize", [vp]), ("hipEventCreate", [pvp]),
                           ("hipEventDestroy", [vp]), ("hipEventRecord", [vp, vp]), ("hipEventSynchronize", [vp]),
                           ("hipEventElapsedTime", [C.POINTER(C.c_float), vp, vp])):
            getattr(L, name).restype, getattr(L, name).argtypes = C.c_int, args
        self.bufs = []

    def ok(self, rc):
        assert rc == 0, f"HIP error {rc}"

    def alloc(self, nbytes, fill=None):
        p = C.c_void_p()
        self.ok(self.L.hipMalloc(C.byref(p), max(int(nbytes), 16)))
        self.bufs.append(p.value)
        if fill is not None:
            self.ok(self.L.hipMemset(p.value, fill, max(int(nbytes), 16)))
        return p.value

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.ok(self.L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1))
        return p

    def download(self, p, nbytes):
        out = np.empty(int(nbytes), np.uint8)
        if nbytes:
            self.ok(self.L.hipMemcpy(out.ctypes.data, p, int(nbytes), 2))
        return out

    def stream(self):
        s = C.c_void_p()
        self.ok(self.L.hipStreamCreate(C.byref(s)))
        return s.value

    def event(self):
        e = C.c_void_p()
        self.ok(self.L.hipEventCreate(C.byref(e)))
        return e.value

    def close(self):
        self.ok(self.L.hipDeviceSynchronize())
        for p in self.bufs:
            self.L.hipFree(p)
        self.bufs = []


def _device_trace(hip, r, rays, incoherent=False):
    n = len(rays)
    d_rays, d_hits = hip.upload(rays), hip.alloc(n * 48)
    r.trace_rays_device(d_rays, d_hits, n, incoherent)
    r.sync()
    return hip.download(d_hits, n * 48).view(HIT_DTYPE)


def test_batch_sizes_and_host_device_paths_agree():
    hip = Hip()
    sc = S.bunny_scene(n=24, aspect=16 / 9)
    osc = oracle_scene(sc)
    r = _renderer(sc)
    rng = np.random.default_rng(3)
    big = 1000003
    lo, hi = _world_box(sc)
    o = rng.uniform(lo, hi, size=(big, 3)).astype(F32)
    cen = _instance_centres(sc)
    d = (cen[rng.integers(0, len(cen), big)] + rng.normal(size=(big, 3)) - o).astype(F32)
    rays = make_rays(o, d)
    whole = _device_trace(hip, r, rays)
    hw = r.trace_rays(o, d)
    for k in hw:
        assert _same_bytes(whole[k], hw[k]), k
    assert (whole["instance"] >= 0).mean() > 0.3
    for n in (0, 1, 63, 64, 65):
        part = _device_trace(hip, r, rays[:n])
        assert part.tobytes() == whole[:n].tobytes(), n
        hh = r.trace_rays(o[:n], d[:n])
        assert all(_same_bytes(hh[k], whole[:n][k]) for k in hh), n
    sub = np.concatenate([rng.integers(0, big, 1500), np.arange(big - 70, big)])
    _assert_trace_matches_oracle(osc, o[sub], d[sub], {k: whole[k][sub] for k in hw})
    # shadow: host and device paths agree
    md = np.full(big, 1e30, F32)
    lit, vis = r.shadow_rays(o, d, md)
    d_rays, d_out = hip.upload(make_rays(o, d, md)), hip.alloc(big * 8)
    r.shadow_rays_device(d_rays, d_out, big)
    r.sync()
    dv = hip.download(d_out, big * 8).view(VISIBILITY_DTYPE)
    r.close()
    hip.close()
    assert ((dv["lit"] != 0) == lit).all() and (_bits(dv["visibility"]) == _bits(vis)).all()


def test_queries_on_a_user_stream_see_the_new_transforms():
    hip = Hip()
    sc = S.instanced_scene(n=24, count=16)
    r = _renderer(sc)
    o, d = _random_rays(sc, r, seed=5, n=1200)
    before = r.trace_rays(o, d)
    rays = make_rays(o, d)
    d_rays, d_hits = hip.upload(rays), hip.alloc(len(rays) * 48)
    stream = hip.stream()
    r.set_stream(stream)
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(t, F32).reshape(16) for t in S.instanced_transforms(11, 16)])
    r.update_transforms(xf)
    r.trace_rays_device(d_rays, d_hits, len(rays))
    r.set_frame(frame_params(sc.camera, 64, 36, len(sc.lights), 2, 1))
    r.render()
    r.sync()
    got = hip.download(d_hits, len(rays) * 48).view(HIT_DTYPE)
    arrays = dict(sc.arrays)
    for b in (S.BIND_INSTANCES, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES):
        arrays[b] = r.read_binding(b)
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()
    osc = rzo.Scene(arrays[S.BIND_TRIANGLES], arrays[S.BIND_MATERIALS], arrays[S.BIND_LIGHTS], arrays[S.BIND_TLAS_NODES],
                    arrays[S.BIND_TLAS_INDICES], arrays[S.BIND_BLAS_NODES], arrays[S.BIND_BLAS_INDICES], arrays[S.BIND_INSTANCES])
    _assert_trace_matches_oracle(osc, o, d, {k: got[k] for k in before})
    assert (got["t"] != before["t"]).any()            # the scene did move


def test_queries_leave_the_render_state_alone():
    hip = Hip()
    sc = S.bunny_scene(n=76, aspect=16 / 9)
    W, H = 96, 54

    def run(with_queries):
        r = _renderer(sc)
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 4, 0))
        r.render()
        if with_queries:
            rng = np.random.default_rng(9)
            n = 1 << 20
            rays = make_rays(rng.normal(size=(n, 3)) * 4, rng.normal(size=(n, 3)))
            _device_trace(hip, r, rays)
            r.shadow_rays(rays["origin"][:4096], rays["dir"][:4096], 1e30)
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 4, 4))
        r.render()
        acc = r.read_accum()
        r.close()
        return acc

    a, b = run(False), run(True)
    hip.close()
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    r = _renderer(sc)
    rays = make_rays(np.zeros((4, 3)), np.ones((4, 3)))
    hp, op = hip.upload(rays), hip.alloc(4 * 48 + 16, fill=0x5A)
    for fn in (L.rz_trace_rays, L.rz_shadow_rays):
        assert fn(None, hp, op, 4, 0) == -1
        assert fn(r._c, None, op, 4, 0) == -1 and L.rz_last_error(r._c)
        assert fn(r._c, hp, None, 4, 0) == -1
        assert fn(r._c, hp + 4, op, 4, 0) == -1 and b"aligned" in L.rz_last_error(r._c)
        assert fn(r._c, hp, op + 8, 4, 0) == -1
        assert fn(r._c, hp, op, (1 << 31), 0) == -1
        assert fn(r._c, hp, op, 4, 0x80) == -1
        assert fn(r._c, None, None, 0, 0) == 0
        assert fn(r._c, hp, op, 0, 0) == 0
    r.sync()
    assert (hip.download(op, 4 * 48 + 16) == 0x5A).all()         # nothing was launched
    empty = Renderer(0)
    for fn in (L.rz_trace_rays, L.rz_shadow_rays):
        assert fn(empty._c, hp, op, 4, 0) == -5 and L.rz_last_error(empty._c)
    empty.close()
    r.close()
    hip.close()


def _camera_rays_tiled(cam, W, H):
    """One ray per pixel centre (FS:204-212's pinhole without jitter), ordered tile by tile (RZ_TILE_W x RZ_TILE_H = 64 rays,
    one wave's worth)."""
    ty, tx, ly, lx = np.meshgrid(np.arange((H + 7) // 8), np.arange((W + 7) // 8), np.arange(8), np.arange(8), indexing="ij")
    px, py = (tx * 8 + lx).ravel(), (ty * 8 + ly).ravel()
    keep = (px < W) & (py < H)
    px, py = px[keep], py[keep]
    ndc = np.stack([(px + 0.5) / W * 2 - 1, (py + 0.5) / H * 2 - 1, -np.ones_like(px, float), np.ones_like(px, float)], 1)
    ip = np.asarray(cam.inv_proj, np.float64).reshape(4, 4).T
    iv = np.asarray(cam.inv_view, np.float64).reshape(4, 4).T
    e = ndc @ ip.T
    e = np.stack([e[:, 0], e[:, 1], -np.ones(len(e)), np.zeros(len(e))], 1)
    d = (e @ iv.T)[:, :3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.repeat(np.asarray(cam.position, F32)[None], len(d), 0), d.astype(F32)


def test_speed_floor_coherent_c2():
    """Deliberately loose (nothing had been measured): 2 M coherent rays on C2 in under 5 ms."""
    hip = Hip()
    sc = S.bunny_scene(n=76, aspect=16 / 9)
    r = _renderer(sc)
    o, d = _camera_rays_tiled(sc.camera, 1920, 1080)
    rays = make_rays(o, d)
    n = len(rays)
    assert n >= 2_000_000
    d_rays, d_hits = hip.upload(rays), hip.alloc(n * 48)
    stream = hip.stream()
    r.set_stream(stream)
    r.trace_rays_device(d_rays, d_hits, n)          # warm-up (re-layout, first launch)
    r.sync()
    times = []
    a, b = hip.event(), hip.event()
    for _ in range(5):
        hip.ok(hip.L.hipEventRecord(a, stream))
        r.trace_rays_device(d_rays, d_hits, n)
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        times.append(ms.value)
    hits = hip.download(d_hits, n * 48).view(HIT_DTYPE)
    r.set_stream(0)
    r.close()
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    hip.L.hipStreamDestroy(stream)
    hip.close()
    assert (hits["instance"] >= 0).mean() > 0.2          # the rays did run
    assert min(times) < 5.0, times

"""A numpy restatement of rz_ambient_occlusion (include/rayzen_hip.h), step by step in binary32.

The references for the two ray queries are the CPU oracle's: rzo.trace on editor_rays(camera, W, H) for the guide (what
tests/coverage_ref.py: oracle_images does) and rzo.shadow for a sample's walk (what tests/test_rays_gpu.py holds rz_shadow_rays
to).  Everything between and after them -- the direction table, the sample rays, the pairwise sum, the gather, the modulation
and the quantisation -- is restated here with one binary32 rounding per operation, so the device is held to these bytes."""
import ctypes as C

import numpy as np

from oracle import rzo
from rayzen_amd import scene as S
from rayzen_amd.renderer import editor_rays, make_rays

F32 = np.float32
N_DIRS = 256


def oracle_scene(arrays):
    a = arrays
    return rzo.Scene(a[S.BIND_TRIANGLES], a[S.BIND_MATERIALS], a[S.BIND_LIGHTS], a[S.BIND_TLAS_NODES], a[S.BIND_TLAS_INDICES],
                     a[S.BIND_BLAS_NODES], a[S.BIND_BLAS_INDICES], a[S.BIND_INSTANCES])


# ---------------------------------------------------------------------------------------------------------------------
# the direction table

def table():
    """(P (256, 3) float32, candidates tried): Marsaglia's sphere points from an R2 lattice, the header's definition."""
    two, one, ulp = F32(2.0), F32(1.0), F32(2.0 ** -23)
    pts, k = [], 0
    while len(pts) < N_DIRS:
        k += 1
        a = ((k * 3242174889) & 0xffffffff) >> 8
        b = ((k * 2447445414) & 0xffffffff) >> 8
        x1 = F32(a) * ulp - one
        x2 = F32(b) * ulp - one
        s = x1 * x1 + x2 * x2
        if not s < one:
            continue
        q = np.sqrt(one - s)
        pts.append(((two * x1) * q, (two * x2) * q, one - two * s))
    out = np.array(pts, F32)
    assert out.dtype == F32 and out.shape == (N_DIRS, 3)
    return out, k


_table = None


def directions():
    global _table
    if _table is None:
        _table = table()[0]
    return _table


# ---------------------------------------------------------------------------------------------------------------------
# the guide

class Guide:
    """The pixel-centre hits of a frame, (h, w) images, row 0 = the bottom row: hit (bool), t, x (.., 3), n (.., 3) and the ray
    directions d (.., 3).  x, n and t of a miss are not read."""

    def __init__(self, hit, t, x, n, d):
        self.hit, self.t, self.x, self.n, self.d = hit, t, x, n, d
        self.h, self.w = hit.shape


def oracle_guide(arrays, camera, w, h):
    osc = oracle_scene(arrays)
    rays = editor_rays(camera, w, h)
    hit = np.zeros(w * h, bool)
    t = np.full(w * h, 1e30, F32)
    x = np.zeros((w * h, 3), F32)
    n = np.zeros((w * h, 3), F32)
    for k in range(w * h):
        r = rzo.trace(osc, rays["origin"][k], rays["dir"][k])
        if r["hit"]:
            hit[k], t[k], x[k], n[k] = True, r["t"], r["point"], r["normal"]
    return Guide(hit.reshape(h, w), t.reshape(h, w), x.reshape(h, w, 3), n.reshape(h, w, 3),
                 np.array(rays["dir"], F32).reshape(h, w, 3))


def guide_of_hits(hits, camera, w, h):
    """The same from rz_denoise's guides (HIT_DTYPE records, (h, w) or flat)."""
    g = np.asarray(hits).reshape(h, w)
    d = np.array(editor_rays(camera, w, h)["dir"], F32).reshape(h, w, 3)
    return Guide(g["instance"] >= 0, np.array(g["t"], F32), np.array(g["point"], F32), np.array(g["normal"], F32), d)


# ---------------------------------------------------------------------------------------------------------------------
# the sample rays and raw

def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sample_rays(g, n_samples, radius, all_directions=False):
    """The walks of a frame: (rays (H * N,) rz_ray records, walked (H, N) bool) for the H hit pixels in pixel order (row-major,
    row 0 = the bottom row), the N samples of a pixel adjacent.  A sample with !(L2 >= 1e-6f) is not walked: its ray points along
    +z from o and its answer is not read.
    all_directions: every pixel takes all 256 directions (n_samples is ignored) -- the reference of the quality measurement."""
    P = directions()
    ys, xs = np.nonzero(g.hit)
    n, x, d = g.n[ys, xs], g.x[ys, xs], g.d[ys, xs]
    flip = _dot(n, d) > F32(0.0)
    nf = np.where(flip[:, None], -n, n).astype(F32)
    o = (x + nf * F32(0.001)).astype(F32)
    if all_directions:
        idx = np.broadcast_to(np.arange(N_DIRS)[None, :], (len(ys), N_DIRS))
    else:
        c = (xs & 3) + 4 * (ys & 3)
        idx = 16 * np.arange(n_samples)[None, :] + c[:, None]
    v = (nf[:, None, :] + P[idx]).astype(F32)
    l2 = _dot(v, v)
    walked = l2 >= F32(1e-6)
    with np.errstate(invalid="ignore", divide="ignore"):
        vn = (v / np.sqrt(l2)[..., None]).astype(F32)
    vn[~walked] = (0.0, 0.0, 1.0)           # (a ray the queries can take; its answer is not read)
    origins = np.broadcast_to(o[:, None, :], vn.shape).copy()
    return make_rays(origins.reshape(-1, 3), vn.reshape(-1, 3), F32(radius)), walked


def oracle_visibility(osc, rays, walked):
    """a_i of every sample: lit ? visibility : 0 by rzo.shadow, 1 for a sample that is not walked.  (H, N) float32."""
    L = rzo.lib()
    o = np.ascontiguousarray(rays["origin"], F32)
    d = np.ascontiguousarray(rays["dir"], F32)
    md = np.asarray(rays["max_dist"], F32)
    a = np.ones(len(rays), F32)
    vis = C.c_float(0)
    po, pd, scene = o.ctypes.data, d.ctypes.data, C.byref(osc.c)
    for k in np.flatnonzero(walked.reshape(-1)):
        lit = L.rzo_shadow(scene, po + 12 * int(k), pd + 12 * int(k), C.c_float(md[k]), C.byref(vis))
        a[k] = F32(vis.value) if lit else F32(0.0)
    return a.reshape(walked.shape)


def visibility_of(records, walked):
    """The same from rz_shadow_rays' records (VISIBILITY_DTYPE, one per ray of sample_rays)."""
    r = np.asarray(records).reshape(walked.shape)
    return np.where(walked, np.where(r["lit"] != 0, r["visibility"], F32(0.0)), F32(1.0)).astype(F32)


def tree(a):
    """s[i] = s[2i] + s[2i+1], level by level, over the last axis (a power of two long)."""
    a = np.asarray(a, F32)
    while a.shape[-1] > 1:
        a = (a[..., 0::2] + a[..., 1::2]).astype(F32)
    return a[..., 0]


def raw_image(g, a):
    """raw (h, w) float32 from the (H, N) sample answers: tree(a) * (1.0f / N) on the hits, 1 on the misses."""
    raw = np.ones((g.h, g.w), F32)
    raw[g.hit] = tree(a) * (F32(1.0) / F32(a.shape[-1]))
    return raw


def oracle_raw(arrays, g, n_samples, radius):
    """(raw (h, w), a (H, N)) with the oracle's walks."""
    rays, walked = sample_rays(g, n_samples, radius)
    a = oracle_visibility(oracle_scene(arrays), rays, walked)
    return raw_image(g, a), a


# ---------------------------------------------------------------------------------------------------------------------
# the gather and the outputs

def pixel_footprint(inv_proj, height):
    """f = 2 |inv_proj[5]| / height, evaluated in binary64 and rounded to binary32."""
    return F32(2.0 * abs(float(np.asarray(inv_proj, F32).reshape(16)[5])) / float(height))


def gather(raw, hit, n, x, t, f, normal_cos=0.9, plane_tol=2.0):
    """ao (h, w) of smooth = 1: the mean of raw over the taps (X + a, Y + b), b = -2..1 outer and a = -2..1 inner, that are inside
    the image, hits and -- but for the centre -- pass the normal and the plane test of a hit p; 1 for a miss."""
    h, w = hit.shape
    raw, n, x, t = np.asarray(raw, F32), np.asarray(n, F32), np.asarray(x, F32), np.asarray(t, F32)
    nc, pt, f = F32(normal_cos), F32(plane_tol), F32(f)

    def shifted(img, a, b, fill):
        out = np.full(img.shape, fill, img.dtype)
        ys0, ys1 = max(0, -b), min(h, h - b)
        xs0, xs1 = max(0, -a), min(w, w - a)
        if ys0 < ys1 and xs0 < xs1:
            out[ys0:ys1, xs0:xs1] = img[ys0 + b:ys1 + b, xs0 + a:xs1 + a]
        return out

    tol = ((pt * t) * f).astype(F32)
    total = np.zeros((h, w), F32)
    count = np.zeros((h, w), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(-2, 2):
            for a in range(-2, 2):
                ok = shifted(hit, a, b, False) & hit
                if (a, b) != (0, 0):
                    nq, xq = shifted(n, a, b, 0), shifted(x, a, b, 0)
                    ok &= _dot(n, nq) >= nc
                    ok &= np.abs(_dot(n, (xq - x).astype(F32))) <= (tol * F32(max(abs(a), abs(b)))).astype(F32)
                total = (total + np.where(ok, shifted(raw, a, b, 0), F32(0.0))).astype(F32)
                count += ok
        ao = np.where(hit, total / np.maximum(count, 1).astype(F32), F32(1.0)).astype(F32)
    assert (count[hit] >= 1).all()
    return ao


def smooth(g, raw, inv_proj, normal_cos=0.9, plane_tol=2.0):
    return gather(raw, g.hit, g.n, g.x, g.t, pixel_footprint(inv_proj, g.h), normal_cos, plane_tol)


def modulate(ao, rgb_in=None, strength=1.0):
    """rgb32f (h, w, 3): rgb_in * m per channel with m = 1.0f - strength * (1.0f - ao); rgb_in None: (1, 1, 1)."""
    m = (F32(1.0) - F32(strength) * (F32(1.0) - np.asarray(ao, F32))).astype(F32)
    if rgb_in is None:
        return np.repeat(m[..., None], 3, -1).astype(F32)
    return (np.asarray(rgb_in, F32) * m[..., None]).astype(F32)


def quantise(rgb):
    """rgba8 (h, w, 4): rz_present's quantisation, rint(clamp(c, 0, 1) * 255), alpha 255."""
    q = np.rint(np.clip(np.asarray(rgb, F32), F32(0.0), F32(1.0)) * F32(255.0)).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:2] + (1,), 255, np.uint8)], -1)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the tests (cached: the tests share them and leave them unchanged)

CASES = {
    "reference": lambda: S.reference_scene(),
    "bunny": lambda: S.bunny_scene(n=12, aspect=4 / 3, extras=True),
    "instanced": lambda: S.instanced_scene(n=8, count=16, aspect=4 / 3),
    "cornell": lambda: S.cornell_scene(),
}
PARTIAL = [(1, 1), (3, 5), (9, 7), (65, 5)]     # frames of partial tiles and of windows that 4 does not divide, reference scene
_scenes, _guides, _raws, _truth = {}, {}, {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = CASES[name]()
    return _scenes[name]


def guide(name, w, h):
    if (name, w, h) not in _guides:
        sc = scene(name)
        _guides[name, w, h] = oracle_guide(sc.arrays, sc.camera, w, h)
    return _guides[name, w, h]


def raw(name, w, h, n_samples, radius):
    """(raw, a) of a case by the oracle."""
    key = (name, w, h, n_samples, float(radius))
    if key not in _raws:
        _raws[key] = oracle_raw(scene(name).arrays, guide(name, w, h), n_samples, radius)
    return _raws[key]


def truth(name, w, h, radius):
    """The mean of a over all 256 directions per hit pixel, binary64: (H,) in pixel order."""
    key = (name, w, h, float(radius))
    if key not in _truth:
        g = guide(name, w, h)
        rays, walked = sample_rays(g, 0, radius, all_directions=True)
        a = oracle_visibility(oracle_scene(scene(name).arrays), rays, walked)
        _truth[key] = a.astype(np.float64).mean(-1)
    return _truth[key]

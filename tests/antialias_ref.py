"""A numpy restatement of rz_antialias (include/rayzen_hip.h, rz_antialias.hip): the edge classification in binary32 exactly as
the header defines it, bit for bit what the kernel decides, and the colours in float64 -- upscale_ref.upscale of the frame at
factor s, box-averaged on the edge pixels; a flat pixel is its input.

Inputs: the colour c (h, w, 3) float32, row 0 = the bottom row; the guides as rz_hit records (HIT_DTYPE: a hit has instance >= 0)
at the frame's size, g (h, w), and for s >= 2 at s h x s w, g_hi; the materials (MATERIAL dtype: the albedo, and the table's
length for the clamped material word); inv_proj of the camera (f = 2 |inv_proj[5]| / h)."""
import numpy as np

import denoise_ref as DR
import upscale_ref as UR

DEFAULTS = dict(factor=2, sigma_normal=128.0, sigma_plane=1.0, demodulate=True, edge_normal=0.9, edge_plane=1.0)
F32 = np.float32


def _dot(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z in binary32, one rounding per operation."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def edge_mask(color, guides, materials, inv_proj, edge_normal=DEFAULTS["edge_normal"], edge_plane=DEFAULTS["edge_plane"]):
    """EDGE per pixel (h, w) bool: c_p is bad, or one of the up to eight neighbours inside the image is DIFFERENT from p."""
    c = np.ascontiguousarray(color, F32)
    g = np.asarray(guides)
    h, w = g.shape
    hit = g["instance"] >= 0
    word = np.where(hit, np.clip(g["material"].astype(np.int64), 0, len(materials) - 1), -1)
    n, x, t = g["normal"].astype(F32), g["point"].astype(F32), g["t"].astype(F32)
    en = F32(edge_normal)
    ke = F32(float(F32(edge_plane)) * DR.pixel_scale(inv_proj, h))      # the product in binary64, rounded once
    edge = DR.bad_pixels(c).copy()
    ys, xs = np.mgrid[0:h, 0:w]
    for b in (-1, 0, 1):
        for a in (-1, 0, 1):
            if a == 0 and b == 0:
                continue
            qy, qx = ys + b, xs + a
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            both = hit & hit[qy, qx]
            with np.errstate(invalid="ignore", over="ignore"):
                nd = _dot(n, n[qy, qx])
                pd = np.abs(_dot(n, x[qy, qx] - x))
                assert nd.dtype == F32 and pd.dtype == F32
                diff = (hit != hit[qy, qx]) | (both & ((word != word[qy, qx]) | (nd < en) | (pd > ke * t)))
            edge |= inside & diff
    return edge


def box_mean(high, s):
    """The mean of every s x s block of a (s h, s w, 3) array."""
    H, W = high.shape[:2]
    return high.reshape(H // s, s, W // s, s, 3).mean(axis=(1, 3))


def box_mean32(high, s):
    """The binary32 mean the kernel forms: (((u_0 + u_1) + ...) + u_{s^2 - 1}) / (float)(s s), b outer and a inner."""
    u = np.ascontiguousarray(high, F32)
    acc = None
    for b in range(s):
        for a in range(s):
            acc = u[b::s, a::s].copy() if acc is None else acc + u[b::s, a::s]
    return acc / F32(s * s)


def antialias(color, guides, g_hi, materials, inv_proj, factor=DEFAULTS["factor"], sigma_normal=DEFAULTS["sigma_normal"],
              sigma_plane=DEFAULTS["sigma_plane"], demodulate=DEFAULTS["demodulate"], edge_normal=DEFAULTS["edge_normal"],
              edge_plane=DEFAULTS["edge_plane"]):
    """(out (h, w, 3) float64, edge (h, w) bool).  factor = 1: out = c (g_hi is not read)."""
    c32 = np.ascontiguousarray(color, F32)
    edge = edge_mask(c32, guides, materials, inv_proj, edge_normal, edge_plane)
    out = c32.astype(np.float64)
    s = int(factor)
    if s == 1:
        return out, edge
    up = UR.upscale(c32, guides, g_hi, materials, inv_proj, factor=s, sigma_normal=sigma_normal, sigma_plane=sigma_plane,
                    demodulate=demodulate)
    return np.where(edge[..., None], box_mean(up, s), out), edge

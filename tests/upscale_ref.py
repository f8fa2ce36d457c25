"""A float64 numpy restatement of the guided upsampling of rz_upscale (include/rayzen_hip.h, rz_upscale.hip): the reference the
kernel's float32 colours are held to.

Inputs: the low colour c (h, w, 3) float32, row 0 = the bottom row; the guides as rz_hit records (HIT_DTYPE: a hit has
instance >= 0), g_lo (h, w) and g_hi (s h, s w); the materials (MATERIAL dtype) for the albedo; inv_proj of the camera (for the
footprint f of a LOW pixel).  The footprint and the bilinear weights are taken in integers and binary32 exactly as the header
states them, so the restatement and the kernel agree on every tap and on the stage every pixel takes."""
import numpy as np

import denoise_ref as DR

DEFAULTS = dict(factor=2, sigma_normal=128.0, sigma_plane=1.0, demodulate=True)
FLOOR = 1e-4
STAGE1 = [(a, b) for b in (0, 1) for a in (0, 1)]
STAGE2 = [(a, b) for b in (-1, 0, 1, 2) for a in (-1, 0, 1, 2) if not (0 <= a <= 1 and 0 <= b <= 1)]


def footprint(X, s):
    """i0 = floor((2X + 1 - s) / 2s) in integers and fx = (float)(r - 2s i0) / (float)(2s) in binary32, for high coordinates X."""
    r = 2 * np.asarray(X, np.int64) + 1 - s
    i0 = r // (2 * s)
    fx = (r - 2 * s * i0).astype(np.float32) / np.float32(2 * s)
    return i0, fx


def upscale(color, g_lo, g_hi, materials, inv_proj, factor=DEFAULTS["factor"], sigma_normal=DEFAULTS["sigma_normal"],
            sigma_plane=DEFAULTS["sigma_plane"], demodulate=DEFAULTS["demodulate"], want_stage=False):
    """The reconstructed colour (s h, s w, 3) float64; with want_stage also the stage (1, 2 or 3) every high pixel took.
    factor = 1 returns c itself (stage 0)."""
    c32 = np.ascontiguousarray(color, np.float32)
    h, w = c32.shape[:2]
    s = int(factor)
    if s == 1:
        out = c32.astype(np.float64)
        return (out, np.zeros((h, w), int)) if want_stage else out
    g_lo, g_hi = np.asarray(g_lo), np.asarray(g_hi)
    H, W = h * s, w * s
    assert g_lo.shape == (h, w) and g_hi.shape == (H, W)
    bad = DR.bad_pixels(c32)
    c = np.where(bad[..., None], 0.0, c32.astype(np.float64))      # (a bad colour is never used in arithmetic)
    a_lo = DR.albedo(g_lo, materials) if demodulate else np.ones_like(c)
    a_hi = DR.albedo(g_hi, materials) if demodulate else np.ones((H, W, 3))
    d = c / np.maximum(a_lo, 1e-3)
    hit_lo, hit_hi = g_lo["instance"] >= 0, g_hi["instance"] >= 0
    n_lo, x_lo = g_lo["normal"].astype(np.float64), g_lo["point"].astype(np.float64)
    n_hi, x_hi, t_hi = g_hi["normal"].astype(np.float64), g_hi["point"].astype(np.float64), g_hi["t"].astype(np.float64)
    f = DR.pixel_scale(inv_proj, h)
    i0, fx = footprint(np.arange(W), s)
    j0, fy = footprint(np.arange(H), s)
    one = np.float32(1.0)

    def gather(taps, bilinear):
        num, den, found = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W), bool)
        for a, b in taps:
            qx, qy = (i0 + a)[None, :], (j0 + b)[:, None]
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            ix, iy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            ix, iy = np.broadcast_to(ix, (H, W)), np.broadcast_to(iy, (H, W))
            ok = inside & ~bad[iy, ix] & (hit_lo[iy, ix] == hit_hi)
            if bilinear:        # binary32, one rounding per operation
                B = ((fx if a else one - fx)[None, :] * (fy if b else one - fy)[:, None]).astype(np.float64)
                ok = ok & (B > 0)
            else:
                B = 1.0
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                nd = np.maximum(np.sum(n_hi * n_lo[iy, ix], -1), 0.0)
                plane = np.abs(np.sum(n_hi * (x_lo[iy, ix] - x_hi), -1)) / (sigma_plane * t_hi * f)
                wg = np.where(hit_hi, nd ** sigma_normal * np.exp(-plane), 1.0)
            wt = np.where(ok, B * np.maximum(wg, FLOOR), 0.0)
            num += wt[..., None] * d[iy, ix]
            den += wt
            found |= ok
        with np.errstate(invalid="ignore", divide="ignore"):
            return a_hi * num / den[..., None], found

    out1, any1 = gather(STAGE1, True)
    out2, any2 = gather(STAGE2, False)
    near = np.ix_(np.arange(H) // s, np.arange(W) // s)
    out3 = np.where(bad[near][..., None], 0.0, c[near])
    out = np.where(any1[..., None], out1, np.where(any2[..., None], out2, out3))
    if want_stage:
        return out, np.where(any1, 1, np.where(any2, 2, 3))
    return out


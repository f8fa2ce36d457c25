"""A numpy restatement of rz_antialias_seethrough (include/rayzen_hip.h, rz_antialias_seethrough.hip), composed of the three
restatements it extends: antialias_ref (the edge rule in binary32, the box mean), seethrough_ref (the chain, the gather with
alpha = T * albedo and the class term) and upscale_ref underneath.

The record of a pixel is its chain record: the guide g (HIT_DTYPE: the FINAL query, t = L), the throughput T and the class cls.
q is DIFFERENT from p when rz_antialias' rule holds on the final records or cls_q != cls_p.  EDGE is an "any" over the
neighbours, so the mask is antialias_ref.edge_mask on the final guides OR "a neighbour inside the image has another class".
An edge pixel is the box mean of seethrough_ref.upscale's output at factor s; a flat pixel is its input."""
import numpy as np

import antialias_ref as AR
import seethrough_ref as SR

DEFAULTS = dict(AR.DEFAULTS, max_depth=SR.MAX_DEPTH)
F32 = np.float32


def class_edges(cls):
    """(h, w) bool: one of the up to eight neighbours inside the image has another class."""
    cls = np.asarray(cls)
    h, w = cls.shape
    out = np.zeros((h, w), bool)
    ys, xs = np.mgrid[0:h, 0:w]
    for b in (-1, 0, 1):
        for a in (-1, 0, 1):
            if a == 0 and b == 0:
                continue
            qy, qx = ys + b, xs + a
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            out |= inside & (cls[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)] != cls)
    return out


def edge_mask(color, guides, cls, materials, inv_proj, edge_normal=DEFAULTS["edge_normal"], edge_plane=DEFAULTS["edge_plane"]):
    """EDGE per pixel (h, w) bool, bit for bit what the kernel decides given these records."""
    return AR.edge_mask(color, guides, materials, inv_proj, edge_normal, edge_plane) | class_edges(cls)


def antialias(color, g, T, cls, g_hi, T_hi, cls_hi, materials, inv_proj, factor=DEFAULTS["factor"],
              sigma_normal=DEFAULTS["sigma_normal"], sigma_plane=DEFAULTS["sigma_plane"], demodulate=DEFAULTS["demodulate"],
              edge_normal=DEFAULTS["edge_normal"], edge_plane=DEFAULTS["edge_plane"]):
    """(out (h, w, 3) float64, edge (h, w) bool) from the chain records at the frame's size (g, T, cls) and, for s >= 2, at
    s h x s w (g_hi, T_hi, cls_hi).  factor = 1: out = c (the high records are not read)."""
    c32 = np.ascontiguousarray(color, F32)
    edge = edge_mask(c32, g, cls, materials, inv_proj, edge_normal, edge_plane)
    out = c32.astype(np.float64)
    s = int(factor)
    if s == 1:
        return out, edge
    up = SR.upscale(c32, g, g_hi, T, T_hi, cls, cls_hi, materials, inv_proj, factor=s, sigma_normal=sigma_normal,
                    sigma_plane=sigma_plane, demodulate=demodulate)
    return np.where(edge[..., None], AR.box_mean(up, s), out), edge

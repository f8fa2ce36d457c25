"""A float64 numpy restatement of rz_denoise_temporal (include/rayzen_hip.h, rz_temporal.hip): temporal accumulation by
reprojection, the variance estimate and the variance-guided a-trous filter (SVGF: Schied et al., HPG 2017) -- the reference the
kernels' float32 results are held to, and what the CPU quality measurement runs.

A history is None (empty) or a dict: col (H, W, 4) colour | N, mom (H, W, 2), guide (H, W) HIT_DTYPE, view, proj, inv_proj (16
floats each, column-major), cam_pos (3), inst (n, 2, 4, 3) float32: per instance inverseTransform and transform as columns 0..3,
rows 0..2 -- exactly what Renderer.debug_read_temporal returns, piece by piece.

Every step also returns `ambiguous` (H, W) bool: the pixels where one of the step's decisions -- clip.w > 0, floor(u) / floor(v)
(and with them the range test and which taps have weight), a tap's normal or plane test, S >= 0.01, N >= 4 -- flips under a
relative perturbation of EPS = 1e-4 of its operands: a comparison a >= b counts as such when |a - b| <= EPS max(|a|, |b|);
floor(u) when u is within EPS |ndc| W / 2 of an integer (its operand is ndc = clip.x / clip.w); N >= 4 only where the counted
taps had different lengths (N_h is exact otherwise, by the way the header forms it).
There a binary32 evaluation may legitimately decide the other way; the GPU tests leave those pixels out and cap their share."""
import numpy as np

import denoise_ref as DR

EPS = 1e-4
DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, max_history=32, normal_cos=0.9, plane_tol=2.0, iterations=5, sigma_l=0.5,
                sigma_normal=128.0, sigma_plane=1.0, demodulate=1)
LUM = (0.2126, 0.7152, 0.0722)


def params(**kw):
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


def lum(d):
    return (LUM[0] * d[..., 0] + LUM[1] * d[..., 1]) + LUM[2] * d[..., 2]


def inst_pack(instances):
    """(n, 2, 4, 3) float32 from rz_bvh_instance records: inverseTransform, transform; columns 0..3, rows 0..2."""
    inv = np.asarray(instances["inverseTransform"], np.float32).reshape(-1, 4, 4)[:, :, :3]
    fwd = np.asarray(instances["transform"], np.float32).reshape(-1, 4, 4)[:, :, :3]
    return np.ascontiguousarray(np.stack([inv, fwd], 1))


def make_history(col, mom, guide, view, proj, inv_proj, cam_pos, inst):
    return dict(col=np.asarray(col), mom=np.asarray(mom), guide=np.asarray(guide), view=np.asarray(view, np.float32).reshape(16),
                proj=np.asarray(proj, np.float32).reshape(16), inv_proj=np.asarray(inv_proj, np.float32).reshape(16),
                cam_pos=np.asarray(cam_pos, np.float32).reshape(3), inst=np.asarray(inst, np.float32).reshape(-1, 2, 4, 3))


def _affine(m, p):
    return (m[..., 0, :] * p[..., 0:1] + m[..., 1, :] * p[..., 1:2]) + m[..., 2, :] * p[..., 2:3] + m[..., 3, :]


def _tdir(m, v):
    return np.stack([np.sum(m[..., k, :] * v, -1) for k in range(3)], -1)


def _near(a, b):
    return np.abs(a - b) <= EPS * np.maximum(np.abs(a), np.abs(b))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def accumulate(hist, color, guides, materials, view, proj, inst, miss_dir, p):
    """Steps 1-4 of the header.  color: c (H, W, 3); guides: this frame's rz_hit records; view, proj: this frame's; inst: this
    frame's (n, 2, 4, 3); miss_dir (H, W, 3): the unit direction of every pixel-centre ray (renderer.editor_rays).
    Returns a dict: D (H, W, 3), N, M (H, W, 2), accepted, S, out0 (the K = 0 output), ambiguous, scale (the largest magnitude
    among the colours a pixel's result was formed from: the m_p of the tolerance), alpha, d, bad.
    A bad pixel (DR.bad_pixels of the binary32 c) takes d := D_h where history is accepted and 0 where not; until then its d is
    masked to 0, so no arithmetic touches the sample, and scale and the ambiguous masks stay finite and do not depend on it."""
    c = np.asarray(color, np.float64)
    bad = DR.bad_pixels(color)
    g = np.asarray(guides)
    H, W = c.shape[:2]
    hit = g["instance"] >= 0
    demod = bool(p["demodulate"])
    alpha = DR.albedo(g, materials) if demod else np.ones_like(c)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(hit[..., None] & demod, c / np.maximum(alpha, 1e-3), c)
    d = np.where(bad[..., None], 0.0, d)
    amb = np.zeros((H, W), bool)
    parts = {k: np.zeros((H, W), bool) for k in ("clip_w", "floor", "normal", "plane", "S")}
    S = np.zeros((H, W))
    dH = np.zeros((H, W, 3))
    nH, m1, m2 = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    n0, n_spread = np.zeros((H, W)), np.zeros((H, W))
    scale = np.abs(d).max(-1)
    have_prev = hist is not None and hist["col"].shape[:2] == (H, W) and len(hist["inst"]) == len(inst)
    if have_prev:
        inst = np.asarray(inst, np.float32).reshape(-1, 2, 4, 3)
        pinst = hist["inst"]
        cam_same = _bits_equal(view, hist["view"]) and _bits_equal(proj, hist["proj"])
        same_inst = (inst[:, 1].view(np.uint32) == pinst[:, 1].view(np.uint32)).all((1, 2))
        ii = np.clip(g["instance"], 0, max(len(inst) - 1, 0))
        x = g["point"].astype(np.float64)
        n = g["normal"].astype(np.float64)
        i64, p64 = inst.astype(np.float64), pinst.astype(np.float64)
        moved = hit & ~same_inst[ii] if len(inst) else np.zeros((H, W), bool)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if len(inst):
                o = _affine(i64[ii, 0], x)
                x2 = _affine(p64[ii, 1], o)
                b = _tdir(p64[ii, 0], _tdir(i64[ii, 1], n))
                n2 = b / np.sqrt(np.sum(b * b, -1))[..., None]
            else:
                x2, n2 = x, n
            xq = np.where(moved[..., None], x2, x)
            nq = np.where(moved[..., None], n2, n)
            xq = np.where(hit[..., None], xq, np.asarray(miss_dir, np.float64).reshape(H, W, 3))
            w4 = hit.astype(np.float64)
            still = cam_same & (~hit | ~moved)
            V = hist["view"].astype(np.float64).reshape(4, 4)
            Pm = hist["proj"].astype(np.float64).reshape(4, 4)
            e = (xq[..., 0:1] * V[0] + xq[..., 1:2] * V[1]) + xq[..., 2:3] * V[2] + w4[..., None] * V[3]
            clip = (e[..., 0:1] * Pm[0] + e[..., 1:2] * Pm[1]) + e[..., 2:3] * Pm[2] + e[..., 3:4] * Pm[3]
            cw = clip[..., 3]
            cw_scale = np.abs(e * Pm[:, 3]).sum(-1)
            parts["clip_w"] = ~still & (np.abs(cw) <= EPS * cw_scale)
            ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
            u = np.where(still, xs, (clip[..., 0] / cw * 0.5 + 0.5) * W - 0.5)
            v = np.where(still, ys, (clip[..., 1] / cw * 0.5 + 0.5) * H - 0.5)
            have = (still | (cw > 0)) & (u > -1) & (u < W) & (v > -1) & (v < H)
            # floor(u), floor(v): near an integer the tap set (and the range test) may differ
            close = ~still & (cw > 0) & (u > -2) & (u < W + 1) & (v > -2) & (v < H + 1)
            # (the operand is ndc = clip.xy / clip.w: EPS of it is EPS |u + 0.5 - W / 2| of a pixel)
            parts["floor"] = close & ((np.abs(u - np.rint(u)) <= EPS * np.abs(u + 0.5 - 0.5 * W)) |
                                      (np.abs(v - np.rint(v)) <= EPS * np.abs(v + 0.5 - 0.5 * H)))
            u = np.where(have, u, 0.0)
            v = np.where(have, v, 0.0)
            fu, fv = np.floor(u), np.floor(v)
            fx, fy = u - fu, v - fv
            x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
            dc = xq - hist["cam_pos"].astype(np.float64)
            f_prev = DR.pixel_scale(hist["inv_proj"], H)
            plane_max = p["plane_tol"] * np.sqrt(np.sum(dc * dc, -1)) * f_prev
            pg = hist["guide"]
            pcol = hist["col"].astype(np.float64)
            pmom = hist["mom"].astype(np.float64)
            for k in range(4):
                qx, qy = x0 + (k & 1), y0 + (k >> 1)
                w = (fx if k & 1 else 1.0 - fx) * (fy if k >> 1 else 1.0 - fy)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                gq = pg[cy, cx]
                hq = gq["instance"] >= 0
                valid = have & (w > 0) & inside & (hq == hit)
                cand = valid & hit & (gq["instance"] == g["instance"])
                nd = np.sum(nq * gq["normal"].astype(np.float64), -1)
                pd = np.abs(np.sum(nq * (gq["point"].astype(np.float64) - xq), -1))
                parts["normal"] |= cand & _near(nd, p["normal_cos"])
                parts["plane"] |= cand & (nd >= p["normal_cos"]) & _near(pd, plane_max)
                valid &= ~hit | (cand & (nd >= p["normal_cos"]) & (pd <= plane_max))
                wv = np.where(valid, w, 0.0)
                n0 = np.where(valid & (S == 0), pcol[cy, cx, 3], n0)        # N_0: the first counted tap's
                S += wv
                dH += wv[..., None] * pcol[cy, cx, :3]
                nH += wv * (pcol[cy, cx, 3] - n0)
                n_spread = np.maximum(n_spread, np.where(valid, np.abs(pcol[cy, cx, 3] - n0), 0.0))
                m1 += wv * pmom[cy, cx, 0]
                m2 += wv * pmom[cy, cx, 1]
                scale = np.maximum(scale, np.where(valid, np.abs(pcol[cy, cx, :3]).max(-1), 0.0))
            parts["S"] = have & (S > 0) & _near(S, 0.01)
        for m in parts.values():
            amb |= m
    accepted = S >= 0.01
    with np.errstate(invalid="ignore", divide="ignore"):
        Ssafe = np.where(accepted, S, 1.0)
        dH, nH, m1, m2 = dH / Ssafe[..., None], n0 + nH / Ssafe, m1 / Ssafe, m2 / Ssafe
    d = np.where(bad[..., None], np.where(accepted[..., None], dH, 0.0), d)
    l = lum(d)
    N = np.where(accepted, np.minimum(nH + 1.0, float(p["max_history"])), 1.0)
    a = np.maximum(p["alpha"], 1.0 / N)
    am = np.maximum(p["alpha_moments"], 1.0 / N)
    D = np.where(accepted[..., None], dH + a[..., None] * (d - dH), d)
    M1 = np.where(accepted, m1 + am * (l - m1), l)
    M2 = np.where(accepted, m2 + am * (l * l - m2), l * l)
    out0 = np.where(accepted[..., None], D * alpha, c)
    # N >= 4 (the variance's branch): exact where every counted tap had one length, else open when N is within EPS of 4
    amb_n = accepted & (n_spread > 0) & _near(N, 4.0)
    return dict(D=D, N=N, M=np.stack([M1, M2], -1), accepted=accepted, S=S, ambiguous_n=amb_n, ambiguous_parts=parts, out0=out0, ambiguous=amb, scale=scale, alpha=alpha, d=d, bad=bad)


def _geometry(guides, inv_proj):
    g = np.asarray(guides)
    return (g["instance"] >= 0, g["normal"].astype(np.float64), g["point"].astype(np.float64), g["t"].astype(np.float64),
            DR.pixel_scale(inv_proj, g.shape[0]))


def _w_geom(hit, n, x, t, f, dx, dy, dist_px, sigma_normal, sigma_plane):
    """[hit_p == hit_q] W_geom for q = p + (dx, dy), 0 outside the image; dist_px = s max(|a|, |b|)."""
    hq, valid = DR._shift(hit, dx, dy, False)
    nq, _ = DR._shift(n, dx, dy, 0.0)
    xq, _ = DR._shift(x, dx, dy, 0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nd = np.maximum(np.sum(n * nq, -1), 0.0)
        plane = np.abs(np.sum(n * (xq - x), -1)) / (sigma_plane * t * f * dist_px)
        w = np.where(hit & hq, nd ** sigma_normal * np.exp(-plane), 1.0)
    w = np.where(valid & (hq == hit), w, 0.0)
    return np.where(w > 0, w, 0.0)


def variance(D, N, M, guides, inv_proj, p):
    """Step 5.  Returns the variance (H, W)."""
    hit, n, x, t, f = _geometry(guides, inv_proj)
    temporal = np.maximum(0.0, M[..., 1] - M[..., 0] * M[..., 0])
    lD = lum(np.asarray(D, np.float64))
    sw, s1, s2 = np.ones_like(lD), lD.copy(), lD * lD
    for b in range(-3, 4):
        for a in range(-3, 4):
            if a == 0 and b == 0:
                continue
            w = _w_geom(hit, n, x, t, f, a, b, max(abs(a), abs(b)), p["sigma_normal"], p["sigma_plane"])
            lq, _ = DR._shift(lD, a, b, 0.0)
            sw += w
            s1 += w * lq
            s2 += w * lq * lq
    mean = s1 / sw
    spatial = np.maximum(0.0, s2 / sw - mean * mean) * (4.0 / N)
    return np.where(N >= 4.0, temporal, spatial)


def gauss3(var):
    """g_p: the variance under (1/4, 1/8, 1/16), renormalised over the taps inside the image."""
    num, den = np.zeros_like(var), np.zeros_like(var)
    for b in (-1, 0, 1):
        for a in (-1, 0, 1):
            k = 0.25 if (a == 0 and b == 0) else (0.0625 if (a != 0 and b != 0) else 0.125)
            vq, valid = DR._shift(var, a, b, 0.0)
            num += k * vq * valid
            den += k * valid
    return num / den


def atrous_pass(d, var, guides, inv_proj, i, p, want_weights=False):
    """Pass i (step 2^i) of step 6 on (d, var).  Returns (d', var') (and, with want_weights, the normalised weights)."""
    hit, n, x, t, f = _geometry(guides, inv_proj)
    s = 1 << i
    l = lum(d)
    inv_l = 1.0 / (p["sigma_l"] * np.sqrt(np.maximum(gauss3(var), 0.0)) + 1e-8)
    num, den, vnum = np.zeros_like(d), np.zeros(d.shape[:2]), np.zeros(d.shape[:2])
    raw = {}
    for b in range(-2, 3):
        for a in range(-2, 3):
            hk = DR.H_KERNEL[a + 2] * DR.H_KERNEL[b + 2]
            if a == 0 and b == 0:
                w = np.full(d.shape[:2], hk)
                dq, vq = d, var
            else:
                dq, _ = DR._shift(d, a * s, b * s, 0.0)
                vq, _ = DR._shift(var, a * s, b * s, 0.0)
                w = hk * _w_geom(hit, n, x, t, f, a * s, b * s, s * max(abs(a), abs(b)), p["sigma_normal"], p["sigma_plane"])
                w = w * np.exp(-np.abs(l - lum(dq)) * inv_l)
            num += w[..., None] * dq
            den += w
            vnum += w * w * vq
            raw[(a, b)] = w
    out = num / den[..., None], vnum / (den * den)
    return out + ({k: w / den for k, w in raw.items()},) if want_weights else out


def filter_from(D, var, alpha, guides, inv_proj, p):
    """Step 6 for K = p["iterations"] >= 1 passes, from the temporal stage's D and variance: the output colour."""
    d, v = np.asarray(D, np.float64), np.asarray(var, np.float64)
    for i in range(p["iterations"]):
        d, v = atrous_pass(d, v, guides, inv_proj, i, p)
    return d * alpha


def step(hist, color, guides, materials, view, proj, inv_proj, cam_pos, inst, miss_dir, p, want_filter=True):
    """One call: returns (result, new history).  result: accumulate()'s dict plus var, out (the call's colour output) and
    ambiguous including the N >= 4 decision."""
    r = accumulate(hist, color, guides, materials, view, proj, inst, miss_dir, p)
    r["var"] = variance(r["D"], r["N"], r["M"], guides, inv_proj, p)
    r["ambiguous_var"] = r["ambiguous"] | r["ambiguous_n"]
    r["out"] = r["out0"] if p["iterations"] == 0 or not want_filter else filter_from(r["D"], r["var"], r["alpha"], guides, inv_proj, p)
    new = make_history(np.concatenate([r["D"], r["N"][..., None]], -1), r["M"], guides, view, proj, inv_proj, cam_pos, inst)
    return r, new


def mse(a, b):
    return DR.mse(a, b)

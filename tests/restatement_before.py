"""The float64 restatements as they stood before the bad-pixel rule (a NaN or infinite sample is contained: include/rayzen_hip.h),
frozen: denoise_ref's atrous_pass and denoise, temporal_ref's accumulate.  test_denoise_abi.py and test_temporal_abi.py hold the
current restatements to these, bit for bit, on the finite inputs of their own tests.  Nothing else may use them: on a non-finite
sample they are not a statement of the kernels (np.where(w > 0, ...) swallows a NaN weight that the old kernel kept)."""
import numpy as np

import denoise_ref as DR
from denoise_ref import H_KERNEL, DEFAULTS, _shift, albedo, pixel_scale
from temporal_ref import _affine, _bits_equal, _near, _tdir, lum, EPS


def atrous_pass(d, hit, n, x, t, f, i, sigma_color, sigma_normal, sigma_plane, want_weights=False):
    """Pass i (step s = 2^i) on the colour d (H, W, 3).  Returns d' (and, with want_weights, the normalised weight of every tap:
    a dict (a, b) -> (H, W) array)."""
    s = 1 << i
    num = np.zeros_like(d)
    den = np.zeros(d.shape[:2])
    raw = {}
    inv_c = float(2.0 ** i) / (sigma_color * sigma_color)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(-2, 3):
            for a in range(-2, 3):
                dq, valid = _shift(d, a * s, b * s, 0.0)
                hq, _ = _shift(hit, a * s, b * s, False)
                w = H_KERNEL[a + 2] * H_KERNEL[b + 2] * (valid & (hq == hit))
                if a != 0 or b != 0:
                    nq, _ = _shift(n, a * s, b * s, 0.0)
                    xq, _ = _shift(x, a * s, b * s, 0.0)
                    both = hit & hq
                    nd = np.maximum(np.sum(n * nq, -1), 0.0)
                    wn = nd ** sigma_normal
                    plane = np.abs(np.sum(n * (xq - x), -1)) / (sigma_plane * t * f * s * max(abs(a), abs(b)))
                    w = w * np.where(both, wn * np.exp(-plane), 1.0)
                w = w * np.exp(-np.sum((d - dq) ** 2, -1) * inv_c)
                w = np.where(w > 0, w, 0.0)         # (a dropped tap stays at 0 whatever its 0 * inf gave)
                num += w[..., None] * dq
                den += w
                if want_weights:
                    raw[(a, b)] = w
    out = num / den[..., None]
    if want_weights:
        return out, {k: v / den for k, v in raw.items()}
    return out


def denoise(color, guides, materials, inv_proj, iterations=DEFAULTS["iterations"], sigma_color=DEFAULTS["sigma_color"],
            sigma_normal=DEFAULTS["sigma_normal"], sigma_plane=DEFAULTS["sigma_plane"], demodulate=DEFAULTS["demodulate"]):
    """The filtered colour (H, W, 3) float64.  iterations = 0 returns c itself."""
    c = np.asarray(color, np.float64)
    if iterations == 0:
        return c.copy()
    g = np.asarray(guides)
    H = c.shape[0]
    hit = g["instance"] >= 0
    n = g["normal"].astype(np.float64)
    x = g["point"].astype(np.float64)
    t = g["t"].astype(np.float64)
    f = pixel_scale(inv_proj, H)
    alpha = albedo(g, materials) if demodulate else np.ones_like(c)
    d = c / np.maximum(alpha, 1e-3) if demodulate else c.copy()
    for i in range(iterations):
        d = atrous_pass(d, hit, n, x, t, f, i, sigma_color, sigma_normal, sigma_plane)
    return d * alpha if demodulate else d


def accumulate(hist, color, guides, materials, view, proj, inst, miss_dir, p):
    """Steps 1-4 of the header.  color: c (H, W, 3); guides: this frame's rz_hit records; view, proj: this frame's; inst: this
    frame's (n, 2, 4, 3); miss_dir (H, W, 3): the unit direction of every pixel-centre ray (renderer.editor_rays).
    Returns a dict: D (H, W, 3), N, M (H, W, 2), accepted, S, out0 (the K = 0 output), ambiguous, scale (the largest magnitude
    among the colours a pixel's result was formed from: the m_p of the tolerance), alpha, d."""
    c = np.asarray(color, np.float64)
    g = np.asarray(guides)
    H, W = c.shape[:2]
    hit = g["instance"] >= 0
    demod = bool(p["demodulate"])
    alpha = DR.albedo(g, materials) if demod else np.ones_like(c)
    d = np.where(hit[..., None] & demod, c / np.maximum(alpha, 1e-3), c)
    l = lum(d)
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
    N = np.where(accepted, np.minimum(nH + 1.0, float(p["max_history"])), 1.0)
    a = np.maximum(p["alpha"], 1.0 / N)
    am = np.maximum(p["alpha_moments"], 1.0 / N)
    D = np.where(accepted[..., None], dH + a[..., None] * (d - dH), d)
    M1 = np.where(accepted, m1 + am * (l - m1), l)
    M2 = np.where(accepted, m2 + am * (l * l - m2), l * l)
    out0 = np.where(accepted[..., None], D * alpha, c)
    # N >= 4 (the variance's branch): exact where every counted tap had one length, else open when N is within EPS of 4
    amb_n = accepted & (n_spread > 0) & _near(N, 4.0)
    return dict(D=D, N=N, M=np.stack([M1, M2], -1), accepted=accepted, S=S, ambiguous_n=amb_n, ambiguous_parts=parts, out0=out0, ambiguous=amb, scale=scale, alpha=alpha, d=d)

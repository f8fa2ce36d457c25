"""A float64 numpy restatement of the edge-avoiding a-trous filter of rz_denoise (include/rayzen_hip.h, rz_denoise.hip;
Dammertz et al., HPG 2010): the reference the kernel's float32 colours are held to.

Inputs: the colour c (H, W, 3), row 0 = the bottom row; the guide G as rz_hit records (H, W) (HIT_DTYPE: a hit has
instance >= 0); the materials (MATERIAL dtype) for the albedo; inv_proj of the camera (for the pixel footprint f)."""
import numpy as np

H_KERNEL = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = dict(iterations=5, sigma_color=0.5, sigma_normal=128.0, sigma_plane=1.0, demodulate=True)


def resolve(accum):
    """c = accum.rgb / n with n = accum.a > 0 ? accum.a : 1, in float32 as the kernels divide (rz_present without the clamp)."""
    a = np.asarray(accum, np.float32)
    n = np.where(a[..., 3] > 0, a[..., 3], np.float32(1.0))
    return (a[..., :3] / n[..., None]).astype(np.float32)


def bad_pixels(color):
    """The pixels the header calls bad: a channel of the binary32 c is NaN or +-Inf (the exponent field all ones)."""
    bits = np.ascontiguousarray(color, np.float32).view(np.uint32)
    return ((bits & 0x7F800000) == 0x7F800000).any(-1)


def pixel_scale(inv_proj, height):
    """f = 2 |inv_proj[5]| / height: the world size of one pixel at unit distance."""
    return 2.0 * abs(float(np.float32(np.asarray(inv_proj, np.float32).reshape(16)[5]))) / float(height)


def albedo(guides, materials):
    """alpha_p: the albedo of the hit's material (index clamped to the table), (1, 1, 1) for a miss."""
    g = np.asarray(guides)
    hit = g["instance"] >= 0
    alb = np.asarray(materials["albedo"], np.float64)
    mi = np.clip(g["material"].astype(np.int64), 0, len(alb) - 1)
    return np.where(hit[..., None], alb[mi], 1.0)


def _shift(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx] where that pixel lies inside the image, else fill; and the validity mask."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    valid = np.zeros((H, W), bool)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        valid[y0:y1, x0:x1] = True
    return out, valid


def atrous_pass(d, hit, n, x, t, f, i, sigma_color, sigma_normal, sigma_plane, want_weights=False, bad=None, want_den=False):
    """Pass i (step s = 2^i) on the colour d (H, W, 3).  bad (H, W) bool: the bad pixels of pass 0 (None: none) -- dropped as
    taps; as centres they drop their own term, weigh every remaining tap's colour term as 1 and come out as num / den, or 0
    where den is 0.  Their d is masked to 0 before any arithmetic touches it.  Returns d' (and, with want_weights, the normalised
    weight of every tap: a dict (a, b) -> (H, W) array; with want_den, the pass's den)."""
    s = 1 << i
    bad = np.zeros(d.shape[:2], bool) if bad is None else np.asarray(bad, bool)
    d = np.where(bad[..., None], 0.0, d)
    num = np.zeros_like(d)
    den = np.zeros(d.shape[:2])
    raw = {}
    inv_c = float(2.0 ** i) / (sigma_color * sigma_color)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(-2, 3):
            for a in range(-2, 3):
                dq, valid = _shift(d, a * s, b * s, 0.0)
                hq, _ = _shift(hit, a * s, b * s, False)
                bq, _ = _shift(bad, a * s, b * s, False)
                w = H_KERNEL[a + 2] * H_KERNEL[b + 2] * (valid & (hq == hit) & ~bq)
                if a != 0 or b != 0:
                    nq, _ = _shift(n, a * s, b * s, 0.0)
                    xq, _ = _shift(x, a * s, b * s, 0.0)
                    both = hit & hq
                    nd = np.maximum(np.sum(n * nq, -1), 0.0)
                    wn = nd ** sigma_normal
                    plane = np.abs(np.sum(n * (xq - x), -1)) / (sigma_plane * t * f * s * max(abs(a), abs(b)))
                    w = w * np.where(both, wn * np.exp(-plane), 1.0)
                w = w * np.where(bad, 1.0, np.exp(-np.sum((d - dq) ** 2, -1) * inv_c))
                w = np.where(w > 0, w, 0.0)         # (a dropped tap stays at 0 whatever the 0 * inf of its geometry gave)
                num += w[..., None] * dq
                den += w
                if want_weights:
                    raw[(a, b)] = w
        out = np.where((bad & ~(den > 0))[..., None], 0.0, num / den[..., None])
    res = (out,)
    if want_weights:
        res += ({k: v / den for k, v in raw.items()},)
    if want_den:
        res += (den,)
    return res if len(res) > 1 else out


def denoise(color, guides, materials, inv_proj, iterations=DEFAULTS["iterations"], sigma_color=DEFAULTS["sigma_color"],
            sigma_normal=DEFAULTS["sigma_normal"], sigma_plane=DEFAULTS["sigma_plane"], demodulate=DEFAULTS["demodulate"],
            want_den=False):
    """The filtered colour (H, W, 3) float64.  iterations = 0 returns c itself.  The bad pixels (bad_pixels of the binary32 c)
    are contained by pass 0, so the result is finite for iterations >= 1.  want_den: also pass 0's den (0 where a bad pixel
    found no tap: its pass-0 colour is exactly 0)."""
    c = np.asarray(color, np.float64)
    if iterations == 0:
        return (c.copy(), None) if want_den else c.copy()
    g = np.asarray(guides)
    H = c.shape[0]
    hit = g["instance"] >= 0
    n = g["normal"].astype(np.float64)
    x = g["point"].astype(np.float64)
    t = g["t"].astype(np.float64)
    f = pixel_scale(inv_proj, H)
    bad = bad_pixels(color)
    alpha = albedo(g, materials) if demodulate else np.ones_like(c)
    with np.errstate(invalid="ignore", over="ignore"):
        d = c / np.maximum(alpha, 1e-3) if demodulate else c.copy()
    d, den0 = atrous_pass(d, hit, n, x, t, f, 0, sigma_color, sigma_normal, sigma_plane, bad=bad, want_den=True)
    for i in range(1, iterations):
        d = atrous_pass(d, hit, n, x, t, f, i, sigma_color, sigma_normal, sigma_plane)
    out = d * alpha if demodulate else d
    return (out, den0) if want_den else out


def mse(a, b):
    return float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))

"""rz_bloom restated in numpy float32 (include/rayzen_hip.h, "Glare", steps 1 to 6): every operation of the definition is one
binary32 operation here, in the definition's order, so the GPU's images are compared with these for equality.  bloom() is the
vectorised form (index arithmetic on whole images); bloom_loops() says the same pixel by pixel in plain loops and exists only
to cross-check the first on small frames."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(threshold=1.0, knee=0.5, limit=64.0, intensity=0.25, spread=1.0, levels=6)


def level_sizes(W, H, levels=6):
    """Step 1: [(w_0, h_0), ...]."""
    out = []
    w, h = W, H
    while True:
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
        if len(out) >= levels or (w, h) == (1, 1):
            return out


def bad_pixels(c):
    """A channel is NaN or +-Inf, decided on the bit pattern."""
    return ((np.ascontiguousarray(c, F32).view(np.uint32) & 0x7F800000) == 0x7F800000).any(axis=-1)


def onset(b, threshold, knee, limit):
    """m of step 2 for brightness b (an array or a scalar)."""
    b = np.asarray(b, F32)
    threshold, knee, limit = F32(threshold), F32(knee), F32(limit)
    with np.errstate(all="ignore"):
        d = b - threshold
        s = np.fmin(np.fmax(d + knee, F32(0)), F32(2) * knee)
        q = (s * s) / (F32(4) * knee) if knee > 0 else np.zeros_like(b)
        return np.fmin(np.fmax(q, d), limit)


def prefilter(c, threshold, knee, limit):
    """Step 2 on an (H, W, 3) image."""
    c = np.ascontiguousarray(c, F32)
    bad = bad_pixels(c)
    with np.errstate(all="ignore"):
        cp = np.where(c > 0, c, F32(0))
        b = np.fmax(np.fmax(cp[..., 0], cp[..., 1]), cp[..., 2])
        m = onset(b, threshold, knee, limit)
        f = np.where(m > 0, m / np.fmax(b, F32(1e-4)), F32(0)).astype(F32)
        p = cp * f[..., None]
    p[bad] = 0
    return p


def _taps4(t0, t1, t2, t3):
    return ((t0 + F32(3) * t1) + F32(3) * t2) + t3


def down(S, w, h):
    """Step 3: an (sh, sw, 3) image to (h, w, 3)."""
    sh, sw = S.shape[:2]
    ix = [np.clip(2 * np.arange(w) - 1 + t, 0, sw - 1) for t in range(4)]
    iy = [np.clip(2 * np.arange(h) - 1 + t, 0, sh - 1) for t in range(4)]
    r = _taps4(S[:, ix[0]], S[:, ix[1]], S[:, ix[2]], S[:, ix[3]])
    return _taps4(r[iy[0]], r[iy[1]], r[iy[2]], r[iy[3]]) * F32(0.015625)


def _near_far(n, cn):
    x = np.arange(n)
    near = np.clip(x // 2, 0, cn - 1)
    far = np.clip(np.where(x % 2 == 0, x // 2 - 1, x // 2 + 1), 0, cn - 1)
    return near, far


def up(S, w, h):
    """Step 4: a coarse (ch, cw, 3) image to (h, w, 3)."""
    ch, cw = S.shape[:2]
    nx, fx = _near_far(w, cw)
    ny, fy = _near_far(h, ch)
    r = F32(3) * S[:, nx] + S[:, fx]
    return (F32(3) * r[ny] + r[fy]) * F32(0.0625)


def norm(spread, L):
    """n of step 6."""
    N, pw = 0.0, 1.0
    for _ in range(L):
        N += pw
        pw *= float(F32(spread))
    return F32(1.0 / N)


def bloom(c, threshold=1.0, knee=0.5, limit=64.0, intensity=0.25, spread=1.0, levels=6):
    """Steps 1 to 6 on an (H, W, 3) float32 image.  Returns (out, glare, info); info: sizes, p (the prefiltered frame), raw (the
    glare before its normalisation, Up(U_0, W, H))."""
    c = np.ascontiguousarray(c, F32)
    H, W = c.shape[:2]
    sizes = level_sizes(W, H, levels)
    p = prefilter(c, threshold, knee, limit)
    with np.errstate(all="ignore"):
        D = []
        src = p
        for w, h in sizes:
            src = down(src, w, h)
            D.append(src)
        U = D[-1]
        for k in range(len(sizes) - 2, -1, -1):
            U = D[k] + F32(spread) * up(U, sizes[k][0], sizes[k][1])
        raw = up(U, W, H)
        glare = raw * norm(spread, len(sizes))
        out = c.copy() if float(intensity) == 0.0 else c + F32(intensity) * glare
    return out, glare, dict(sizes=sizes, p=p, raw=raw)


# ---------------------------------------------------------------------------------------------------------------------
# the same, pixel by pixel

def _clampi(v, hi):
    return 0 if v < 0 else (hi if v > hi else v)


def _far(x, cn):
    return _clampi(x // 2 - 1 if x % 2 == 0 else x // 2 + 1, cn - 1)


def _up_loops(S, w, h):
    ch, cw = S.shape[:2]
    out = np.zeros((h, w, 3), F32)
    for y in range(h):
        ny, fy = _clampi(y // 2, ch - 1), _far(y, ch)
        for x in range(w):
            nx, fx = _clampi(x // 2, cw - 1), _far(x, cw)
            for k in range(3):
                rn = F32(3) * S[ny, nx, k] + S[ny, fx, k]
                rf = F32(3) * S[fy, nx, k] + S[fy, fx, k]
                out[y, x, k] = (F32(3) * rn + rf) * F32(0.0625)
    return out


def bloom_loops(c, threshold=1.0, knee=0.5, limit=64.0, intensity=0.25, spread=1.0, levels=6):
    """bloom() in plain loops: (out, glare).  For frames of a few dozen pixels."""
    c = np.ascontiguousarray(c, F32)
    H, W = c.shape[:2]
    threshold, knee, limit, intensity, spread = F32(threshold), F32(knee), F32(limit), F32(intensity), F32(spread)
    with np.errstate(all="ignore"):
        src = np.zeros((H, W, 3), F32)
        for y in range(H):
            for x in range(W):
                px = c[y, x]
                if any((int(v.view(np.uint32)) & 0x7F800000) == 0x7F800000 for v in px):
                    continue
                cp = [v if v > 0 else F32(0) for v in px]
                b = max(max(cp[0], cp[1]), cp[2])
                d = b - threshold
                s = min(max(d + knee, F32(0)), F32(2) * knee)
                q = (s * s) / (F32(4) * knee) if knee > 0 else F32(0)
                m = min(max(q, d), limit)
                f = m / max(b, F32(1e-4)) if m > 0 else F32(0)
                src[y, x] = [v * f for v in cp]
        D = []
        for w, h in level_sizes(W, H, levels):
            sh, sw = src.shape[:2]
            dst = np.zeros((h, w, 3), F32)
            for Y in range(h):
                for X in range(w):
                    for k in range(3):
                        rows = []
                        for j in range(4):
                            t = [src[_clampi(2 * Y - 1 + j, sh - 1), _clampi(2 * X - 1 + i, sw - 1), k] for i in range(4)]
                            rows.append(_taps4(*t))
                        dst[Y, X, k] = _taps4(*rows) * F32(0.015625)
            D.append(dst)
            src = dst
        U = D[-1]
        for k in range(len(D) - 2, -1, -1):
            U = D[k] + spread * _up_loops(U, D[k].shape[1], D[k].shape[0])
        glare = _up_loops(U, W, H) * norm(spread, len(D))
        out = c.copy() if float(intensity) == 0.0 else c + intensity * glare
    return out, glare


# ---------------------------------------------------------------------------------------------------------------------
# test frames

def frame(W, H, seed=1):
    """A seeded (H, W, 3) frame: per pixel b = 2^u, u uniform in [-6, 6]; one random channel is b, the others b times a factor
    in [0.25, 1].  With threshold 1 and knee 0 about half its pixels glare.  The 1 x 1 and 2 x 1 frames hold 4.0."""
    if W * H <= 2:
        return np.full((H, W, 3), 4.0, F32)
    rng = np.random.default_rng(seed * 1000003 + W * 4099 + H)
    b = np.exp2(rng.uniform(-6.0, 6.0, (H, W))).astype(F32)
    c = b[..., None] * rng.uniform(0.25, 1.0, (H, W, 3)).astype(F32)
    lead = rng.integers(0, 3, (H, W))
    np.put_along_axis(c, lead[..., None], b[..., None], axis=-1)
    return np.ascontiguousarray(c, F32)


def with_bad_pixels(c):
    """c with a NaN channel, a +Inf pixel, a -Inf pixel and a pixel of negative channels, spread over the frame (frames of 63
    pixels or more).  Returns (frame, [(y, x)] of the three bad ones, (y, x) of the negative one)."""
    c = c.copy()
    H, W = c.shape[:2]
    at = [(H // 2, W // 2), (0, 0), (H - 1, W - 1)]
    c[at[0]][1] = np.nan
    c[at[1]] = np.inf
    c[at[2]] = -np.inf
    neg = (H // 3, 2 * W // 3)
    c[neg] = (-3.0, 8.0, -0.0)
    return c, at, neg

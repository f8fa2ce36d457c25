"""Binary32 numpy restatement of rz_draw_lines (include/rayzen_hip.h, steps 1 to 7), for tests/test_lines_abi.py (no GPU) and
tests/test_lines_gpu.py.  Every pixel meets every line, in index order: nothing is binned and nothing is culled.

  project     steps 1 to 4 for all lines at once: which are dropped, the screen ends, ia and ib
  draw        steps 5 to 7 over a frame or a crop of it: the blended images, and which pixels some line covered visibly, covered
              occluded, touched
  cull        the rectangle and the reach the kernels cull with, written from the LINE CULL comment of
              rayzen_amd/csrc/hip/rz_lines.hip; meets() is the test a cell or a tile applies

Every array is float32 and every scalar an np.float32, so numpy rounds once per operation as the C code does; numpy fuses
nothing, divides and takes roots correctly rounded, and fmin / fmax drop a NaN as minNum / maxNum do."""
import numpy as np

from present_ref import view_proj
from rayzen_amd._lib import LINE_DTYPE

F32 = np.float32
ONE, HALF, ZERO, B255 = F32(1.0), F32(0.5), F32(0.0), F32(255.0)
BIG = F32(3.0e38)
DEFAULTS = dict(width=1.5, near_w=0.01, depth_bias=2.0 ** -8, hidden_alpha=0.0, smooth=0)
CELL, TILE_W, TILE_H = 128, 32, 8
CELL_R, TILE_R = F32(90.0), F32(16.0)


def m4v(m, x, y, z):
    """Rows 0..3 of the column-major m applied to (x, y, z, 1), each ((m0 x + m4 y) + m8 z) + m12 * 1."""
    return [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * ONE for r in range(4)]


def project(lines, view, proj, fw, fh, near_w=0.01, transforms=None):
    """Steps 1 to 4.  transforms: (n_instances, 16) float32, binding 9's `transform` as it stands on the device; None: no scene.
    Returns a dict of (n,) arrays: drop, sax, say, sbx, sby, ia, ib."""
    lines = np.asarray(lines, LINE_DTYPE).reshape(-1)
    vp = view_proj(view, proj)
    a, b = lines["a"].astype(F32).copy(), lines["b"].astype(F32).copy()
    inst = lines["instance"]
    n_inst = 0 if transforms is None else len(transforms)
    drop = inst >= n_inst                                       # (instance < 0 is below every count)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero((inst >= 0) & ~drop):
            m = np.asarray(transforms[inst[i]], F32).reshape(16)
            a[i] = m4v(m, a[i, 0], a[i, 1], a[i, 2])[:3]
            b[i] = m4v(m, b[i, 0], b[i, 1], b[i, 2])[:3]
        ax, ay, _, aw = m4v(vp, a[:, 0], a[:, 1], a[:, 2])
        bx, by, _, bw = m4v(vp, b[:, 0], b[:, 1], b[:, 2])
        nw = F32(near_w)
        aok, bok = aw >= nw, bw >= nw
        drop = drop | (~aok & ~bok)
        ka, kb = (nw - aw) / (bw - aw), (nw - bw) / (aw - bw)
        only_a, only_b = ~aok & bok, aok & ~bok
        ax2 = np.where(only_a, ax + ka * (bx - ax), ax)
        ay2 = np.where(only_a, ay + ka * (by - ay), ay)
        bx2 = np.where(only_b, bx + kb * (ax - bx), bx)
        by2 = np.where(only_b, by + kb * (ay - by), by)
        aw2, bw2 = np.where(only_a, nw, aw), np.where(only_b, nw, bw)
        rx, ry = F32(fw), F32(fh)
        sax, say = (ax2 / aw2 * HALF + HALF) * rx, (ay2 / aw2 * HALF + HALF) * ry
        sbx, sby = (bx2 / bw2 * HALF + HALF) * rx, (by2 / bw2 * HALF + HALF) * ry
        drop = drop | ~(np.isfinite(sax) & np.isfinite(say) & np.isfinite(sbx) & np.isfinite(sby))
        ia, ib = ONE / aw2, ONE / bw2
    return dict(drop=drop, sax=sax.astype(F32), say=say.astype(F32), sbx=sbx.astype(F32), sby=sby.astype(F32), ia=ia.astype(F32),
                ib=ib.astype(F32))


def seg_t_d(fx, fy, sax, say, abx, aby, L):
    """Step 5's t and d for pixel centres (arrays) and one line (scalars)."""
    with np.errstate(all="ignore"):
        pax, pay = fx - sax, fy - say
        if L == ZERO:
            t = np.zeros_like(fx)
        else:
            t = np.fmin(np.fmax((pax * abx + pay * aby) / L, ZERO), ONE)
        dx, dy = fx - (sax + t * abx), fy - (say + t * aby)
        return t, np.sqrt(dx * dx + dy * dy)


def cull(P, width=1.5, smooth=0):
    """(rect (n, 4): lox, loy, hix, hiy; reach (n,)) of projected lines; a dropped line has the empty rectangle."""
    hw = F32(width) * HALF
    with np.errstate(all="ignore"):
        lox, hix = np.fmin(P["sax"], P["sbx"]), np.fmax(P["sax"], P["sbx"])
        loy, hiy = np.fmin(P["say"], P["sby"]), np.fmax(P["say"], P["sby"])
        mx, my = np.fmax(np.abs(lox), np.abs(hix)), np.fmax(np.abs(loy), np.abs(hiy))
        gx, gy = (hw + ONE) + mx * F32(2.0 ** -21), (hw + ONE) + my * F32(2.0 ** -21)
        if smooth:
            gx, gy = gx + HALF, gy + HALF
        rect = np.stack([lox - gx, loy - gy, hix + gx, hiy + gy], axis=1).astype(F32)
        reach = (np.fmax(gx, gy) + np.fmax(mx, my) * F32(2.0 ** -19)).astype(F32)
    rect[P["drop"]] = (BIG, BIG, -BIG, -BIG)
    reach[P["drop"]] = ZERO
    return rect, reach


def meets(P, rect, reach, i, x0, y0, radius, w=None, h=None):
    """Can line i touch a pixel of the block whose first pixel is (x0, y0)?  radius CELL_R: a 128 x 128 cell; TILE_R: a 32 x 8
    tile.  The rectangle against the block's pixel centres, then the line's distance from their middle against radius + reach."""
    bw, bh = (CELL, CELL) if radius == CELL_R else (TILE_W, TILE_H)
    cx0, cy0 = F32(x0) + HALF, F32(y0) + HALF
    cx1, cy1 = cx0 + F32(bw - 1), cy0 + F32(bh - 1)
    lox, loy, hix, hiy = rect[i]
    if hix < cx0 or lox > cx1 or hiy < cy0 or loy > cy1:
        return False
    abx, aby = P["sbx"][i] - P["sax"][i], P["sby"][i] - P["say"][i]
    with np.errstate(all="ignore"):
        L = abx * abx + aby * aby
        _, d = seg_t_d(np.array([(cx0 + cx1) * HALF], F32), np.array([(cy0 + cy1) * HALF], F32), P["sax"][i], P["say"][i], abx, aby, L)
        return not bool(d[0] > radius + reach[i])


def draw(lines, view, proj, fw, fh, hits=None, rgba8=None, rgb32f=None, transforms=None, crop=None, order=None,
         quantise_each=False, **params):
    """Steps 5 to 7 on a frame of fw x fh pixels; the keyword `width` is the line width of rz_lines_params.  hits: (fh, fw) rz_hit
    records or None; rgba8 (fh, fw, 4) uint8 and rgb32f (fh, fw, 3) float32, each optional, are not modified.  crop = (x0, y0,
    x1, y1): only those pixels are computed and the images returned are the crops.  order: the line indices in blending order (default ascending).  quantise_each: quantise rgba8 after every
    line instead of once (what the definition does NOT do).  Returns (out8, out32, info), info = dict of (h, w) bool masks:
    visible (some line covers the pixel unoccluded), occluded (some line covers it occluded), touched."""
    p = dict(DEFAULTS)
    p.update(params)
    lines = np.asarray(lines, LINE_DTYPE).reshape(-1)
    P = project(lines, view, proj, fw, fh, p["near_w"], transforms)
    vp = view_proj(view, proj)
    x0, y0, x1, y1 = crop if crop is not None else (0, 0, fw, fh)
    xs, ys = np.meshgrid(np.arange(x0, x1, dtype=F32) + HALF, np.arange(y0, y1, dtype=F32) + HALF)
    hw = F32(p["width"]) * HALF
    keep = ONE - F32(p["depth_bias"])
    hidden = F32(p["hidden_alpha"])
    shape = xs.shape
    is_hit = np.zeros(shape, bool)
    wh = np.zeros(shape, F32)
    if hits is not None:
        hc = np.asarray(hits).reshape(fh, fw)[y0:y1, x0:x1]
        is_hit = hc["instance"] >= 0
        X, Y, Z = (hc["point"][..., k].astype(F32) for k in range(3))
        with np.errstate(all="ignore"):
            wh = ((vp[3] * X + vp[7] * Y) + vp[11] * Z) + vp[15]
    out32 = None if rgb32f is None else np.array(rgb32f, F32).reshape(fh, fw, 3)[y0:y1, x0:x1].copy()
    in8 = None if rgba8 is None else np.array(rgba8, np.uint8).reshape(fh, fw, 4)[y0:y1, x0:x1].copy()
    q = None if in8 is None else in8[..., :3].astype(F32) / B255
    touched, visible, occluded = np.zeros(shape, bool), np.zeros(shape, bool), np.zeros(shape, bool)
    with np.errstate(all="ignore"):
        for i in (range(len(lines)) if order is None else order):
            if P["drop"][i]:
                continue
            abx, aby = P["sbx"][i] - P["sax"][i], P["sby"][i] - P["say"][i]
            L = abx * abx + aby * aby
            t, d = seg_t_d(xs, ys, P["sax"][i], P["say"][i], abx, aby, L)
            if p["smooth"]:
                cov = np.fmin(np.fmax((hw + HALF) - d, ZERO), ONE)
                covered = cov > ZERO
            else:
                cov = np.ones(shape, F32)
                covered = d < hw
            if not covered.any():
                continue
            col = lines["color"][i]
            alpha = np.full(shape, F32(col[3]) / B255, F32)
            ws = ONE / (P["ia"][i] + t * (P["ib"][i] - P["ia"][i]))
            occ = covered & is_hit & (ws * keep > wh)
            alpha = np.where(occ, alpha * hidden, alpha) * cov
            touch = covered & (alpha != ZERO)
            visible |= covered & ~occ
            occluded |= occ
            touched |= touch
            k_in = ONE - alpha
            for ch in range(3):
                c = F32(col[ch]) / B255
                if out32 is not None:
                    out32[..., ch] = np.where(touch, out32[..., ch] * k_in + c * alpha, out32[..., ch])
                if q is not None:
                    q[..., ch] = np.where(touch, q[..., ch] * k_in + c * alpha, q[..., ch])
                    if quantise_each:
                        q[..., ch] = np.where(touch, np.rint(np.fmin(np.fmax(q[..., ch], ZERO), ONE) * B255) / B255, q[..., ch])
        out8 = None
        if in8 is not None:
            out8 = in8.copy()
            quant = np.rint(np.fmin(np.fmax(q, ZERO), ONE) * B255).astype(np.uint8)
            out8[..., :3] = np.where(touched[..., None], quant, in8[..., :3])
    return out8, out32, dict(visible=visible, occluded=occluded, touched=touched)

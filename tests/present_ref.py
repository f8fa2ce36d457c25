"""Binary32 numpy restatements around the wireframe overlay of rz_present, for tests/test_present_cases.py (no GPU):

  view_proj, project_corners   the corner projection of FS:243-249 as the oracle and the kernel spell it (one rounding per
                               operation, terms summed left to right)
  cull_rect                    the rectangle outside which the kernel skips a box -- written from the comment above
                               `struct ProjBox` in rayzen_amd/csrc/hip/rz_present.hip, not from project_box's code
  seg_dist                     distanceToSegment (FS:222-226), operation by operation, no FMA
  scene_boxes                  the boxes bvh_mode 0 draws, in the kernel's order: TLAS leaves (thickness 1.5), then the instances'
                               root boxes as they stand in the BLAS, untransformed (thickness 2)

Every array is float32 and every operation takes float32 operands, so numpy rounds once per operation as the C code does."""
import numpy as np

from rayzen_amd import scene as S

F32 = np.float32
BIG = F32(3.0e38)
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]     # FS:232-239: 1 = max
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]  # FS:240-242


def view_proj(view, proj):
    """proj * view, column-major, ((a0*b0 + a1*b1) + a2*b2) + a3*b3."""
    a, b = np.asarray(proj, F32).reshape(16), np.asarray(view, F32).reshape(16)
    out = np.zeros(16, F32)
    for c in range(4):
        for r in range(4):
            out[c * 4 + r] = ((a[r] * b[c * 4] + a[4 + r] * b[c * 4 + 1]) + a[8 + r] * b[c * 4 + 2]) + a[12 + r] * b[c * 4 + 3]
    return out


def project_corners(bmin, bmax, vp, width, height):
    """(sx, sy, w) of the eight corners, float32 (8,) each."""
    bmin, bmax, m = np.asarray(bmin, F32), np.asarray(bmax, F32), np.asarray(vp, F32)
    sx, sy, sw = np.zeros(8, F32), np.zeros(8, F32), np.zeros(8, F32)
    rx, ry, one, half = F32(width), F32(height), F32(1.0), F32(0.5)
    with np.errstate(all="ignore"):
        for k, (cx, cy, cz) in enumerate(CORNERS):
            x, y, z = (bmax if cx else bmin)[0], (bmax if cy else bmin)[1], (bmax if cz else bmin)[2]
            q = [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * one for r in range(4)]
            sw[k] = q[3]
            sx[k] = (q[0] / q[3] * half + half) * rx
            sy[k] = (q[1] / q[3] * half + half) * ry
    return sx, sy, sw


def cull_rect(sx, sy, sw, thickness, error_term=True):
    """(lox, loy, hix, hiy).  error_term=False: the rectangle as it stood before the M * 2^-21 term (thickness + 1 alone)."""
    valid = sw > 0
    if not valid.any():
        return BIG, BIG, -BIG, -BIG                       # empty
    x, y = sx[valid], sy[valid]
    if np.isinf(x).any() or np.isinf(y).any():
        return -BIG, -BIG, BIG, BIG                       # the whole plane
    x, y = x[~np.isnan(x)], y[~np.isnan(y)]               # a NaN coordinate takes no part
    if not (len(x) and len(y)):
        return BIG, BIG, -BIG, -BIG
    g0 = F32(thickness) + F32(1.0)
    with np.errstate(all="ignore"):
        gx = g0 + max(abs(x.min()), abs(x.max())) * F32(2.0 ** -21) if error_term else g0
        gy = g0 + max(abs(y.min()), abs(y.max())) * F32(2.0 ** -21) if error_term else g0
        return x.min() - gx, y.min() - gy, x.max() + gx, y.max() + gy


def outside(rect, px, py):
    lox, loy, hix, hiy = rect
    return (px < lox) | (px > hix) | (py < loy) | (py > hiy)


def seg_dist(px, py, ax, ay, bx, by):
    """All arguments float32 arrays (broadcast).  clamp is min(max(x, 0), 1) with minNum / maxNum: a NaN quotient gives t = 0."""
    px, py, ax, ay, bx, by = (np.asarray(v, F32) for v in (px, py, ax, ay, bx, by))
    with np.errstate(all="ignore"):
        abx, aby, pax, pay = bx - ax, by - ay, px - ax, py - ay
        t = np.fmin(np.fmax((pax * abx + pay * aby) / (abx * abx + aby * aby), F32(0.0)), F32(1.0))
        dx, dy = px - (ax + t * abx), py - (ay + t * aby)
        return np.sqrt(dx * dx + dy * dy)


def scene_boxes(arrays):
    """[(name, bmin, bmax, thickness)] of bvh_mode 0."""
    out = []
    for k, nd in enumerate(arrays[S.BIND_TLAS_NODES]):
        if nd["count"] > 0:
            out.append((f"tlas{k}", nd["boundsMin"].copy(), nd["boundsMax"].copy(), 1.5))
    for k, inst in enumerate(arrays[S.BIND_INSTANCES]):
        root = arrays[S.BIND_BLAS_NODES][inst["blasNodeOffset"]]
        out.append((f"root{k}", root["boundsMin"].copy(), root["boundsMax"].copy(), 2.0))
    return out


def valid_corners(arrays, view, proj, width, height):
    """Per box of scene_boxes, how many corners have w > 0."""
    vp = view_proj(view, proj)
    return [int((project_corners(mn, mx, vp, width, height)[2] > 0).sum()) for _, mn, mx, _ in scene_boxes(arrays)]


def pixel_centres(width, height):
    xs, ys = np.meshgrid(np.arange(width, dtype=F32) + F32(0.5), np.arange(height, dtype=F32) + F32(0.5))
    return xs, ys

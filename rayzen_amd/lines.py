"""Line sets for Renderer.draw_lines (include/rayzen_hip.h: rz_draw_lines), pure numpy: each function returns an array of
LINE_DTYPE records (rz_line: ends a and b, colour bytes r, g, b, alpha, instance < 0 for world space).  Concatenate them with
numpy.concatenate; the lines of one call are blended in array order."""
import numpy as np

from ._lib import LINE_DTYPE

BOX_CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]   # 1 = the max plane
BOX_EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def color_bytes(color):
    """(r, g, b, a) as uint8: a sequence of 3 or 4 numbers, floats in 0..1 (scaled and rounded) or integers 0..255; alpha
    defaults to opaque."""
    c = list(color)
    if len(c) not in (3, 4):
        raise ValueError(f"a colour has 3 or 4 components, got {len(c)}")
    if all(isinstance(v, (int, np.integer)) for v in c):
        c = [int(v) for v in c] + [255] * (4 - len(c))
    else:
        c = [int(round(min(max(float(v), 0.0), 1.0) * 255.0)) for v in c] + [255] * (4 - len(c))
    if min(c) < 0 or max(c) > 255:
        raise ValueError(f"colour bytes outside 0..255: {c}")
    return np.array(c, np.uint8)


def segments(a, b, color, instance=-1):
    """Lines from (n, 3) ends a and b, one colour and one instance for all."""
    a, b = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
    if len(a) != len(b):
        raise ValueError(f"{len(a)} first ends, {len(b)} second ends")
    out = np.zeros(len(a), LINE_DTYPE)
    out["a"], out["b"] = a, b
    out["color"] = color_bytes(color)
    out["instance"] = int(instance)
    return out


def grid(size, step, color, y=0.0):
    """A ground grid in the plane y = `y`: the lines x = k * step and z = k * step for |k * step| <= size, each from -size to size;
    first the lines along z in ascending x, then the lines along x in ascending z."""
    size, step = float(np.float32(size)), float(np.float32(step))      # (as Overlay.h: gridLines takes them)
    if not (size > 0.0 and step > 0.0):
        raise ValueError("grid: size and step must be positive")
    k = int(np.floor(size / step + 1e-6))
    at = np.arange(-k, k + 1, dtype=np.float64) * step
    n = len(at)
    a, b = np.zeros((2 * n, 3)), np.zeros((2 * n, 3))
    a[:, 1] = b[:, 1] = float(y)
    a[:n, 0] = b[:n, 0] = at
    a[:n, 2], b[:n, 2] = -size, size
    a[n:, 2] = b[n:, 2] = at
    a[n:, 0], b[n:, 0] = -size, size
    return segments(a, b, color)


def box(bmin, bmax, color, instance=-1):
    """The 12 edges of an axis-aligned box, rz_present's corner and edge order; instance >= 0: in that instance's space."""
    lo, hi = np.asarray(bmin, np.float32).reshape(3), np.asarray(bmax, np.float32).reshape(3)
    corners = np.array([[hi[k] if c[k] else lo[k] for k in range(3)] for c in BOX_CORNERS], np.float32)
    return segments(corners[[e[0] for e in BOX_EDGES]], corners[[e[1] for e in BOX_EDGES]], color, instance)


def axes(origin, length, instance=-1):
    """Gizmo axes: x red, y green, z blue, from `origin`."""
    o = np.asarray(origin, np.float32).reshape(3)
    out = []
    for k, col in enumerate(((255, 48, 48), (48, 255, 48), (64, 96, 255))):
        e = o.copy()
        e[k] = e[k] + np.float32(length)
        out.append(segments(o[None], e[None], col, instance))
    return np.concatenate(out)


def frustum(inv_view, inv_proj, color):
    """The 12 edges of a camera's frustum from its inverse matrices (column-major, 16 floats each): the clip-space cube's
    corners through inv_proj, the perspective divide and inv_view; near rectangle, far rectangle, then the four sides."""
    iv = np.asarray(inv_view, np.float64).reshape(4, 4).T
    ip = np.asarray(inv_proj, np.float64).reshape(4, 4).T
    corners = []
    for c in BOX_CORNERS:
        q = ip @ np.array([2.0 * c[0] - 1.0, 2.0 * c[1] - 1.0, 2.0 * c[2] - 1.0, 1.0])
        corners.append((iv @ (q / q[3]))[:3])
    corners = np.array(corners)
    return segments(corners[[e[0] for e in BOX_EDGES]], corners[[e[1] for e in BOX_EDGES]], color)


def mesh_edges(triangles, color, instance=-1):
    """The unique undirected edges of a triangle array (scene.TRIANGLE records, or (n, 3, 3) vertices), each once, in the order
    of their first appearance (edges v0-v1, v1-v2, v2-v0 of each triangle in turn); vertices are the same when their three
    floats are, bit for bit."""
    t = np.asarray(triangles)
    if t.dtype.names:
        v = np.stack([t["v0"], t["v1"], t["v2"]], axis=1).astype(np.float32)
    else:
        v = np.asarray(t, np.float32).reshape(-1, 3, 3)
    flat = np.ascontiguousarray(v.reshape(-1, 3))
    _, vid = np.unique(flat.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    vid = vid.reshape(-1, 3)
    e0 = np.stack([vid[:, 0], vid[:, 1], vid[:, 2]], axis=1).reshape(-1)           # per triangle: v0-v1, v1-v2, v2-v0
    e1 = np.stack([vid[:, 1], vid[:, 2], vid[:, 0]], axis=1).reshape(-1)
    key = np.minimum(e0, e1).astype(np.int64) * (int(vid.max()) + 1 if len(vid) else 1) + np.maximum(e0, e1)
    _, first = np.unique(key, return_index=True)
    first = np.sort(first)
    src = np.arange(len(flat)).reshape(-1, 3)
    a_idx = src.reshape(-1)[first]                                                  # corner k of triangle j ...
    b_idx = np.stack([src[:, 1], src[:, 2], src[:, 0]], axis=1).reshape(-1)[first]  # ... and the corner after it
    return segments(flat[a_idx], flat[b_idx], color, instance)

"""One comparison of an editor frame with RayZen's own raster pass (tests/golden/glref_editor_*.npz), shared by the CPU suite
(tests/test_glref_editor.py) and the GPU suite (tests/test_glref_editor_gpu.py).

The fixtures hold what llvmpipe drew with editor_vertex.glsl + editor_fragment.glsl and a depth test (oracle/glref, editor
mode): the colour (float32 rgb and RGBA8) and, from an ID pass over the same fragments, the object, gl_PrimitiveID and the
24-bit window depth of every pixel.  A candidate -- rz_render_editor's frame, or the oracle's closest hits shaded by
editor_ref.py -- is the instance, mesh-local triangle, hit point, normal, material and colour per pixel.  classify() puts EVERY
pixel into exactly one class, and a pixel in none fails the comparison; there is no budget of pixels allowed to be off.

  agree   the same instance and triangle, or background in both.  Background is the clear colour exactly (both sides) and
          its RGBA8 within 1 LSB.  A surface's colour c must satisfy |c - gl| <= A + R |gl| + K S_p per channel, and its RGBA8
          be within 1 LSB of GL's.  S_p = |shade64 - shade32| (editor_ref.shade in binary64 and in binary32, at the candidate's
          hit): how far binary32 arithmetic alone moves this pixel's colour.  GL evaluates the shader in binary32 (in its own
          order, from its own interpolated inputs), so near a sharp highlight (roughness clamped to 0.05) llvmpipe's colour is
          itself far from the formula's exact value, and S_p says how far.  The constants are measured on the seven frames.
          With R = 2e-5 and K = 0, highlight pixels exceed the bound by up to 1.8x (skewed, cornell, coverage).  R = 6e-5 is set
          by a bright pixel of the coverage scene (colour 1.03, S_p 2.8e-7) that differs by 2.7e-5 relative: the raster pass's
          interpolated inputs differ from the ray's hit by more than binary32 arithmetic alone moves them.  With A = 2e-6,
          R = 6e-5 and K = 8 the worst pixel of all frames uses 0.49 of its bound, for the oracle and rz_render_editor alike.
          The power checks' misreadings move pixels by far more: ambient 0.0305 changes a dark pixel by 1.7 %.
  edge    a different triangle, or a hit against background: allowed only if the pixel centre lies within DELTA pixels of an
          edge of either triangle's screen projection (float64, after clipping the triangle to the near and far planes;
          a far-plane cut counts as an edge).  llvmpipe snaps vertices to 1/256 px (8 sub-pixel bits), which moves an edge by at
          most 1/512 sqrt(2) = 0.0028 px; DELTA = 1/256.  Measured: the farthest edge pixel of all frames lies 0.0027 px from
          its edge (coverage): the snapping is real, and DELTA = 1/1024 would fail there.  That pixel is a sliver of a blob
          that the render's own triangle test skips at a grazing angle (|det| < 1e-4 in object space, FS:398) while the
          rasteriser draws it; its projection is thinner than 0.003 px.
  near    the pixel ray's first hit lies in front of the near plane (cand["front"]; without it no pixel is in this class),
          the outcome differs, and the pixel centre lies within DELTA of where either triangle's clipped polygon meets the
          near plane.  The ray cast restarts its query there from a rounded point; the rasteriser clips the triangle.
  tie     a different triangle whose window depth at the pixel centre (float64) is within one 24-bit quantum of the other's:
          which of two equal depths wins is the order of drawing for GL_LESS, the query's order for the ray cast.
"""
import json
import os
import types

import numpy as np

import editor_ref as ER
from rayzen_amd import scene as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NAMES = sorted(f[len("glref_editor_"):-len(".npz")] for f in os.listdir(GOLDEN) if f.startswith("glref_editor_") and f.endswith(".npz"))

A, R, K = 2e-6, 6e-5, 8.0
DELTA = 1.0 / 256.0
QUANTUM = 1.0 / (2 ** 24 - 1)
CLASSES = ("agree", "edge", "near", "tie", "skipped", "unclassified")


def load(name):
    """-> (scene shim with .arrays / .camera / .lights / .materials, [dict(W, H, num_lights)], [dict of GL outputs], GL string)"""
    z = np.load(os.path.join(GOLDEN, f"glref_editor_{name}.npz"))
    arrays = {b: np.frombuffer(z[f"b{b}"].tobytes(), dt).copy() for b, dt in S.BINDING_DTYPES.items()}
    cam = types.SimpleNamespace(view=z["cam_view"], proj=z["cam_proj"], inv_view=z["cam_inv_view"], inv_proj=z["cam_inv_proj"],
                                position=z["cam_pos"])
    sc = types.SimpleNamespace(arrays=arrays, camera=cam, lights=arrays[S.BIND_LIGHTS], materials=arrays[S.BIND_MATERIALS])
    renders = json.loads(str(z["renders"]))
    outs = [{key: z[f"{key}{k}"] for key in ("rgb", "rgba8", "object", "prim", "depth")} for k in range(len(renders))]
    return sc, renders, outs, str(z["gl"])


def cases():
    return [(name, k) for name in NAMES for k in range(len(load(name)[1]))]


def _mat(m16):
    return np.asarray(m16, np.float64).reshape(4, 4).T          # column-major 16 -> row-major 4 x 4


def world_triangle(sc, inst, tri):
    """The triangle's world vertices (3, 3) in float64."""
    I = sc.arrays[S.BIND_INSTANCES][inst]
    t = sc.arrays[S.BIND_TRIANGLES][int(I["globalTriOffset"]) + tri]
    M = _mat(I["transform"])
    v = np.stack([np.asarray(t[k], np.float64) for k in ("v0", "v1", "v2")])
    return v @ M[:3, :3].T + M[:3, 3]


def _clip_poly(sc, verts):
    """Clip-space polygon of a world triangle cut to -w <= z <= w; each edge tagged 0 (a side of the triangle), 1 (the
    near-plane cut) or 2 (the far-plane cut).  -> [(clip vertex (4,), tag of the edge that leaves it)]"""
    PV = _mat(sc.camera.proj) @ _mat(sc.camera.view)
    poly = [(PV @ np.append(v, 1.0), 0) for v in verts]
    for tag, sign in ((1, 1.0), (2, -1.0)):             # near: z + w >= 0; far: w - z >= 0
        out = []
        for i, (p, e) in enumerate(poly):
            q = poly[(i + 1) % len(poly)][0]
            dp, dq = p[3] + sign * p[2], q[3] + sign * q[2]
            if dp >= 0:
                out.append((p, e))
            if (dp >= 0) != (dq >= 0):
                x = p + (q - p) * (dp / (dp - dq))
                out.append((x, tag if dp >= 0 else e))      # leaving: x runs on along the cut; entering: along the side
        poly = out
        if not poly:
            break
    return poly


def edge_distances(sc, W, H, inst, tri, px, py):
    """Distance in pixels from the centre of pixel (px, py) to the nearest side / far-plane cut, and to the nearest near-plane
    cut, of the triangle's clipped screen projection (inf where there is none)."""
    poly = _clip_poly(sc, world_triangle(sc, inst, tri))
    c = np.array([px + 0.5, py + 0.5])
    best = [np.inf, np.inf]
    for i, (p, tag) in enumerate(poly):
        q = poly[(i + 1) % len(poly)][0]
        a = np.array([(p[0] / p[3] + 1) * 0.5 * W, (p[1] / p[3] + 1) * 0.5 * H])
        b = np.array([(q[0] / q[3] + 1) * 0.5 * W, (q[1] / q[3] + 1) * 0.5 * H])
        ab = b - a
        s = np.clip(np.dot(c - a, ab) / max(np.dot(ab, ab), 1e-300), 0.0, 1.0)
        d = float(np.linalg.norm(c - (a + s * ab)))
        k = 1 if tag == 1 else 0
        best[k] = min(best[k], d)
    return best


def window_depth(sc, W, H, inst, tri, px, py):
    """Window depth (float64) of the triangle's plane under the centre of pixel (px, py), or nan if the ray misses the plane."""
    v = world_triangle(sc, inst, tri)
    ivp = np.linalg.inv(_mat(sc.camera.proj) @ _mat(sc.camera.view))
    ndc = np.array([(px + 0.5) / W * 2 - 1, (py + 0.5) / H * 2 - 1])
    a, b = ivp @ np.array([ndc[0], ndc[1], -1.0, 1.0]), ivp @ np.array([ndc[0], ndc[1], 1.0, 1.0])
    o, d = a[:3] / a[3], b[:3] / b[3] - a[:3] / a[3]
    n = np.cross(v[1] - v[0], v[2] - v[0])
    den = np.dot(n, d)
    if den == 0:
        return np.nan
    p = o + d * (np.dot(n, v[0] - o) / den)
    c = _mat(sc.camera.proj) @ _mat(sc.camera.view) @ np.append(p, 1.0)
    return (c[2] / c[3] + 1) * 0.5


def _glm_row(m, r, x, y, z, w):
    """GLM's mat4 * vec4, row r, in binary32 (rz_editor.hip: glm_row)."""
    m = np.asarray(m, np.float32)
    return (m[r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r] * w)


def clip_zw(cam, p):
    """rz_editor.hip's clip_zw for points p (n, 3): proj * (view * (p, 1)), rows 2 and 3, binary32.  A point is kept iff
    -w <= z <= w; z < -w lies in front of the near plane."""
    x, y, z = (np.asarray(p)[:, i].astype(np.float32) for i in range(3))
    one = np.float32(1.0)
    e = [_glm_row(cam.view, r, x, y, z, one) for r in range(4)]
    return _glm_row(cam.proj, 2, *e), _glm_row(cam.proj, 3, *e)


def sensitivity(sc, points, normals, mats, num_lights, ambient=ER.AMBIENT):
    """S_p: |shade64 - shade32| per channel at the candidate's hits."""
    args = (points, normals, mats, sc.materials, sc.lights, sc.camera.position, num_lights, ambient)
    return np.abs(ER.shade(*args) - ER.shade(*args, dtype=np.float32).astype(np.float64))


def classify(sc, render, gl, cand, skip=None, delta=DELTA, k=K):
    """cand: dict of (H, W[, c]) arrays instance, triangle, point, normal, material, rgb, rgba8 (instance -1: background),
    and optionally front: the first hit along the pixel ray (before any clipping) lies in front of the near plane.
    skip: (H, W) bool, pixels the candidate does not decide (left out, counted as 'skipped').
    Returns a report: counts per class, the worst agree-pixel error relative to its bound, the farthest edge / near pixel from
    its edge, and the unclassified pixels (y, x, why) -- the first 20."""
    W, H, nl = render["W"], render["H"], render["num_lights"]
    cls = np.full((H, W), -1, np.int8)
    skip = np.zeros((H, W), bool) if skip is None else skip
    ci, ct = cand["instance"], cand["triangle"]
    gi, gt = gl["object"], gl["prim"]
    bad = []
    cls[skip] = CLASSES.index("skipped")
    both_bg = (ci < 0) & (gi < 0) & ~skip
    same = (ci >= 0) & (ci == gi) & (ct == gt) & ~skip
    clear = np.asarray(ER.CLEAR[:3], np.float32)
    ok_bg = both_bg & (cand["rgb"] == clear).all(-1) & (gl["rgb"] == clear).all(-1) & \
        (np.abs(cand["rgba8"].astype(int) - gl["rgba8"].astype(int)) <= 1).all(-1)
    for y, x in zip(*np.nonzero(both_bg & ~ok_bg)):
        if len(bad) >= 20:
            bad.append((int(y), int(x), ""))
            continue
        bad.append((int(y), int(x), f"background: candidate {cand['rgb'][y, x]} / {cand['rgba8'][y, x]}, GL {gl['rgb'][y, x]} / {gl['rgba8'][y, x]}"))
    cls[ok_bg] = 0
    worst = 0.0
    if same.any():
        p, n, m = cand["point"][same], cand["normal"][same], cand["material"][same]
        sp = sensitivity(sc, p, n, m, nl)
        g = gl["rgb"][same].astype(np.float64)
        err = np.abs(cand["rgb"][same].astype(np.float64) - g)
        bound = A + R * np.abs(g) + k * sp
        ratio = (err / bound).max(-1)
        worst = float(ratio.max())
        ok8 = (np.abs(cand["rgba8"][same].astype(int) - gl["rgba8"][same].astype(int)) <= 1).all(-1)
        ok = (ratio <= 1.0) & ok8
        ys, xs = np.nonzero(same)
        cls[ys[ok], xs[ok]] = 0
        for j in np.flatnonzero(~ok):
            if len(bad) >= 20:          # (the rest are counted, not described)
                bad.append((int(ys[j]), int(xs[j]), ""))
                continue
            bad.append((int(ys[j]), int(xs[j]), f"colour {cand['rgb'][ys[j], xs[j]]} vs GL {gl['rgb'][ys[j], xs[j]]}: {ratio[j]:.3g} x bound "
                        f"(S_p {sp[j].max():.3g}), rgba8 {cand['rgba8'][ys[j], xs[j]]} vs {gl['rgba8'][ys[j], xs[j]]}"))
    far_edge = far_near = 0.0
    front = cand.get("front")
    for y, x in zip(*np.nonzero(~skip & ~both_bg & ~same)):
        tris = [(int(a), int(b)) for a, b in ((ci[y, x], ct[y, x]), (gi[y, x], gt[y, x])) if a >= 0]
        d = [edge_distances(sc, W, H, a, b, x, y) for a, b in tris]
        de, dn = min(e[0] for e in d), min(e[1] for e in d)
        if de <= delta:
            cls[y, x] = 1
            far_edge = max(far_edge, de)
        elif front is not None and front[y, x] and dn <= delta:
            cls[y, x] = 2
            far_near = max(far_near, dn)
        elif len(tris) == 2 and abs(window_depth(sc, W, H, *tris[0], x, y) - window_depth(sc, W, H, *tris[1], x, y)) <= QUANTUM:
            cls[y, x] = 3
        else:
            bad.append((int(y), int(x), f"candidate {tris[0] if ci[y, x] >= 0 else 'background'} vs GL "
                        f"{(int(gi[y, x]), int(gt[y, x])) if gi[y, x] >= 0 else 'background'}: {de:.4f} px from an edge, {dn:.4f} from the near cut"))
    for y, x, _ in bad:
        cls[y, x] = CLASSES.index("unclassified")
    assert (cls >= 0).all()
    counts = {c: int((cls == i).sum()) for i, c in enumerate(CLASSES)}
    return dict(counts=counts, worst=worst, far_edge=far_edge, far_near=far_near, bad=bad[:20], classes=cls)


def summary(rep):
    c = rep["counts"]
    return (" ".join(f"{k} {v}" for k, v in c.items() if v) + f"; worst agree {rep['worst']:.3g} x bound, edge pixels within "
            f"{rep['far_edge']:.4f} px, near within {rep['far_near']:.4f} px" + (f"; unclassified e.g. {rep['bad'][:3]}" if rep["bad"] else ""))

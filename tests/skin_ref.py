"""rz_skin_pose's posed triangle (include/rayzen_hip.h, "THE POSED TRIANGLE") restated in numpy float32, and the rigs the skinning
tests run.  Every product and every sum is its own numpy operation on float32 arrays, so each is rounded once and nothing is
fused -- by construction, not by a compiler flag.  The host library (rzh_skin_triangles) and the device kernel are both held to
these bytes."""
import numpy as np

from rayzen_amd import scene as S

CORNERS = ("v0", "v1", "v2")


class Rig:
    """One test rig: rest pose, per-triangle skin (or None), bones (n_bones x 16, column-major), morph targets [k, n] (or None)
    and their weights."""

    def __init__(self, name, rest, skin=None, bones=None, morphs=None, morph_weights=None):
        self.name, self.rest, self.skin = name, np.ascontiguousarray(rest, S.TRIANGLE), skin
        self.bones = None if bones is None else np.ascontiguousarray(bones, np.float32).reshape(-1, 16)
        self.n_bones = 0 if self.bones is None else len(self.bones)
        self.morphs = None if morphs is None else np.ascontiguousarray(morphs, S.MORPH_TRIANGLE).reshape(-1, len(rest))
        self.n_morphs = 0 if self.morphs is None else len(self.morphs)
        self.morph_weights = None if morph_weights is None else np.ascontiguousarray(morph_weights, np.float32)

    def sub(self, lo, hi):
        """The rig of the triangles [lo, hi)."""
        return Rig(f"{self.name}[{lo}:{hi}]", self.rest[lo:hi], None if self.skin is None else self.skin[lo:hi], self.bones,
                   None if self.morphs is None else self.morphs[:, lo:hi], self.morph_weights)

    def pose(self):
        return pose(self.rest, self.skin, self.bones, self.morphs, self.morph_weights)


def pose(rest, skin=None, bones=None, morphs=None, morph_weights=None):
    """The specification.  rest: TRIANGLE[n]; skin: SKIN_TRIANGLE[n] or None; bones: [n_bones, 16]; morphs: MORPH_TRIANGLE[k, n]."""
    out = np.ascontiguousarray(rest, S.TRIANGLE).copy()         # pads and materialIndex are the rest triangle's
    n_morphs = 0 if morphs is None else len(morphs)
    with np.errstate(all="ignore"):
        for c, field in enumerate(CORNERS):
            p = out[field].astype(np.float32).copy()            # [n, 3]
            for k in range(n_morphs):                           # every target, a zero weight included
                w = np.float32(morph_weights[k])
                prod = (w * morphs[k]["d"][:, c, :3]).astype(np.float32)
                p = (p + prod).astype(np.float32)
            if skin is not None:
                word = skin["bones"][:, c]
                o = p.copy()
                kept_any = np.zeros(len(p), bool)
                for j in range(4):
                    w = skin["weights"][:, c, j].astype(np.float32)
                    kept = ~(w == np.float32(0.0))              # "compares equal to 0": -0.0 is skipped, NaN is kept
                    idx = np.where(kept, (word >> np.uint32(8 * j)) & np.uint32(255), 0).astype(np.int64)     # a skipped bone is not read
                    m = bones[idx]                              # [n, 16], column-major
                    q = np.empty_like(p)
                    for r in range(3):
                        a = (m[:, r] * p[:, 0]).astype(np.float32)
                        b = (m[:, 4 + r] * p[:, 1]).astype(np.float32)
                        ab = (a + b).astype(np.float32)
                        cc = (m[:, 8 + r] * p[:, 2]).astype(np.float32)
                        q[:, r] = ((ab + cc).astype(np.float32) + m[:, 12 + r]).astype(np.float32)
                    wq = (w[:, None] * q).astype(np.float32)
                    summed = (o + wq).astype(np.float32)
                    first = kept & ~kept_any
                    later = kept & kept_any
                    o = np.where(first[:, None], wq, np.where(later[:, None], summed, o))
                    kept_any |= kept
                p = np.where(kept_any[:, None], o, p)
            out[field] = p
    return out


# ---- the rigs ---------------------------------------------------------------------------------------------------------------

def _corners(tris):
    return np.stack([tris[f] for f in CORNERS], axis=1)         # [n, 3, 3]


def _rot_z(angle, pivot=(0.0, 0.0, 0.0)):
    c, s = np.float32(np.cos(angle)), np.float32(np.sin(angle))
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    pv = np.asarray(pivot, np.float32)
    m[:3, 3] = pv - m[:3, :3] @ pv
    return m.T.reshape(16).copy()                               # column-major


def bend_skin(tris):
    """Two bones, weights (1 - t, t) from the corner's height t in [0, 1]: at the bottom and the top one of them is exactly 0."""
    v = _corners(tris)
    y = v[:, :, 1]
    lo, hi = np.float32(y.min()), np.float32(y.max())
    t = np.clip((y - lo) / max(np.float32(hi - lo), np.float32(1e-20)), 0, 1).astype(np.float32)
    skin = np.zeros(len(tris), S.SKIN_TRIANGLE)
    skin["bones"] = S.pack_bones(np.broadcast_to(np.array([0, 1, 0, 0]), (len(tris), 3, 4)))
    skin["weights"][:, :, 0] = np.float32(1.0) - t
    skin["weights"][:, :, 1] = t
    return skin, (float(lo), float(hi))


def bend_bones(tris_range, angle):
    lo, hi = tris_range
    return np.stack([S.identity(), _rot_z(angle, (0.0, 0.5 * (lo + hi), 0.0))])


def bend(tris, angle=0.5):
    skin, rng = bend_skin(tris)
    return Rig("bend", tris, skin, bend_bones(rng, angle))


def random_bones(rng, n_bones):
    """Affine bones: rotations, shears, mirrors, and translations from tiny to 1e3."""
    out = np.zeros((n_bones, 16), np.float32)
    for b in range(n_bones):
        kind = b % 4
        a = rng.normal(size=(3, 3))
        qm, _ = np.linalg.qr(a)
        if np.linalg.det(qm) < 0:
            qm[:, 0] = -qm[:, 0]                                # a rotation
        if kind == 1:
            qm = qm @ (np.eye(3) + np.triu(rng.uniform(-0.7, 0.7, (3, 3)), 1))      # ... sheared
        elif kind == 2:
            qm = qm @ np.diag([-1.0, 1.0, 1.0])                 # ... mirrored
        elif kind == 3:
            qm = qm * rng.uniform(0.5, 1.5)
        m = np.eye(4)
        m[:3, :3] = qm
        m[:3, 3] = rng.choice([-1.0, 1.0], 3) * rng.uniform(0.5, 1.0, 3) * 10.0 ** (3, -2, 0, 1, 2, -1)[b % 6]    # bone 0: to 1e3
        m[3] = rng.normal(size=4)                               # the fourth row is ignored: garbage on purpose
        out[b] = m.T.reshape(16).astype(np.float32)
    return out


def random_skin(rng, n, n_bones, wild=False):
    """Corners with 0, 1, 2, 3 and 4 nonzero weights; a skipped slot names bone 255 (outside every rig of fewer bones)."""
    idx = rng.integers(0, n_bones, (n, 3, 4))
    w = rng.uniform(0.05, 1.0, (n, 3, 4)).astype(np.float32)
    count = np.arange(n * 3).reshape(n, 3) % 5                  # 0..4 kept influences, every count present from 2 triangles on
    order = np.argsort(rng.random((n, 3, 4)), axis=2)           # which slots are kept: any, not the leading ones
    rank = np.argsort(order, axis=2)
    kept = rank < count[:, :, None]
    if wild:                                                    # unnormalised and negative
        w = (w * rng.choice(np.array([-2.5, -1.0, 0.3, 1.0, 4.0], np.float32), (n, 3, 4))).astype(np.float32)
    else:
        tot = np.where(kept, w, 0).sum(axis=2, keepdims=True)
        w = (w / np.where(tot > 0, tot, 1)).astype(np.float32)
    w = np.where(kept, w, np.float32(0.0)).astype(np.float32)
    neg_zero = (~kept) & (rng.random((n, 3, 4)) < 0.3)
    w[neg_zero] = np.float32(-0.0)                              # compares equal to 0: skipped too
    idx = np.where(kept, idx, 255)
    skin = np.zeros(n, S.SKIN_TRIANGLE)
    skin["bones"] = S.pack_bones(idx)
    skin["pad"] = 0xDEADBEEF                                    # ignored
    skin["weights"] = w
    return skin


def random_morphs(rng, tris, k, scale=0.2):
    m = np.zeros((k, len(tris)), S.MORPH_TRIANGLE)
    m["d"][..., :3] = rng.normal(scale=scale, size=(k, len(tris), 3, 3)).astype(np.float32)
    m["d"][..., 3] = rng.normal(size=(k, len(tris), 3)).astype(np.float32)          # the 4th word is ignored
    flat = m["d"].reshape(-1, 4)
    flat[::7, 0] = np.float32(-0.0)                             # -0.0 deltas
    flat[3::11, :3] = np.float32(0.0)
    return m


def odd_rest(tris):
    """The mesh with some coordinates replaced by -0.0 and by denormals."""
    t = tris.copy()
    for k, f in enumerate(CORNERS):
        v = t[f]
        v[k::9, 0] = np.float32(-0.0)
        v[k + 1::13, 1] = np.float32(1e-41)
        v[k + 2::17, 2] = np.float32(-3e-45)
        t[f] = v
    t["pad0"], t["pad1"], t["pad2"] = np.float32(7.25), np.float32(-1.5), np.float32(3e-41)
    t["tail_pad"] = np.array([11, -22, 33], np.int32)
    return t


def rigs(tris, seed=5):
    """Every generator of the issue on one mesh."""
    n = len(tris)
    v = _corners(tris)
    extent = float(np.abs(v).max()) if n else 1.0
    rng = np.random.default_rng(seed + n)
    out = [bend(tris)]
    for nb in (1, 2, 7, 256):
        out.append(Rig(f"random{nb}", tris, random_skin(rng, n, nb), random_bones(rng, nb)) )
    out.append(Rig("wild_weights", tris, random_skin(rng, n, 7, wild=True), random_bones(rng, 7)) )
    out.append(Rig("odd_rest", odd_rest(tris), random_skin(rng, n, 2), random_bones(rng, 2)) )
    out.append(Rig("morph1", tris, morphs=random_morphs(rng, tris, 1, 0.1 * extent), morph_weights=[0.75]))
    out.append(Rig("morph3", odd_rest(tris), morphs=random_morphs(rng, tris, 3, 0.1 * extent), morph_weights=[0.5, 0.0, -1.25]))
    out.append(Rig("skin7_morph1", tris, random_skin(rng, n, 7), random_bones(rng, 7), random_morphs(rng, tris, 1, 0.1 * extent), [-0.0]))
    out.append(Rig("skin256_morph3", tris, random_skin(rng, n, 256, wild=True), random_bones(rng, 256),
                   random_morphs(rng, tris, 3, 0.1 * extent), [1.0, 0.0, 0.3]))
    return out

"""Kernel time (rz_skin_last_kernel_ms: device events around the launch, median of 25) of the three instantiations of
rz_skin_tris on rigs of growing weight -- a two-bone bend, four influences per corner over 16 and over 256 random bones,
two morph targets, both halves -- at 69 312 and 1 002 252 triangles.

    python profiles/skin/kernel_variants.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import skin_ref as K  # noqa: E402
from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer  # noqa: E402

for n in (76, 289):
    cube, blob = S.make_cube(4), S.make_blob(n, 2.8, 0)
    objects = [(0, S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0))), (1, S.translate(S.identity(), (0.0, 2.0, 0.0)))]
    r = Renderer(0)
    r.upload_scene_built_on_device([cube, blob], objects, S.reference_materials(), S.reference_lights())
    rng = np.random.default_rng(1)
    N = len(blob)

    def full_skin(nb):
        sk = np.zeros(N, S.SKIN_TRIANGLE)
        sk["bones"] = S.pack_bones(rng.integers(0, nb, (N, 3, 4)))
        w = rng.uniform(0.1, 1, (N, 3, 4)).astype(np.float32)
        sk["weights"] = w / w.sum(axis=2, keepdims=True)
        return sk

    def near_identity(nb):
        return np.tile(S.identity(), (nb, 1)) + (rng.normal(size=(nb, 16)) * 1e-3).astype(np.float32)

    bend_skin, yr = K.bend_skin(blob)
    mor = np.zeros((2, N), S.MORPH_TRIANGLE)
    mor["d"] = rng.normal(scale=0.01, size=(2, N, 3, 4)).astype(np.float32)
    rigs = [("bend: 2 bones, 2 influences", bend_skin, K.bend_bones(yr, 0.3), None, None, 192),
            ("4 influences, 16 random bones", full_skin(16), near_identity(16), None, None, 192),
            ("4 influences, 256 random bones", full_skin(256), near_identity(256), None, None, 192),
            ("morph only, 2 targets", None, None, mor, [0.5, 0.25], 224),
            ("bend + 2 targets", bend_skin, K.bend_bones(yr, 0.3), mor, [0.5, 0.25], 288)]
    for name, sk, bones, mo, mw, bytes_per_tri in rigs:
        rid = r.skin_create(12, blob, sk, 0 if bones is None else len(bones), mo)
        ms = []
        for k in range(26):
            r.skin_pose(rid, bones, mw)
            if k:
                ms.append(r.skin_last_kernel_ms())
        r.skin_destroy(rid)
        med = float(np.median(ms))
        print(f"[skin] {N} triangles, {name}: {med:.4f} ms (min {np.min(ms):.4f}), {bytes_per_tri} B/triangle: "
              f"{bytes_per_tri * N / (med * 1e-3) / 1e12:.2f} TB/s", flush=True)
    r.close()

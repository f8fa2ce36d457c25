"""A numpy statement of RZ_TLAS_ENTRY's verdict, independent of the library (CPU only, no GPU):

  entry_verdict(dfs)   rz_scene_dev.h: tlas_entry_verdict -- may a closest-hit query enter the TLAS's pop-order list behind
                       its root?
  primary_hits(...)    the oracle's first hit through every pixel centre, for the census of tests/test_tlas_entry_gpu.py.

The pop-order list comes from tests/tlas_shapes.py: pop_order, which is independent of the library's too."""
import numpy as np

from rayzen_amd import scene as S
import tlas_shapes as T


def dfs_of(scene):
    return T.pop_order(scene.arrays[S.BIND_TLAS_NODES], scene.arrays[S.BIND_TLAS_INDICES])


def entry_verdict(dfs):
    n = len(dfs)
    if n < 3 or dfs[0]["count"] != -1:
        return 0
    left = int(dfs[1]["skip"])
    if left < 2 or left >= n:
        return 0
    boxes = [dfs[0], dfs[1], dfs[left]]
    for b in boxes:
        lo, hi = np.asarray(b["bmin"], np.float32), np.asarray(b["bmax"], np.float32)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
            return 0
    for b in boxes[1:]:
        if not ((boxes[0]["bmin"] <= b["bmin"]).all() and (boxes[0]["bmax"] >= b["bmax"]).all()):
            return 0
    return 1


def primary_hits(scene, width, height):
    """(height, width) bool: the oracle's closest-hit query through the pixel's centre finds something."""
    from oracle import rzo
    from backface_ref import centre_dirs
    from helpers import oracle_scene
    osc, cam = oracle_scene(scene), scene.camera
    dirs = centre_dirs(cam, width, height)
    return np.array([[bool(rzo.trace(osc, cam.position, dirs[y, x])["hit"]) for x in range(width)] for y in range(height)])

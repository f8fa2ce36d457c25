"""CPU census of the first hits of a frame with the oracle's ray queries (rzo.trace / rzo.shadow): for which hit pixels does a
light lie behind the surface -- dot(n, l) <= 0, the shadow queries whose answer cannot change an opaque pixel (rz_path.h:
RZ_BACKFACE_SKIP)?  One ray per pixel, through its centre.  Used by tests/test_backface_shadow_gpu.py (its cases must not be
vacuous) and by profiles/r06_backface/cpu_count.py (the estimate of what the skip saves)."""
import time

import numpy as np

from oracle import rzo

f32 = np.float32


def centre_dirs(camera, width, height):
    """The camera ray directions through the pixel centres (rz_path.h: camera_dir with a jitter of zero), (H, W, 3) float32."""
    ip = np.asarray(camera.inv_proj, f32).reshape(4, 4).T      # column-major storage -> ip[row, col]
    iv = np.asarray(camera.inv_view, f32).reshape(4, 4).T
    ux = ((np.arange(width, dtype=f32) + f32(0.5)) / f32(width))[None, :]
    uy = ((np.arange(height, dtype=f32) + f32(0.5)) / f32(height))[:, None]
    cx, cy = ux * f32(2) - f32(1), uy * f32(2) - f32(1)
    ex = ip[0, 0] * cx + ip[0, 1] * cy - ip[0, 2] + ip[0, 3]
    ey = ip[1, 0] * cx + ip[1, 1] * cy - ip[1, 2] + ip[1, 3]
    eye = np.stack([ex + 0 * ey, ey + 0 * ex, np.full_like(ex + ey, -1.0)], axis=-1).astype(f32)
    world = eye @ iv[:3, :3].T
    return (world / np.linalg.norm(world, axis=-1, keepdims=True)).astype(f32)


def light_dir(light, hp):
    """(direction towards the light, distance limit of its shadow query) at the surface point hp: FS:622-635."""
    pd = np.asarray(light["positionOrDirection"], f32)
    if pd[3] == 1.0:
        lv = pd[:3] - hp
        dist = max(float(np.linalg.norm(lv)), 0.001)
        return (lv / f32(np.linalg.norm(lv))).astype(f32), dist
    return (pd[:3] / f32(np.linalg.norm(pd[:3]))).astype(f32), 1e30


def census(scene, width, height, shadows=False):
    """Walks the frame's pixel centres.  Returns a dict:
    pixels, hits          pixels of the frame / of them with a first hit
    behind[li]            hit pixels with dot(n, l) <= 0 for light li
    any_behind, all_front hit pixels with at least one light behind / with every light in front
    by_instance[i]        [shadow queries, of them behind] of the hits on instance i
    and with shadows=True (every shadow query is traced as the shader would):
    occluded              shadow queries that found an occluder; seconds / seconds_behind: time in rzo.shadow, all / behind ones"""
    from helpers import oracle_scene
    osc = oracle_scene(scene)
    cam = scene.camera
    dirs = centre_dirs(cam, width, height)
    nl = len(scene.lights)
    out = dict(pixels=width * height, hits=0, behind=[0] * nl, any_behind=0, all_front=0, by_instance={},
               queries=0, occluded=0, seconds=0.0, seconds_behind=0.0)
    for y in range(height):
        for x in range(width):
            h = rzo.trace(osc, cam.position, dirs[y, x])
            if not h["hit"]:
                continue
            out["hits"] += 1
            nbehind = 0
            inst = out["by_instance"].setdefault(h["instance"], [0, 0])
            for li in range(nl):
                d, dist = light_dir(scene.lights[li], h["point"])
                behind = not (float(np.dot(h["normal"], d)) > 0.0)
                nbehind += behind
                out["behind"][li] += behind
                out["queries"] += 1
                inst[0] += 1
                inst[1] += behind
                if shadows:
                    t0 = time.perf_counter()
                    lit, _ = rzo.shadow(osc, h["point"] + d * f32(0.001), d, dist)
                    dt = time.perf_counter() - t0
                    out["occluded"] += not lit
                    out["seconds"] += dt
                    if behind:
                        out["seconds_behind"] += dt
            out["any_behind"] += nbehind > 0
            out["all_front"] += nbehind == 0
    return out

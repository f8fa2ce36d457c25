"""Throughput of the batched ray queries (rz_trace_rays) and the latency of one pick; prints ONE JSON line.

    python3 examples/trace_rays.py [--reps 20] [--warmup 3]

Scenes: C2 (rayzen_amd.scene.named_config("c2"), the bench workload) and c2close (the same mesh, camera 0.9 units outside it).
Batches, 1920 x 1080 rays each:
  * coherent:   one camera ray per pixel centre, tile by tile (RZ_TILE_W x RZ_TILE_H = 64 rays: one wave per tile, as the
                render hands out pixels);
  * incoherent: each ray starts at a camera ray's first hit (offset 1e-3 along the normal) in a seeded uniform-hemisphere
                direction; camera rays that miss start from a random point on the mesh instead.
Each batch is traced in both modes (the wave-cursor walk, and RZ_RAYS_INCOHERENT's lane-by-lane walk) from device memory,
timed with device events over `--reps` launches after `--warmup`.  Pick latency: Renderer.pick (host path, one ray) against
a numpy restatement of RayZen's brute-force loop (main.cpp:515-547) over the scene's ~69 k triangles."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rayzen_amd import _lib                                                      # noqa: E402
from rayzen_amd import scene as S                                               # noqa: E402
from rayzen_amd.renderer import HIT_DTYPE, Renderer, make_rays, pick_ray        # noqa: E402

F32 = np.float32


def camera_rays_tiled(cam, W, H):
    ty, tx, ly, lx = np.meshgrid(np.arange((H + 7) // 8), np.arange((W + 7) // 8), np.arange(8), np.arange(8), indexing="ij")
    px, py = (tx * 8 + lx).ravel(), (ty * 8 + ly).ravel()
    keep = (px < W) & (py < H)
    px, py = px[keep], py[keep]
    ndc = np.stack([(px + 0.5) / W * 2 - 1, (py + 0.5) / H * 2 - 1, -np.ones(len(px)), np.ones(len(px))], 1)
    ip = np.asarray(cam.inv_proj, np.float64).reshape(4, 4).T
    iv = np.asarray(cam.inv_view, np.float64).reshape(4, 4).T
    e = ndc @ ip.T
    e = np.stack([e[:, 0], e[:, 1], -np.ones(len(e)), np.zeros(len(e))], 1)
    d = (e @ iv.T)[:, :3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.repeat(np.asarray(cam.position, F32)[None], len(d), 0), d.astype(F32)


def mesh_points(sc, inst, n, rng):
    """n random points on the world-space surface of instance `inst`."""
    it = sc.arrays[S.BIND_INSTANCES][inst]
    g = int(it["globalTriOffset"])
    starts = sorted(set(int(x) for x in sc.arrays[S.BIND_INSTANCES]["globalTriOffset"])) + [len(sc.arrays[S.BIND_TRIANGLES])]
    T = sc.arrays[S.BIND_TRIANGLES][g:starts[starts.index(g) + 1]]
    t = T[rng.integers(0, len(T), n)]
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    p = t["v0"] + u[:, None] * (t["v1"] - t["v0"]) + v[:, None] * (t["v2"] - t["v0"])
    m = np.asarray(it["transform"], np.float64).reshape(4, 4).T
    return (p @ m[:3, :3].T + m[:3, 3]).astype(F32)


def incoherent_rays(sc, r, o_cam, d_cam, rng):
    h = r.trace_rays(o_cam, d_cam)
    hit = h["instance"] >= 0
    o = np.where(hit[:, None], h["point"], 0).astype(F32)
    nrm = np.where(hit[:, None], h["normal"], 0).astype(F32)
    miss = np.nonzero(~hit)[0]
    o[miss] = mesh_points(sc, 1, len(miss), rng)            # instance 1: the bunny stand-in
    nrm[miss] = (o[miss] - np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][1][12:15], F32))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d = rng.normal(size=o.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(((d * nrm).sum(1) < 0)[:, None], -d, d)    # uniform over the hemisphere around the normal
    return (o + nrm * F32(1e-3)).astype(F32), d.astype(F32)


class Hip:
    """Device buffers, a stream and events through the HIP runtime librayzen_hip.so is linked against (ctypes)."""

    def __init__(self):
        _lib.hip()
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
        L = self.L = C.CDLL(path)
        vp, sz, pvp = C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)
        for name, args in (("hipMalloc", [pvp, sz]), ("hipFree", [vp]), ("hipMemcpy", [vp, vp, sz, C.c_int]),
                           ("hipStreamCreate", [pvp]), ("hipStreamDestroy", [vp]), ("hipEventCreate", [pvp]),
                           ("hipEventDestroy", [vp]), ("hipEventRecord", [vp, vp]), ("hipEventSynchronize", [vp]),
                           ("hipEventElapsedTime", [C.POINTER(C.c_float), vp, vp])):
            getattr(L, name).restype, getattr(L, name).argtypes = C.c_int, args

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def new(self, fn):
        h = C.c_void_p()
        self.ok(fn(C.byref(h)))
        return h.value

    def upload(self, a):
        p = C.c_void_p()
        self.ok(self.L.hipMalloc(C.byref(p), a.nbytes))
        self.ok(self.L.hipMemcpy(p.value, a.ctypes.data, a.nbytes, 1))
        return p.value

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.L.hipMalloc(C.byref(p), nbytes))
        return p.value


def time_batch(hip, stream, r, rays, incoherent, reps, warmup):
    n = len(rays)
    d_rays, d_hits = hip.upload(rays), hip.alloc(n * 48)
    for _ in range(warmup):
        r.trace_rays_device(d_rays, d_hits, n, incoherent)
    r.sync()
    ev = [(hip.new(hip.L.hipEventCreate), hip.new(hip.L.hipEventCreate)) for _ in range(reps)]
    for a, b in ev:                                   # back to back on the context's stream, bracketed by events
        hip.ok(hip.L.hipEventRecord(a, stream))
        r.trace_rays_device(d_rays, d_hits, n, incoherent)
        hip.ok(hip.L.hipEventRecord(b, stream))
    r.sync()
    ms = []
    for a, b in ev:
        t = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(t), a, b))
        ms.append(t.value)
        hip.L.hipEventDestroy(a)
        hip.L.hipEventDestroy(b)
    ms.sort()
    med = ms[len(ms) // 2]
    hits = np.empty(n * 48, np.uint8)
    hip.ok(hip.L.hipMemcpy(hits.ctypes.data, d_hits, n * 48, 2))
    hip.L.hipFree(d_rays)
    hip.L.hipFree(d_hits)
    hits = hits.view(HIT_DTYPE)
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "grays_per_s": round(n / (med * 1e-3) / 1e9, 3),
            "hit_frac": round(float((hits["instance"] >= 0).mean()), 4)}, hits.tobytes()


def brute_pick_numpy(sc, o, d):
    """main.cpp:515-547 vectorised per object, float32."""
    tris, inst = sc.arrays[S.BIND_TRIANGLES], sc.arrays[S.BIND_INSTANCES]
    starts = sorted(set(int(g) for g in inst["globalTriOffset"])) + [len(tris)]
    best = (1e30, -1, -1)
    for k, it in enumerate(inst):
        g = int(it["globalTriOffset"])
        T = tris[g:starts[starts.index(g) + 1]]
        m = np.asarray(it["inverseTransform"], F32).reshape(4, 4)
        lo = (m[0, :3] * o[0] + m[1, :3] * o[1]) + (m[2, :3] * o[2] + m[3, :3])
        ld = m[0, :3] * d[0] + m[1, :3] * d[1] + m[2, :3] * d[2]
        ld = ld / np.sqrt((ld * ld).sum())
        e1, e2 = T["v1"] - T["v0"], T["v2"] - T["v0"]
        h = np.cross(ld, e2)
        a = (e1 * h).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = F32(1) / a
            s = lo - T["v0"]
            u = f * (s * h).sum(1)
            q = np.cross(s, e1)
            v = f * (q * ld).sum(1)
            t = f * (e2 * q).sum(1)
            ok = (np.abs(a) >= 1e-6) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 1e-4)
        if ok.any():
            j = int(np.argmin(np.where(ok, t, np.inf)))
            if t[j] < best[0]:
                best = (float(t[j]), k, j)
    return best


def main():
    hip = Hip()
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    warmup = int(sys.argv[sys.argv.index("--warmup") + 1]) if "--warmup" in sys.argv else 3
    out = {"metric": "G rays/s of rz_trace_rays (1920x1080 rays per batch)", "reps": reps, "warmup": warmup, "scenes": {}}
    rng = np.random.default_rng(2024)
    for name in ("c2", "c2close"):
        sc, W, H, _, _ = S.named_config(name)
        r = Renderer(0)
        r.upload_scene(sc)
        stream = hip.new(hip.L.hipStreamCreate)
        r.set_stream(stream)
        o, d = camera_rays_tiled(sc.camera, W, H)
        batches = {"coherent": make_rays(o, d), "incoherent": make_rays(*incoherent_rays(sc, r, o, d, rng))}
        res = {}
        for bname, rays in batches.items():
            res[bname] = {}
            ref = None
            for mode in ("default", "incoherent_walk"):
                res[bname][mode], raw = time_batch(hip, stream, r, rays, mode != "default", reps, warmup)
                ref = raw if ref is None else ref
                res[bname][mode]["same_bytes_as_default"] = raw == ref
            res[bname]["n_rays"] = len(rays)
        out["scenes"][name] = res
        r.set_stream(0)
        hip.L.hipStreamDestroy(stream)
        if name == "c2":
            lat = []
            for k in range(200):
                t0 = time.perf_counter()
                r.pick(400 + (k % 20) * 3, 300 + (k // 20) * 3, 800, 600, sc.camera)
                lat.append(time.perf_counter() - t0)
            lat.sort()
            out["pick_us_median"] = round(lat[len(lat) // 2] * 1e6, 1)
            out["pick_us_p90"] = round(lat[int(len(lat) * 0.9)] * 1e6, 1)
            po, pd = pick_ray(400, 300, 800, 600, sc.camera)
            nl = []
            for _ in range(5):
                t0 = time.perf_counter()
                brute_pick_numpy(sc, po, pd)
                nl.append(time.perf_counter() - t0)
            out["numpy_brute_pick_ms_median"] = round(sorted(nl)[2] * 1e3, 2)
            out["numpy_brute_pick_triangles"] = int(len(sc.arrays[S.BIND_TRIANGLES]))
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

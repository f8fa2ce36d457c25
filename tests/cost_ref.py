"""numpy restatement of the cost map's arithmetic (include/rayzen_hip.h: rz_cost_view): the value of a pixel per metric in uint64,
the frame's statistics with the maximum going to the lowest pixel index on ties, and the false-colour ramp in np.float32 with the
header's operand order -- one rounding per operation, no fused multiply-add, so the linear curve is bit for bit the device's.
The per-pixel records themselves come from the CPU oracle: one single-pixel crop per pixel (oracle_records)."""
import numpy as np

from rayzen_amd import _lib

F32 = np.float32
U64 = np.uint64
DTYPE = _lib.PIXEL_COST_DTYPE
FIELDS = DTYPE.names
METRICS = dict(_lib.COST_METRICS)
STOPS = np.array([(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 1, 0), (1, 0, 0)], F32)


def records(columns):
    """(..., 8) integers in the record's field order -> PIXEL_COST_DTYPE records."""
    a = np.asarray(columns)
    out = np.zeros(a.shape[:-1], DTYPE)
    for k, f in enumerate(FIELDS):
        out[f] = a[..., k]
    return out


def value(rec, metric="bytes"):
    """v per pixel, uint64."""
    m = METRICS[metric] if isinstance(metric, str) else int(metric)
    c = {f: rec[f].astype(U64) for f in FIELDS}
    if m == 0:
        return (U64(32) * c["tlas_nodes"] + U64(4) * c["tlas_leaf_indices"] + U64(144) * c["instances"] + U64(32) * c["blas_nodes"]
                + U64(68) * c["triangles"] + U64(32) * c["materials"] + U64(32) * c["light_fetches"] + U64(16))
    if m == 1:
        return c["tlas_nodes"] + c["blas_nodes"]
    return {2: c["triangles"], 3: c["traversals"], 4: c["instances"]}[m]


def stats(rec, metric="bytes", scale=0.0):
    """The rz_cost_stats of an (H, W) frame of records as a dict."""
    v = value(rec, metric)
    h, w = v.shape
    mx = int(v.max())
    first = int(np.argmax(v.reshape(-1)))               # (argmax returns the first of the maxima: the lowest pixel index)
    s = F32(scale) if scale > 0 else (F32(U64(mx)) if mx > 0 else F32(1))
    return dict(max_value=mx, sum_value=int(v.sum(dtype=U64)), max_x=first % w, max_y=first // w, scale_used=float(s))


def colour(rec, metric="bytes", curve="linear", scale=0.0):
    """(H, W, 3) float32: the ramp, with np.float32 operations in the header's order."""
    S = F32(stats(rec, metric, scale)["scale_used"])
    fv = value(rec, metric).astype(F32)                 # (uint64 -> binary32, round to nearest even, as the device converts)
    with np.errstate(all="ignore"):
        if curve in ("linear", 0):
            u = np.minimum(fv / S, F32(1))
        else:
            u = np.minimum(np.log2(F32(1) + fv) / np.log2(F32(1) + S), F32(1)).astype(F32)
    u4 = u * F32(4)
    k = np.minimum(u4.astype(np.int32), 3)
    w = u4 - k.astype(F32)
    a, b = STOPS[k], STOPS[k + 1]
    c = (a + (b - a) * w[..., None]).astype(F32)
    c[fv > S] = F32(1)
    return c


# name: (scene, width, height, spp, bounces, distinct per-pixel byte values, their range without the pixel's own 16 bytes) -- the
# figures are the oracle's own
CASES = {
    "reference": (lambda S: S.reference_scene(aspect=4 / 3), 24, 18, 2, 5, 166, (1192, 34868)),
    "bunny": (lambda S: S.bunny_scene(n=12, aspect=4 / 3, extras=True, camera_position=(3, 1, 7)), 24, 18, 3, 4, 332, (480, 58708)),
    "instanced": (lambda S: S.instanced_scene(n=8, count=16, aspect=16 / 9), 32, 18, 1, 2, 194, (32, 21524)),
}
_CASE_CACHE = {}


def case(name):
    """(scene, width, height, spp, bounces, oracle records, oracle totals) of a CASES entry, computed once per process."""
    if name not in _CASE_CACHE:
        from rayzen_amd import scene as S
        make, w, h, spp, bounces = CASES[name][:5]
        sc = make(S)
        rec, total = oracle_records(sc, w, h, spp, bounces)
        rec.setflags(write=False)
        _CASE_CACHE[name] = (sc, w, h, spp, bounces, rec, total)
    return _CASE_CACHE[name]


def oracle_records(scene, width, height, spp, bounces, num_lights=None):
    """(H, W) records from the CPU oracle: the counters of one single-pixel crop per pixel; and the ten first counters summed."""
    from helpers import oracle_frame, oracle_scene
    from oracle import rzo
    osc = oracle_scene(scene)
    fr = oracle_frame(scene, width, height, spp, bounces, num_lights=num_lights)
    out = np.zeros((height, width), DTYPE)
    total = {n: 0 for n in rzo.COUNTER_FIELDS}
    for y in range(height):
        for x in range(width):
            _, c = rzo.render(osc, fr, crop=(x, y, x + 1, y + 1), want_counters=True)
            for f in FIELDS:
                out[y, x][f] = c[f]
            for n in total:
                total[n] += c[n]
    return out, total

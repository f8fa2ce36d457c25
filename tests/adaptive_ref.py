"""Restatement of rz_render_adaptive (include/rayzen_hip.h, "Adaptive sampling"): the CPU oracle driven batch by batch over the
planned runs of tiles -- rzo.render(accum=, ior_state=, crop=) with the frame's sample_base, one crop per tile -- the meter in
np.float32 with the header's operand order and the xor butterfly 32, 16, 8, 4, 2, 1, and the plan rule as the header words it, in
plain Python (merge the smallest all-current gap, one pair at a time).  One rounding per operation, no fused multiply-add, so
every number is the device's bit for bit."""
import numpy as np

from helpers import oracle_frame, oracle_scene
from oracle import rzo

F32 = np.float32
TILE = 8
DEFAULTS = dict(batch_spp=8, min_batches=4, max_batches=8, threshold=0.02, luminance_floor=0.01, merge_gap=8, max_runs=1)


# ---------------------------------------------------------------------------------------------------------------------
# the plan

def plan(active, current, merge_gap, max_runs):
    """[(first, len), ...] in ascending order."""
    active = [bool(a) for a in active]
    current = [bool(c) for c in current]
    runs, i, n = [], 0, len(active)
    while i < n:                                        # (1) the maximal intervals of active tiles
        if not active[i]:
            i += 1
            continue
        j = i
        while j < n and active[j]:
            j += 1
        runs.append([i, j - i])
        i = j

    def gap(k):                                         # the gap behind run k: (its length, all of it current)
        g0, g1 = runs[k][0] + runs[k][1], runs[k + 1][0]
        return g1 - g0, all(current[g0:g1])

    def merge(k):
        runs[k][1] = runs[k + 1][0] + runs[k + 1][1] - runs[k][0]
        del runs[k + 1]

    k = 0
    while k + 1 < len(runs):                            # (2) neighbours a short all-current gap apart
        length, cur = gap(k)
        if cur and length <= merge_gap:
            merge(k)
        else:
            k += 1
    while len(runs) > max_runs:                         # (3) the smallest all-current gap, the lowest index among equals
        best = None
        for k in range(len(runs) - 1):
            length, cur = gap(k)
            if cur and (best is None or length < best[0]):
                best = (length, k)
        if best is None:
            break                                       # (4) the plan stands with more runs
        merge(best[1])
    return [tuple(r) for r in runs]


# ---------------------------------------------------------------------------------------------------------------------
# the meter

def butterfly(v):
    """The sum of 64 binary32 lanes by t[l] = t[l] + t[l ^ o], o = 32 ... 1 (every lane ends with the same bits)."""
    t = np.asarray(v, F32).copy()
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            t = (t + t[lanes ^ o]).astype(F32)
    return t[0]


def meter_tile(I, prev, S1, S2, inside, s, B, floor):
    """One tile after batch B.  I, prev: (64, 4) float32 in lane order (lane = x + 8 y); S1, S2: (64,); inside: (64,) bool.
    Returns (E, prev', S1', S2'); lanes outside the frame keep their state."""
    fs, fB = F32(s), F32(B)
    with np.errstate(all="ignore"):
        d = ((I[:, :3] - prev[:, :3]) / fs).astype(F32)
        L = (F32(0.2126) * d[:, 0] + F32(0.7152) * d[:, 1]) + F32(0.0722) * d[:, 2]
        S1n = (S1 + L).astype(F32)
        S2n = (S2 + L * L).astype(F32)
        m = S1n / fB
        if B >= 2:
            x = (S2n - S1n * m) / F32(B - 1)
            v = np.where(x > 0, x, np.where(np.isnan(x), x, F32(0))).astype(F32)
            e = np.sqrt(v / fB).astype(F32)
        else:
            e = np.zeros(64, F32)
        e = np.where(inside, e, F32(0)).astype(F32)
        am = np.where(inside, np.abs(m), F32(0)).astype(F32)
        den = butterfly(am) + F32(floor) * F32(int(inside.sum()))
        E = F32(butterfly(e) / den)
    keep = ~inside
    return E, np.where(keep[:, None], prev, I), np.where(keep, S1, S1n).astype(F32), np.where(keep, S2, S2n).astype(F32)


def retires(E, B, min_batches, threshold):
    return bool(B >= min_batches and F32(E) <= F32(threshold))


class Meter:
    """The context's metering state for a w x h frame."""

    def __init__(self, w, h, s, min_batches, threshold, floor):
        self.w, self.h, self.s, self.min_batches, self.threshold, self.floor = w, h, s, min_batches, threshold, floor
        self.tx, self.ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
        n = self.tx * self.ty
        self.prev = np.zeros((n, 64, 4), F32)
        self.S1, self.S2 = np.zeros((n, 64), F32), np.zeros((n, 64), F32)
        self.error = np.zeros(n, F32)
        self.batches = np.zeros(n, np.int32)
        self.active = np.ones(n, bool)
        self.current = np.ones(n, bool)

    def rect(self, t):
        x0, y0 = (t % self.tx) * TILE, (t // self.tx) * TILE
        return x0, y0, min(x0 + TILE, self.w), min(y0 + TILE, self.h)

    def lanes(self, accum, t):
        """(64, 4) of tile t in lane order and the inside mask."""
        x0, y0, x1, y1 = self.rect(t)
        I = np.zeros((TILE, TILE, 4), F32)
        I[:y1 - y0, :x1 - x0] = accum[y0:y1, x0:x1]
        inside = np.zeros((TILE, TILE), bool)
        inside[:y1 - y0, :x1 - x0] = True
        return I.reshape(64, 4), inside.reshape(64)

    def run(self, accum, tiles, B):
        """Meters the tiles batch B rendered; the others stop being current."""
        seen = np.zeros(len(self.active), bool)
        for t in tiles:
            I, inside = self.lanes(accum, t)
            E, self.prev[t], self.S1[t], self.S2[t] = meter_tile(I, self.prev[t], self.S1[t], self.S2[t], inside, self.s, B, self.floor)
            self.error[t] = E
            self.batches[t] += 1
            self.active[t] = self.active[t] and not retires(E, B, self.min_batches, self.threshold)
            self.current[t] = self.batches[t] == B
            seen[t] = True
        self.current &= seen


# ---------------------------------------------------------------------------------------------------------------------
# the call

def render_adaptive(scene, w, h, bounces, batch_spp, min_batches, max_batches, threshold, luminance_floor=0.01, merge_gap=8, max_runs=1,
                    num_lights=None, nthreads=8):
    """dict(accum (H, W, 4), tile_batches (ty, tx) int32, tile_error (ty, tx) float32, batches, tiles_active, tiles_rendered, runs,
    samples_traced, samples_uniform) -- the last seven as rz_adaptive_info reports them."""
    osc = oracle_scene(scene)
    accum = np.zeros((h, w, 4), F32)
    ior = np.ones((h, w), F32)
    M = Meter(w, h, batch_spp, min_batches, threshold, luminance_floor)
    n = M.tx * M.ty
    runs = [(0, n)]
    out = dict(tiles_active=[], tiles_rendered=[], runs=[], samples_traced=0, samples_uniform=w * h * max_batches * batch_spp)
    B = 0
    while True:
        B += 1
        fr = oracle_frame(scene, w, h, batch_spp, bounces, sample_base=(B - 1) * batch_spp, num_lights=num_lights)
        tiles = [t for first, length in runs for t in range(first, first + length)]
        if B == 1:
            rzo.render(osc, fr, accum=accum, ior_state=ior, nthreads=nthreads)
        else:
            for t in tiles:
                rzo.render(osc, fr, accum=accum, ior_state=ior, crop=M.rect(t), nthreads=1)
        M.run(accum, tiles, B)
        for t in tiles:
            x0, y0, x1, y1 = M.rect(t)
            out["samples_traced"] += (x1 - x0) * (y1 - y0) * batch_spp
        out["tiles_active"].append(int(M.active.sum()))
        out["tiles_rendered"].append(len(tiles))
        out["runs"].append(len(runs))
        if not M.active.any() or B == max_batches:
            break
        runs = plan(M.active, M.current, merge_gap, max_runs)
    out.update(accum=accum, batches=B, tile_batches=M.batches.reshape(M.ty, M.tx).copy(), tile_error=M.error.reshape(M.ty, M.tx).copy())
    return out


def pixel_spp(accum):
    """Every pixel's own sample count, as integers."""
    a = accum[..., 3]
    n = a.astype(np.int64)
    assert (n == a).all()
    return n


def one_shot_at_own_spp(scene, w, h, bounces, accum, num_lights=None, nthreads=8):
    """The oracle's one-shot frames at every sample count that occurs in `accum`, taken pixel by pixel: (H, W, 4)."""
    n = pixel_spp(accum)
    osc = oracle_scene(scene)
    want = np.zeros_like(accum)
    for spp in np.unique(n):
        if spp == 0:
            continue
        fr = oracle_frame(scene, w, h, int(spp), bounces, num_lights=num_lights)
        full = rzo.render(osc, fr, nthreads=nthreads)
        want[n == spp] = full[n == spp]
    return want


# the frames of the issue: name -> (scene maker, width, height, bounces)
def _scenes():
    from rayzen_amd import scene as S
    return {
        "cornell": (lambda: S.cornell_scene(), 64, 48, 4),
        "bunny": (lambda: S.bunny_scene(n=12, extras=True), 64, 40, 4),
        "reference": (lambda: S.reference_scene(), 64, 48, 5),
    }


# (the issue's settings; the plan's two knobs stated so that the small frames take several launches per batch: the default
# max_runs of 1 always gives one)
SETTINGS = dict(batch_spp=4, min_batches=4, max_batches=8, threshold=0.02, luminance_floor=0.01, merge_gap=8, max_runs=64)
# bunny: at 0.02 the tile that retires at batch 7 lies inside a merged run and is rendered on, so only the counts 4 and 8 occur;
# at 0.05 (of 0.01 / 0.02 / 0.05) there are three -- 4, 6 and 8
THRESHOLD = {"cornell": 0.02, "bunny": 0.05, "reference": 0.02}
_CACHE = {}


def scene(name):
    key = ("scene", name)
    if key not in _CACHE:
        make, w, h, bounces = _scenes()[name]
        _CACHE[key] = (make(), w, h, bounces)
    return _CACHE[key]


def case(name, size=None, **over):
    """(scene, w, h, bounces, restated result) of a frame of the issue (size: another width and height) under SETTINGS and the
    frame's THRESHOLD (with overrides), computed once per process and left unchanged."""
    key = (name, size, tuple(sorted(over.items())))
    if key not in _CACHE:
        sc, w, h, bounces = scene(name)
        if size is not None:
            w, h = size
        res = render_adaptive(sc, w, h, bounces, **{**SETTINGS, "threshold": THRESHOLD[name], **over})
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (sc, w, h, bounces, res)
    return _CACHE[key]

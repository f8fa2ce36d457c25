"""rz_render_adaptive without a GPU: the C-ABI structs and symbols, the metering kernel's code-object metadata, rz_adaptive_plan
against the restatement (adaptive_ref.py) on hand-made masks, the meter's restatement on hand-made sums, and -- with the CPU
oracle alone -- that the frames the GPU test runs bite and that the restated result is, pixel by pixel, the oracle's one-shot
frame at that pixel's own sample count.  The figures in the last group are conditions computed with the oracle; they are not
measurements of the device."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as AR
from rayzen_amd import _lib
from test_rays_abi import _kernel_metadata

F32 = np.float32


def test_struct_sizes_offsets_and_symbols():
    L = _lib.hip()
    assert (_lib.SIZEOF_ADAPTIVE_PARAMS, _lib.SIZEOF_ADAPTIVE_INFO, _lib.SIZEOF_TILE_RUN) == (38, 39, 40)
    assert L.rz_sizeof(38) == 32 == C.sizeof(_lib.AdaptiveParams)
    assert L.rz_sizeof(39) == 800 == C.sizeof(_lib.AdaptiveInfo)
    assert L.rz_sizeof(40) == 8 == _lib.TILE_RUN_DTYPE.itemsize
    assert L.rz_sizeof(41) == 0
    want = {
        _lib.AdaptiveParams: {"batch_spp": 0, "min_batches": 4, "max_batches": 8, "threshold": 12, "luminance_floor": 16, "merge_gap": 20,
                              "max_runs": 24, "flags": 28},
        _lib.AdaptiveInfo: {"batches": 0, "n_tiles": 4, "samples_traced": 8, "samples_uniform": 16, "render_ms": 24, "meter_ms": 28,
                            "tiles_active": 32, "tiles_rendered": 288, "runs": 544},
    }
    for struct, offs in want.items():
        assert [f for f, _ in struct._fields_] == list(offs), struct
        for f, off in offs.items():
            assert getattr(struct, f).offset == off, (struct, f)
    assert [_lib.TILE_RUN_DTYPE.fields[f][1] for f in ("first", "len")] == [0, 4]
    assert _lib.ADAPTIVE_HOST == 1 and _lib.ADAPTIVE_MAX_BATCHES == 64
    assert _lib.ADAPTIVE_DEFAULTS == AR.DEFAULTS
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5      # additive: the revision stays
    lib = C.CDLL(_lib.HIP_SO)
    for name in ("rz_render_adaptive", "rz_adaptive_plan"):
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name
    from rayzen_amd import renderer
    assert callable(renderer.adaptive_plan)
    for m in ("render_adaptive", "render_adaptive_device"):
        assert callable(getattr(renderer.Renderer, m)), m


def test_meter_kernel_spills_nothing():
    meta = _kernel_metadata(_lib.HIP_SO)
    ours = {k: v for k, v in meta.items() if "rz_adaptive_meter" in k}
    assert len(ours) == 1, sorted(ours)
    for name, (spill, priv) in ours.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


# ---------------------------------------------------------------------------------------------------------------------
# rz_adaptive_plan against the restatement

def _mask(n, *intervals):
    m = np.zeros(n, np.uint8)
    for a, b in intervals:
        m[a:b] = 1
    return m


def _both(active, current, merge_gap, max_runs):
    from rayzen_amd.renderer import adaptive_plan
    got = adaptive_plan(active, current, merge_gap, max_runs)
    want = np.array(AR.plan(active, current, merge_gap, max_runs), np.int32).reshape(-1, 2)
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes(), (got.tolist(), want.tolist())
    return [tuple(r) for r in got.tolist()]


G = 3       # the merge gap of the hand-made masks

PLAN_CASES = {
    # name: (active, current, merge_gap, max_runs, the runs)
    "empty set": (_mask(40), _mask(40, (0, 40)), G, 4, []),
    "no tiles": (_mask(0), _mask(0), G, 4, []),
    "full set": (_mask(40, (0, 40)), _mask(40, (0, 40)), G, 4, [(0, 40)]),
    "single tile": (_mask(40, (17, 18)), _mask(40, (0, 40)), G, 4, [(17, 1)]),
    "last tile": (_mask(40, (39, 40)), _mask(40), G, 4, [(39, 1)]),
    "alternating, gap 1": (_mask(9, (0, 1), (2, 3), (4, 5), (6, 7), (8, 9)), _mask(9, (0, 9)), G, 9, [(0, 9)]),
    "gap = merge_gap": (_mask(20, (0, 2), (2 + G, 4 + G)), _mask(20, (0, 20)), G, 9, [(0, 4 + G)]),
    "gap = merge_gap + 1": (_mask(20, (0, 2), (3 + G, 5 + G)), _mask(20, (0, 20)), G, 9, [(0, 2), (3 + G, 2)]),
    "merge_gap 0 merges nothing": (_mask(9, (0, 1), (2, 3), (4, 5)), _mask(9, (0, 9)), 0, 9, [(0, 1), (2, 1), (4, 1)]),
    "one non-current tile in the gap": (_mask(20, (0, 2), (4, 6), (8, 10)), _mask(20, (0, 3), (4, 20)), G, 9, [(0, 2), (4, 6)]),
    "max_runs 1, all gaps current": (_mask(64, (0, 2), (20, 22), (50, 52)), _mask(64, (0, 64)), G, 1, [(0, 52)]),
    "max_runs 1, no mergeable pair": (_mask(64, (0, 2), (20, 22), (50, 52)), _mask(64, (0, 2), (20, 22), (50, 52)), G, 1,
                                      [(0, 2), (20, 2), (50, 2)]),
    "max_runs 2, the smaller gap goes": (_mask(64, (0, 2), (20, 22), (30, 32)), _mask(64, (0, 64)), G, 2, [(0, 2), (20, 12)]),
    "max_runs 2, the smaller gap is not current": (_mask(64, (0, 2), (20, 22), (30, 32)), _mask(64, (0, 25), (26, 64)), G, 2,
                                                   [(0, 22), (30, 2)]),
    "a tie between two equal gaps": (_mask(64, (0, 2), (12, 14), (24, 26)), _mask(64, (0, 64)), G, 2, [(0, 14), (24, 2)]),
    "a tie, then the other": (_mask(64, (0, 2), (12, 14), (24, 26), (60, 62)), _mask(64, (0, 64)), G, 2, [(0, 26), (60, 2)]),
    # 8 tiles per row: a run from the end of row 0 into row 1, and one merged across the row's end
    "a run that wraps a tile row": (_mask(24, (6, 11)), _mask(24, (0, 24)), G, 4, [(6, 5)]),
    "merged across a tile row": (_mask(24, (6, 8), (9, 11)), _mask(24, (0, 24)), G, 4, [(6, 5)]),
    "step 2 chains": (_mask(30, (0, 1), (3, 4), (6, 7), (9, 10), (20, 21)), _mask(30, (0, 30)), 2, 9, [(0, 10), (20, 1)]),
}


@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_on_hand_made_masks(name):
    active, current, gap, max_runs, runs = PLAN_CASES[name]
    assert _both(active, current, gap, max_runs) == runs


def test_plan_on_random_masks():
    rng = np.random.default_rng(11)
    for k in range(200):
        n = int(rng.integers(1, 120))
        active = (rng.random(n) < rng.choice([0.1, 0.4, 0.8])).astype(np.uint8)
        current = (active | (rng.random(n) < rng.choice([0.3, 0.9, 1.0]))).astype(np.uint8)
        runs = _both(active, current, int(rng.integers(0, 6)), int(rng.integers(1, 8)))
        covered = _mask(n, *[(a, a + b) for a, b in runs])
        assert (covered >= active).all() and (current[(covered == 1) & (active == 0)] == 1).all()
        assert all(a + b < c for (a, b), (c, _) in zip(runs, runs[1:]))


def test_plan_cap_too_small_and_bad_arguments():
    L = _lib.hip()
    active, current = _mask(20, (0, 2), (10, 12), (18, 20)), _mask(20)
    runs = np.full(3, -1, _lib.TILE_RUN_DTYPE)
    n = C.c_size_t(99)
    a, c = active.ctypes.data, current.ctypes.data
    assert L.rz_adaptive_plan(a, c, 20, 8, 64, runs.ctypes.data, 2, C.byref(n)) == -7          # RZ_ERR_BUFFER_SIZE
    assert n.value == 3 and (runs["first"] == -1).all()
    assert b"3 runs" in L.rz_last_error(None)
    assert L.rz_adaptive_plan(a, c, 20, 8, 64, runs.ctypes.data, 3, C.byref(n)) == 0
    assert n.value == 3 and runs.tolist() == [(0, 2), (10, 2), (18, 2)]
    assert L.rz_adaptive_plan(a, c, 20, 8, 64, None, 0, C.byref(n)) == -7 and n.value == 3        # a size query
    for args in ((None, c, 20, 8, 64, runs.ctypes.data, 3, C.byref(n)), (a, None, 20, 8, 64, runs.ctypes.data, 3, C.byref(n)),
                 (a, c, 20, 8, 64, runs.ctypes.data, 3, None), (a, c, 20, 8, 64, None, 3, C.byref(n)),
                 (a, c, 20, -1, 64, runs.ctypes.data, 3, C.byref(n)), (a, c, 20, 8, 0, runs.ctypes.data, 3, C.byref(n)),
                 (a, c, (1 << 30) + 1, 8, 64, runs.ctypes.data, 3, C.byref(n))):
        assert L.rz_adaptive_plan(*args) == -1, args                                            # RZ_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# the meter's restatement on hand-made sums

def _tile(values, s, floor=0.01, inside=None, min_batches=2, threshold=0.02):
    """Runs the meter over one tile whose accumulation after batch k is the running sum of values[k] ((64, 3) per batch, the
    batch's colour SUM).  Returns the list of (E, retires) per batch."""
    inside = np.ones(64, bool) if inside is None else inside
    prev, S1, S2 = np.zeros((64, 4), F32), np.zeros(64, F32), np.zeros(64, F32)
    I = np.zeros((64, 4), F32)
    out = []
    for B, v in enumerate(values, 1):
        I = I.copy()
        I[:, :3] = (I[:, :3] + np.asarray(v, F32)).astype(F32)
        I[:, 3] += s
        E, prev, S1, S2 = AR.meter_tile(I, prev, S1, S2, inside, s, B, floor)
        out.append((E, AR.retires(E, B, min_batches, threshold)))
    return out


def test_meter_equal_batches_give_zero():
    # 0.5 per channel per sample, s = 4: binary32 holds the accumulation exactly, and S1 = 2 L, S2 = 2 L * L, m = L at B = 2
    res = _tile([np.full((64, 3), 2.0)] * 4, 4)
    assert [float(E) for E, _ in res[:2]] == [0.0, 0.0]
    # B = 3, 4: 3 L and 3 L * L round, so S2 - S1 * m is a few ulp of S2 (2^-24 L * L each) and e about sqrt(1e-7) L: the floor
    # of the running sums the header speaks of, far under any threshold that means something
    assert all(0.0 <= float(E) < 1e-3 for E, _ in res[2:]), res
    assert [r for _, r in res] == [False, True, True, True]           # B = 1 never retires (min_batches >= 2)


def test_meter_two_batches_that_differ():
    # luminance 1 then 0 on every pixel: S1 = 1, S2 = 1, m = 0.5, v = (1 - 0.5) / 1, e = sqrt(0.25) = 0.5; E = 32 / (32 + 0.64)
    white = np.full((64, 3), 4.0)                                       # s = 4: d = (1, 1, 1), L = 0.2126 + 0.7152 + 0.0722
    res = _tile([white, np.zeros((64, 3))], 4)
    L = (F32(0.2126) + F32(0.7152)) + F32(0.0722)
    S1, S2 = L, L * L
    m = S1 / F32(2)
    e = np.sqrt(((S2 - S1 * m) / F32(1)) / F32(2))
    want = F32(F32(64) * e) / (F32(64) * m + F32(0.01) * F32(64))      # (64 equal lanes: every partial sum of the butterfly is exact)
    assert res[1][0] == F32(want) and abs(float(res[1][0]) - 0.5 / 0.51) < 1e-6
    assert not res[1][1]
    assert float(res[0][0]) == 0.0


def test_meter_the_butterfly_order_is_part_of_the_definition():
    rng = np.random.default_rng(3)
    v = (rng.random(64) * 10.0 ** rng.integers(-6, 3, 64)).astype(F32)
    b = AR.butterfly(v)
    t = v.copy()
    for o in (1, 2, 4, 8, 16, 32):                                      # the other order
        t = (t + t[np.arange(64) ^ o]).astype(F32)
    exact = float(v.astype(np.float64).sum())
    assert b.dtype == F32 and abs(float(b) - exact) <= 6 * 2.0 ** -24 * exact          # six levels, one rounding each
    assert abs(float(t[0]) - exact) <= 6 * 2.0 ** -24 * exact
    # the pinned order, written out: pairs 32 apart first
    u = v.astype(F32)
    for half in (32, 16, 8, 4, 2, 1):
        u = (u[:half] + u[half:2 * half]).astype(F32)
    assert u[0] == b


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_meter_a_non_finite_sample_keeps_the_tile_active(bad):
    first = np.full((64, 3), 2.0)
    first[13, 1] = bad
    res = _tile([first] + [np.full((64, 3), 2.0)] * 3, 4, threshold=np.inf)
    assert all(np.isnan(E) for E, _ in res[1:]), res
    assert not any(r for _, r in res)
    clean = _tile([np.full((64, 3), 2.0)] * 4, 4, threshold=np.inf)
    assert [r for _, r in clean] == [False, True, True, True]
    assert not any(r for _, r in _tile([np.full((64, 3), 2.0)] * 4, 4, threshold=-1.0))


def test_meter_a_partial_tile_counts_only_its_inside_pixels():
    inside = np.zeros((8, 8), bool)
    inside[:5, :1] = True                                               # a 1 x 5 corner tile
    inside = inside.reshape(64)
    white, rubbish = np.full((64, 3), 4.0), np.full((64, 3), 4.0)
    rubbish[~inside] = 1e30                                             # what lies outside does not count
    a = _tile([white, np.zeros((64, 3))], 4, inside=inside)
    b = _tile([rubbish, np.zeros((64, 3))], 4, inside=inside)
    assert a[1][0] == b[1][0]
    L = (F32(0.2126) + F32(0.7152)) + F32(0.0722)
    m = L / F32(2)
    e = np.sqrt(((L * L - L * m) / F32(1)) / F32(2))
    num, den = AR.butterfly(np.where(inside, e, F32(0))), AR.butterfly(np.where(inside, m, F32(0)))
    assert a[1][0] == F32(num / (den + F32(0.01) * F32(5)))
    full = _tile([white, np.zeros((64, 3))], 4)
    assert a[1][0] != F32(num / (den + F32(0.01) * F32(64))) and abs(float(a[1][0]) - float(full[1][0])) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the oracle alone: the frames bite, and the restated result is exact

@pytest.mark.parametrize("name", ["cornell", "bunny"])
def test_oracle_the_frames_bite(name):
    sc, w, h, bounces, res = AR.case(name)
    tb = res["tile_batches"].ravel()
    n = tb.size
    retired_at_min = n - res["tiles_active"][AR.SETTINGS["min_batches"] - 1]
    to_the_end = int((tb == AR.SETTINGS["max_batches"]).sum())
    print(f"{name}: threshold {AR.THRESHOLD[name]}, {n} tiles, {retired_at_min} retire at batch 4, {to_the_end} run to batch 8, counts "
          f"{sorted(set(tb.tolist()))}, active {res['tiles_active']}, rendered {res['tiles_rendered']}, runs {res['runs']}")
    assert res["batches"] == 8
    assert 4 * retired_at_min >= n
    assert 10 * to_the_end >= n
    assert len(set(tb.tolist())) >= 3
    assert res["samples_traced"] < res["samples_uniform"] == w * h * 32
    assert res["samples_traced"] == int(AR.pixel_spp(res["accum"]).sum())


def test_oracle_the_glass_frame_bites():
    sc, w, h, bounces, res = AR.case("reference")
    n = res["tile_batches"].size
    retired_at_min = n - res["tiles_active"][3]
    print(f"reference: {n} tiles, {retired_at_min} retire at batch 4, active {res['tiles_active']}")
    assert 4 * retired_at_min >= 3 * n
    assert res["tiles_active"][3] >= 1 and res["batches"] > 4          # at least one tile later
    assert AR.oracle_scene is not None and (sc.arrays[1]["transparency"] > 0).any()     # its glass carries currentIor across launches


def test_oracle_several_runs_per_batch_without_merging():
    sc, w, h, bounces, res = AR.case("cornell", merge_gap=0)
    assert max(res["runs"]) >= 5 and res["runs"][:4] == [1, 1, 1, 1]
    merged = AR.case("cornell")[4]
    assert res["tiles_active"] == merged["tiles_active"]                # who retires does not depend on the plan,
    assert res["samples_traced"] < merged["samples_traced"]            # only who is rendered on


@pytest.mark.parametrize("name,over", [("cornell", {}), ("bunny", {}), ("reference", {}), ("cornell", {"merge_gap": 0})],
                         ids=["cornell", "bunny", "reference", "cornell-unmerged"])
def test_oracle_every_pixel_is_the_one_shot_frame_at_its_own_sample_count(name, over):
    sc, w, h, bounces, res = AR.case(name, **over)
    accum = res["accum"]
    spp = AR.pixel_spp(accum)
    tiles = np.repeat(np.repeat(res["tile_batches"], 8, axis=0), 8, axis=1)[:h, :w]
    assert (spp == tiles * AR.SETTINGS["batch_spp"]).all()
    want = AR.one_shot_at_own_spp(sc, w, h, bounces, accum)
    assert accum.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()

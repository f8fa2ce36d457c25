"""The per-pixel traversal cost map (rz_render_cost, rz_cost_view, rz_present_cost): the C-ABI structs and symbols, the code-object
metadata of its kernels, properties of the restatement (cost_ref.py) on hand-made records, and -- with the CPU oracle alone --
that the cases the GPU test runs bite: the per-pixel crops take many distinct values and sum to the frame's totals, and a
degrading refit raises the frame's byte sum.  Everything that can be checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

import cost_ref as CR
import helpers
import refit_ref as R
from oracle import rzo
from rayzen_amd import _lib
from rayzen_amd import scene as S
from test_rays_abi import _kernel_metadata

F32 = np.float32


def test_cost_structs_sizes_offsets_and_symbols():
    L = _lib.hip()
    assert (_lib.SIZEOF_PIXEL_COST, _lib.SIZEOF_COST_PARAMS, _lib.SIZEOF_COST_VIEW_PARAMS, _lib.SIZEOF_COST_STATS) == (28, 29, 30, 31)
    for which, struct in ((28, _lib.PixelCost), (29, _lib.CostParams), (30, _lib.CostViewParams), (31, _lib.CostStats)):
        assert L.rz_sizeof(which) == 32 == C.sizeof(struct), (which, struct)
    assert L.rz_sizeof(25) == 0 and L.rz_sizeof(27) == 0 and L.rz_sizeof(32) == 0
    want = {
        _lib.PixelCost: {"traversals": 0, "tlas_nodes": 4, "tlas_leaf_indices": 8, "instances": 12, "blas_nodes": 16, "triangles": 20,
                         "materials": 24, "light_fetches": 28},
        _lib.CostParams: {"spp": 0, "reserved": 4},
        _lib.CostViewParams: {"metric": 0, "curve": 4, "scale": 8, "reserved": 12},
        _lib.CostStats: {"max_value": 0, "sum_value": 8, "max_x": 16, "max_y": 20, "scale_used": 24, "reserved": 28},
    }
    for struct, offs in want.items():
        assert [f for f, _ in struct._fields_] == list(offs), struct
        for f, off in offs.items():
            assert getattr(struct, f).offset == off, (struct, f)
    assert _lib.PIXEL_COST_DTYPE.itemsize == 32 and _lib.PIXEL_COST_DTYPE.names == tuple(want[_lib.PixelCost])
    assert [_lib.PIXEL_COST_DTYPE.fields[f][1] for f in _lib.PIXEL_COST_DTYPE.names] == list(want[_lib.PixelCost].values())
    assert _lib.COST_HOST == 1 and _lib.COST_DEFAULTS == dict(spp=0) and _lib.COST_VIEW_DEFAULTS == dict(metric=0, curve=0, scale=0.0)
    assert _lib.COST_METRICS == {"bytes": 0, "nodes": 1, "triangles": 2, "traversals": 3, "instances": 4}
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5       # additive: the revision stays
    lib = C.CDLL(_lib.HIP_SO)
    for name in ("rz_render_cost", "rz_cost_view", "rz_present_cost"):
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name
    from rayzen_amd.renderer import PIXEL_COST_DTYPE, Renderer
    assert PIXEL_COST_DTYPE is _lib.PIXEL_COST_DTYPE
    for m in ("render_cost", "render_cost_device", "cost_view", "cost_view_device", "present_cost"):
        assert callable(getattr(Renderer, m)), m


def test_cost_kernels_spill_nothing():
    """rz_cost_view and the two reduce kernels: no spill, no scratch.  rz_cost_pixels is the one-lane-per-pixel path loop, whose
    register budget (2 waves per SIMD) is rz_render_pixels': its figures are printed, not bounded."""
    meta = _kernel_metadata(_lib.HIP_SO)
    cost = {k: v for k, v in meta.items() if "rz_cost_" in k}
    small = {k: v for k, v in cost.items() if "rz_cost_pixels" not in k}
    assert len(small) == 3 and all(any(n in k for k in small) for n in ("rz_cost_view", "rz_cost_reduce_partials", "rz_cost_reduce_final")), sorted(cost)
    for name, (spill, priv) in small.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"
    pixels = {k: v for k, v in cost.items() if "rz_cost_pixels" in k}
    assert len(pixels) == 1, sorted(cost)
    for name, (spill, priv) in {**pixels, **{k: v for k, v in meta.items() if "rz_render_pixels" in k}}.items():
        print(f"{name}: {spill} VGPRs spilled, {priv} B of scratch")


# ---------------------------------------------------------------------------------------------------------------------
# the restatement on hand-made records

def _with_bytes(values):
    """Records whose byte value is 16 + 32 k: k blas_nodes each."""
    v = np.asarray(values, np.uint64)
    cols = np.zeros(v.shape + (8,), np.uint64)
    cols[..., 4] = v
    return CR.records(cols)


def test_ref_value_per_metric():
    rec = CR.records(np.array([[[1, 2, 3, 4, 5, 6, 7, 8]]]))
    assert int(CR.value(rec, "bytes")[0, 0]) == 32 * 2 + 4 * 3 + 144 * 4 + 32 * 5 + 68 * 6 + 32 * 7 + 32 * 8 + 16
    assert [int(CR.value(rec, m)[0, 0]) for m in ("nodes", "triangles", "traversals", "instances")] == [7, 6, 1, 4]
    top = CR.records(np.full((1, 1, 8), 0xFFFFFFFF))
    assert int(CR.value(top, 0)[0, 0]) == (32 + 4 + 144 + 32 + 68 + 32 + 32) * 0xFFFFFFFF + 16         # no wrap in uint64
    # the frame's sum is the oracle's algorithmic_bytes of the column sums with pixels = the pixel count
    rng = np.random.default_rng(5)
    rec = CR.records(rng.integers(0, 800, (5, 7, 8)))
    tot = {f: int(rec[f].sum()) for f in CR.FIELDS}
    tot["pixels"] = 35
    assert CR.stats(rec)["sum_value"] == rzo.algorithmic_bytes(tot)


def test_ref_the_five_stops_exactly_and_the_maximum_is_red():
    # triangle counts 0, 1, 2, 3, 4 under the "triangles" metric: u = 0, 1/4, 1/2, 3/4, 1
    cols = np.zeros((1, 5, 8), np.int64)
    cols[0, :, 5] = np.arange(5)
    rec = CR.records(cols)
    c = CR.colour(rec, "triangles")
    assert np.array_equal(c[0], CR.STOPS) and c.dtype == F32
    st = CR.stats(rec, "triangles")
    assert st == dict(max_value=4, sum_value=10, max_x=4, max_y=0, scale_used=4.0)
    # halfway between two stops
    c = CR.colour(rec, "triangles", scale=8.0)
    assert np.array_equal(c[0, 1], (0, 0, 0.5)) and np.array_equal(c[0, 3], (0, 0.5, 0.5)) and np.array_equal(c[0, 4], (0, 1, 0))
    # the logarithmic curve has the same ends
    c = CR.colour(rec, "triangles", curve="log")
    assert np.array_equal(c[0, 0], (0, 0, 0)) and np.array_equal(c[0, 4], (1, 0, 0)) and (np.diff(c[0, :, 0]) >= 0).all()


def test_ref_white_above_a_caller_scale_and_ties_go_to_the_lowest_index():
    rec = _with_bytes([[1, 9, 3], [9, 2, 9]])
    st = CR.stats(rec)
    assert (st["max_value"], st["max_x"], st["max_y"]) == (16 + 32 * 9, 1, 0) and st["sum_value"] == 6 * 16 + 32 * 33
    c = CR.colour(rec, scale=float(16 + 32 * 3))
    assert (c[rec["blas_nodes"] == 9] == 1).all()                           # above the scale: white
    assert np.array_equal(c[0, 2], (1, 0, 0))                               # at the scale: red
    assert CR.stats(rec, scale=100.0)["scale_used"] == 100.0
    assert (CR.colour(rec)[rec["blas_nodes"] == 9] == (1, 0, 0)).all()      # auto scale: the maxima are red, none white


def test_ref_values_above_2_pow_24_and_an_all_zero_frame():
    big = CR.records(np.array([[[0, 0, 0, 0, 0x00FFFFFF, 0, 0, 0], [0, 0, 0, 0, 0x01000001, 0, 0, 0], [0, 0, 0, 0, 5, 0, 0, 0]]]))
    v = CR.value(big, "nodes")
    assert int(v[0, 1]) == (1 << 24) + 1 and F32(v[0, 1]) == F32(1 << 24)   # binary32 cannot hold it: it rounds to even
    st = CR.stats(big, "nodes")
    assert st["max_value"] == (1 << 24) + 1 and st["max_x"] == 1 and st["scale_used"] == float(1 << 24)
    c = CR.colour(big, "nodes")
    assert np.array_equal(c[0, 1], (1, 0, 0)) and not (c == 1).all(axis=-1).any()
    bytes_ = CR.value(big, "bytes")
    assert int(bytes_.max()) > (1 << 29) and CR.stats(big)["sum_value"] == int(bytes_.sum())
    zero = np.zeros((3, 4), CR.DTYPE)
    for m in ("nodes", "triangles", "traversals", "instances"):
        st = CR.stats(zero, m)
        assert st == dict(max_value=0, sum_value=0, max_x=0, max_y=0, scale_used=1.0)
        assert (CR.colour(zero, m) == 0).all() and (CR.colour(zero, m, "log") == 0).all()
    assert CR.stats(zero)["max_value"] == 16 and (CR.colour(zero) == (1, 0, 0)).all()     # bytes: every pixel pays its own 16


# ---------------------------------------------------------------------------------------------------------------------
# the oracle alone: the GPU test's cases bite

@pytest.mark.parametrize("name", sorted(CR.CASES))
def test_oracle_crops_sum_to_the_frame_and_take_many_values(name):
    sc, w, h, spp, bounces, rec, total = CR.case(name)
    _, frame = helpers.oracle_render(sc, w, h, spp, bounces, want_counters=True)
    first_ten = rzo.COUNTER_FIELDS[:10]
    assert {n: total[n] for n in first_ten} == {n: frame[n] for n in first_ten}
    assert total["samples"] == w * h * spp and total["pixels"] == w * h
    v = CR.value(rec, "bytes")
    distinct, (lo, hi) = CR.CASES[name][5:]
    print(f"{name}: {len(np.unique(v))} distinct byte values, {int(v.min())} .. {int(v.max())}; largest counter {max(int(rec[f].max()) for f in CR.FIELDS)}")
    # (the recorded ranges are the traversal's bytes alone, without the 16 of the pixel's own RGBA32F write)
    assert len(np.unique(v)) == distinct and (int(v.min()) - 16, int(v.max()) - 16) == (lo, hi)
    assert max(int(rec[f].max()) for f in CR.FIELDS) <= 761
    assert int(v.sum()) == rzo.algorithmic_bytes(frame) == CR.stats(rec)["sum_value"]


def test_oracle_a_degrading_refit_raises_the_byte_sum():
    """The blob displaced by a wobble and refitted through rzh_scene_refit_mesh keeps its tree's topology: the boxes grow and
    overlap, and the same camera pays more bytes.  (8 x 6 pixels: a frame total, not the GPU test's per-pixel case.)"""
    sc = S.bunny_scene(n=12, aspect=4 / 3)
    w, h, spp, bounces = 16, 12, 1, 2
    _, before = helpers.oracle_render(sc, w, h, spp, bounces, want_counters=True)
    blob = S.make_blob(12, 2.8, 0)
    sc.refit_mesh(1, R.wobble(blob, 0.5))
    _, refitted = helpers.oracle_render(sc, w, h, spp, bounces, want_counters=True)
    sc.rebuild_mesh(1)
    _, rebuilt = helpers.oracle_render(sc, w, h, spp, bounces, want_counters=True)
    b0, b1, b2 = (rzo.algorithmic_bytes(c) for c in (before, refitted, rebuilt))
    print(f"bytes: built {b0}, wobbled and refitted {b1} (x{b1 / b0:.3f}), rebuilt {b2} (x{b2 / b0:.3f})")
    assert b1 > b0 and b2 < b1

"""rz_coverage and rz_outline without a GPU: the C-ABI structs and symbols, the code-object metadata of the new kernels, the
restatement (coverage_ref.py) on hand-made id images, and -- with the CPU oracle alone -- that the cases the GPU test runs
(coverage_cases.py) exercise what they claim.  The figures in the last group are conditions on the inputs, computed with the
oracle; they are not measurements of the device."""
import ctypes as C

import numpy as np
import pytest

import coverage_cases as CC
import coverage_ref as CR
import tie_cases as TC
from rayzen_amd import _lib
from test_rays_abi import _kernel_metadata

F32 = np.float32


def test_structs_sizes_offsets_and_symbols():
    L = _lib.hip()
    assert (_lib.SIZEOF_COVERAGE_PARAMS, _lib.SIZEOF_INSTANCE_COVERAGE, _lib.SIZEOF_OUTLINE_PARAMS) == (33, 34, 35)
    for which, struct in ((33, _lib.CoverageParams), (34, _lib.InstanceCoverage), (35, _lib.OutlineParams)):
        assert L.rz_sizeof(which) == 32 == C.sizeof(struct), (which, struct)
    for which in (13, 16, 19, 22, 25, 27, 32):              # the unassigned indices stay unknown
        assert L.rz_sizeof(which) == 0, which
    want = {
        _lib.CoverageParams: {"x0": 0, "y0": 4, "x1": 8, "y1": 12, "reserved": 16},
        _lib.InstanceCoverage: {"pixels": 0, "x_min": 4, "y_min": 8, "x_max": 12, "y_max": 16, "t_min": 20, "t_max": 24, "reserved": 28},
        _lib.OutlineParams: {"width": 0, "height": 4, "radius": 8, "color": 12, "alpha": 24, "reserved": 28},
    }
    for struct, offs in want.items():
        assert [f for f, _ in struct._fields_] == list(offs), struct
        for f, off in offs.items():
            assert getattr(struct, f).offset == off, (struct, f)
    dt = _lib.INSTANCE_COVERAGE_DTYPE
    assert dt.itemsize == 32 and dt.names == tuple(want[_lib.InstanceCoverage])
    assert [dt.fields[f][1] for f in dt.names] == list(want[_lib.InstanceCoverage].values())
    assert _lib.COVERAGE_HOST == 1 and _lib.OUTLINE_HOST == 1
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5      # additive: the revision stays
    lib = C.CDLL(_lib.HIP_SO)
    for name in ("rz_coverage", "rz_outline"):
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name
    from rayzen_amd.renderer import INSTANCE_COVERAGE_DTYPE, Renderer
    assert INSTANCE_COVERAGE_DTYPE is dt
    for m in ("coverage", "coverage_device", "select_rect", "outline", "outline_device", "selection_bits", "n_instances"):
        assert callable(getattr(Renderer, m)), m


def test_kernels_spill_nothing():
    """No kernel of the two files spills a VGPR or uses scratch.  rz_coverage_runs carries the closest-hit walk and, on top of it,
    a lane's entry of the wave's table (a key and seven words) at the other casts' register budget of four waves per SIMD: it is
    held to rz_denoise_guides' figures, which are zero."""
    meta = _kernel_metadata(_lib.HIP_SO)
    ours = {k: v for k, v in meta.items() if any(n in k for n in ("rz_coverage_init", "rz_coverage_merge", "rz_coverage_runs", "rz_outline_kernel"))}
    assert len(ours) == 5, sorted(ours)                     # rz_coverage_runs with and without the overflow columns of the BLAS stack
    guides = {k: v for k, v in meta.items() if "rz_denoise_guides" in k}
    assert len(guides) == 2 and all(v == (0, 0) for v in guides.values()), guides
    for name, (spill, priv) in ours.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


# ---------------------------------------------------------------------------------------------------------------------
# the restatement on hand-made images

def test_ref_records_of_a_hand_made_image():
    ids = np.array([[0, 0, -1, 2], [0, -1, -1, 2], [5, 5, 5, 2]], np.int32)
    t = np.where(ids >= 0, np.arange(12, dtype=F32).reshape(3, 4) + F32(1.5), F32(1e30)).astype(F32)
    rec = CR.records(ids, t, 6)
    assert rec["pixels"].tolist() == [3, 0, 3, 0, 0, 3, 3] and int(rec["pixels"].sum()) == 12
    assert rec[0].tolist() == (3, 0, 0, 1, 1, 1.5, 5.5, 0)
    assert rec[2].tolist() == (3, 3, 0, 3, 2, 4.5, 12.5, 0)
    assert rec[5].tolist() == (3, 0, 2, 2, 2, 9.5, 11.5, 0)
    assert rec[6].tolist() == (3, 1, 0, 2, 1, F32(1e30), 0.0, 0)      # the misses: pixels and box, t as in an empty record
    for k in (1, 3, 4):
        assert rec[k].tobytes() == CR.empty_records(0)[0].tobytes()
    assert CR.empty_records(0)[0].tolist() == (0, 0x7fffffff, 0x7fffffff, -1, -1, F32(1e30), 0.0, 0)
    # rectangles: clipped, and empty after clipping
    sub = CR.records(ids, t, 6, (1, 1, 9, 9))
    assert sub["pixels"].tolist() == [0, 0, 2, 0, 0, 2, 2] and sub[5].tolist() == (2, 1, 2, 2, 2, 10.5, 11.5, 0)
    assert CR.area((1, 1, 9, 9), 4, 3) == 6 == int(sub["pixels"].sum())
    for rect in ((4, 0, 8, 3), (2, 1, 2, 3), (-5, -5, 0, 0)):
        assert CR.records(ids, t, 6, rect).tobytes() == CR.empty_records(6).tobytes() and CR.area(rect, 4, 3) == 0
    assert CR.expected_ids(ids, (1, 1, 9, 9), 77).tolist() == [[77, 77, 77, 77], [77, -1, -1, 2], [77, 5, 5, 2]]
    with pytest.raises(AssertionError):
        CR.clip((3, 0, 2, 1), 4, 3)


def test_ref_select_order():
    rec = CR.empty_records(6)
    rec["pixels"] = [7, 0, 9, 7, 1, 9, 100]                 # (the last record is the misses: never selected)
    assert CR.select_order(rec) == [(2, 9), (5, 9), (0, 7), (3, 7), (4, 1)]
    assert CR.select_order(rec, 7) == [(2, 9), (5, 9), (0, 7), (3, 7)]
    assert CR.select_order(rec, 0) == CR.select_order(rec, 1) and CR.select_order(rec, 10) == []


def test_ref_bitset_and_selection():
    words = CR.bitset([0, 31, 32, 37, 38, 99, -1], 38)      # 38 instances: two words; 38, 99 and -1 are outside
    assert words.tolist() == [0x80000001, 0x21]
    ids = np.array([[0, 31, 32, 37, 38, 40, 63, 64, -1, 1, 0x7fffffff, -0x80000000]], np.int32)
    assert CR.sel_mask(ids, words, 38).tolist() == [[True, True, True, True, False, False, False, False, False, False, False, False]]
    assert not CR.sel_mask(ids, CR.bitset([], 0), 0).any()


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_ref_outline_of_a_corner_pixel(radius):
    ids, n, sel = CC.OUTLINE_CASES["corner"]
    m = CR.outline_mask(ids, CR.bitset(sel, n), n, radius)
    want = np.zeros(ids.shape, bool)
    want[:radius + 1, :radius + 1] = True
    want[0, 0] = False                                      # the selected pixel itself is no outline pixel
    assert (m == want).all() and int(m.sum()) == (radius + 1) ** 2 - 1


def test_ref_outline_at_borders_and_out_of_range_ids():
    ids, n, sel = CC.OUTLINE_CASES["border"]
    m = CR.outline_mask(ids, CR.bitset(sel, n), n, 2)
    region = np.isin(ids, sel)
    assert not (m & region).any() and m[3:10, 13:15].all() and m[1:3, 13:20].all() and not m[4:, :12].any()
    assert m[2:4, 0:8].all() and m[0:2, 6:8].all() and not m[4, 0:8].any()
    ids, n, sel = CC.OUTLINE_CASES["out-of-range"]
    assert n % 32 != 0
    s = CR.sel_mask(ids, CR.bitset(sel, n), n)
    assert s[5:8, 8:12].all() and s[1, 12] and int(s.sum()) == 13          # 7 and 37; 40, 38, INT_MAX and INT_MIN are not
    m = CR.outline_mask(ids, CR.bitset(sel, n), n, 1)
    assert not m[2:5, 2:5].any() and m[0, 11] and m[2, 13] and not m[8, 0] and not m[7, 1]
    for name in ("one-pixel", "one-pixel-unselected", "nothing-selected"):
        ids, n, sel = CC.OUTLINE_CASES[name]
        assert not CR.outline_mask(ids, CR.bitset(sel, n), n, 4).any(), name
    for name in ("65x5", "257x3"):
        ids, n, sel = CC.OUTLINE_CASES[name]
        m = CR.outline_mask(ids, CR.bitset(sel, n), n, 4)
        cols = np.flatnonzero(m.any(axis=0))
        assert m.any() and {31, 32, 33} <= set(cols.tolist()), name        # outline pixels on both sides of a 32-pixel tile border


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_ref_blend(alpha):
    ids, n, sel = CC.OUTLINE_CASES["border"]
    rgb, rgba8 = CC.images_for(ids)
    rgb[0, 19] = np.nan                                     # not an outline pixel
    m = CR.outline_mask(ids, CR.bitset(sel, n), n, 2)
    assert not m[0, 19]
    color = (1.0, 0.6, 0.0)
    out = CR.outline_rgb32f(rgb, m, color, alpha)
    out8 = CR.outline_rgba8(rgba8, m, color, alpha)
    assert out.dtype == F32 and out8.dtype == np.uint8
    assert out[~m].tobytes() == rgb[~m].tobytes() and out8[~m].tobytes() == rgba8[~m].tobytes()
    assert (out8[..., 3] == rgba8[..., 3]).all()
    if alpha == 0.0:        # in * 1 + color * 0: the floats keep their values, the bytes make the round trip byte / 255 * 255
        assert (out == rgb)[~np.isnan(rgb)].all() and out8.tobytes() == rgba8.tobytes()
    if alpha == 1.0:        # in * 0 + color: the colour itself (a finite input), quantised as rz_present quantises
        assert (out[m] == np.asarray(color, F32)).all() and (out8[m][:, :3] == [255, 153, 0]).all()
    if alpha == 0.5:
        k = tuple(np.argwhere(m)[0])
        want = rgb[k] * F32(0.5) + np.asarray(color, F32) * F32(0.5)
        assert out[k].tobytes() == want.astype(F32).tobytes()
        b = rgba8[k][:3].astype(F32) / F32(255) * F32(0.5) + np.asarray(color, F32) * F32(0.5)
        assert out8[k][:3].tolist() == np.rint(b * F32(255)).astype(int).tolist()


def test_ref_rgba8_round_trip():
    """rint((byte / 255) * 255) is the byte for all 256 values in binary32: alpha = 0 keeps an rgba8 image byte for byte."""
    b = np.arange(256, dtype=np.uint8)
    assert (np.rint(b.astype(F32) / F32(255.0) * F32(255.0)).astype(np.uint8) == b).all()


# ---------------------------------------------------------------------------------------------------------------------
# the cases bite (the oracle alone)

def _records(name):
    sc, w, h, ids, t = CC.case(name)
    return CR.records(ids, t, CC.n_instances(sc)), ids


def test_case_reference_has_big_small_and_absent_instances():
    rec, _ = _records("reference")
    px = rec["pixels"]
    assert [int(px[k]) for k in (0, 1, 2, 4)] == [1300, 42, 35, 109] and int(px[-1]) == 1586
    assert int((px[:-1] == 0).sum()) >= 2 and int(px.sum()) == 64 * 48


def test_case_instanced_has_tiny_instances_and_busy_tiles():
    rec, ids = _records("instanced")
    px = rec["pixels"]
    assert len(px) == 18 and (px[:-1] > 0).all()            # all 16 instances and the floor
    assert int(px[1:-1].min()) <= 3 and CC.tile_keys(ids) >= 9


def test_case_lattice_drives_the_grouping_loop():
    rec, ids = _records("lattice")
    assert len(rec) == 193 and (rec["pixels"][:-1] > 0).all()
    assert CC.tile_keys(ids) >= 24


def test_case_axis_hides_an_instance():
    rec, _ = _records("axis")
    assert rec["pixels"][0] > 0 and rec[1].tobytes() == CR.empty_records(0)[0].tobytes()


def test_case_ties_depend_on_the_visiting_order():
    rec, _ = _records("ties")
    other = TC.scene("stack", 1)
    ids1, t1 = CC.images("ties-order-1", other, 64, 48)
    rec1 = CR.records(ids1, t1, CC.n_instances(other))
    assert rec.tobytes() != rec1.tobytes() and rec["pixels"].tolist() != rec1["pixels"].tolist()
    assert int(rec["pixels"].sum()) == int(rec1["pixels"].sum()) == 64 * 48


def test_rectangles_cover_what_they_claim():
    for w, h in [(65, 5), (48, 36)]:
        r = CC.rectangles(w, h)
        assert CR.area(r["whole"], w, h) == CR.area(r["stated"], w, h) == w * h and CR.area(r["pixel"], w, h) == 1
        x0, y0, x1, y1 = r["crossing"]
        assert x0 % 8 and x1 % 8 and x0 // 8 != (x1 - 1) // 8 and CR.area(r["crossing"], w, h) == 30
        assert 0 < CR.area(r["partly-outside"], w, h) < 14 * 6
        assert CR.area(r["outside"], w, h) == 0 == CR.area(r["degenerate"], w, h)

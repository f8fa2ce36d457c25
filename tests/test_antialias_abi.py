"""Edge anti-aliasing (rz_antialias): the C-ABI struct, properties of the restatement (antialias_ref.py) on hand-made guide records
-- every clause of DIFFERENT on its own, the coverage mix, bad pixels -- and the quality on frames of the CPU oracle against the
oracle's own frame at twice the size, box-averaged.  Everything that can be checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

import antialias_ref as AR
import denoise_ref as DR
import helpers
from rayzen_amd import _lib
from rayzen_amd import scene as S
from test_denoise_abi import _mats, _oracle_guides
from test_upscale_abi import INV_PROJ, _miss, _plane

F32 = np.float32


def test_antialias_params_size_and_offsets():
    L = _lib.hip()
    assert L.rz_sizeof(_lib.SIZEOF_ANTIALIAS_PARAMS) == 32 and _lib.SIZEOF_ANTIALIAS_PARAMS == 26 and C.sizeof(_lib.AntialiasParams) == 32
    want = {"factor": 0, "sigma_normal": 4, "sigma_plane": 8, "demodulate": 12, "edge_normal": 16, "edge_plane": 20, "reserved": 24}
    assert [f for f, _ in _lib.AntialiasParams._fields_] == list(want)
    for f, off in want.items():
        assert getattr(_lib.AntialiasParams, f).offset == off, f
    assert _lib.ANTIALIAS_HOST == 1
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5       # additive: the revision stays
    lib = C.CDLL(_lib.HIP_SO)
    for name in ("rz_antialias", "rz_present_antialiased"):
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name
    assert L.rz_sizeof(25) == 0 and L.rz_sizeof(27) == 0
    assert AR.DEFAULTS == {**_lib.ANTIALIAS_DEFAULTS, "demodulate": True}


# ---------------------------------------------------------------------------------------------------------------------
# properties of the restatement on hand-made guides (test_upscale_abi.py's plane: a 1 x 1 window at z = -depth, 90-degree field)

def _split(h, w, s, edge_hi):
    """A plane whose high columns >= edge_hi are sky, at both sizes; a low pixel is a hit or a miss by its centre."""
    hi = _miss(_plane(h * s, w * s), np.s_[:, edge_hi:])
    lo = _plane(h, w)
    lo = _miss(lo, np.broadcast_to(((np.arange(w) * s + s / 2.0) > edge_hi)[None, :], (h, w)).copy())
    return lo, hi


def test_ref_factor_1_is_the_identity():
    rng = np.random.default_rng(1)
    c = rng.random((6, 7, 3)).astype(F32)
    c[2, 3, 1] = np.nan
    lo, _ = _split(6, 7, 2, 7)
    out, edge = AR.antialias(c, lo, None, _mats((0.5, 0.6, 0.7)), INV_PROJ, factor=1)
    assert np.array_equal(out, c.astype(np.float64), equal_nan=True)
    assert edge[2, 3] and edge[:, 3].all() and edge[:, 4].all() and not edge[[0, 1, 3, 4, 5], :3].any()      # classified all the same


@pytest.mark.parametrize("s", [2, 3, 4])
def test_ref_constant_stays_constant_on_any_guides_borders_included(s):
    h, w = 5, 7
    const = np.full((h, w, 3), 0.3, F32)
    rng = np.random.default_rng(s)
    for k in range(3):
        lo, hi = _plane(h, w), _plane(h * s, w * s)
        if k:                                           # random silhouettes at the high size; the low pixel takes a sub-pixel's record
            sky = rng.random((h * s, w * s)) < 0.3
            hi = _miss(hi, sky)
            hi["normal"][~sky] = (0.0, 0.6, 0.8) if k == 2 else (0.0, 0.0, 1.0)
            lo = hi[s // 2::s, s // 2::s].copy()
        out, edge = AR.antialias(const, lo, hi, _mats((1.0, 1.0, 1.0)), INV_PROJ, factor=s, demodulate=False)
        assert out.shape == (h, w, 3) and (k == 0) == (not edge.any())
        assert np.allclose(out, F32(0.3), rtol=1e-12, atol=0)


@pytest.mark.parametrize("s", [2, 3])
def test_ref_flat_pixels_are_bit_identical_to_the_input(s):
    rng = np.random.default_rng(3)
    h, w = 6, 12
    c = rng.random((h, w, 3)).astype(F32)
    lo, hi = _split(h, w, s, 5 * s + 1)
    out, edge = AR.antialias(c, lo, hi, _mats((0.5, 0.6, 0.7)), INV_PROJ, factor=s)
    m = int(np.argmax(lo["instance"][0] < 0))           # the first sky column: it and the column before it are the edge
    assert 0 < m < w - 1 and np.array_equal(edge, np.isin(np.arange(w), (m - 1, m))[None, :].repeat(h, 0))
    assert np.array_equal(out[~edge], c[~edge].astype(np.float64))
    assert (out[edge] != c[edge]).any()


def test_ref_coverage_mix_on_a_silhouette_through_a_pixel_column():
    """The silhouette runs through the middle of low column 3 (in front of high column 7): its left sub-pixel column is the plane,
    its right one the sky.  With colours A on the plane and B on the sky and demodulate = 0 the column comes out as (A + B) / 2,
    its coverage-weighted mix; column 4, all sky but next to a hit, stays B; hits and misses exchange nothing elsewhere."""
    h, w, s = 4, 8, 2
    lo, hi = _split(h, w, s, 7)
    assert (lo["instance"][:, 3] >= 0).all() and (lo["instance"][:, 4] < 0).all()
    A, B = np.array([0.2, 0.4, 0.8], F32), np.array([1.0, 0.5, 0.25], F32)
    c = np.where((lo["instance"] >= 0)[..., None], A, B).astype(F32)
    out, edge = AR.antialias(c, lo, hi, _mats((0.5, 0.25, 1.0)), INV_PROJ, factor=s, demodulate=False)
    assert np.array_equal(edge, np.isin(np.arange(w), (3, 4))[None, :].repeat(h, 0))
    mix = (A.astype(np.float64) + B.astype(np.float64)) / 2
    assert np.allclose(out[:, 3], mix, rtol=1e-12, atol=0)
    assert np.array_equal(out[:, :3], np.broadcast_to(A.astype(np.float64), (h, 3, 3)))
    assert np.allclose(out[:, 4], B, rtol=1e-12, atol=0) and np.array_equal(out[:, 5:], np.broadcast_to(B.astype(np.float64), (h, 3, 3)))


def _edges(g, mats=None, c=None, **kw):
    c = np.zeros(g.shape + (3,), F32) if c is None else c
    return AR.edge_mask(c, g, _mats((1.0, 1.0, 1.0), (0.5, 0.5, 0.5)) if mats is None else mats, INV_PROJ, **kw)


def test_different_hit_and_miss_and_the_image_borders():
    g = _plane(5, 6)
    assert not _edges(g).any()                          # borders: the neighbours outside the image do not count
    g = _miss(g, np.s_[0, 0])
    want = np.zeros((5, 6), bool)
    want[:2, :2] = True                                 # the corner and its three neighbours, each way round
    assert np.array_equal(_edges(g), want)
    assert not _edges(_miss(_plane(5, 6), np.s_[:, :])).any()       # sky next to sky


def test_different_material_step_on_the_clamped_word():
    g = _plane(4, 8)
    g["material"][:, 4:] = 1
    want = np.isin(np.arange(8), (3, 4))[None, :].repeat(4, 0)
    assert np.array_equal(_edges(g), want)
    assert not _edges(g, mats=_mats((1.0, 1.0, 1.0))).any()         # one material: both words clamp to 0
    g["material"][:, 4:] = 7
    assert np.array_equal(_edges(g), want)                          # 7 clamps to 1


def test_different_crease_just_under_and_just_over_edge_normal():
    g = _plane(4, 8)
    g["normal"][:, 4:] = (0.6, 0.0, 0.8)
    nd = (F32(0.0) * F32(0.6) + F32(0.0) * F32(0.0)) + F32(1.0) * F32(0.8)
    want = np.isin(np.arange(8), (3, 4))[None, :].repeat(4, 0)
    big = 1e6                                           # (the tilted side sees its neighbours off its plane: keep that clause out)
    assert not _edges(g, edge_normal=nd, edge_plane=big).any()      # nd < edge_normal fails at equality
    assert np.array_equal(_edges(g, edge_normal=np.nextafter(nd, F32(1)), edge_plane=big), want)
    assert not _edges(g, edge_normal=np.nextafter(nd, F32(-1)), edge_plane=big).any()
    assert not _edges(g, edge_normal=-1.0, edge_plane=big).any()    # nothing is below -1


def test_different_plane_step_just_under_and_just_over_edge_plane():
    """h = 4 and inv_proj[5] = 1: f = 1 / 2, so k_e = edge_plane / 2 and, with t = 5 on both sides, the bound is 2.5 edge_plane.
    The step is 2.5 deep: pd = 2.5 exactly, and pd > k_e t fails at edge_plane = 1 and holds one ulp below it."""
    g = _plane(4, 8)
    g["point"][:, 4:, 2] = -7.5
    want = np.isin(np.arange(8), (3, 4))[None, :].repeat(4, 0)
    assert not _edges(g, edge_plane=1.0).any()
    assert np.array_equal(_edges(g, edge_plane=np.nextafter(F32(1), F32(0))), want)
    assert not _edges(g, edge_plane=np.nextafter(F32(1), F32(2))).any()
    assert np.array_equal(_edges(g, edge_plane=0.0), want)          # 0: any step off the plane counts, none on it
    # the bound scales with t_p: the near side (t = 5) sees the step, the far side (t = 10) does not
    g["t"][:, 4:] = 10.0
    assert np.array_equal(_edges(g, edge_plane=0.75), np.isin(np.arange(8), (3,))[None, :].repeat(4, 0))  # 1.875 < 2.5 < 3.75


def test_a_1x1_frame_is_flat_unless_it_is_bad():
    g = _plane(1, 1)
    assert not _edges(g).any() and not _edges(_miss(_plane(1, 1), np.s_[:, :])).any()
    c = np.zeros((1, 1, 3), F32)
    c[0, 0, 2] = np.inf
    assert _edges(g, c=c).all()
    out, edge = AR.antialias(c, g, _plane(2, 2), _mats((1.0, 1.0, 1.0)), INV_PROJ)
    assert edge.all() and (out == 0).all()              # no tap, and stage 3 reads the bad pixel as black


BAD_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("value", sorted(BAD_VALUES))
def test_ref_bad_pixels_are_edges_and_contained(value, s):
    """An isolated bad pixel, the corner and a 5 x 5 block, on a plane with a silhouette.  They are edge pixels, the output is
    finite, and a pixel with no bad pixel within two pixels of it -- the reach of its sub-samples' 4 x 4 windows -- is bit for bit
    what the clean frame gives."""
    rng = np.random.default_rng(11)
    h, w = 16, 20
    lo, hi = _split(h, w, s, 17 * s - 1)
    mats = _mats((0.5, 0.6, 0.7))
    clean = rng.random((h, w, 3)).astype(F32)
    bad = np.zeros((h, w), bool)
    bad[3, 14] = bad[0, 0] = True
    bad[8:13, 4:9] = True
    c = clean.copy()
    c[bad, 1] = BAD_VALUES[value]
    c[3, 14] = BAD_VALUES[value]
    assert np.array_equal(DR.bad_pixels(c), bad)
    near = np.zeros((h, w), bool)
    for y, x in zip(*np.nonzero(bad)):
        near[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = True
    for demod in (True, False):
        out, edge = AR.antialias(c, lo, hi, mats, INV_PROJ, factor=s, demodulate=demod)
        want, edge0 = AR.antialias(clean, lo, hi, mats, INV_PROJ, factor=s, demodulate=demod)
        assert np.isfinite(out).all()
        assert np.array_equal(edge, edge0 | bad) and edge0.any() and not (edge0 & bad).any()
        assert (~near).any() and np.array_equal(out[~near], want[~near])
        assert (out[10, 6] == 0).all()                  # the middle of the block: every tap within reach is bad


# ---------------------------------------------------------------------------------------------------------------------
# quality on the oracle's frames (the GPU's frames equal the oracle's bit for bit)
#
# The truth is the oracle's frame at twice the size, box-averaged, and the figure is the mean absolute error on the edge pixels,
# s = 2.  MEASURED_1B: 160 x 120 at 1 spp and 1 bounce (noise-free shading), truth 320 x 240 likewise.  MEASURED_NOISY: 80 x 60 at
# 8 spp and 5 bounces, truth 160 x 120 at 64 spp.  The pixels classed flat carry 0.0012 to 0.0020 against the same truth.

QUALITY_SCENES = {"cornell": lambda: S.cornell_scene(), "reference": lambda: S.reference_scene(aspect=4 / 3),
                  "bunny": lambda: S.bunny_scene(extras=True)}
# scene: (edge share, input error, output error) as measured with this restatement (DESIGN.md 4.3 has the table)
MEASURED_1B = {"cornell": (0.069, 0.0426, 0.00135), "reference": (0.053, 0.0238, 0.00592), "bunny": (0.062, 0.0476, 0.00497)}
MEASURED_NOISY = {"cornell": (0.136, 0.057, 0.020), "reference": (0.092, 0.037, 0.019), "bunny": (0.128, 0.055, 0.017)}


def _edge_errors(sc, w, h, spp, bounces, truth_spp, s=2):
    frame = DR.resolve(helpers.oracle_render(sc, w, h, spp, bounces))
    truth = AR.box_mean(DR.resolve(helpers.oracle_render(sc, w * s, h * s, truth_spp, bounces)).astype(np.float64), s)
    g, g_hi = _oracle_guides(sc, w, h), _oracle_guides(sc, w * s, h * s)
    out, edge = AR.antialias(frame, g, g_hi, sc.materials, sc.camera.inv_proj, factor=s)
    assert np.isfinite(out).all() and np.array_equal(out[~edge], frame[~edge].astype(np.float64))
    e_in = float(np.abs(frame.astype(np.float64) - truth)[edge].mean())
    e_out = float(np.abs(out - truth)[edge].mean())
    return float(edge.mean()), e_in, e_out


@pytest.mark.parametrize("name", sorted(QUALITY_SCENES))
def test_quality_one_bounce_frames(name):
    share, e_in, e_out = _edge_errors(QUALITY_SCENES[name](), 160, 120, 1, 1, 1)
    print(f"{name}: edge share {share:.3f}, mean |error| on edge pixels {e_in:.4g} -> {e_out:.4g} (ratio {e_in / e_out:.1f}); "
          f"recorded {MEASURED_1B[name]}")
    assert e_out <= 0.5 * e_in, (share, e_in, e_out)   # measured ratios 4.0 to 31.6
    assert share <= 0.15, share                        # measured 0.053 to 0.069


@pytest.mark.parametrize("name", sorted(QUALITY_SCENES))
def test_quality_noisy_frames(name):
    share, e_in, e_out = _edge_errors(QUALITY_SCENES[name](), 80, 60, 8, 5, 64)
    print(f"{name}: edge share {share:.3f}, mean |error| on edge pixels {e_in:.4g} -> {e_out:.4g} (ratio {e_in / e_out:.1f}); "
          f"recorded {MEASURED_NOISY[name]}")
    assert e_out <= e_in, (share, e_in, e_out)         # measured ratios 2.0 to 3.2

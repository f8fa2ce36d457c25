"""Guided upsampling (rz_upscale): the C-ABI struct, the kernel's register budget, properties of the float64 restatement
(upscale_ref.py) on synthetic guides, and the reconstruction's quality on frames of the CPU oracle -- everything that can be
checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as DR
import helpers
import upscale_ref as UR
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE
from test_denoise_abi import _mats, _oracle_guides
from test_rays_abi import _kernel_metadata


def test_upscale_params_size_and_offsets():
    L = _lib.hip()
    assert L.rz_sizeof(_lib.SIZEOF_UPSCALE_PARAMS) == 32 and _lib.SIZEOF_UPSCALE_PARAMS == 21 and C.sizeof(_lib.UpscaleParams) == 32
    want = {"factor": 0, "sigma_normal": 4, "sigma_plane": 8, "demodulate": 12, "reserved": 16}
    assert [f for f, _ in _lib.UpscaleParams._fields_] == list(want)
    for f, off in want.items():
        assert getattr(_lib.UpscaleParams, f).offset == off, f
    assert _lib.UPSCALE_HOST == 1
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5       # additive: the revision stays
    lib = C.CDLL(_lib.HIP_SO)
    for name in ("rz_upscale", "rz_present_upscaled"):
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name
    assert L.rz_sizeof(22) == 0


def test_upscale_kernel_spills_nothing():
    meta = _kernel_metadata(_lib.HIP_SO)
    gather = {k: v for k, v in meta.items() if "rz_upscale_gather" in k}
    assert len(gather) == 1, sorted(meta)
    for name, (spill, priv) in gather.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


# ---------------------------------------------------------------------------------------------------------------------
# properties of the restatement on synthetic guides
#
# The synthetic G-buffer is a plane z = -depth facing the camera, seen through a window of 1 x 1 world units: pixel (X, Y) of a
# W x H buffer has its point at ((X + 0.5) / W, (Y + 0.5) / H, -depth), so a low and a high buffer of one plane agree on where
# things are, as two casts of one scene do.

INV_PROJ = np.eye(4, dtype=np.float32).reshape(16)      # a 90-degree vertical field: inv_proj[5] = 1


def _plane(H, W, depth=5.0, mat=0, inst=0):
    g = np.zeros((H, W), HIT_DTYPE)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    g["t"] = depth
    g["point"][..., 0] = (xs + 0.5) / W
    g["point"][..., 1] = (ys + 0.5) / H
    g["point"][..., 2] = -depth
    g["normal"] = (0.0, 0.0, 1.0)
    g["material"] = mat
    g["instance"] = inst
    return g


def _miss(g, where):
    g["instance"][where] = -1
    g["material"][where] = -1
    g["t"][where] = 1e30
    g["point"][where] = 0
    g["normal"][where] = 0
    return g


def test_ref_factor_1_is_the_identity():
    rng = np.random.default_rng(1)
    c = rng.random((6, 7, 3)).astype(np.float32)
    c[2, 3, 1] = np.nan
    g = _plane(6, 7)
    out = UR.upscale(c, g, g, _mats((0.5, 0.6, 0.7)), INV_PROJ, factor=1)
    assert np.array_equal(out, c.astype(np.float64), equal_nan=True)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_ref_constant_stays_constant_borders_included(s):
    h, w = 5, 7
    const = np.full((h, w, 3), 0.3, np.float32)
    lo, hi = _plane(h, w), _plane(h * s, w * s)
    for demod in (True, False):
        out, stage = UR.upscale(const, lo, hi, _mats((0.5, 0.6, 0.7)), INV_PROJ, factor=s, demodulate=demod, want_stage=True)
        assert out.shape == (h * s, w * s, 3) and (stage == 1).all()
        assert np.allclose(out, np.float32(0.3), rtol=1e-12, atol=0)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_ref_hits_and_misses_never_exchange_colour(s):
    """The silhouette (in front of high column 5 s + 1) does not fall on a low pixel boundary: high column 5 s is a hit whose
    nearest low pixel is a miss.  It takes the hit taps only, and no sky pixel takes a hit tap."""
    h, w = 4, 12
    H, W = h * s, w * s
    edge = 5 * s + 1
    hi = _miss(_plane(H, W), np.s_[:, edge:])
    lo = _plane(h, w)
    lo = _miss(lo, np.broadcast_to(((np.arange(w) * s + s / 2.0) >= edge)[None, :], (h, w)).copy())     # by its centre
    c = np.where((lo["instance"] >= 0)[..., None], 0.0, 1.0).astype(np.float32)
    out = UR.upscale(c, lo, hi, _mats((1.0, 1.0, 1.0)), INV_PROJ, factor=s)
    assert (out[:, :edge] == 0).all() and (out[:, edge:] == 1).all()
    assert (lo["instance"][:, 5] < 0).all() and (hi["instance"][:, 5 * s] >= 0).all()       # ... and it is misaligned


@pytest.mark.parametrize("s", [2, 3, 4])
def test_ref_parallel_planes_bleed_no_more_than_the_floor(s):
    """Two parallel planes, one a unit behind the other, split down the middle (on a low pixel boundary): with a narrow field of
    view the plane term of a tap on the other plane is far below the floor, so the tap counts with 1e-4.  The nearest low pixel
    is always a tap on the pixel's own plane with a bilinear weight of at least 1/2 per axis, so at most 1e-4 of the other
    plane's colour arrives -- and something does, because the floor exists."""
    h, w = 4, 8
    H, W = h * s, w * s
    inv_proj = INV_PROJ.copy()
    inv_proj[5] = 1e-3
    lo, hi = _plane(h, w), _plane(H, W)
    lo[:, w // 2:] = _plane(h, w, depth=6.0, inst=1)[:, w // 2:]
    hi[:, W // 2:] = _plane(H, W, depth=6.0, inst=1)[:, W // 2:]
    c = np.zeros((h, w, 3), np.float32)
    c[:, w // 2:] = 1.0
    out = UR.upscale(c, lo, hi, _mats((1.0, 1.0, 1.0)), inv_proj, factor=s, demodulate=False)
    bleed = np.maximum(np.abs(out[:, :W // 2]).max(), np.abs(out[:, W // 2:] - 1).max())
    assert 0 < bleed <= 1.0001e-4, bleed


def test_ref_a_sliver_no_low_tap_hits_takes_stage_2_then_stage_3():
    """Everything is sky except a wide post (low column 6 = high columns 12, 13) and two slivers one high pixel wide that no low
    pixel centre lands on.  The sliver at high column 16 has the post in the ring around its footprint (low columns 6..9): stage
    2, the post's colour through the sliver's albedo.  The sliver at high column 4 has only sky within reach: stage 3, the nearest
    low pixel's colour as it is."""
    s, h, w = 2, 4, 12
    H, W = h * s, w * s
    sky = np.ones((H, W), bool)
    sky[:, [4, 12, 13, 16]] = False
    hi = _miss(_plane(H, W, mat=1), sky)
    hi["material"][:, 16] = 0
    lo_sky = np.ones((h, w), bool)
    lo_sky[:, 6] = False
    lo = _miss(_plane(h, w, mat=1), lo_sky)
    rng = np.random.default_rng(5)
    c = rng.random((h, w, 3)).astype(np.float32)
    c[:, 6] = (0.2, 0.4, 0.8)
    mats = _mats((0.5, 0.25, 1.0), (1.0, 0.5, 0.25))
    out, stage = UR.upscale(c, lo, hi, mats, INV_PROJ, factor=s, want_stage=True)
    assert (stage[:, 16] == 2).all() and (stage[:, 4] == 3).all()
    assert (np.delete(stage, [4, 16], axis=1) == 1).all()
    d_post = np.array([0.2, 0.4, 0.8], np.float32).astype(np.float64) / np.array([1.0, 0.5, 0.25])
    assert np.allclose(out[:, 16], d_post * np.array([0.5, 0.25, 1.0]), rtol=1e-12, atol=0)
    assert np.array_equal(out[:, 4], c[np.arange(H) // s, 2].astype(np.float64))            # not demodulated
    # a bad nearest pixel: (0, 0, 0)
    c[1, 2] = np.inf
    out = UR.upscale(c, lo, hi, mats, INV_PROJ, factor=s)
    assert (out[2:4, 4] == 0).all() and np.isfinite(out).all()


BAD_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("value", sorted(BAD_VALUES))
def test_ref_bad_low_pixels_are_contained(value, s):
    """An isolated bad low pixel, the corner and a 5 x 5 block.  The output is finite everywhere; a high pixel whose 4 x 4 low
    window holds no bad pixel is bit for bit what the clean frame gives; and a high pixel whose every tap inside the image is
    bad -- the middle of the block -- is exactly 0 (stage 3 on a bad pixel)."""
    rng = np.random.default_rng(11)
    h, w = 16, 20
    H, W = h * s, w * s
    lo, hi = _plane(h, w), _plane(H, W)
    lo = _miss(lo, np.s_[:, 17:])
    hi = _miss(hi, np.s_[:, 17 * s:])
    mats = _mats((0.5, 0.6, 0.7))
    clean = rng.random((h, w, 3)).astype(np.float32)
    bad = np.zeros((h, w), bool)
    bad[3, 14] = bad[0, 0] = True
    bad[8:13, 4:9] = True
    c = clean.copy()
    c[bad, 1] = BAD_VALUES[value]
    c[3, 14] = BAD_VALUES[value]
    assert np.array_equal(DR.bad_pixels(c), bad)
    for demod in (True, False):
        out, stage = UR.upscale(c, lo, hi, mats, INV_PROJ, factor=s, demodulate=demod, want_stage=True)
        want = UR.upscale(clean, lo, hi, mats, INV_PROJ, factor=s, demodulate=demod)
        assert np.isfinite(out).all()
        i0, _ = UR.footprint(np.arange(W), s)
        j0, _ = UR.footprint(np.arange(H), s)
        near = np.zeros((H, W), bool)                       # a bad pixel within the 4 x 4 window
        for b in range(-1, 3):
            for a in range(-1, 3):
                qy, qx = np.clip(j0 + b, 0, h - 1), np.clip(i0 + a, 0, w - 1)
                near |= bad[np.ix_(qy, qx)]
        assert (~near).any() and np.array_equal(out[~near], want[~near])
        mid = np.s_[10 * s:11 * s, 6 * s:7 * s]             # low pixel (6, 10): its whole 4 x 4 windows lie in the block
        assert (stage[mid] == 3).all() and (out[mid] == 0).all()
        assert (stage[~near] == 1).all()


def test_ref_integer_footprint_s3_centre_pixel_has_fx_0():
    X = np.arange(0, 30)
    i0, fx = UR.footprint(X, 3)
    centre = X % 3 == 1
    assert (fx[centre] == 0).all() and (i0[centre] == X[centre] // 3).all()
    assert (i0[X % 3 == 0] == X[X % 3 == 0] // 3 - 1).all() and (i0[0] == -1)
    assert fx.dtype == np.float32 and set(np.unique(fx)) == {np.float32(0), np.float32(2) / np.float32(6), np.float32(4) / np.float32(6)}
    # ... so the centre pixel of each triple is its low pixel, whatever lies next to it
    rng = np.random.default_rng(7)
    h, w = 4, 5
    c = rng.random((h, w, 3)).astype(np.float32)
    out = UR.upscale(c, _plane(h, w), _plane(3 * h, 3 * w), _mats((1.0, 1.0, 1.0)), INV_PROJ, factor=3, demodulate=False)
    assert np.allclose(out[1::3, 1::3], c.astype(np.float64), rtol=1e-15, atol=0)
    for s in (2, 4):
        i0, fx = UR.footprint(np.arange(0, 16), s)
        assert (fx > 0).all() and (i0[0] == -1) and (i0[s // 2] == 0)


# ---------------------------------------------------------------------------------------------------------------------
# quality on the oracle's frames (the GPU's frames equal the oracle's bit for bit)
#
# The target is 160 x 120 at 256 spp.  The input is 80 x 60 at 4 spp, upsampled with s = 2: the ray budget of a native 160 x 120
# frame at 1 spp.  Three errors per scene, MSE against the target, 5 bounces:
#                                  guided     bilinear (numpy, below)   native 1 spp
#   cornell_scene                  0.00534   0.00790                0.0572 
#   reference_scene(aspect 4/3)    0.000886   0.00147                0.000955
# The assertion is guided <= bilinear; the baseline is written here and shares no code with the filter.  No ratio against the
# native frame is claimed.

QUALITY_SCENES = {"cornell": lambda: S.cornell_scene(), "reference": lambda: S.reference_scene(aspect=4 / 3)}


def _bilinear(color, s):
    """The plain bilinear upsample of the low frame with the same pixel-centre geometry, taps clamped at the border."""
    c = np.asarray(color, np.float64)
    h, w = c.shape[:2]
    u = (np.arange(w * s) + 0.5) / s - 0.5
    v = (np.arange(h * s) + 0.5) / s - 0.5
    x0, y0 = np.floor(u).astype(int), np.floor(v).astype(int)
    fx, fy = (u - x0)[None, :, None], (v - y0)[:, None, None]
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    bot = c[np.ix_(ya, xa)] * (1 - fx) + c[np.ix_(ya, xb)] * fx
    top = c[np.ix_(yb, xa)] * (1 - fx) + c[np.ix_(yb, xb)] * fx
    return bot * (1 - fy) + top * fy


def test_bilinear_baseline_is_what_it_says():
    ramp = np.broadcast_to(np.arange(6, dtype=np.float64)[None, :, None], (4, 6, 3))
    up = _bilinear(ramp, 2)
    assert np.allclose(up[0, 1:-1, 0], (np.arange(1, 11) + 0.5) / 2 - 0.5) and up[0, 0, 0] == 0 and up[0, -1, 0] == 5
    assert np.allclose(_bilinear(np.full((3, 3, 3), 0.25), 3), 0.25)


@pytest.mark.parametrize("name", sorted(QUALITY_SCENES))
def test_quality_guided_is_no_worse_than_bilinear(name):
    sc = QUALITY_SCENES[name]()
    W, H, s = 160, 120, 2
    tgt = DR.resolve(helpers.oracle_render(sc, W, H, 256, 5))
    native = DR.resolve(helpers.oracle_render(sc, W, H, 1, 5))
    low = DR.resolve(helpers.oracle_render(sc, W // s, H // s, 4, 5))
    g_hi, g_lo = _oracle_guides(sc, W, H), _oracle_guides(sc, W // s, H // s)
    guided = UR.upscale(low, g_lo, g_hi, sc.materials, sc.camera.inv_proj, factor=s)
    e_g, e_b, e_n = DR.mse(guided, tgt), DR.mse(_bilinear(low, s), tgt), DR.mse(native, tgt)
    print(f"{name}: MSE guided {e_g:.6g}, bilinear {e_b:.6g}, native 1 spp {e_n:.6g}")
    assert np.isfinite(guided).all()
    assert e_g <= e_b, (e_g, e_b, e_n)

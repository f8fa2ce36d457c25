"""rz_ambient_occlusion without a GPU: the C-ABI struct and symbols, the code-object metadata of the new kernels, the direction
table against its restatement (ao_ref.py), the gather on hand-made records, and -- with the CPU oracle alone -- that the cases
the GPU test runs exercise what they claim and that the pass is worth its cost.  The figures in the last two groups are
conditions on the definition, computed with the oracle; they are not measurements of the device."""
import ctypes as C

import numpy as np
import pytest

import ao_ref as AR
from rayzen_amd import _lib
from test_rays_abi import _kernel_metadata

F32 = np.float32


def test_struct_size_offsets_and_symbols():
    L = _lib.hip()
    assert _lib.SIZEOF_AO_PARAMS == 37
    assert L.rz_sizeof(37) == 32 == C.sizeof(_lib.AoParams)
    assert L.rz_sizeof(36) == 0                             # stays unassigned
    offs = {"samples": 0, "radius": 4, "smooth": 8, "strength": 12, "normal_cos": 16, "plane_tol": 20, "reserved": 24}
    assert [f for f, _ in _lib.AoParams._fields_] == list(offs)
    for f, off in offs.items():
        assert getattr(_lib.AoParams, f).offset == off, f
    assert _lib.AO_HOST == 1 and _lib.AO_DIRECTIONS == 256
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5      # additive: the revision stays
    lib = C.CDLL(_lib.HIP_SO)
    for name in ("rz_ambient_occlusion", "rz_ao_directions"):
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name
    from rayzen_amd import renderer
    assert callable(renderer.ao_directions)
    for m in ("ambient_occlusion", "ambient_occlusion_device"):
        assert callable(getattr(renderer.Renderer, m)), m


def test_kernels_spill_nothing():
    """rz_ao_walks carries the shadow walk and, beside it, an item's record: it is held to rz_shadow_rays_kernel's figures, which
    are zero spilled VGPRs and no scratch; rz_ao_resolve likewise."""
    meta = _kernel_metadata(_lib.HIP_SO)
    ours = {k: v for k, v in meta.items() if "rz_ao_walks" in k or "rz_ao_resolve" in k}
    assert len(ours) == 4, sorted(ours)     # the walks with and without the overflow columns; the resolve with and without the gather
    shadow = {k: v for k, v in meta.items() if "rz_shadow_rays_kernel" in k}
    assert len(shadow) == 4 and all(v == (0, 0) for v in shadow.values()), shadow
    for name, (spill, priv) in ours.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


# ---------------------------------------------------------------------------------------------------------------------
# the direction table

def test_directions_equal_the_restatement():
    from rayzen_amd.renderer import ao_directions
    want, tried = AR.table()
    assert tried == 321                                     # candidates that yield the 256 points
    got = ao_directions()
    assert got.dtype == F32 and got.shape == (256, 3) and got.nbytes == 3072
    assert got.tobytes() == want.tobytes()
    length = np.sqrt((want.astype(np.float64) ** 2).sum(-1))
    assert np.abs(length - 1.0).max() <= 2e-7, np.abs(length - 1.0).max()
    assert len({p.tobytes() for p in want}) == 256


def test_directions_error_codes():
    L = _lib.hip()
    buf = np.zeros(768, F32)
    assert L.rz_ao_directions(None, 3072) == -1             # RZ_ERR_INVALID_ARG
    assert L.rz_ao_directions(buf.ctypes.data, 3071) == -7  # RZ_ERR_BUFFER_SIZE
    assert not buf.any()
    assert L.rz_ao_directions(buf.ctypes.data, 3072) == 0 and buf.tobytes() == AR.directions().tobytes()


def test_tree_is_the_pairwise_sum():
    a = np.array([0.1, 0.7, 1.0, 0.3, 0.9, 1e-8, 0.25, 0.6, 1.0, 1.0, 0.05, 0.0, 0.4, 0.2, 0.8, 0.33], F32)
    s8 = [a[2 * i] + a[2 * i + 1] for i in range(8)]
    s4 = [s8[2 * i] + s8[2 * i + 1] for i in range(4)]
    s2 = [s4[0] + s4[1], s4[2] + s4[3]]
    assert AR.tree(a).tobytes() == F32(s2[0] + s2[1]).tobytes()
    assert AR.tree(a[:1]) == a[0] and AR.tree(a[:2]) == a[0] + a[1]
    assert AR.tree(a[:4]).tobytes() == F32((a[0] + a[1]) + (a[2] + a[3])).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the gather on hand-made records

def _flat(h, w, z=-5.0):
    """A wall facing the camera at depth z: every pixel a hit, normal (0, 0, 1), points 0.01 apart, t = |z|."""
    ys, xs = np.mgrid[0:h, 0:w]
    x = np.stack([xs * 0.01, ys * 0.01, np.full((h, w), z)], -1).astype(F32)
    n = np.zeros((h, w, 3), F32)
    n[..., 2] = 1
    return np.ones((h, w), bool), n, x, np.full((h, w), abs(z), F32)


def _ramp(h, w):
    return (np.arange(h * w, dtype=F32).reshape(h, w) / F32(h * w)).astype(F32)


def _mean_in_order(raw, taps):
    s = F32(0.0)
    for y, x in taps:
        s = F32(s + raw[y, x])
    return F32(s / F32(len(taps)))


def _window(y, x, h, w):
    return [(y + b, x + a) for b in range(-2, 2) for a in range(-2, 2) if 0 <= y + b < h and 0 <= x + a < w]


def test_gather_windows_cut_by_each_border():
    h, w = 6, 7
    hit, n, x, t = _flat(h, w)
    raw = _ramp(h, w)
    ao = AR.gather(raw, hit, n, x, t, F32(0.01))
    for (y, xx), taps in {(3, 3): 16, (0, 3): 8, (1, 3): 12, (5, 3): 12, (3, 0): 8, (3, 1): 12, (3, 6): 12, (0, 0): 4, (5, 6): 9,
                          (0, 6): 6, (5, 0): 6}.items():
        win = _window(y, xx, h, w)
        assert len(win) == taps, (y, xx)
        assert ao[y, xx].tobytes() == _mean_in_order(raw, win).tobytes(), (y, xx)
    # the interior window holds each of the 16 patterns exactly once
    assert sorted((xx & 3) + 4 * (y & 3) for y, xx in _window(3, 3, h, w)) == list(range(16))


def test_gather_stops_at_a_normal_edge():
    h, w = 5, 8
    hit, n, x, t = _flat(h, w)
    n[:, 4:] = (np.sqrt(F32(0.5)), 0.0, np.sqrt(F32(0.5)))         # a crease: dot = 0.707 < 0.9
    raw = _ramp(h, w)
    ao = AR.gather(raw, hit, n, x, t, F32(1.0))                     # (a footprint so wide that the plane test passes everywhere)
    left = [q for q in _window(2, 3, h, w) if q[1] < 4]
    right = [q for q in _window(2, 4, h, w) if q[1] >= 4]
    assert len(left) == 12 and len(right) == 8
    assert ao[2, 3].tobytes() == _mean_in_order(raw, left).tobytes()
    assert ao[2, 4].tobytes() == _mean_in_order(raw, right).tobytes()
    # at the threshold the tap counts (>=): from (2, 4) the dot with the left half is (s * 0 + 0 * 0) + s * 1 = s exactly
    at = AR.gather(raw, hit, n, x, t, F32(1.0), normal_cos=float(np.sqrt(F32(0.5))))
    assert at[2, 4].tobytes() == _mean_in_order(raw, _window(2, 4, h, w)).tobytes() != ao[2, 4].tobytes()
    assert AR.gather(raw, hit, n, x, t, F32(1.0), normal_cos=-1.0)[2, 3].tobytes() == _mean_in_order(raw, _window(2, 3, h, w)).tobytes()


def test_gather_stops_at_a_plane_step():
    h, w = 5, 8
    hit, n, x, t = _flat(h, w)
    x[:, 4:, 2] += F32(0.5)                                         # the right half half a unit nearer: same normals
    t[:, 4:] -= F32(0.5)
    raw = _ramp(h, w)
    f = F32(0.01)                                                   # tolerance: 2 * 5 * 0.01 = 0.1 per pixel of distance, 0.2 at two
    ao = AR.gather(raw, hit, n, x, t, f)
    left = [q for q in _window(2, 3, h, w) if q[1] < 4]
    assert ao[2, 3].tobytes() == _mean_in_order(raw, left).tobytes()
    assert ao[2, 5].tobytes() == _mean_in_order(raw, [q for q in _window(2, 5, h, w) if q[1] >= 4]).tobytes()
    # max(|a|, |b|) scales the tolerance: a step of 0.15 passes two pixels away (0.2) and fails one pixel away (0.1)
    hit2, n2, x2, t2 = _flat(h, w)
    x2[:, :3, 2] -= F32(0.15)
    got = AR.gather(raw, hit2, n2, x2, t2, f)
    want = [q for q in _window(2, 4, h, w) if q[1] >= 3 or q[1] == 2]
    assert len(want) == 16 and got[2, 4].tobytes() == _mean_in_order(raw, want).tobytes()
    # from column 3: column 1 is two away; column 2 is one away but for the row two below, where max(|a|, |b|) = 2
    want = [q for q in _window(2, 3, h, w) if q[1] >= 3 or q[1] == 1 or q == (0, 2)]
    assert len(want) == 13 and got[2, 3].tobytes() == _mean_in_order(raw, want).tobytes()


def test_gather_stops_at_a_hit_miss_edge():
    h, w = 5, 8
    hit, n, x, t = _flat(h, w)
    hit[:, 5:] = False
    hit[0, 0] = False
    raw = _ramp(h, w)
    raw[~hit] = 1
    ao = AR.gather(raw, hit, n, x, t, F32(0.01))
    assert (ao[~hit] == 1).all()
    assert ao[2, 4].tobytes() == _mean_in_order(raw, [q for q in _window(2, 4, h, w) if q[1] < 5]).tobytes()
    assert ao[1, 1].tobytes() == _mean_in_order(raw, [q for q in _window(1, 1, h, w) if q != (0, 0)]).tobytes()
    # NaN and infinite records of the misses' neighbours reach nothing
    x[~hit] = np.nan
    n[~hit] = np.inf
    assert AR.gather(raw, hit, n, x, t, F32(0.01)).tobytes() == ao.tobytes()


def test_gather_of_a_one_pixel_image():
    hit, n, x, t = _flat(1, 1)
    raw = np.array([[0.375]], F32)
    assert AR.gather(raw, hit, n, x, t, F32(0.01)).tobytes() == raw.tobytes()
    assert AR.gather(raw, ~hit, n, x, t, F32(0.01)).tolist() == [[1.0]]


def test_outputs_restated():
    ao = np.array([[0.0, 0.25, 1.0]], F32)
    rgb = np.array([[[0.5, 1.5, -0.25], [0.2, 0.44, 0.8], [0.12, 0.31, 2.0]]], F32)
    assert AR.modulate(ao).tolist() == [[[0.0] * 3, [0.25] * 3, [1.0] * 3]]
    assert AR.modulate(ao, strength=0.0).tolist() == [[[1.0] * 3] * 3]
    half = AR.modulate(ao, rgb, 0.5)
    assert half[0, 1].tobytes() == (rgb[0, 1] * (F32(1.0) - F32(0.5) * F32(0.75))).astype(F32).tobytes()
    assert AR.quantise(AR.modulate(ao, rgb)).tolist() == [[[0, 0, 0, 255], [13, 28, 51, 255], [31, 79, 255, 255]]]
    assert AR.quantise(np.array([[[0.5, 0.0, 1.0]]], F32)).tolist() == [[[128, 0, 255, 255]]]       # 127.5: rint rounds half to even
    assert AR.pixel_footprint(np.arange(16, dtype=F32), 10) == F32(1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the cases bite (the oracle alone, 32 x 24, N = 4, radius 2)

@pytest.mark.parametrize("name,occluded,attenuated", [("reference", 60, 0), ("bunny", 110, 50), ("instanced", 130, 0),
                                                      ("cornell", 160, 0)])
def test_the_cases_bite(name, occluded, attenuated):
    g = AR.guide(name, 32, 24)
    raw, a = AR.raw(name, 32, 24, 4, 2.0)
    assert 0 < g.hit.sum() and (raw[~g.hit] == 1).all()
    assert int((raw < 1).sum()) >= occluded, int((raw < 1).sum())
    assert int(((a > 0) & (a < 1)).sum()) >= attenuated, int(((a > 0) & (a < 1)).sum())       # glass attenuates, it does not block
    assert ((raw >= 0) & (raw <= 1)).all()


def test_partial_frames_have_hits_and_misses_between_them():
    hits = sum(int(AR.guide("reference", w, h).hit.sum()) for w, h in AR.PARTIAL)
    total = sum(w * h for w, h in AR.PARTIAL)
    assert 0 < hits < total


# ---------------------------------------------------------------------------------------------------------------------
# quality (the oracle alone, 48 x 36, radius 2): RMSE over the hit pixels against the mean over all 256 directions

def _rmse(name, img):
    g = AR.guide(name, 48, 36)
    return float(np.sqrt(((img[g.hit].astype(np.float64) - AR.truth(name, 48, 36, 2.0)) ** 2).mean()))


@pytest.mark.parametrize("name", sorted(AR.CASES))
def test_smoothing_pays(name):
    """Measured: the ratio is 1.8 (reference), 2.1 (bunny), 2.2 (instanced), 3.9 (cornell)."""
    g, inv_proj = AR.guide(name, 48, 36), AR.scene(name).camera.inv_proj
    raw4, raw1 = AR.raw(name, 48, 36, 4, 2.0)[0], AR.raw(name, 48, 36, 1, 2.0)[0]
    e_raw4, e_smooth4, e_smooth1 = _rmse(name, raw4), _rmse(name, AR.smooth(g, raw4, inv_proj)), _rmse(name, AR.smooth(g, raw1, inv_proj))
    print(f"{name}: RMSE raw N=4 {e_raw4:.4f}, smoothed N=4 {e_smooth4:.4f} ({e_raw4 / e_smooth4:.2f} x), smoothed N=1 {e_smooth1:.4f}")
    assert e_raw4 >= 1.5 * e_smooth4, (e_raw4, e_smooth4)
    assert e_smooth1 < e_raw4, (e_smooth1, e_raw4)

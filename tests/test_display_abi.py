"""The display stage (rz_display, rz_present_display, rz_display_reset, rz_display_state): the C-ABI structs and symbols, the
argument checks of the Python wrapper, the kernels' register budget and the restatement's metering (display_ref.py) --
everything that can be checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

import display_ref as R
from rayzen_amd import _lib
from rayzen_amd.renderer import Renderer
from test_rays_abi import _kernel_metadata

F32 = np.float32


def test_display_structs_and_symbols():
    L = _lib.hip()
    assert L.rz_sizeof(14) == 64 and C.sizeof(_lib.DisplayParams) == 64
    assert L.rz_sizeof(15) == 536 and C.sizeof(_lib.DisplayInfo) == 536
    assert L.rz_sizeof(13) == 0 and L.rz_sizeof(16) == 0      # 13 stays unassigned (test_temporal_abi.py probes it)
    want = {"exposure_mode": 0, "exposure": 4, "key": 8, "min_exposure": 12, "max_exposure": 16, "adapt": 20, "low_permille": 24,
            "high_permille": 28, "curve": 32, "white": 36, "transfer": 40, "reserved": 44}
    assert [f for f, _ in _lib.DisplayParams._fields_] == list(want)
    for f, off in want.items():
        assert getattr(_lib.DisplayParams, f).offset == off, f
    assert _lib.DisplayInfo.histogram.offset == 24 and _lib.DisplayInfo.counted.offset == 12
    assert (_lib.DISPLAY_HOST, _lib.DISPLAY_KEEP) == (1, 4)
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5       # additive: the revision stays
    lib = C.CDLL(_lib.HIP_SO)
    for name in ("rz_display", "rz_present_display", "rz_display_reset", "rz_display_state"):
        assert hasattr(lib, name) and name in _lib.HIP_SYMBOLS, name


def test_display_kernels_use_no_scratch():
    meta = _kernel_metadata(_lib.HIP_SO)
    for kernel, variants in (("rz_display_meter", 3), ("rz_display_expose", 1), ("rz_display_tone", 1)):
        found = {k: v for k, v in meta.items() if kernel in k}
        assert len(found) == variants, (kernel, sorted(meta))
        for name, (spill, priv) in found.items():
            assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"


BAD = [dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=float("inf")), dict(exposure=float("nan")),
       dict(key=0.0), dict(key=float("nan")), dict(key=float("inf")),
       dict(min_exposure=0.0), dict(min_exposure=float("nan")), dict(max_exposure=float("inf")), dict(min_exposure=2.0, max_exposure=1.0),
       dict(adapt=-0.01), dict(adapt=1.01), dict(adapt=float("nan")),
       dict(low=-0.001), dict(high=-0.001), dict(low=0.5, high=0.5), dict(low=1.0), dict(low=float("nan")),
       dict(curve="filmic"), dict(curve=1), dict(white=0.0), dict(white=float("inf")), dict(white=float("nan")),
       dict(transfer="pq"), dict(transfer=1)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_wrapper_rejects_out_of_range_fields(kw):
    """Renderer._display_params is what display(), display_device() and present_display() run their keyword arguments through
    before any call into the library (a static method: no context, no GPU)."""
    with pytest.raises(ValueError):
        Renderer._display_params(**kw)


def test_wrapper_defaults_are_the_reference_display():
    assert Renderer._display_params() is None                       # params NULL
    assert Renderer._display_params(**R.DEFAULTS) is None
    with pytest.raises(TypeError):
        Renderer._display_params(gamma=2.2)
    p = Renderer._display_params(auto=True, key=0.25, min_exposure=0.5, max_exposure=8, adapt=0.25, low=0.1, high=0.05,
                                 curve="aces", white=2.0, transfer="srgb")
    assert (p.exposure_mode, p.key, p.min_exposure, p.max_exposure, p.adapt, p.low_permille, p.high_permille, p.curve, p.white,
            p.transfer, list(p.reserved)) == (1, 0.25, 0.5, 8.0, 0.25, 100, 50, 2, 2.0, 1, [0] * 5)
    assert Renderer._display_params(low=0.5, high=0.499).high_permille == 499


def test_restatement_bin_edges():
    prev = lambda v: np.nextafter(F32(v), F32(-np.inf))
    cases = [(F32(2.0) ** -16, 0), (prev(F32(2.0) ** -16), -1), (F32(1.0), 64), (F32(1.25), 65), (prev(1.25), 64),
             (F32(65535.996), 127), (F32(65536.0), 128), (F32(np.inf), 128), (F32(np.nan), 128),
             (F32(0.0), -1), (F32(-0.0), -1), (F32(-1.0), -1), (F32(-np.inf), -1), (F32(1e-40), -1), (F32(-1e-40), -1),
             (F32(0.18), 53), (F32(1.5), 66), (F32(1.75), 67), (F32(2.0), 68)]
    vals = np.array([v for v, _ in cases], F32)
    assert R.bins(vals).tolist() == [b for _, b in cases]
    hist, below, above = R.meter(vals)
    assert below == 7 and above == 3 and hist.sum() == len(cases) - 10
    assert hist[64] == 2 and hist[0] == 1 and hist[127] == 1


def test_restatement_trim_keeps_something():
    lo, hi = R.trim(1, 499, 500)
    assert hi - lo == 1 > 0
    for n in (1, 2, 3, 999, 1000, 1001, 2 ** 28):
        for low, high in ((0, 0), (100, 50), (500, 499), (999, 0), (0, 999)):
            lo, hi = R.trim(n, low, high)
            assert hi - lo > 0, (n, low, high)
    hist = np.zeros(128, np.uint32)
    hist[70] = 1
    t, mean = R.target(hist, low_permille=499, high_permille=500)
    assert mean == 17 - 16 + R.G[2]


def test_restatement_uniform_grey_meters_to_one_bin_of_unity():
    """A frame of 0.18 everywhere: the mean is the mid-point of the bin 0.18 falls in, so the exposure that brings it to the key
    0.18 is within one bin (a factor of at most 1.25) of 1 -- 1.0516."""
    img = np.full((5, 7, 3), 0.18, F32)
    hist, below, above = R.meter(R.luminance(img))
    assert below == above == 0 and hist.sum() == 35 and np.count_nonzero(hist) == 1
    t, mean = R.target(hist)
    assert abs(float(t) - 1.0516) < 5e-5
    assert 1 / 1.25 <= float(t) <= 1.25
    # trimming a one-bin frame changes nothing
    assert R.target(hist, low_permille=100, high_permille=50)[0] == t
    # adaptation: a fresh state or adapt = 1 jumps, otherwise a share of the way in binary32
    assert R.adapt(None, t, 0.25) == t and R.adapt(F32(3.0), t, 1.0) == t
    assert R.adapt(F32(3.0), t, 0.25) == F32(F32(3.0) + F32(0.25) * F32(t - F32(3.0)))
    assert R.target(np.zeros(128, np.uint32)) is None


def test_restatement_curves():
    x = np.array([[-0.5, 0.0, 0.18], [1.0, 4.0, 1e4]], F32)
    assert np.array_equal(R.tone(x, 1.0), np.clip(x.astype(np.float64), 0, 1))
    r = R.tone(x, 1.0, "reinhard", white=4.0)
    assert r[0, 0] == 0 and r[1, 1] == 1.0 and abs(r[1, 0] - (1 + 1 / 16) / 2) < 1e-15 and r[1, 2] == 1.0
    a = R.tone(x, 1.0, "aces")
    assert abs(a[0, 2] - 0.18 * (2.51 * 0.18 + 0.03) / (0.18 * (2.43 * 0.18 + 0.59) + 0.14)) < 1e-7 and a[1, 2] == 1.0
    s = R.tone(np.array([[0.0, 0.002, 1.0]], F32), 1.0, transfer="srgb")
    assert s[0, 0] == 0 and abs(s[0, 1] - 12.92 * float(F32(0.002))) < 1e-15 and abs(s[0, 2] - 1.0) < 1e-15
    assert R.quantise(np.array([[0.5, 2.0, -1.0]], F32)).tolist() == [[128, 255, 0, 255]]

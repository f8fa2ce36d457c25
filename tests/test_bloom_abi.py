"""rz_bloom without a GPU: the C-ABI struct and symbols, and the numpy restatement (bloom_ref.py) on cases whose answers are
known by hand -- level sizes, a constant frame, an impulse, the onset curve, bad pixels, intensity 0 -- and the built kernels'
metadata."""
import ctypes as C
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import bloom_ref as BR
from rayzen_amd import _lib

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 1), (9, 7), (33, 9), (65, 5), (1920, 1080)]
SMALL = [(1, 1), (2, 1), (9, 7)]


def _header_fields(name):
    text = open(os.path.join(ROOT, "include", "rayzen_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*\]", "", d.split()[-1]) for d in body.split(";") if d.strip()]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the ABI

def test_struct_size_field_order_and_symbols():
    L = _lib.hip()
    assert _lib.SIZEOF_BLOOM_PARAMS == 45
    assert L.rz_sizeof(45) == 32 == C.sizeof(_lib.BloomParams)
    assert L.rz_sizeof(44) == 0
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5      # additive: the revision stays
    assert _header_fields("rz_bloom_params") == [f for f, _ in _lib.BloomParams._fields_]
    assert [getattr(_lib.BloomParams, f).offset for f, _ in _lib.BloomParams._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert _lib.BLOOM_DEFAULTS == BR.DEFAULTS == dict(threshold=1.0, knee=0.5, limit=64.0, intensity=0.25, spread=1.0, levels=6)
    assert _lib.BLOOM_HOST == 1
    so = C.CDLL(_lib.HIP_SO)
    for sym in ("rz_bloom", "rz_present_bloomed"):
        assert hasattr(so, sym) and sym in _lib.HIP_SYMBOLS, sym
    from rayzen_amd.renderer import Renderer
    for m in ("bloom", "bloom_device", "present_bloomed"):
        assert callable(getattr(Renderer, m)), m
    assert Renderer._bloom_params() is None and Renderer._bloom_params(levels=6, limit=64.0) is None
    p = Renderer._bloom_params(limit=float("inf"), spread=4.0, levels=8, knee=0.0, threshold=0.0, intensity=0.0)
    assert (p.limit, p.spread, p.levels, p.knee) == (float("inf"), 4.0, 8, 0.0) and tuple(p.reserved) == (0, 0)
    for bad in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(knee=float("inf")), dict(limit=0.0), dict(limit=float("nan")),
                dict(intensity=-0.5), dict(intensity=float("inf")), dict(spread=0.0), dict(spread=4.5), dict(spread=float("nan")),
                dict(levels=0), dict(levels=9)):
        with pytest.raises(ValueError):
            Renderer._bloom_params(**bad)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement

def test_level_sizes():
    assert BR.level_sizes(1, 1) == [(1, 1)] and BR.level_sizes(2, 1) == [(1, 1)]
    assert BR.level_sizes(9, 7) == [(5, 4), (3, 2), (2, 1), (1, 1)]
    assert BR.level_sizes(33, 9, 6)[-1] == (1, 1)
    assert BR.level_sizes(65, 5, 6)[-1] == (2, 1) and len(BR.level_sizes(65, 5, 6)) == 6
    assert BR.level_sizes(1920, 1080, 6) == [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]
    assert BR.level_sizes(1920, 1080, 1) == [(960, 540)] and len(BR.level_sizes(1920, 1080, 8)) == 8


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_a_constant_frame(w, h):
    """Constant 3 with threshold 1, knee 0 and no limit: every level holds exactly 2 (the filters' weights sum to 64 and to 16,
    and the clamped border repeats the constant), so U_0 = 2 L with spread 1."""
    c = np.full((h, w, 3), 3.0, F32)
    kw = dict(threshold=1.0, knee=0.0, limit=float("inf"), spread=1.0)
    out, glare, info = BR.bloom(c, **kw)
    L = len(info["sizes"])
    assert (info["p"] == 2.0).all() and (info["raw"] == F32(2 * L)).all()
    two = F32(2.0)
    assert (np.abs(glare.astype(np.float64) - 2.0) <= float(np.spacing(two))).all()
    assert (out == c + F32(0.25) * glare).all()
    if (w, h) in SMALL:
        out2, glare2 = BR.bloom_loops(c, **kw)
        assert (_bits(out) == _bits(out2)).all() and (_bits(glare) == _bits(glare2)).all()


@pytest.mark.parametrize("w,h", SMALL + [(5, 4), (8, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("kw", [dict(), dict(knee=0.0, spread=0.5, levels=2), dict(spread=2.0, limit=float("inf"), levels=8)],
                         ids=["defaults", "hard-half-2", "double-nolimit-8"])
def test_both_forms_of_the_restatement_agree(w, h, kw):
    c = BR.frame(w, h, seed=3)
    if w * h >= 12:
        c[1, 2] = (np.nan, 1.0, 2.0)
        c[0, 1] = (-1.0, 5.0, -0.0)
    out, glare, _ = BR.bloom(c, **kw)
    out2, glare2 = BR.bloom_loops(c, **kw)
    assert (_bits(out) == _bits(out2)).all() and (_bits(glare) == _bits(glare2)).all()


@pytest.mark.parametrize("w,h", [(9, 7), (33, 9), (65, 5), (67, 35), (130, 70), (1920, 1080)], ids=lambda v: str(v))
def test_about_half_of_a_test_frame_glares(w, h):
    c = BR.frame(w, h)
    p = BR.prefilter(c, 1.0, 0.0, 64.0)
    share = (p != 0).any(axis=-1).mean()
    assert 0.3 <= share <= 0.7, share
    assert (c.max(axis=-1) >= 2.0 ** -6).all() and (c.max(axis=-1) <= 2.0 ** 6).all() and (c.min(axis=-1) >= 2.0 ** -8).all()


def test_an_impulse():
    """One pixel of 100 in a black 64 x 64 frame, the defaults: it glares with the limit, m = 64; the six levels (down to 1 x 1)
    each hand on what they were given, so the glare before its normalisation sums to 64 * 6; and the 1 x 1 level reaches every
    pixel."""
    c = np.zeros((64, 64, 3), F32)
    c[31, 30] = 100.0
    _, glare, info = BR.bloom(c)
    assert len(info["sizes"]) == 6 and info["sizes"][-1] == (1, 1)
    assert (info["p"][31, 30] == 64.0).all() and np.count_nonzero(info["p"]) == 3
    assert BR.onset(100.0, 1.0, 0.5, 64.0) == 64.0
    # summed in binary32, as the images are; in binary64 the 4 096 values' own roundings show: each is the end of at most 16
    # rounded operations, 2^-24 relative each
    for k in range(3):
        assert info["raw"][..., k].sum() == F32(64.0 * 6)
        assert abs(info["raw"][..., k].sum(dtype=np.float64) - 64.0 * 6) <= 64.0 * 6 * 16 * 2.0 ** -24
    assert (glare > 0).all() and np.isfinite(glare).all()


def test_the_onset():
    t, k = F32(1.0), F32(0.5)
    m = lambda b, knee=k, limit=np.inf: float(BR.onset(b, t, knee, limit))
    assert m(t - k) == 0.0 and m(0.25) == 0.0 and m(0.0) == 0.0
    assert m(t) == float(k) / 4
    assert m(t + k) == float(k)
    assert m(1.75) == 0.75 and m(3.0) == 2.0 and m(101.0) == 100.0 and m(101.0, limit=64.0) == 64.0
    bs = np.linspace(0.5, 1.5, 257).astype(F32)
    ms = BR.onset(bs, t, k, np.inf)
    assert (np.diff(ms) >= 0).all() and (ms >= np.maximum(bs - t, 0)).all()         # monotone, never under the hard step
    # knee 0: a hard step
    assert m(1.0, knee=0.0) == 0.0 and m(np.nextafter(F32(1.0), F32(2.0)), knee=0.0) > 0.0 and m(0.999, knee=0.0) == 0.0
    assert m(4.0, knee=0.0) == 3.0
    # b just above 0 with knee > threshold: s > 0 there, f = m / max(b, 1e-4) stays finite
    tiny = np.full((1, 1, 3), 1e-30, F32)
    p = BR.prefilter(tiny, 1.0, 2.0, 64.0)
    assert BR.onset(1e-30, 1.0, 2.0, 64.0) == 0.125 and np.isfinite(p).all() and (p > 0).all() and (p < 1e-20).all()
    assert (BR.prefilter(np.zeros((1, 1, 3), F32), 1.0, 2.0, 64.0) == 0).all()


def test_bad_pixels_and_negative_channels():
    c, bad, neg = BR.with_bad_pixels(BR.frame(33, 9))
    out, glare, info = BR.bloom(c)
    assert np.isfinite(glare).all() and np.isfinite(info["p"]).all()
    for at in bad:
        assert (info["p"][at] == 0).all() and not np.isfinite(out[at]).all()
    fine = np.ones(c.shape[:2], bool)
    for at in bad:
        fine[at] = False
    assert np.isfinite(out[fine]).all()
    # they add nothing: the glare is that of the frame with black there
    black = c.copy()
    for at in bad:
        black[at] = 0.0
    assert (_bits(BR.bloom(black)[1]) == _bits(glare)).all()
    # negative channels count as 0: (-3, 8, -0) glares as (0, 8, 0)
    assert info["p"][neg][0] == 0 and info["p"][neg][2] == 0 and info["p"][neg][1] == F32(8) * (F32(7) / F32(8))
    zeroed = c.copy()
    zeroed[neg] = (0.0, 8.0, 0.0)
    assert (_bits(BR.bloom(zeroed)[1]) == _bits(glare)).all()


def test_intensity_zero_returns_the_input():
    c, _, _ = BR.with_bad_pixels(BR.frame(33, 9))
    c[0, 3] = (-0.0, 0.0, -0.0)
    c.view(np.uint32)[1, 1] = (0x7FC12345, 0xFFC00001, 0x7F800001)         # NaN payloads
    out, glare, _ = BR.bloom(c, intensity=0.0)
    assert out.tobytes() == c.tobytes()
    assert (_bits(glare) == _bits(BR.bloom(c)[1])).all() and (glare > 0).any()
    out2, _ = BR.bloom_loops(c[:4, :6], intensity=0.0)
    assert out2.tobytes() == np.ascontiguousarray(c[:4, :6]).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the kernels

def _kernel_records(so_path):
    """{kernel symbol: {field: int}} of the gfx950 code objects inside a HIP library, from the AMDGPU metadata note: every
    integer field, the LDS size among them (test_rays_abi._kernel_metadata keeps the spill count and the scratch size only)."""
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf of the ROCm toolchain is needed to read the code-object metadata"
    blob = open(so_path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = {}
    k = blob.find(magic)
    while k >= 0:
        (n,) = struct.unpack_from("<Q", blob, k + 24)
        p = k + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" not in triple:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(blob[k + off:k + off + size])
                f.flush()
                notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True, check=True).stdout
            for rec in re.split(r"\n\s+- \.", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", rec)
                if name:
                    out[name.group(1)] = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.(\w+):\s+(\d+)\s*$", rec, re.M)}
        k = blob.find(magic, k + 1)
    return out


def test_kernels_spill_nothing_and_keep_their_lds():
    ours = {k: v for k, v in _kernel_records(_lib.HIP_SO).items() if "rz_bloom_" in k}
    assert len(ours) == 5, sorted(ours)                     # down<0>, down<1>, down<2>, up, combine
    staged = (34 * (34 * 3 + 1) + 34 * 56) * 4              # rz_bloom.hip: src and rows
    for name, rec in ours.items():
        assert rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0 and rec["private_segment_fixed_size"] == 0, (name, rec)
        lds = rec["group_segment_fixed_size"]               # (each array may be padded to 16 bytes)
        assert (staged <= lds <= staged + 32) if "down" in name else lds == 0, (name, lds)
        assert rec["max_flat_workgroup_size"] == 256, name

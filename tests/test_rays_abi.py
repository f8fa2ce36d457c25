"""Ray queries (rz_trace_rays / rz_shadow_rays): the C-ABI structs, the host-side picking ray and the kernels' register
budget -- everything that can be checked without a GPU."""
import ctypes as C
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from rayzen_amd import _lib
from rayzen_amd import renderer as R
from rayzen_amd import scene as S


def test_ray_struct_sizes_and_offsets():
    L = _lib.hip()
    assert [L.rz_sizeof(k) for k in (7, 8, 9)] == [32, 48, 8]
    assert (C.sizeof(_lib.Ray), C.sizeof(_lib.Hit), C.sizeof(_lib.Visibility)) == (32, 48, 8)
    assert (R.RAY_DTYPE.itemsize, R.HIT_DTYPE.itemsize, R.VISIBILITY_DTYPE.itemsize) == (32, 48, 8)
    ray = {"origin": 0, "max_dist": 12, "dir": 16, "reserved": 28}
    hit = {"t": 0, "point": 4, "normal": 16, "material": 28, "instance": 32, "triangle": 36, "prim": 40, "reserved": 44}
    vis = {"visibility": 0, "lit": 4}
    for st, dt, want in ((_lib.Ray, R.RAY_DTYPE, ray), (_lib.Hit, R.HIT_DTYPE, hit), (_lib.Visibility, R.VISIBILITY_DTYPE, vis)):
        assert [f for f, _ in st._fields_] == list(want) == list(dt.names)
        for f, off in want.items():
            assert getattr(st, f).offset == off, (st.__name__, f)
            assert dt.fields[f][1] == off, (dt, f)
    # the ABI revision stays: the change only adds structs and entry points
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5


def _pick_ray_restated(mx, my, w, h, cam):
    """main.cpp:505-513 written out scalar by scalar in float32 (column-major matrices: element (row r, col c) at 4c + r)."""
    f = np.float32
    ip, iv = np.asarray(cam.inv_proj, f), np.asarray(cam.inv_view, f)
    ndc_x = f(f(f(2.0) * f(mx)) / f(w)) - f(1.0)
    ndc_y = f(1.0) - f(f(f(2.0) * f(my)) / f(h))
    clip = (ndc_x, ndc_y, f(-1.0), f(1.0))
    eye = [f(f(ip[0 * 4 + r] * clip[0]) + f(ip[1 * 4 + r] * clip[1])) + f(f(ip[2 * 4 + r] * clip[2]) + f(ip[3 * 4 + r] * clip[3]))
           for r in range(4)]
    e = (eye[0], eye[1], f(-1.0), f(0.0))
    v = [f(f(iv[0 * 4 + r] * e[0]) + f(iv[1 * 4 + r] * e[1])) + f(f(iv[2 * 4 + r] * e[2]) + f(iv[3 * 4 + r] * e[3]))
         for r in range(3)]
    d = f(f(v[0] * v[0]) + f(v[1] * v[1])) + f(v[2] * v[2])
    k = f(f(1.0) / np.sqrt(d))
    return np.asarray(cam.position, f), np.array([v[0] * k, v[1] * k, v[2] * k], f)


def test_pick_ray_is_main_cpp_505_513_bit_for_bit():
    """Bit for bit (not merely within an ulp): both sides normalise as glm::normalize does, v * (1 / sqrt(dot(v, v)))."""
    cam = S.reference_scene().camera
    W, H = 800, 600
    n = 0
    for mx in np.linspace(0.0, W, 17):
        for my in np.linspace(0.0, H, 13):
            o, d = R.pick_ray(mx, my, W, H, cam)
            o2, d2 = _pick_ray_restated(mx, my, W, H, cam)
            assert o.dtype == d.dtype == np.float32
            assert o.view(np.uint32).tolist() == o2.view(np.uint32).tolist()
            assert d.view(np.uint32).tolist() == d2.view(np.uint32).tolist(), (mx, my, d, d2)
            n += 1
    assert n == 17 * 13
    # the centre of the screen looks down the camera's axis (0, 0, -1)
    _, d = R.pick_ray(W / 2, H / 2, W, H, cam)
    assert np.allclose(d, (0.0, 0.0, -1.0), atol=1e-6)


def _kernel_metadata(so_path):
    """{kernel symbol: (vgpr_spill_count, private_segment_fixed_size)} of the gfx950 code objects inside a HIP library
    (clang offload bundles in its fat binary; the AMDGPU metadata note read by llvm-readelf)."""
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
                spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", rec)
                priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", rec)
                if name and spill and priv:
                    out[name.group(1)] = (int(spill.group(1)), int(priv.group(1)))
        k = blob.find(magic, k + 1)
    return out


def test_ray_kernels_spill_nothing():
    """Measured on the first build: 75-86 VGPRs per instantiation, no spill, no scratch."""
    meta = _kernel_metadata(_lib.HIP_SO)
    rays = {k: v for k, v in meta.items() if "rz_trace_rays" in k or "rz_shadow_rays" in k}
    assert len([k for k in rays if "rz_trace_rays" in k]) == 4 and len([k for k in rays if "rz_shadow_rays" in k]) == 4, sorted(rays)
    for name, (spill, priv) in rays.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"

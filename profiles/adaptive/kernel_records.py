"""The record of the render kernels in a built librayzen_hip.so -- VGPRs, SGPRs, spilled VGPRs, scratch and code bytes of every
rz_render_pixels / rz_render_samples / rz_cost_pixels instantiation -- from the AMDGPU metadata note and the symbol table of the
gfx950 code objects inside the library.  Two libraries built from trees whose render kernels are the same print the same lines.

    python profiles/adaptive/kernel_records.py [path/to/librayzen_hip.so]
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
PATTERN = re.compile(r"rz_render_pixels|rz_render_samples|rz_cost_pixels")


def code_objects(so_path):
    blob = open(so_path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    k = blob.find(magic)
    while k >= 0:
        (n,) = struct.unpack_from("<Q", blob, k + 24)
        p = k + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple:
                yield blob[k + off:k + off + size]
        k = blob.find(magic, k + 1)


def records(so_path):
    out = {}
    for co in code_objects(so_path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
            syms = subprocess.run([READELF, "--symbols", "--wide", f.name], capture_output=True, text=True, check=True).stdout
        size = {}
        for ln in syms.splitlines():
            t = ln.split()
            if len(t) >= 8 and t[3] == "FUNC":
                size[t[7]] = int(t[2], 0)
        for rec in re.split(r"\n\s+- \.", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", rec)
            if not name or not PATTERN.search(name.group(1)):
                continue
            get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, rec).group(1))
            out[name.group(1)] = (get("vgpr_count"), get("sgpr_count"), get("vgpr_spill_count"), get("private_segment_fixed_size"),
                                  size.get(name.group(1), -1))
    return out


if __name__ == "__main__":
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "rayzen_amd", "lib", "librayzen_hip.so")
    rec = records(so)
    print(f"{len(rec)} kernels; vgpr sgpr spilled scratch code-bytes")
    for name in sorted(rec):
        print(name, *rec[name])

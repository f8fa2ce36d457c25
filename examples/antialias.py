"""Measures the edge anti-aliasing pass: rz_antialias at 1920 x 1080 on the C2 frame (bunny_scene) and on RayZen's own scene
(reference_scene), for s = 2, 3, 4 -- milliseconds on the device (events on a user stream, median of 25), the share of edge pixels,
and beside it rz_upscale at factor s FROM THE SAME FRAME, which casts every sub-ray of every pixel and writes s w x s h, and
rz_denoise's guide cast at the frame's size alone (rz_antialias with only `guides` asked for), which both calls contain.

    python examples/antialias.py [--kernels]
    python examples/antialias.py --see-through [--config c2g]

--kernels prints the registers, scratch, LDS and occupancy of rz_antialias_edges, rz_antialias_seethrough_classify and _edges,
rz_seethrough_guides and rz_denoise_guides from the code object's metadata (needs llvm-readelf of the ROCm toolchain, no GPU).
--see-through measures rz_antialias_seethrough (max_depth 0 and 8) at s = 2 next to rz_antialias and rz_upscale_seethrough from
the same frame, on C2 or, with --config c2g, on C2 plus a glass blob and a mirror cube; it prints the edge share, the share of
edge pixels whose chain moves and the mean number of queries per sub-sample.  With RAYZEN_HIP_SO naming a library from before
the see-through pass it times rz_antialias alone.
"""
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from rayzen_amd import _lib  # noqa: E402
from rayzen_amd import scene as S  # noqa: E402
from rayzen_amd.renderer import Renderer, frame_params  # noqa: E402


def timed(r, hip, stream, fn, reps=25):
    a, b = hip.event(), hip.event()
    fn()
    r.sync()
    out = []
    for _ in range(reps):
        hip.ok(hip.L.hipEventRecord(a, stream))
        fn()
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        out.append(ms.value)
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    return float(np.median(out))


def kernels():
    """The AMDGPU metadata of the two kernels in the built library: VGPRs, AGPRs, SGPRs, spills, scratch, static LDS."""
    readelf = "/opt/rocm/llvm/bin/llvm-readelf"
    blob = open(_lib.HIP_SO, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    k = blob.find(magic)
    fields = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
              "group_segment_fixed_size")
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
                if not name or not re.search(r"rz_antialias_edges|rz_antialias_seethrough_edges|rz_antialias_seethrough_classify|rz_seethrough_guides|rz_denoise_guides", name.group(1)):
                    continue
                vals = {f: int(m.group(1)) for f in fields if (m := re.search(rf"\.?{f}:\s+(\d+)", rec))}
                # waves per SIMD by registers: 512 VGPRs per lane, allocated in blocks of 8, at most 8 waves
                regs = vals.get("vgpr_count", 0) + vals.get("agpr_count", 0)
                waves = min(8, 512 // max(8, -(-regs // 8) * 8))
                print(f"{name.group(1)}: " + ", ".join(f"{f} {vals.get(f, 0)}" for f in fields) + f"; waves per SIMD by registers {waves}")
        k = blob.find(magic, k + 1)


def see_through():
    from test_rays_gpu import Hip
    hip = Hip()
    W, H, s = 1920, 1080, 2
    glass = "--config" in sys.argv and sys.argv[sys.argv.index("--config") + 1] == "c2g"
    sc = S.bunny_scene(n=76, aspect=W / H, extras=glass)
    label = "c2g (C2 plus a glass blob and a mirror cube)" if glass else "C2 (bunny_scene, nothing specular)"
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 1, 0))
    stream = hip.stream()
    r.set_stream(stream)
    r.render()
    d_aa = hip.alloc(W * H * 12)
    t_first = timed(r, hip, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s))
    print(f"{label}, {W}x{H}, s = {s}, library {_lib.hip().rz_source_hash().decode()}: rz_antialias {t_first:.3f} ms")
    if hasattr(_lib.hip(), "rz_antialias_seethrough"):
        first = r.antialias(factor=1, edges=True)[1]
        _, ch, edge = r.antialias(factor=1, see_through=8, chains=True, edges=True)
        moved = (ch["word"] & 0xFF) > 0
        del ch
        k_hi = r.upscale(factor=s, see_through=8, chains=True)[1]["word"] & 0xFF        # a chain of k steps is k + 1 queries
        q_edge = (k_hi.reshape(H, s, W, s).transpose(0, 2, 1, 3)[edge] + 1).mean()
        print(f"  edge share first-hit {first.mean():.4f}, see-through {edge.mean():.4f}; edge pixels whose chain moves {(edge & moved).mean():.4f} "
              f"of the frame; chain pixels {moved.mean():.4f}; mean queries per sub-sample of an edge pixel {q_edge:.3f}, deepest chain "
              f"{int(k_hi.max())}")
        del k_hi
        d_up = hip.alloc(W * H * s * s * 12)
        t0 = timed(r, hip, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s, see_through=0))
        t8 = timed(r, hip, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s, see_through=8))
        t_rec = timed(r, hip, stream, lambda: r.upscale_device(None, None, d_up, factor=1, see_through=8))
        t_up = timed(r, hip, stream, lambda: r.upscale_device(None, d_up, None, factor=s, see_through=8))
        print(f"  rz_antialias_seethrough max_depth 0 {t0:.3f} ms, max_depth 8 {t8:.3f} ms; the frame-size chain records alone {t_rec:.3f} ms; "
              f"rz_upscale_seethrough from the same frame ({W * s}x{H * s}, max_depth 8) {t_up:.3f} ms; ratio {t_up / t8:.2f}")
        # the spread of repeated medians of 25
        rep = [timed(r, hip, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s, see_through=8)) for _ in range(5)]
        rep1 = [timed(r, hip, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s)) for _ in range(5)]
        print(f"  five more medians of 25: rz_antialias_seethrough {min(rep):.3f} .. {max(rep):.3f} ms, rz_antialias {min(rep1):.3f} .. {max(rep1):.3f} ms")
    else:
        rep1 = [timed(r, hip, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s)) for _ in range(5)]
        print(f"  five more medians of 25: rz_antialias {min(rep1):.3f} .. {max(rep1):.3f} ms")
    r.set_stream(0)
    hip.L.hipStreamDestroy(stream)
    r.close()
    hip.close()


def main():
    if "--kernels" in sys.argv:
        return kernels()
    if "--see-through" in sys.argv:
        return see_through()
    from test_rays_gpu import Hip
    hip = Hip()
    W, H = 1920, 1080
    for label, make in (("C2 (bunny_scene)", lambda: S.bunny_scene(n=76, aspect=W / H)),
                        ("RayZen's own scene (reference_scene)", lambda: S.reference_scene(aspect=W / H))):
        sc = make()
        r = Renderer(0)
        r.upload_scene(sc)
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 1, 0))
        stream = hip.stream()
        r.set_stream(stream)
        r.render()
        share = float(r.antialias(factor=1, edges=True)[1].mean())
        d_aa, dg, de = hip.alloc(W * H * 12), hip.alloc(W * H * 48), hip.alloc(W * H)
        t_guide = timed(r, hip, stream, lambda: r.antialias_device(None, None, dg, None))
        t_class = timed(r, hip, stream, lambda: r.antialias_device(None, d_aa, None, de, factor=1))
        print(f"{label}, {W}x{H}: edge share {share:.4f}; the frame-size guide cast alone {t_guide:.3f} ms (it writes rz_hit records "
              f"here); with the classification and the copy of c (factor 1, edges asked for) {t_class:.3f} ms")
        for s in (2, 3, 4):
            d_up = hip.alloc(W * H * s * s * 12)
            t_aa = timed(r, hip, stream, lambda: r.antialias_device(None, d_aa, None, None, factor=s))
            t_up = timed(r, hip, stream, lambda: r.upscale_device(None, d_up, None, factor=s))
            print(f"  s = {s}: rz_antialias {t_aa:.3f} ms; rz_upscale from the same frame ({W * s}x{H * s}) {t_up:.3f} ms; ratio {t_up / t_aa:.2f}")
            hip.ok(hip.L.hipDeviceSynchronize())
            hip.L.hipFree(C.c_void_p(d_up))
            hip.bufs.remove(d_up)
        r.set_stream(0)
        hip.L.hipStreamDestroy(stream)
        r.close()
    hip.close()


if __name__ == "__main__":
    main()

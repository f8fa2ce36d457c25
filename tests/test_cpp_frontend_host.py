"""Host-only checks of the C++ front end (rayzen_amd/csrc/host/Renderer.h): no GPU, no library.  The GPU side is
tests/test_cpp_frontend_gpu.py."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marshalling_is_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/marshalling_check.cpp, built with AddressSanitizer and UBSan: createRig hands rz_skin_create the counts and
    NULL conventions the ABI states (morphs.size() / n targets, skin NULL for a morph-only rig), and a skin or morph vector of
    the wrong size throws before the library -- here a stub that reads every record it is promised -- is given the pointer;
    traceRays, shadowRays and denoiseTemporal pass the flags their arguments ask for and outputs of the size they state,
    presentUpscaled sizes its buffer by the factor; and pickRay's 28 bytes are pick_ray's (the same binary32 arithmetic)."""
    exe = str(tmp_path / "marshalling_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rayzen_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "marshalling_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "marshalling_check ok" in out.stdout
    from rayzen_amd import scene as S
    from rayzen_amd.renderer import make_rays, pick_ray
    cam = S.Camera(position=(0.5, 2.5, 10.0), target=(0.1, -0.2, -1.0), fov=70.0, aspect=np.float32(33) / np.float32(17))
    rays = [line.split() for line in out.stdout.splitlines() if line.startswith("pick_ray ")]
    assert len(rays) == 16
    for _, mx, my, hexbytes in rays:
        o, d = pick_ray(float.fromhex(mx), float.fromhex(my), 33, 17, cam)
        assert make_rays(o[None], d[None]).tobytes()[:28].hex() == hexbytes, (mx, my)

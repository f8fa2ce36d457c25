"""Runs RayZen's own fragment shader on Mesa llvmpipe (oracle/glref/glref.c) -- the reference itself, run here.

TEST INFRASTRUCTURE ONLY, and only usable in the build container: it needs /root/reference (the shaders are read from
there at run time, never copied) and Mesa's swrast_dri.so.  The GPU box has neither; tests there use the fixtures this
module generated (tests/golden/glref_*.npz, made by tests/golden/make_glref.py).
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(os.path.dirname(_HERE), "_ref")            # oracle/_ref/: git-ignored build outputs
BINARY = os.path.join(REF_DIR, "glref")
SHADER_DIR = "/root/reference/RayZen/shaders"
DRIVER = "/usr/lib/x86_64-linux-gnu/dri/swrast_dri.so"


def available():
    """The reference's shaders and Mesa's software driver are both here (true in the build container only)."""
    return os.path.exists(os.path.join(SHADER_DIR, "fragment_shader.glsl")) and os.path.exists(DRIVER)


_USABLE = None


def usable():
    """available(), the harness builds, and Mesa hands out an OpenGL >= 4.3 core context to it (probed once per process).
    Returns (True, GL string) or (False, reason): the live tests skip with the reason instead of failing on a box whose Mesa differs."""
    global _USABLE
    if _USABLE is None:
        if not available():
            _USABLE = (False, "RayZen's shaders / Mesa's swrast driver not present")
        else:
            try:
                build()
                with tempfile.TemporaryDirectory() as td:
                    blob = os.path.join(td, "probe.blob")
                    eye = np.eye(4, dtype=np.float32).reshape(16)
                    write_blob(blob, {}, eye, eye, eye, eye, np.zeros(3, np.float32), 1, 1, 1, 0)
                    p = subprocess.run([BINARY, blob, os.path.join(td, "o"), SHADER_DIR], env=dict(os.environ, GLREF_DRIVER=DRIVER, GLREF_PROBE="1"),
                                       capture_output=True, text=True, timeout=120)
                _USABLE = (p.returncode == 0, p.stderr.strip()[-300:])
            except Exception as e:          # no gcc, no headers, a driver that will not load ...
                _USABLE = (False, f"{type(e).__name__}: {e}"[:300])
    return _USABLE


def build(force=False):
    src = os.path.join(_HERE, "glref.c")
    if not force and os.path.exists(BINARY) and os.path.getmtime(BINARY) >= os.path.getmtime(src):
        return BINARY
    os.makedirs(REF_DIR, exist_ok=True)
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wno-unused-parameter", src, "-o", BINARY, "-ldl"])
    return BINARY


def write_blob(path, arrays, view, proj, inv_view, inv_proj, cam_pos, width, height, bounce_budget, num_lights,
               fps=0.0, show_lights=False, show_bvh=False, bvh_mode=0, selected_blas=0, selected_tri=0, num_samples=1):
    """arrays: binding index -> numpy array (the SSBO bytes as RayZen's main.cpp:1072-1119 uploads them)."""
    f32 = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n).tobytes()
    n_tris = int(arrays[0].shape[0]) if 0 in arrays else 0
    with open(path, "wb") as f:
        f.write(b"RZGL")
        f.write(struct.pack("<12i", 2, int(width), int(height), int(bounce_budget), int(num_lights), n_tris,
                            int(bool(show_lights)), int(bool(show_bvh)), int(bvh_mode), int(selected_blas), int(selected_tri),
                            int(num_samples)))
        f.write(struct.pack("<f", float(fps)))
        f.write(f32(view, 16) + f32(proj, 16) + f32(inv_view, 16) + f32(inv_proj, 16) + f32(cam_pos, 3))
        for b in range(10):
            a = arrays.get(b)
            raw = np.ascontiguousarray(a).tobytes() if a is not None and a.size else b""
            f.write(struct.pack("<Q", len(raw)))
            f.write(raw)


def render(arrays, view, proj, inv_view, inv_proj, cam_pos, width, height, bounce_budget, num_lights, timeout=1800, **kw):
    """FragColor of RayZen's shader for this scene and camera: (H, W, 4) float32, row 0 = the bottom row.
    The shader renders ONE sample per pixel (`numSamples = 1`, FS:676) and draws its FPS digits in the top-left corner.
    num_samples > 1 sets that one constant in the text the harness loads (glref.c) -- the product's `spp`."""
    build()
    with tempfile.TemporaryDirectory() as td:
        blob, out = os.path.join(td, "scene.blob"), os.path.join(td, "out.f32")
        write_blob(blob, arrays, view, proj, inv_view, inv_proj, cam_pos, width, height, bounce_budget, num_lights, **kw)
        env = dict(os.environ, GLREF_DRIVER=DRIVER)
        p = subprocess.run([BINARY, blob, out, SHADER_DIR], env=env, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            raise RuntimeError(f"glref failed ({p.returncode}): {p.stderr[-2000:]}")
        img = np.fromfile(out, np.float32).reshape(height, width, 4)
    return img, p.stderr.strip().splitlines()[0] if p.stderr.strip() else ""


def render_scene(scene, width, height, bounce_budget, num_lights=None, **kw):
    """`scene` is a rayzen_amd.scene.Scene (arrays + camera)."""
    cam = scene.camera
    nl = len(scene.lights) if num_lights is None else num_lights
    return render(scene.arrays, cam.view, cam.proj, cam.inv_view, cam.inv_proj, cam.position, width, height, bounce_budget,
                  nl, **kw)


def probe_math(x, y, mode):
    """Tables of llvmpipe's OWN built-ins (oracle/glref/probe_math.glsl, not RayZen's shader): for each pair (x[i], y[i])
    four values -- mode 0: sin(x), cos(x), acos(y), fract(sin(x) * 43758.5453); 1: x / y, sqrt(x), inversesqrt(x), pow(x, y);
    2: dot((x, y), (12.9898, 78.233)), x * y + x, fract(x), length((x, y, 1)); 3: normalize((x, y, 1)), 1 / x.  -> (n, 4) float32."""
    build()
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    n, W = len(x), 1024
    H = (n + W - 1) // W
    buf = np.zeros(2 * W * H, np.float32)
    buf[0:2 * n:2], buf[1:2 * n:2] = x, y
    eye = np.eye(4, dtype=np.float32).reshape(16)
    with tempfile.TemporaryDirectory() as td:
        blob, out = os.path.join(td, "probe.blob"), os.path.join(td, "out.f32")
        write_blob(blob, {0: buf.view(np.uint8)}, eye, eye, eye, eye, np.zeros(3, np.float32), W, H, 1, 0)
        with open(blob, "r+b") as f:            # the header's numTriangles field carries the mode
            f.seek(4 + 4 * 5)
            f.write(struct.pack("<i", int(mode)))
        env = dict(os.environ, GLREF_DRIVER=DRIVER, GLREF_FRAGMENT=os.path.join(_HERE, "probe_math.glsl"))
        p = subprocess.run([BINARY, blob, out, SHADER_DIR], env=env, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"glref probe failed ({p.returncode}): {p.stderr[-2000:]}")
        return np.fromfile(out, np.float32).reshape(H * W, 4)[:n].copy()


# ---- editor mode: RayZen's raster pass (editor_vertex.glsl + editor_fragment.glsl, main.cpp:1210-1297) ----

EDITOR_AMBIENT = (0.03, 0.03, 0.03)         # sendRasterSceneData's uAmbientColor (main.cpp:1269)
EDITOR_CLEAR = (0.05, 0.05, 0.07, 1.0)      # the window's glClearColor (main.cpp:260)


def raster_normals(v0, v1, v2):
    """buildRasterMeshes' per-triangle normal (main.cpp:1220-1224) in binary32: normalize(cross(v1 - v0, v2 - v0)) with GLM's
    cross, dot ((x*x + y*y) + z*z) and normalize (v * (1 / sqrt(dot))); (0, 1, 0) where it is not finite or shorter than 1e-5."""
    f = np.float32
    e1, e2 = (np.asarray(v1, f) - np.asarray(v0, f)).astype(f), (np.asarray(v2, f) - np.asarray(v0, f)).astype(f)
    c = np.stack([e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2], e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0],
                  e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]], 1).astype(f)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        n = (c * (f(1.0) / np.sqrt(d))[:, None]).astype(f)
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        bad = ~np.isfinite(n).all(1) | ~(length >= f(1e-5))
    n[bad] = (0.0, 1.0, 0.0)
    return n


def normal_matrix(model):
    """transpose(inverse(mat3(model))) in binary32 (renderRasterized, main.cpp:1287), as 9 floats column-major.  The inverse is
    the adjugate over the determinant, the form of GLM's compute_inverse<3, 3> (m[c][r]: column c, row r; one reciprocal of
    the determinant, then nine products).  GLM's exact operation order is not reproduced bit for bit: an ulp of difference in
    the normal is within the comparison's per-pixel bound (tests/editor_glref.py)."""
    f = np.float32
    M = np.asarray(model, f).reshape(16)
    m = [[M[4 * c + r] for r in range(3)] for c in range(3)]
    one_over_det = f(1.0) / (m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2])
                             - m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2])
                             + m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]))
    inv = [[None] * 3 for _ in range(3)]
    inv[0][0] = (m[1][1] * m[2][2] - m[2][1] * m[1][2]) * one_over_det
    inv[1][0] = -(m[1][0] * m[2][2] - m[2][0] * m[1][2]) * one_over_det
    inv[2][0] = (m[1][0] * m[2][1] - m[2][0] * m[1][1]) * one_over_det
    inv[0][1] = -(m[0][1] * m[2][2] - m[2][1] * m[0][2]) * one_over_det
    inv[1][1] = (m[0][0] * m[2][2] - m[2][0] * m[0][2]) * one_over_det
    inv[2][1] = -(m[0][0] * m[2][1] - m[2][0] * m[0][1]) * one_over_det
    inv[0][2] = (m[0][1] * m[1][2] - m[1][1] * m[0][2]) * one_over_det
    inv[1][2] = -(m[0][0] * m[1][2] - m[1][0] * m[0][2]) * one_over_det
    inv[2][2] = (m[0][0] * m[1][1] - m[1][0] * m[0][1]) * one_over_det
    return np.array([inv[r][c] for c in range(3) for r in range(3)], f)      # transpose: column c of it is row c of inv


def editor_meshes(arrays):
    """The raster meshes and game objects behind a scene's arrays.  Binding 0 holds each mesh's triangles in Mesh::triangles
    order, one instance per object in object order (csrc/host/Scene.cpp: the flatten loop), so mesh k of object o is the run of
    binding 0 from globalTriOffset; its length runs to the next mesh's offset.  Asserted here, not assumed: instance o is object
    o (meshIndex == o) and each object's run is disjoint from the others' or the very same (a shared mesh).
    -> (meshes: [(offset, count)], objects: [(mesh or -1, transform)])."""
    tris, inst, nodes = arrays[0], arrays[9], arrays[7]
    assert (inst["meshIndex"] == np.arange(len(inst))).all(), "instance index != object index"
    empty = [bool(nodes[b]["count"] == 0 and nodes[b]["boundsMin"][0] > nodes[b]["boundsMax"][0]) for b in inst["blasNodeOffset"]]
    starts = sorted({int(g) for g, e in zip(inst["globalTriOffset"], empty) if not e})
    ends = starts[1:] + [len(tris)]
    meshes, index, objects = [], {}, []
    for g, e, xf in zip(inst["globalTriOffset"], empty, inst["transform"]):
        if e:
            objects.append((-1, xf))
            continue
        g = int(g)
        if g not in index:
            index[g] = len(meshes)
            meshes.append((g, ends[starts.index(g)] - g))
        objects.append((index[g], xf))
    assert sum(c for _, c in meshes) == len(tris), "binding 0 is not the objects' meshes back to back"
    return meshes, objects


def write_editor_blob(path, arrays, view, proj, cam_pos, width, height, num_lights, ambient=EDITOR_AMBIENT, clear=EDITOR_CLEAR):
    f32 = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n).tobytes()
    tris = arrays[0]
    meshes, objects = editor_meshes(arrays)
    vert = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("m", "<i4")])      # RasterVertex: glm::vec3, glm::vec3, int (28 B)
    with open(path, "wb") as f:
        f.write(b"RZED")
        f.write(struct.pack("<6i", 1, int(width), int(height), int(num_lights), len(meshes), len(objects)))
        f.write(f32(view, 16) + f32(proj, 16) + f32(cam_pos, 3) + f32(ambient, 3) + f32(clear, 4))
        for b in (1, 2):
            raw = np.ascontiguousarray(arrays[b]).tobytes()
            f.write(struct.pack("<Q", len(raw)))
            f.write(raw)
        for g, cnt in meshes:
            t = tris[g:g + cnt]
            v = np.zeros((cnt, 3), vert)
            nrm = raster_normals(t["v0"], t["v1"], t["v2"])
            for k, key in enumerate(("v0", "v1", "v2")):
                v[:, k]["p"] = t[key]
                v[:, k]["n"] = nrm
                v[:, k]["m"] = t["materialIndex"]
            f.write(struct.pack("<i", 3 * cnt))
            f.write(v.tobytes())
        for m, xf in objects:
            f.write(struct.pack("<i", m) + f32(xf, 16) + normal_matrix(xf).tobytes())


def render_editor(arrays, view, proj, cam_pos, width, height, num_lights, ambient=EDITOR_AMBIENT, clear=EDITOR_CLEAR, timeout=600):
    """RayZen's editor frame (renderRasterized) on llvmpipe, and an ID pass over the same fragments.  Rows: row 0 = the bottom
    row.  Returns a dict: rgb (H, W, 3) float32 -- FragColor from an RGBA32F attachment; rgba8 (H, W, 4) uint8 -- from an RGBA8
    one; object, prim, material (H, W) int32 (-1: background); world_pos, normal (H, W, 3) float32 (the fragment shader's
    inputs, the normal not yet normalised); frag_z (H, W) float32 (gl_FragCoord.z); depth (H, W) uint32, the 24-bit depth
    buffer (0xFFFFFF: cleared); gl: the GL string."""
    build()
    with tempfile.TemporaryDirectory() as td:
        blob, out = os.path.join(td, "scene.blob"), os.path.join(td, "out.bin")
        write_editor_blob(blob, arrays, view, proj, cam_pos, width, height, num_lights, ambient, clear)
        env = dict(os.environ, GLREF_DRIVER=DRIVER, GLREF_FRAGMENT=os.path.join(_HERE, "editor_ids.glsl"))
        p = subprocess.run([BINARY, blob, out, SHADER_DIR], env=env, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            raise RuntimeError(f"glref (editor) failed ({p.returncode}): {p.stderr[-2000:]}")
        raw = np.fromfile(out, np.uint8)
    n = width * height
    sizes = (16 * n, 4 * n, 16 * n, 16 * n, 16 * n, 4 * n)
    assert len(raw) == sum(sizes)
    parts = np.split(raw, np.cumsum(sizes)[:-1])
    rgba = parts[0].view(np.float32).reshape(height, width, 4)
    ids = parts[2].view(np.int32).reshape(height, width, 4)
    posz = parts[3].view(np.float32).reshape(height, width, 4)
    assert (rgba[..., 3] == 1.0).all()                  # FragColor = vec4(color, 1.0), and the clear colour's alpha
    return dict(rgb=np.ascontiguousarray(rgba[..., :3]), rgba8=parts[1].reshape(height, width, 4).copy(),
                object=ids[..., 0].copy(), prim=ids[..., 1].copy(), material=ids[..., 2].copy(),
                world_pos=np.ascontiguousarray(posz[..., :3]), frag_z=posz[..., 3].copy(),
                normal=np.ascontiguousarray(parts[4].view(np.float32).reshape(height, width, 4)[..., :3]),
                depth=(parts[5].view(np.uint32).reshape(height, width) >> 8).copy(),
                gl=p.stderr.strip().splitlines()[0] if p.stderr.strip() else "")


def render_editor_scene(scene, width, height, num_lights=None, **kw):
    """`scene`: anything with .arrays and .camera (view, proj, position)."""
    cam = scene.camera
    nl = len(scene.arrays[2]) if num_lights is None else num_lights
    return render_editor(scene.arrays, cam.view, cam.proj, cam.position, width, height, nl, **kw)

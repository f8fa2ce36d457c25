"""Editor preview (rz_render_editor, rz_editor.hip) on the GPU: its hit buffer against rz_trace_rays on the same pixel rays, bit
for bit; its colours against the float64 restatement of editor_fragment.glsl (editor_ref.py); clipping, isolation from the
render state, host / device paths, errors, the C++ frontend and a speed floor."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import editor_ref as ER
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, Renderer, editor_rays, frame_params, make_rays
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

RZ_FLAG_HOST_RELAYOUT = 4
F32 = np.float32
HIT_FIELDS = ("t", "point", "normal", "material", "instance", "triangle", "prim")


def _renderer(sc, flags=0):
    r = Renderer(0, flags)
    r.upload_scene(sc)
    return r


def _trace_pixels(r, cam, W, H, incoherent=False):
    rays = editor_rays(cam, W, H)
    return r.trace_rays(rays["origin"], rays["dir"], incoherent=incoherent)


def _assert_same_hits(ed, tr, what=""):
    flat = ed.reshape(-1)
    for k in HIT_FIELDS:
        a, b = np.ascontiguousarray(flat[k]), np.ascontiguousarray(tr[k])
        bad = (a.view(np.uint8).reshape(len(flat), -1) != b.view(np.uint8).reshape(len(flat), -1)).any(1)
        assert not bad.any(), f"{what} {k}: {int(bad.sum())} of {len(flat)} pixels differ (first {np.flatnonzero(bad)[:5]})"


def _assert_shading(sc, hits, rgb, rgba8, num_lights=None, ambient=ER.AMBIENT, clear=ER.CLEAR, materials=None, lights=None):
    mats = sc.materials if materials is None else materials
    lts = sc.lights if lights is None else lights
    flat = hits.reshape(-1)
    c = rgb.reshape(-1, 3)
    q = rgba8.reshape(-1, 4)
    hit = flat["instance"] >= 0
    assert hit.any()
    # miss pixels: the clear colour, exactly
    assert (c[~hit] == np.asarray(clear[:3], F32)).all()
    assert (q[~hit] == ER.quantise(np.asarray(clear[:3], F32)[None])[0]).all()
    want = ER.shade(flat["point"][hit], flat["normal"][hit], flat["material"][hit], mats, lts, sc.camera.position,
                    len(lts) if num_lights is None else num_lights, ambient)
    got = c[hit].astype(np.float64)
    err = np.abs(got - want)
    ok = (err <= 2e-5 * np.abs(want)) | (err <= 1e-6)
    assert ok.all(), f"{int((~ok).any(1).sum())} pixels off; worst {err.max():.3g} at {want[np.unravel_index(err.argmax(), err.shape)]:.6g}"
    # RGBA8 within one LSB of the quantised reference, and exactly rz_present's quantisation of rgb32f
    ref8 = ER.quantise(want.astype(F32))
    assert (np.abs(q[hit].astype(int) - ref8.astype(int)) <= 1).all()
    assert (q == ER.quantise(c)).all()


# ---------------------------------------------------------------------------------------------------------------------
# geometry and shading on the bench scenes

SCENES = {
    "c1": (lambda: S.cornell_scene(), 256, 256),
    "c2": (lambda: S.bunny_scene(n=76, aspect=16 / 9), 1920, 1080),
    "c4": (lambda: S.instanced_scene(n=76, count=16, aspect=16 / 9), 1920, 1080),
    "ref": (lambda: S.reference_scene(aspect=800 / 600), 800, 600),
    "c5": (lambda: S.stress_scene(n=289, aspect=16 / 9), 960, 540),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_editor_hits_equal_trace_rays_and_shading_matches(name):
    make, W, H = SCENES[name]
    sc = make()
    r = _renderer(sc)
    rgba8, rgb, hits = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
    assert rgba8.shape == (H, W, 4) and rgb.shape == (H, W, 3) and hits.shape == (H, W)
    tr = _trace_pixels(r, sc.camera, W, H)
    _assert_same_hits(hits, tr, name)
    _assert_shading(sc, hits, rgb, rgba8)
    if name in ("c4", "ref"):
        # the lane-by-lane walk: the same bytes
        e2, c2, h2 = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True, incoherent=True)
        assert e2.tobytes() == rgba8.tobytes() and c2.tobytes() == rgb.tobytes() and h2.tobytes() == hits.tobytes()
    if name == "c2":
        # the comparison has power: rays one ulp off differ on many pixels
        rays = editor_rays(sc.camera, W, H)
        d = rays["dir"].copy()
        d[:, 0] = np.nextafter(d[:, 0], np.float32(np.inf))
        moved = r.trace_rays(rays["origin"], d)
        diff = (moved["t"].view(np.uint32) != hits.reshape(-1)["t"].view(np.uint32)).sum()
        assert diff > 10000, diff
    r.close()
    if name in ("c1", "ref"):
        r2 = _renderer(sc, RZ_FLAG_HOST_RELAYOUT)
        e3, c3, h3 = r2.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
        r2.close()
        assert e3.tobytes() == rgba8.tobytes() and c3.tobytes() == rgb.tobytes() and h3.tobytes() == hits.tobytes()


@pytest.mark.parametrize("window", [None, "2"])
def test_editor_deep_blas_with_and_without_overflow(window, monkeypatch):
    if window:
        monkeypatch.setenv("RZ_BLAS_STACK_WINDOW", window)
    sc = S.stress_scene()
    assert sc.max_blas_depth >= 21
    W, H = 320, 180
    r = _renderer(sc)
    rgba8, rgb, hits = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
    _assert_same_hits(hits, _trace_pixels(r, sc.camera, W, H), "stress")
    e2, _, h2 = r.render_editor(sc.camera, W, H, hits=True, incoherent=True)
    r.close()
    assert h2.tobytes() == hits.tobytes() and e2.tobytes() == rgba8.tobytes()
    _assert_shading(sc, hits, rgb, rgba8)


# ---------------------------------------------------------------------------------------------------------------------
# a scene built for coverage: every branch of the shader

def _coverage_scene(lights):
    mats = np.zeros(7, S.MATERIAL)
    rows = [((0.8, 0.3, 0.3), 0.0, 1.0, 0.0), ((0.1, 0.7, 0.1), 1.0, 0.35, 0.0), ((1.0, 1.0, 1.0), 1.0, 0.01, 0.0),
            ((0.85, 0.95, 1.0), 0.0, 0.02, 0.94), ((0.6, 0.4, 0.2), 0.0, 0.9, 2.5), ((0.9, 0.8, 0.2), 0.5, 0.05, 0.0),
            ((0.3, 0.3, 0.9), 0.0, 0.6, 0.0)]
    for i, (alb, met, rough, tr) in enumerate(rows):
        mats[i] = (alb, met, rough, 0.0, tr, 1.5)
    sc = S.Scene(materials=mats, lights=lights, camera=S.Camera(position=(0.0, 1.0, 6.0), aspect=4 / 3))
    floor = sc.add_mesh(S.make_quad((-6, -1, 6), (6, -1, 6), (6, -1, -6), (-6, -1, -6), 6))
    # a wall facing AWAY from the camera: seen from behind (no culling, NdotV = 0)
    back = sc.add_mesh(S.make_quad((-5, -1, -2), (-5, 3, -2), (-1, 3, -2), (-1, -1, -2), 1))
    sc.add_object(floor)
    sc.add_object(back)
    for k in range(6):
        blob = sc.add_mesh(S.make_blob(12, 0.55, k))
        sc.add_object(blob, S.translate(S.identity(), (-2.5 + k * 1.0, 0.0 + 0.3 * (k % 2), 0.5 - 0.2 * k)))
    return sc.build()


def _coverage_lights():
    l = np.zeros(4, S.LIGHT)
    l[0] = ((3.0, 4.0, 3.0, 1.0), (1.0, 0.9, 0.8), 60.0)       # point
    l[1] = ((0.4, 1.0, 0.6, 0.0), (0.7, 0.8, 1.0), 1.5)        # directional (not unit)
    l[2] = ((0.0, -1.0, 0.0, 0.0), (1.0, 1.0, 1.0), 3.0)       # from below: behind most surfaces
    l[3] = ((-2.0, 0.5, 2.0, 0.999), (1.0, 0.2, 0.2), 2.0)     # w != 1: directional
    return l


@pytest.mark.parametrize("num_lights", [0, 2, 4, 9])
def test_editor_coverage_scene(num_lights):
    lights = _coverage_lights()
    sc = _coverage_scene(lights)
    W, H = 320, 240
    r = _renderer(sc)
    rgba8, rgb, hits = r.render_editor(sc.camera, W, H, num_lights=num_lights, rgb32f=True, hits=True)
    _assert_same_hits(hits, _trace_pixels(r, sc.camera, W, H), "coverage")
    mats_hit = set(hits.reshape(-1)["material"][hits.reshape(-1)["instance"] >= 0].tolist())
    assert {0, 1, 2, 3, 4, 5, 6} <= mats_hit, mats_hit
    _assert_shading(sc, hits, rgb, rgba8, num_lights=num_lights)
    # ambient and clear colour of the caller's choosing
    amb, clr = (0.2, 0.1, 0.05), (0.5, 0.25, 0.125, 1.0)
    e2, c2, h2 = r.render_editor(sc.camera, W, H, num_lights=num_lights, ambient=amb, clear=clr, rgb32f=True, hits=True)
    r.close()
    assert h2.tobytes() == hits.tobytes()
    _assert_shading(sc, h2, c2, e2, num_lights=num_lights, ambient=amb, clear=clr)


def test_editor_zero_lights_uploaded():
    sc = _coverage_scene(np.zeros(0, S.LIGHT))
    r = _renderer(sc)
    rgba8, rgb, hits = r.render_editor(sc.camera, 160, 120, rgb32f=True, hits=True)
    r.close()
    _assert_shading(sc, hits, rgb, rgba8, num_lights=0)


# ---------------------------------------------------------------------------------------------------------------------
# clipping

def _clip_scene(extra=None):
    sc = S.Scene(camera=S.Camera(position=(0.0, 0.0, 3.0), aspect=4 / 3, near=0.1, far=100.0))
    m = sc.add_mesh(S.make_blob(16, 1.2, 1))
    sc.add_object(m)
    if extra == "near":
        # a quad 0.05 in front of the camera, wider than the view there: it covers every pixel, inside the near plane
        q = sc.add_mesh(S.make_quad((-1, -1, 2.95), (1, -1, 2.95), (1, 1, 2.95), (-1, 1, 2.95), 2))
        sc.add_object(q)
    if extra == "far":
        q = sc.add_mesh(S.make_quad((-300, -300, -120), (300, -300, -120), (300, 300, -120), (-300, 300, -120), 4))
        sc.add_object(q)
    return sc.build()


def test_editor_near_plane_restart_shows_what_lies_behind():
    W, H = 160, 120
    base = _clip_scene()
    r = _renderer(base)
    e0, c0, h0 = r.render_editor(base.camera, W, H, rgb32f=True, hits=True)
    r.close()
    sc = _clip_scene("near")
    r = _renderer(sc)
    # the quad is what rz_trace_rays sees first on every pixel ...
    tr = _trace_pixels(r, sc.camera, W, H)
    assert (tr["instance"] == 1).all()
    e1, c1, h1 = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
    r.close()
    f0, f1 = h0.reshape(-1), h1.reshape(-1)
    # ... but the editor frame skips it: the same surfaces as without the quad.  (The restarted ray starts from a rounded
    # point on the near plane, and the triangle test sees a different origin: a ray through an edge shared by two triangles
    # may land in the neighbour, a ray that grazes the silhouette on its other side -- a few pixels in a thousand at most.)
    same_inst = f0["instance"] == f1["instance"]
    assert (~same_inst).sum() <= 3, np.flatnonzero(~same_inst)
    same = same_inst.copy()
    for k in ("triangle", "prim", "material"):
        same &= f0[k] == f1[k]
    assert (~same).mean() <= 1e-3, np.flatnonzero(~same)
    hit = (f0["instance"] >= 0) & same
    assert hit.mean() > 0.2 and (f0["instance"] < 0).any()
    assert np.allclose(f1["t"][hit], f0["t"][hit], rtol=1e-5)
    c0, c1 = c0.reshape(-1, 3)[same], c1.reshape(-1, 3)[same]
    assert np.allclose(c1, c0, rtol=2e-4, atol=1e-5)
    assert (np.abs(e1.reshape(-1, 4)[same].astype(int) - e0.reshape(-1, 4)[same].astype(int)) <= 1).all()


def test_editor_beyond_far_plane_is_background():
    W, H = 160, 120
    sc = _clip_scene("far")
    r = _renderer(sc)
    tr = _trace_pixels(r, sc.camera, W, H)
    assert (tr["instance"] == 1).sum() > 1000          # the far quad is there for rz_trace_rays
    e, c, h = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
    r.close()
    f = h.reshape(-1)
    assert not (f["instance"] == 1).any()
    bg = f["instance"] < 0
    assert ((tr["instance"] == 1) <= bg).all()
    assert (f["t"][bg] == F32(1e30)).all() and (f["prim"][bg] == -1).all() and (f["triangle"][bg] == -1).all()
    assert (c.reshape(-1, 3)[bg] == np.asarray(ER.CLEAR[:3], F32)).all()


# ---------------------------------------------------------------------------------------------------------------------
# isolation, paths, streams, errors

def test_editor_leaves_the_render_state_alone():
    sc = S.bunny_scene(n=24, aspect=16 / 9)
    W, H = 96, 54

    def run(with_editor):
        r = _renderer(sc)
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 4, 0))
        r.render()
        plan = r.debug_last_plan()
        if with_editor:
            other = S.Camera(position=(1.0, 3.0, 7.0), aspect=4 / 3)
            r.render_editor(other, 200, 150, num_lights=1, rgb32f=True, hits=True)
            assert r.debug_last_plan() == plan
        acc0 = r.read_accum()
        r.set_frame(frame_params(sc.camera, W, H, len(sc.lights), 4, 4, 4))
        r.render()
        acc = r.read_accum()
        # the frame rz_set_frame set is the one that renders next: resolve reads width / height from it
        rgba = r.resolve_rgba8()
        r.close()
        return acc0, acc, rgba

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_editor_host_and_device_paths_agree_and_null_outputs():
    hip = Hip()
    sc = S.instanced_scene(n=24, count=16, aspect=16 / 9)
    W, H = 333, 187                                         # partial tiles on both edges
    r = _renderer(sc)
    e, c, h = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
    n = W * H
    d8, d32, dh = hip.alloc(n * 4, fill=0x5A), hip.alloc(n * 12, fill=0x5A), hip.alloc(n * 48, fill=0x5A)
    r.render_editor_device(sc.camera, W, H, d8, d32, dh)
    r.sync()
    assert hip.download(d8, n * 4).tobytes() == e.tobytes()
    assert hip.download(d32, n * 12).tobytes() == c.tobytes()
    assert hip.download(dh, n * 48).tobytes() == h.tobytes()
    # NULL outputs: each alone, and none at all
    for which in ("rgba8", "rgb32f", "hits"):
        p8, p32, ph = hip.alloc(n * 4, fill=0), hip.alloc(n * 12, fill=0), hip.alloc(n * 48, fill=0)
        r.render_editor_device(sc.camera, W, H, p8 if which == "rgba8" else None, p32 if which == "rgb32f" else None,
                               ph if which == "hits" else None)
        r.sync()
        want = {"rgba8": (p8, e, n * 4), "rgb32f": (p32, c, n * 12), "hits": (ph, h, n * 48)}
        for k, (p, ref, nb) in want.items():
            got = hip.download(p, nb)
            assert (got.tobytes() == ref.tobytes()) if k == which else not got.any(), (which, k)
    r.render_editor_device(sc.camera, W, H)
    r.sync()
    e2, c2, h2 = r.render_editor(sc.camera, W, H)
    assert c2 is None and h2 is None and e2.tobytes() == e.tobytes()
    r.close()
    hip.close()


def test_editor_on_a_user_stream_sees_the_new_transforms():
    hip = Hip()
    sc = S.instanced_scene(n=24, count=16, aspect=16 / 9)
    W, H = 192, 108
    r = _renderer(sc)
    _, _, before = r.render_editor(sc.camera, W, H, hits=True)
    stream = hip.stream()
    r.set_stream(stream)
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(t, F32).reshape(16) for t in S.instanced_transforms(11, 16)])
    r.update_transforms(xf)
    dh = hip.alloc(W * H * 48)
    r.render_editor_device(sc.camera, W, H, hits_ptr=dh)
    r.sync()
    got = hip.download(dh, W * H * 48).view(HIT_DTYPE)
    tr = _trace_pixels(r, sc.camera, W, H)          # after the update, on the same stream
    r.set_stream(0)
    r.close()
    hip.L.hipStreamDestroy(stream)
    hip.close()
    _assert_same_hits(got, tr, "after update_transforms")
    assert (got["t"] != before.reshape(-1)["t"]).any()


def test_editor_error_paths():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    r = _renderer(sc)
    W, H = 16, 8
    n = W * H
    fp = frame_params(sc.camera, W, H, 2, 0, 1)
    p8, p32, ph = hip.alloc(n * 4 + 16, fill=0x5A), hip.alloc(n * 12 + 16, fill=0x5A), hip.alloc(n * 48 + 16, fill=0x5A)
    ok = (p8, n * 4, p32, n * 12, ph, n * 48)

    def call(ctx, frame, args=ok, flags=0):
        a = list(args)
        return L.rz_render_editor(ctx, frame, None, C.c_void_p(a[0]), a[1], C.c_void_p(a[2]), a[3], C.c_void_p(a[4]), a[5], flags)

    assert call(None, C.byref(fp)) == -1
    assert call(r._c, None) == -1 and L.rz_last_error(r._c)
    for w, h in ((0, 8), (16, 0), (-3, 8)):
        bad = frame_params(sc.camera, w, h, 2, 0, 1)
        assert call(r._c, C.byref(bad)) == -1
    assert call(r._c, C.byref(fp), (p8, n * 4, p32, n * 12, ph + 8, n * 48)) == -1 and b"aligned" in L.rz_last_error(r._c)
    assert call(r._c, C.byref(fp), (p8 + 2, n * 4, p32, n * 12, ph, n * 48)) == -1
    assert call(r._c, C.byref(fp), (p8, n * 4, p32 + 1, n * 12, ph, n * 48)) == -1
    assert call(r._c, C.byref(fp), flags=0x80) == -1
    assert call(r._c, C.byref(fp), (p8, n * 4 - 1, p32, n * 12, ph, n * 48)) == -7
    assert call(r._c, C.byref(fp), (p8, n * 4, p32, n * 12 - 4, ph, n * 48)) == -7
    assert call(r._c, C.byref(fp), (p8, n * 4, p32, n * 12, ph, n * 48 - 48)) == -7
    r.sync()
    for p, nb in ((p8, n * 4 + 16), (p32, n * 12 + 16), (ph, n * 48 + 16)):
        assert (hip.download(p, nb) == 0x5A).all()          # nothing was launched
    assert call(r._c, C.byref(fp), (p8 + 4, n * 4, p32 + 4, n * 12, ph + 16, n * 48)) == 0     # 4- and 16-byte aligned are fine
    assert call(r._c, C.byref(fp), (None, 0, None, 0, None, 0)) == 0
    r.sync()
    empty = Renderer(0)
    assert call(empty._c, C.byref(fp)) == -5 and L.rz_last_error(empty._c)
    empty.close()
    nomat = Renderer(0)
    for b in S.BINDING_DTYPES:
        nomat.upload(b, sc.arrays[b][:0] if b == S.BIND_MATERIALS else sc.arrays[b])
    assert call(nomat._c, C.byref(fp)) == -5 and b"material" in L.rz_last_error(nomat._c)
    nomat.close()
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# the C++ frontend

def test_cpp_render_editor_equals_python(tmp_path):
    """examples/render_editor.cpp: Renderer::renderEditor on a RayZen-style scene; its RGBA8 equals what the Python binding
    renders from the arrays and matrices the program used."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "rayzen_amd", "lib")
    exe = str(tmp_path / "render_editor")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(root, "rayzen_amd", "csrc", "host"), os.path.join(root, "examples", "render_editor.cpp"),
                           "-L", lib, "-lrayzen_host", "-lrayzen_hip", f"-Wl,-rpath,{lib}", "-o", exe])
    W, H = 200, 150
    out = subprocess.run([exe, str(tmp_path), str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rgba = np.fromfile(tmp_path / "editor.rgba", np.uint8).reshape(H, W, 4)
    frame = np.fromfile(tmp_path / "frame.f32", np.float32)
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.fromfile(tmp_path / f"binding{b}.bin", dt))

    class Cam:
        inv_view, inv_proj, view, proj = (frame[16 * k:16 * k + 16] for k in range(4))
        position = frame[64:67]

    e, _, h = r.render_editor(Cam, W, H, num_lights=int(frame[67]), hits=True)
    r.close()
    assert (h["instance"] >= 0).mean() > 0.2
    assert e.tobytes() == rgba.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# speed

def test_editor_speed_floor_c2():
    """The editor frame traces the same rays as rz_trace_rays without loading them or storing 48-B hits: at most 1.5x its
    time (medians of 25 runs each, device events)."""
    hip = Hip()
    sc = S.bunny_scene(n=76, aspect=16 / 9)
    W, H = 1920, 1080
    r = _renderer(sc)
    rays = editor_rays(sc.camera, W, H)
    n = len(rays)
    d_rays, d_hits, d8 = hip.upload(rays), hip.alloc(n * 48), hip.alloc(n * 4)
    stream = hip.stream()
    r.set_stream(stream)
    a, b = hip.event(), hip.event()

    def timed(fn, reps=25):
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
        return float(np.median(out))

    t_trace = timed(lambda: r.trace_rays_device(d_rays, d_hits, n))
    t_edit = timed(lambda: r.render_editor_device(sc.camera, W, H, rgba8_ptr=d8))
    px = hip.download(d8, n * 4).reshape(H, W, 4)
    r.set_stream(0)
    r.close()
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    hip.L.hipStreamDestroy(stream)
    hip.close()
    print(f"editor {t_edit:.3f} ms, trace_rays {t_trace:.3f} ms")
    assert px.std() > 5                                      # the frame did render
    assert t_edit <= 1.5 * t_trace, (t_edit, t_trace)


def test_editor_tile_waves_give_the_same_bytes(monkeypatch):
    """RZ_EDITOR_TILES=1 (the A/B of the wave shape: an 8 x 8 tile instead of 64 pixels of one row) changes no byte."""
    sc = S.bunny_scene(n=24, aspect=16 / 9)
    W, H = 203, 117
    r = _renderer(sc)
    a = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
    monkeypatch.setenv("RZ_EDITOR_TILES", "1")
    b = r.render_editor(sc.camera, W, H, rgb32f=True, hits=True)
    r.close()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()

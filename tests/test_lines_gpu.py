"""rz_draw_lines on the GPU.  Every operation of the definition is one binary32 operation, so the images are compared for
equality with tests/lines_ref.py, which lets every pixel meet every line in index order: no lists, no cull.  The timing test at
the end states its own bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lines_ref as LR
from rayzen_amd import _lib
from rayzen_amd import lines as LN
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, RayZenError, Renderer, frame_params
from test_rays_gpu import Hip

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEGAKERNEL = 1                      # RZ_FLAG_MEGAKERNEL
FRAMES = [(1, 1), (9, 7), (33, 9), (65, 5)]         # the last two cross the 32 x 8 tile in both axes


def _camera(w, h):
    return S.Camera(position=(0.0, 0.5, 4.5), aspect=w / h)


def _frame(cam, w, h):
    return frame_params(cam, w, h, 0, 1, 1)


def _random_lines(n, seed, alpha=None):
    """n world-space lines in front of _camera, random colours; alpha None: random bytes."""
    rng = np.random.default_rng(seed)
    a = rng.uniform((-4.0, -2.5, -3.0), (4.0, 3.5, 3.0), (n, 3))
    b = a + rng.normal(0.0, 1.5, (n, 3))
    out = LN.segments(a, b, (0, 0, 0, 0))
    out["color"] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    if alpha is not None:
        out["color"][:, 3] = alpha
    return out


def _images(w, h, seed=5):
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(-0.25, 1.5, (h, w, 3)).astype(F32)
    return rgb, rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def _same(got8, got32, want8, want32, what):
    if want8 is not None:
        bad = np.argwhere((got8 != want8).any(axis=-1))
        assert not len(bad), f"{what}: rgba8 differs on {len(bad)} pixels; first (y, x) {bad[0].tolist()}: {got8[tuple(bad[0])]} != {want8[tuple(bad[0])]}"
    if want32 is not None:
        bad = np.argwhere((got32.view(np.uint32) != want32.view(np.uint32)).any(axis=-1))
        assert not len(bad), f"{what}: rgb32f differs on {len(bad)} pixels; first (y, x) {bad[0].tolist()}: {got32[tuple(bad[0])]} != {want32[tuple(bad[0])]}"


def _check(r, lines, cam, w, h, what, hits=None, transforms=None, rgb=None, rgba8=None, both=True, **params):
    """The host form against the restatement; returns the images."""
    if rgb is None and rgba8 is None and both:
        rgb, rgba8 = _images(w, h)
    got8, got32 = r.draw_lines(lines, rgba8=rgba8, rgb32f=rgb, hits=hits, frame=_frame(cam, w, h), **params)
    want8, want32, info = LR.draw(lines, cam.view, cam.proj, w, h, hits=hits, rgba8=rgba8, rgb32f=rgb, transforms=transforms, **params)
    _same(got8, got32, want8, want32, what)
    return got8, got32, info


# ---------------------------------------------------------------------------------------------------------------------
# 1. frames, counts, widths

@pytest.mark.parametrize("w,h", FRAMES, ids=lambda v: str(v))
def test_frames_and_line_counts(w, h):
    """n = 0, 1, 257 and 1 025 cross the chunk of 256 records a workgroup scans and stages at a time."""
    cam = _camera(w, h)
    r = Renderer(0)                                         # no scene, no rz_set_frame
    rgb, rgba8 = _images(w, h)
    for n in (0, 1, 257, 1025):
        got8, got32, info = _check(r, _random_lines(n, 100 + n), cam, w, h, f"{w}x{h}, n = {n}", rgb=rgb, rgba8=rgba8)
        if n == 0:
            assert got8.tobytes() == rgba8.tobytes() and got32.tobytes() == rgb.tobytes()
        elif n > 1:
            assert info["touched"].any()
    r.close()


def test_300_half_transparent_lines_blend_in_index_order_and_the_same_twice():
    hip = Hip()
    w, h = 65, 5
    cam = _camera(w, h)
    lines = _random_lines(300, 7, alpha=128)
    lines["a"][:, 1] = lines["a"][:, 1] * 0.1 + 0.5          # across the strip the frame shows
    lines["b"][:, 1] = lines["b"][:, 1] * 0.1 + 0.5
    P = LR.project(lines, cam.view, cam.proj, w, h)
    rect, reach = LR.cull(P)
    held = [sum(LR.meets(P, rect, reach, i, tx, 0, LR.TILE_R) for i in range(300)) for tx in (0, 32)]
    assert min(held) >= 24, held                             # both whole tiles hold dozens (the third is one column)
    r = Renderer(0)
    rgb, rgba8 = _images(w, h)
    got8, got32, info = _check(r, lines, cam, w, h, "300 lines", rgb=rgb, rgba8=rgba8)
    _, rev, _ = LR.draw(lines, cam.view, cam.proj, w, h, rgb32f=rgb, order=range(299, -1, -1))
    assert info["touched"].mean() > 0.5 and (rev != got32).any()                # ... and the order decides
    d_lines = hip.upload(lines)
    outs = []
    for _ in range(2):
        d8, d32 = hip.upload(rgba8), hip.upload(rgb)
        r.draw_lines_device(d_lines, len(lines), d8, d32, frame=_frame(cam, w, h))
        r.sync()
        outs.append((hip.download(d8, rgba8.nbytes).tobytes(), hip.download(d32, rgb.nbytes).tobytes()))
    assert outs[0] == outs[1] == (got8.tobytes(), got32.tobytes())
    r.close()
    hip.close()


@pytest.mark.parametrize("width", [1.0, 1.5, 16.0])
@pytest.mark.parametrize("smooth", [0, 1], ids=["hard", "smooth"])
def test_widths_hard_and_smooth(width, smooth):
    r = Renderer(0)
    for w, h in ((33, 9), (65, 5)):
        _check(r, _random_lines(40, 11), _camera(w, h), w, h, f"{w}x{h} width {width} smooth {smooth}", width=width, smooth=smooth)
    r.close()


def test_lines_through_the_camera_plane_and_far_ends():
    w, h = 65, 37
    cam = _camera(w, h)
    rng = np.random.default_rng(3)
    n = 64
    a = rng.uniform((-2.0, -1.0, -2.0), (2.0, 2.0, 2.0), (n, 3))
    b = a.copy()
    b[:, 2] = rng.uniform(4.6, 9.0, n)                       # behind the camera at z = 4.5
    b[:, :2] += rng.normal(0.0, 2.0, (n, 2))
    through = LN.segments(a, b, (255, 255, 255, 200))
    through[::2] = LN.segments(b[::2], a[::2], (255, 0, 255, 200))             # either end may be the one that fails
    behind = LN.segments(b, b + (0.0, 1.0, 1.0), (0, 255, 0, 255))
    far = LN.segments(a, a + rng.choice([-1.0, 1.0], (n, 3)) * (3.0e5, 3.0e5, 0.0), (255, 200, 0, 160))   # ends some 2^20 px away
    bad = LN.segments([(np.nan, 0, 0), (0, 0, 0), (0, 0, 0)], [(0, 0, 0), (np.inf, 0, 0), (0, -np.inf, 1)], (255, 255, 255, 255))
    P = LR.project(far, cam.view, cam.proj, w, h)
    assert not P["drop"].any() and np.abs(P["sbx"]).max() > 2.0 ** 20
    assert LR.project(behind, cam.view, cam.proj, w, h)["drop"].all() and LR.project(bad, cam.view, cam.proj, w, h)["drop"].all()
    r = Renderer(0)
    for width, smooth in ((1.5, 0), (16.0, 1)):
        _, _, info = _check(r, np.concatenate([through, behind, far, bad]), cam, w, h, f"width {width}", width=width, smooth=smooth)
        assert info["touched"].any()
    rgb, rgba8 = _images(w, h)
    got8, got32 = r.draw_lines(np.concatenate([behind, bad]), rgba8=rgba8, rgb32f=rgb, frame=_frame(cam, w, h), width=16.0)
    assert got8.tobytes() == rgba8.tobytes() and got32.tobytes() == rgb.tobytes()
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. call forms

def test_each_image_alone_both_and_the_device_form():
    hip = Hip()
    w, h = 33, 9
    cam = _camera(w, h)
    fp = _frame(cam, w, h)
    lines = _random_lines(60, 21)
    rgb, rgba8 = _images(w, h)
    keep32, keep8 = rgb.copy(), rgba8.copy()
    want8, want32, _ = LR.draw(lines, cam.view, cam.proj, w, h, rgba8=rgba8, rgb32f=rgb)
    r = Renderer(0)
    both = r.draw_lines(lines, rgba8=rgba8, rgb32f=rgb, frame=fp)
    _same(both[0], both[1], want8, want32, "both")
    assert rgb.tobytes() == keep32.tobytes() and rgba8.tobytes() == keep8.tobytes()     # the caller's arrays are not modified
    only8, only32 = r.draw_lines(lines, rgba8=rgba8, frame=fp), r.draw_lines(lines, rgb32f=rgb, frame=fp)
    assert only8[1] is None and only32[0] is None
    _same(only8[0], only32[1], want8, want32, "each alone")
    r.set_frame(fp)                                         # frame None: the frame of set_frame
    _same(*r.draw_lines(lines, rgba8=rgba8, rgb32f=rgb), want8, want32, "frame of set_frame")
    d_lines = hip.upload(lines)
    for use8, use32 in ((True, True), (True, False), (False, True)):
        d8, d32 = hip.upload(rgba8), hip.upload(rgb)
        r.draw_lines_device(d_lines, len(lines), d8 if use8 else None, d32 if use32 else None, frame=fp)
        r.sync()
        got8 = hip.download(d8, rgba8.nbytes).reshape(h, w, 4)
        got32 = hip.download(d32, rgb.nbytes).view(F32).reshape(h, w, 3)
        _same(got8, got32, want8 if use8 else rgba8, want32 if use32 else rgb, f"device {use8} {use32}")
    r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the depth test and the instances

def _gizmos(sc):
    cam = sc.camera
    return np.concatenate([LN.segments([(-3.0, -0.5, -1.5)], [(3.0, -0.5, -1.5)], (255, 255, 0, 255)),     # passes behind the cube
                           LN.grid(3.0, 0.5, (200, 200, 200, 180), y=-1.5),
                           LN.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (255, 160, 0, 255), instance=2),
                           LN.axes((0.3, -0.5, 0.0), 1.5), LN.frustum(cam.inv_view, cam.inv_proj, (0, 255, 255, 255))])


def test_hits_from_the_editor_from_the_denoiser_and_none():
    hip = Hip()
    sc = S.cornell_scene()
    w, h = 65, 37
    cam = sc.camera
    fp = frame_params(cam, w, h, len(sc.lights), 1, 1)
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(fp)
    r.render()
    _, _, e_hits = r.render_editor(cam, w, h, rgb32f=True, hits=True)
    _, guides = r.denoise(iterations=0, guides=True)
    assert e_hits.dtype == HIT_DTYPE and guides.dtype == HIT_DTYPE
    xf = r.read_binding(S.BIND_INSTANCES)["transform"]
    lines = _gizmos(sc)
    rgb, rgba8 = _images(w, h)
    seen = {}
    for name, hits in (("editor", e_hits.reshape(h, w)), ("guides", guides.reshape(h, w)), ("none", None)):
        for hidden in (0.0, 0.25):
            got8, got32 = r.draw_lines(lines, rgba8=rgba8, rgb32f=rgb, hits=hits, frame=fp, hidden_alpha=hidden)
            want8, want32, info = LR.draw(lines, cam.view, cam.proj, w, h, hits=hits, rgba8=rgba8, rgb32f=rgb, transforms=xf,
                                          hidden_alpha=hidden)
            _same(got8, got32, want8, want32, f"{name} hidden_alpha {hidden}")
            seen[name, hidden] = (got32, info)
    occ = seen["editor", 0.0][1]["occluded"]
    assert occ.any() and seen["editor", 0.0][1]["visible"].any() and not seen["none", 0.0][1]["occluded"].any()
    assert (seen["editor", 0.25][0][occ] != seen["editor", 0.0][0][occ]).any()
    assert (seen["none", 0.0][0] != seen["editor", 0.0][0]).any()
    # the device form on the editor's device hits
    d_hits, d_lines, d8, d32 = hip.alloc(w * h * 48), hip.upload(lines), hip.upload(rgba8), hip.upload(rgb)
    r.render_editor_device(cam, w, h, hits_ptr=d_hits)
    r.draw_lines_device(d_lines, len(lines), d8, d32, d_hits, frame=fp)
    r.sync()
    want8, want32, _ = LR.draw(lines, cam.view, cam.proj, w, h, hits=e_hits.reshape(h, w), rgba8=rgba8, rgb32f=rgb, transforms=xf)
    _same(hip.download(d8, rgba8.nbytes).reshape(h, w, 4), hip.download(d32, rgb.nbytes).view(F32).reshape(h, w, 3), want8, want32, "device")
    r.close()
    hip.close()


def test_instance_local_boxes_follow_update_transforms():
    sc = S.instanced_scene(n=12)
    w, h = 64, 36
    cam = sc.camera
    fp = frame_params(cam, w, h, len(sc.lights), 1, 1)
    r = Renderer(0)
    r.upload_scene(sc)
    n = r.n_instances()
    roots = sc.arrays[S.BIND_BLAS_NODES][sc.arrays[S.BIND_INSTANCES]["blasNodeOffset"]]
    lines = np.concatenate([LN.box(roots["boundsMin"][k], roots["boundsMax"][k], (255, 160, 0, 200), instance=k) for k in range(n)])
    _, _, hits = r.render_editor(cam, w, h, rgb32f=True, hits=True)
    before = r.read_binding(S.BIND_INSTANCES)["transform"]
    first = _check(r, lines, cam, w, h, "before", hits=hits.reshape(h, w), transforms=before)
    xf = np.stack([np.asarray(sc.arrays[S.BIND_INSTANCES]["transform"][0], F32)] +
                  [np.asarray(m, F32).reshape(16) for m in S.instanced_transforms(7, 16)])
    r.update_transforms(xf)
    _, _, hits2 = r.render_editor(cam, w, h, rgb32f=True, hits=True)
    after = r.read_binding(S.BIND_INSTANCES)["transform"]
    second = _check(r, lines, cam, w, h, "after", hits=hits2.reshape(h, w), transforms=after)
    assert (after != before).any() and second[1].tobytes() != first[1].tobytes() and first[2]["touched"].sum() > 100
    r.close()


def test_1080p_mesh_edges_binned_counted_and_unbinned(monkeypatch):
    """A few thousand edges of a small mesh at 1920 x 1080, against the restatement on a 64 x 64 crop; then the same call with
    the lists sized from the counts (RZ_LINES_DIRECT_BYTES=0: the call waits for them) and with no lists at all
    (RZ_LINES_UNBINNED=1): the same bytes on the whole frame."""
    hip = Hip()
    sc = S.bunny_scene(n=12)
    w, h = 1920, 1080
    cam = sc.camera
    fp = frame_params(cam, w, h, len(sc.lights), 1, 1)
    r = Renderer(0)
    r.upload_scene(sc)
    inst = sc.arrays[S.BIND_INSTANCES]
    tris = sc.arrays[S.BIND_TRIANGLES]
    k = 1                                                   # the mesh over the floor
    first = int(inst["globalTriOffset"][k])
    assert len(inst) == 2 and len(tris) - first == 12 * 12 * 12
    lines = LN.mesh_edges(tris[first:], (20, 20, 20, 160), instance=k)
    assert 2000 < len(lines) < 5000
    d_hits, d_lines = hip.alloc(w * h * 48), hip.upload(lines)
    r.render_editor_device(cam, w, h, hits_ptr=d_hits)
    base = np.full((h, w, 4), 0x80, np.uint8)
    outs = []
    for env in ({}, {"RZ_LINES_DIRECT_BYTES": "0"}, {"RZ_LINES_UNBINNED": "1"}):
        for name in ("RZ_LINES_DIRECT_BYTES", "RZ_LINES_UNBINNED"):
            monkeypatch.delenv(name, raising=False)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        d8 = hip.upload(base)
        r.draw_lines_device(d_lines, len(lines), d8, None, d_hits, frame=fp, smooth=True)
        r.sync()
        outs.append(hip.download(d8, base.nbytes).reshape(h, w, 4))
    hits = hip.download(d_hits, w * h * 48).view(HIT_DTYPE).reshape(h, w)
    xf = r.read_binding(S.BIND_INSTANCES)["transform"]
    r.close()
    hip.close()
    changed = np.argwhere((outs[0] != base).any(axis=-1))
    assert len(changed) > 5000
    cy, cx = (int(v) for v in np.median(changed, axis=0))
    crop = (cx - 32, cy - 32, cx + 32, cy + 32)
    want8, _, info = LR.draw(lines, cam.view, cam.proj, w, h, hits=hits, rgba8=base, transforms=xf, crop=crop, smooth=1)
    assert info["touched"].sum() > 200 and info["occluded"].any()
    _same(outs[0][crop[1]:crop[3], crop[0]:crop[2]], None, want8, None, "crop")
    assert outs[1].tobytes() == outs[0].tobytes() and outs[2].tobytes() == outs[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 4. isolation

def _display_bytes(r):
    return tuple(v.tobytes() if hasattr(v, "tobytes") else v for v in r.display_state().values())


@pytest.mark.parametrize("flags", [0, MEGAKERNEL], ids=["samples", "pixels"])
def test_the_call_leaves_render_temporal_and_display_state_alone(flags):
    sc = S.reference_scene()                                # (its glass carries currentIor from chunk to chunk)
    w, h, spp, bounces = 40, 30, 2, 5
    nl = len(sc.lights)
    lines = np.concatenate([LN.grid(4.0, 1.0, (255, 255, 255, 128)), LN.box((-1, -1, -1), (1, 1, 1), (255, 0, 0, 255), instance=0)])

    def run(with_calls):
        r = Renderer(0, flags)
        r.upload_scene(sc)
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, 0))
        r.render()
        first = r.read_accum()
        r.denoise_temporal()
        r.display(first[..., :3] / np.maximum(first[..., 3:], 1), auto=True)
        if with_calls:
            plan, kernel, ms = r.debug_last_plan(), r.last_kernel_name(), r.last_render_ms()
            hist = [r.debug_read_temporal(k).tobytes() for k in range(5)]
            disp = _display_bytes(r)
            _, rgba8 = r.present(show_fps=False)
            _, guides = r.denoise(iterations=0, guides=True)
            other = _camera(65, 5)
            r.draw_lines(lines, rgba8=rgba8, hits=guides.reshape(h, w))
            r.draw_lines(lines, rgb32f=np.zeros((5, 65, 3), F32), frame=_frame(other, 65, 5))        # another frame: rz_set_frame's stays
            assert r.read_accum().tobytes() == first.tobytes()
            assert (r.debug_last_plan(), r.last_kernel_name(), r.last_render_ms()) == (plan, kernel, ms)
            assert (r.width, r.height) == (w, h)
            assert [r.debug_read_temporal(k).tobytes() for k in range(5)] == hist and _display_bytes(r) == disp
        r.set_frame(frame_params(sc.camera, w, h, nl, bounces, spp, spp))
        r.render()
        r.sync()
        out = r.read_accum(), len(r.render_history_ms())
        r.close()
        return out

    plain, n_plain = run(False)
    mixed, n_mixed = run(True)
    assert mixed.tobytes() == plain.tobytes()
    assert n_mixed == n_plain == 2


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors

def test_error_codes_leave_the_images_untouched():
    hip = Hip()
    L = _lib.hip()
    sc = S.cornell_scene()
    w, h = 20, 6
    npx = w * h
    cam = sc.camera
    fp = frame_params(cam, w, h, 2, 1, 1)
    lines = np.concatenate([LN.grid(2.0, 1.0, (255, 255, 255, 255)), LN.box((-1, -1, -1), (1, 1, 1), (255, 0, 0, 255), instance=2)])
    n = len(lines)
    r = Renderer(0)
    r.upload_scene(sc)
    d_lines, d_hits = hip.upload(np.concatenate([lines, lines[:1]])), hip.alloc(npx * 48 + 16, 0)
    d8, d32 = hip.alloc(npx * 4 + 16, 0x5A), hip.alloc(npx * 12 + 16, 0x5A)

    def params(width=1.5, near_w=0.01, depth_bias=2.0 ** -8, hidden_alpha=0.0, smooth=0, reserved=None):
        p = _lib.LinesParams(width, near_w, depth_bias, hidden_alpha, smooth)
        if reserved is not None:
            p.reserved[reserved] = 1
        return C.byref(p)

    def call(ctx, frame=fp, p=None, args=None, flags=0):
        a = args if args is not None else (d_lines, n, d_hits, npx * 48, d8, npx * 4, d32, npx * 12)
        return L.rz_draw_lines(ctx, None if frame is None else C.byref(frame), p, *a, flags)

    nan, inf = float("nan"), float("inf")
    assert call(None) == -1 and call(r._c, frame=None) == -1
    assert call(r._c, flags=2) == -1 and call(r._c, flags=0x80000000) == -1
    for bad in ((0, 8), (16, 0), (-1, 8), (1 << 16, 1 << 16), ((1 << 23) + 1, 1)):
        assert call(r._c, frame=frame_params(cam, bad[0], bad[1], 2, 1, 1)) == -1, bad
    for bad in (dict(width=0.99), dict(width=16.5), dict(width=nan), dict(width=inf), dict(near_w=0.0), dict(near_w=-1.0), dict(near_w=nan),
                dict(near_w=inf), dict(depth_bias=-0.01), dict(depth_bias=1.0), dict(depth_bias=nan), dict(hidden_alpha=-0.1),
                dict(hidden_alpha=1.1), dict(hidden_alpha=nan), dict(smooth=2), dict(smooth=-1), dict(reserved=0), dict(reserved=1),
                dict(reserved=2)):
        assert call(r._c, p=params(**bad)) == -1, bad
    assert call(r._c, args=(None, n, d_hits, npx * 48, d8, npx * 4, d32, npx * 12)) == -1 and b"null lines" in L.rz_last_error(r._c)
    assert call(r._c, args=(d_lines, (1 << 20) + 1, d_hits, npx * 48, d8, npx * 4, d32, npx * 12)) == -1
    assert call(r._c, args=(d_lines, n, d_hits, npx * 48, None, 0, None, 0)) == -1 and b"neither" in L.rz_last_error(r._c)
    for k, off in ((0, 8), (2, 8), (4, 2), (6, 2)):
        a = [d_lines, n, d_hits, npx * 48, d8, npx * 4, d32, npx * 12]
        a[k] += off
        assert call(r._c, args=tuple(a)) == -1 and b"aligned" in L.rz_last_error(r._c), k
    assert call(r._c, args=(d_lines, n, d_hits, npx * 48 - 1, d8, npx * 4, d32, npx * 12)) == -7
    assert call(r._c, args=(d_lines, n, d_hits, npx * 48, d8, npx * 4 - 1, d32, npx * 12)) == -7
    assert call(r._c, args=(d_lines, n, d_hits, npx * 48, d8, npx * 4, d32, npx * 12 - 1)) == -7
    # the host path reads the lines: an instance past the count, and an instance without a scene
    host8 = np.full((h, w, 4), 0x5A, np.uint8)
    wrong = lines.copy()
    wrong["instance"][-1] = 3
    hargs = lambda ln, b8=npx * 4: (ln.ctypes.data, len(ln), None, 0, host8.ctypes.data, b8, None, 0)
    assert call(r._c, args=hargs(wrong), flags=_lib.LINES_HOST) == -1 and b"instance 3 of 3" in L.rz_last_error(r._c)
    assert call(r._c, args=hargs(lines, npx * 4 - 1), flags=_lib.LINES_HOST) == -7
    empty = Renderer(0)
    assert call(empty._c, args=hargs(lines), flags=_lib.LINES_HOST) == -5 and b"no scene" in L.rz_last_error(empty._c)
    assert (host8 == 0x5A).all()
    assert call(empty._c, args=hargs(lines[:8]), flags=_lib.LINES_HOST) == 0 and (host8 != 0x5A).any()       # world-space lines need none
    empty.close()
    # nothing was launched
    r.sync()
    assert (hip.download(d8, npx * 4 + 16) == 0x5A).all() and (hip.download(d32, npx * 12 + 16) == 0x5A).all()
    # n = 0 is RZ_OK and writes nothing, with or without a lines pointer
    assert call(r._c, args=(None, 0, d_hits, npx * 48, d8, npx * 4, d32, npx * 12)) == 0
    assert call(r._c, args=(d_lines, 0, None, 0, d8, npx * 4, None, 0)) == 0
    r.sync()
    assert (hip.download(d8, npx * 4 + 16) == 0x5A).all() and (hip.download(d32, npx * 12 + 16) == 0x5A).all()
    # the context stays usable; nothing is written past the buffers; on the device path an instance past the count is dropped
    hip.ok(hip.L.hipMemcpy(d_lines, wrong.ctypes.data, wrong.nbytes, 1))
    assert call(r._c) == 0
    r.sync()
    got8 = hip.download(d8, npx * 4 + 16)
    assert (got8[npx * 4:] == 0x5A).all() and (hip.download(d32, npx * 12 + 16)[npx * 12:] == 0x5A).all()
    hits0 = np.zeros((h, w), HIT_DTYPE)                     # (instance 0 everywhere, point at the origin: w_h = the camera's distance)
    want8, _, _ = LR.draw(wrong, cam.view, cam.proj, w, h, hits=hits0, rgba8=np.full((h, w, 4), 0x5A, np.uint8),
                          transforms=r.read_binding(S.BIND_INSTANCES)["transform"])
    assert got8[:npx * 4].tobytes() == want8.tobytes() and (want8 != 0x5A).any()
    r.close()
    hip.close()


def test_a_failed_workspace_allocation_returns_the_error_and_writes_nothing(monkeypatch):
    """rz_debug_fail_alloc fails the n-th allocation site of the call: the records, the cells, the lists taken whole, and -- with
    RZ_LINES_DIRECT_BYTES=0 -- the lists sized from the counts, which is reached after the projection and the counting pass."""
    hip = Hip()
    w, h = 65, 37
    cam = _camera(w, h)
    fp = _frame(cam, w, h)
    lines = _random_lines(500, 9)
    rgb, rgba8 = _images(w, h)
    want8, want32, _ = LR.draw(lines, cam.view, cam.proj, w, h, rgba8=rgba8, rgb32f=rgb)
    d_lines = hip.upload(lines)
    for direct in (None, "0"):
        if direct is None:
            monkeypatch.delenv("RZ_LINES_DIRECT_BYTES", raising=False)
        else:
            monkeypatch.setenv("RZ_LINES_DIRECT_BYTES", direct)
        r = Renderer(0)
        d8, d32 = hip.upload(rgba8), hip.upload(rgb)
        for nth in (1, 2, 3):
            r.debug_fail_alloc(nth)
            with pytest.raises(RayZenError) as e:
                r.draw_lines_device(d_lines, len(lines), d8, d32, frame=fp)
            assert e.value.code == -8, (direct, nth, str(e.value))
            r.sync()
            assert hip.download(d8, rgba8.nbytes).tobytes() == rgba8.tobytes() and hip.download(d32, rgb.nbytes).tobytes() == rgb.tobytes()
        r.debug_fail_alloc(0)
        r.draw_lines_device(d_lines, len(lines), d8, d32, frame=fp)
        r.sync()
        _same(hip.download(d8, rgba8.nbytes).reshape(h, w, 4), hip.download(d32, rgb.nbytes).view(F32).reshape(h, w, 3), want8, want32,
              f"after the failures, direct {direct}")
        r.close()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the C++ front end

def test_cpp_free_functions_equal_the_python_binding(tmp_path):
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    exe = str(tmp_path / "overlay_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rayzen_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "overlay_driver.cpp"), "-L", lib, "-lrayzen_host", "-lrayzen_hip",
                           f"-Wl,-rpath,{lib}", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"overlay_driver returned {p.returncode}: {p.stderr[-2000:]}"

    def raw(name):
        return (out / f"{name}.bin").read_bytes()

    fp = _lib.FrameParams.from_buffer_copy(raw("frame"))
    w, h = fp.width, fp.height
    r = Renderer(0)
    for b, dt in S.BINDING_DTYPES.items():
        r.upload(b, np.frombuffer(raw(f"b{b}"), dt))
    assert raw("grid") == LN.grid(6.0, 1.5, (160, 160, 160, 200), y=-1.5).tobytes()
    assert raw("box") == LN.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (255, 160, 0, 255), instance=1).tobytes()
    lines = np.frombuffer(raw("lines"), _lib.LINE_DTYPE)
    assert len(lines) == 18 + 12 + 12
    in8 = np.frombuffer(raw("in8"), np.uint8).reshape(h, w, 4)
    in32 = np.frombuffer(raw("in32"), F32).reshape(h, w, 3)
    hits = np.frombuffer(raw("hits"), HIT_DTYPE).reshape(h, w)
    lp = _lib.LinesParams.from_buffer_copy(raw("params"))
    plain8, _ = r.draw_lines(lines, rgba8=in8, frame=fp)
    out8, out32 = r.draw_lines(lines, rgba8=in8, rgb32f=in32, hits=hits, frame=fp, width=lp.width, near_w=lp.near_w,
                               depth_bias=lp.depth_bias, hidden_alpha=lp.hidden_alpha, smooth=lp.smooth)
    r.close()
    assert plain8.tobytes() == raw("plain8") and raw("plain8") != raw("in8")
    assert out8.tobytes() == raw("out8") and out32.tobytes() == raw("out32") and raw("out8") != raw("plain8")


# ---------------------------------------------------------------------------------------------------------------------
# 7. what the call costs

def _alternate(hip, stream, calls, rounds):
    """GPU time (ms, a HIP event pair on the context's stream) of each call of `calls`, alternating them `rounds` times; the
    first round warms them up and is dropped."""
    a, b = hip.event(), hip.event()
    times = [[] for _ in calls]
    for k in range(rounds + 1):
        for i, call in enumerate(calls):
            hip.ok(hip.L.hipEventRecord(a, stream))
            call()
            hip.ok(hip.L.hipEventRecord(b, stream))
            hip.ok(hip.L.hipEventSynchronize(b))
            ms = C.c_float()
            hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
            if k:
                times[i].append(float(ms.value))
    for e in (a, b):
        hip.L.hipEventDestroy(e)
    return times


def editor_set(sc):
    """About 300 lines: a ground grid, the box of the big mesh in its own space, and axes."""
    root = sc.arrays[S.BIND_BLAS_NODES][sc.arrays[S.BIND_INSTANCES]["blasNodeOffset"][1]]
    return np.concatenate([LN.grid(14.0, 0.2, (180, 180, 180, 160), y=-3.0),
                           LN.box(root["boundsMin"], root["boundsMax"], (255, 160, 0, 255), instance=1), LN.axes((0.0, 0.0, 0.0), 2.0)])


# A handful of lines must not cost more than the cast that makes the depth image they are tested against, so the factor is at
# most 1.  It is set from the first measurement runs (profiles/lines/README.md): rz_draw_lines 0.0360, 0.0356 and 0.0354 ms
# against 0.1623, 0.1621 and 0.1605 ms for the guide cast, ratios 0.222, 0.220 and 0.221.  The call is five small launches and
# most of its 35 microseconds is their latency, which moves with the machine and the driver more than a kernel's run time does
# (single samples of 0.044 among the twelve; rz_outline's 16 microseconds had samples of 0.026 and 0.050): the margin is a
# little over twice the measured ratio, half of what the issue allows.  Medians are compared.
LINES_MARGIN = 0.5


def test_300_lines_cost_no_more_than_the_guide_cast():
    """bunny_scene() (69 312 triangles and a floor) at 1920 x 1080: the GPU time of rz_draw_lines (device form, rgba8 in place,
    the guides as hits, 297 lines) against rz_denoise with iterations = 0 and guides, which makes those hits.  The two calls
    alternate for 12 rounds after a warm-up round; medians are compared."""
    hip = Hip()
    L = _lib.hip()
    sc = S.bunny_scene()
    w, h = 1920, 1080
    r = Renderer(0)
    r.upload_scene(sc)
    fp = frame_params(sc.camera, w, h, len(sc.lights), 1, 1)
    r.set_frame(fp)
    lines = editor_set(sc)
    assert 250 <= len(lines) <= 350
    d_lines, d8, d_guides = hip.upload(lines), hip.alloc(w * h * 4, 0x40), hip.alloc(w * h * 48)
    r.denoise_device(guides_ptr=d_guides, iterations=0)
    stream = L.rz_stream_handle(r._c)
    line_ms, guide_ms = _alternate(hip, stream, [lambda: r.draw_lines_device(d_lines, len(lines), d8, None, d_guides, frame=fp),
                                                 lambda: r.denoise_device(guides_ptr=d_guides, iterations=0)], 12)
    r.sync()
    changed = int((hip.download(d8, w * h * 4) != 0x40).reshape(-1, 4).any(axis=1).sum())
    r.close()
    hip.close()
    a, g = float(np.median(line_ms)), float(np.median(guide_ms))
    print(f"1920x1080 bunny 69 312, {len(lines)} lines: rz_draw_lines {a:.4f} ms [{min(line_ms):.4f}, {max(line_ms):.4f}], rz_denoise guides "
          f"{g:.4f} ms [{min(guide_ms):.4f}, {max(guide_ms):.4f}]; ratio {a / g:.3f}; margin {LINES_MARGIN}; {changed} pixels drawn")
    assert changed > 10000
    assert a <= LINES_MARGIN * g, (line_ms, guide_ms)

"""Editor preview (rz_render_editor): the C-ABI struct, the shading restatement on hand-computed cases, the host-side pixel rays
and the kernels' register budget -- everything that can be checked without a GPU."""
import ctypes as C

import numpy as np

import editor_ref as ER
from rayzen_amd import _lib
from rayzen_amd import renderer as R
from rayzen_amd import scene as S
from test_rays_abi import _kernel_metadata


def test_editor_params_size_and_offsets():
    L = _lib.hip()
    assert L.rz_sizeof(10) == 32 and C.sizeof(_lib.EditorParams) == 32
    want = {"ambient": 0, "pad0": 12, "clear": 16}
    assert [f for f, _ in _lib.EditorParams._fields_] == list(want)
    for f, off in want.items():
        assert getattr(_lib.EditorParams, f).offset == off, f
    assert (_lib.EDITOR_HOST, _lib.EDITOR_INCOHERENT) == (1, 2)
    assert L.rz_abi_version() == _lib.ABI_VERSION == 5       # additive: the revision stays


def _mats(*rows):
    m = np.zeros(len(rows), S.MATERIAL)
    for i, (alb, met, rough, transp) in enumerate(rows):
        m[i] = (alb, met, rough, 0.0, transp, 1.5)
    return m


def _lights(*rows):
    out = np.zeros(len(rows), S.LIGHT)
    for i, (pd, col, power) in enumerate(rows):
        out[i] = (pd, col, power)
    return out


def _one(p, n, mi, mats, lights, cam, num=None):
    return ER.shade(np.array([p], float), np.array([n], float), [mi], mats, lights, cam, len(lights) if num is None else num)[0]


def test_shade_ambient_only_and_light_behind():
    mats = _mats(((0.5, 0.25, 1.0), 0.0, 0.5, 0.0))
    # a directional light from below: NdotL = 0, skipped; ambient 0.03 * albedo remains
    lights = _lights(((0.0, -1.0, 0.0, 0.0), (1.0, 1.0, 1.0), 5.0))
    c = _one((0, 0, 0), (0, 1, 0), 0, mats, lights, (0, 1, 0))
    assert np.allclose(c, [0.015, 0.0075, 0.03], rtol=1e-6, atol=0)
    # zero lights and num_lights = 0 give the same
    assert np.allclose(_one((0, 0, 0), (0, 1, 0), 0, mats, _lights(), (0, 1, 0)), c, atol=1e-15)
    assert np.allclose(_one((0, 0, 0), (0, 1, 0), 0, mats, lights, (0, 1, 0), num=0), c, atol=1e-15)


def test_shade_directional_head_on_by_hand():
    """N = V = L = H = +y, roughness 1, dielectric: every term by hand."""
    alb = np.array([0.5, 0.5, 0.5])
    mats = _mats((tuple(alb), 0.0, 1.0, 0.0))
    lights = _lights(((0.0, 2.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2.0))          # not unit: normalised
    c = _one((0, 0, 0), (0, 3, 0), 0, mats, lights, (0, 5, 0))             # normal not unit: normalised
    a2 = 1.0
    D = a2 / max(3.14159 * 1.0, 1e-4)                                       # denom = 1
    k = (2.0 * 2.0) / 8.0
    g = 1.0 / (1.0 * (1 - k) + k + 1e-6)
    F = 0.04                                                                 # VdotH = 1: F = F0
    spec = D * g * g * F / 4.0
    diffuse = (1 - F) * 0.5 / 3.14159
    want = 0.03 * alb + (diffuse + spec) * 2.0 * 1.0
    assert np.allclose(c, want, rtol=1e-6, atol=0)


def test_shade_point_light_falloff_and_min_distance():
    mats = _mats(((1.0, 1.0, 1.0), 0.0, 1.0, 0.0))
    near = _one((0, 0, 0), (0, 1, 0), 0, mats, _lights(((0, 2, 0, 1), (1, 1, 1), 8.0)), (0, 2, 0))
    far = _one((0, 0, 0), (0, 1, 0), 0, mats, _lights(((0, 4, 0, 1), (1, 1, 1), 8.0)), (0, 4, 0))
    amb = float(np.float32(0.03))
    assert np.allclose((near - amb) / (far - amb), 4.0, rtol=1e-12)         # power / d^2
    # a light AT the surface point: distance clamped to 0.001, L = 0 / 0.001 = 0, NdotL = 0: skipped
    c = _one((0, 0, 0), (0, 1, 0), 0, mats, _lights(((0, 0, 0, 1), (1, 1, 1), 8.0)), (0, 2, 0))
    assert np.allclose(c, amb, rtol=1e-6, atol=0)
    # w other than exactly 1 is directional
    d = _one((0, 0, 0), (0, 1, 0), 0, mats, _lights(((0, 2, 0, 0.5), (1, 1, 1), 8.0)), (0, 2, 0))
    assert np.allclose(d - amb, (near - amb) * 4.0, rtol=1e-12)


def test_shade_back_face_is_diffuse_only():
    """No flip toward the viewer: a surface seen from behind gets NdotV = 0, so G = 0 and no specular."""
    mats = _mats(((0.2, 0.4, 0.6), 0.0, 0.3, 0.0))
    lights = _lights(((0.0, 1.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1.0))
    F0 = 0.04
    # camera below the surface, off to the side; the light above
    c = _one((0, 0, 0), (0, 1, 0), 0, mats, lights, (3, -1, 0))
    V = np.array([3.0, -1.0, 0.0]) / np.sqrt(10.0)
    H = (V + [0, 1, 0]) / np.linalg.norm(V + [0, 1, 0])
    Fv = F0 + (1 - F0) * (1 - max(V @ H, 0)) ** 5
    alb = mats["albedo"][0].astype(np.float64)
    want = 0.03 * alb + (1 - Fv) * alb / 3.14159
    assert np.allclose(c, want, rtol=1e-6, atol=0)


def test_shade_metallic_roughness_clamp_transparency_and_index_clamp():
    lights = _lights(((0.3, 1.0, 0.2, 0.0), (1.0, 0.9, 0.8), 3.0))
    base = ((0.9, 0.5, 0.1), 0.0, 0.4, 0.0)
    metal = ((0.9, 0.5, 0.1), 1.0, 0.4, 0.0)
    smooth = ((0.9, 0.5, 0.1), 1.0, 0.001, 0.0)
    clamped = ((0.9, 0.5, 0.1), 1.0, 0.05, 0.0)
    glass = ((0.9, 0.5, 0.1), 0.0, 0.4, 0.8)
    over = ((0.9, 0.5, 0.1), 0.0, 0.4, 3.0)
    mats = _mats(base, metal, smooth, clamped, glass, over)
    p, n, cam = (0, 0, 0), (0.1, 1.0, 0.0), (0.4, 2.0, 0.6)
    c = [_one(p, n, i, mats, lights, cam) for i in range(len(mats))]
    # metallic 1: no diffuse, F0 = albedo -- the colour changes
    assert not np.allclose(c[0], c[1])
    # roughness below 0.05 is clamped to 0.05
    assert np.array_equal(c[2], c[3])
    # transparency: mix(color, albedo, clamp(t, 0, 1) * 0.5)
    alb = mats["albedo"][0].astype(np.float64)
    assert np.allclose(c[4], c[0] * 0.6 + alb * 0.4, rtol=1e-7)
    assert np.allclose(c[5], c[0] * 0.5 + alb * 0.5, rtol=1e-14)
    # the material index is clamped to [0, n - 1]
    assert np.array_equal(_one(p, n, -4, mats, lights, cam), c[0])
    assert np.array_equal(_one(p, n, 99, mats, lights, cam), c[5])


def test_shade_num_lights_clamped_to_buffer():
    mats = _mats(((0.5, 0.5, 0.5), 0.0, 0.5, 0.0))
    lights = _lights(((0, 1, 0, 0), (1, 1, 1), 1.0), ((1, 1, 0, 0), (1, 0, 0), 2.0))
    p, n, cam = (0, 0, 0), (0, 1, 0), (0, 3, 1)
    one = _one(p, n, 0, mats, lights, cam, num=1)
    two = _one(p, n, 0, mats, lights, cam, num=2)
    assert not np.allclose(one, two)
    assert np.array_equal(_one(p, n, 0, mats, lights, cam, num=7), two)
    assert np.array_equal(_one(p, n, 0, mats, lights, cam, num=-1), _one(p, n, 0, mats, lights, cam, num=0))


def test_quantise_matches_present():
    q = ER.quantise(np.array([[-1.0, 0.5, 2.0], [0.00196, 0.998, 1.0]], np.float32))
    assert q.tolist() == [[0, 128, 255, 255], [0, 254, 255, 255]]


def test_editor_rays_match_float64_unprojection():
    for sc, W, H in ((S.reference_scene(), 80, 60), (S.bunny_scene(n=6, aspect=16 / 9), 64, 36),
                     (S.instanced_scene(n=6, count=4), 37, 23)):
        cam = sc.camera
        rays = R.editor_rays(cam, W, H)
        assert rays.dtype == R.RAY_DTYPE and rays.shape == (W * H,)
        assert (rays["origin"] == np.asarray(cam.position, np.float32)).all()
        assert (rays["max_dist"] == np.float32(1e30)).all()
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ndc = np.stack([(px.ravel() + 0.5) / W * 2 - 1, (py.ravel() + 0.5) / H * 2 - 1, -np.ones(W * H), np.ones(W * H)], 1)
        ip = np.asarray(cam.inv_proj, np.float64).reshape(4, 4).T
        iv = np.asarray(cam.inv_view, np.float64).reshape(4, 4).T
        e = ndc @ ip.T
        e = np.stack([e[:, 0], e[:, 1], -np.ones(len(e)), np.zeros(len(e))], 1)
        d = (e @ iv.T)[:, :3]
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        assert np.abs(rays["dir"].astype(np.float64) - d).max() <= 1e-6
        # unit directions, row 0 = the bottom row: the first ray looks down-left, the last up-right
        assert np.allclose(np.linalg.norm(rays["dir"].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_editor_rays_bit_for_bit_against_scalar_restatement():
    """rz_path.h: camera_ray_centre written out for a few pixels, scalar by scalar in float32."""
    f = np.float32
    cam = S.reference_scene().camera
    W, H = 801, 599
    rays = R.editor_rays(cam, W, H)
    ip, iv = np.asarray(cam.inv_proj, f), np.asarray(cam.inv_view, f)
    for px, py in ((0, 0), (400, 299), (800, 598), (17, 512), (799, 3)):
        ux, uy = f(f(px) + f(0.5)) / f(W), f(f(py) + f(0.5)) / f(H)
        cx, cy = f(ux * f(2)) - f(1), f(uy * f(2)) - f(1)
        ex = f(f(f(ip[0] * cx) + f(ip[4] * cy)) + f(ip[8] * f(-1))) + f(ip[12])
        ey = f(f(f(ip[1] * cx) + f(ip[5] * cy)) + f(ip[9] * f(-1))) + f(ip[13])
        w = [f(f(f(iv[r] * ex) + f(iv[4 + r] * ey)) + f(iv[8 + r] * f(-1))) for r in range(3)]
        s = np.sqrt(f(f(f(w[0] * w[0]) + f(w[1] * w[1])) + f(w[2] * w[2])))
        want = np.array([w[0] / s, w[1] / s, w[2] / s], f)
        assert rays["dir"][py * W + px].view(np.uint32).tolist() == want.view(np.uint32).tolist(), (px, py)


def test_editor_kernels_spill_nothing():
    meta = _kernel_metadata(_lib.HIP_SO)
    ed = {k: v for k, v in meta.items() if "rz_editor_kernel" in k}
    assert len(ed) == 4, sorted(ed)
    for name, (spill, priv) in ed.items():
        assert spill == 0 and priv == 0, f"{name}: {spill} VGPRs spilled, {priv} B of scratch"

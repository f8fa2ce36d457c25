"""A numpy restatement of RayZen's editor_fragment.glsl (the editor preview's shading, main.cpp:1266-1275 for its uniforms),
vectorised over surface points.  Float64 by default: the reference the kernel's float32 colours are held to.  With
dtype=np.float32 every operation is rounded to float32 in the kernel's order (rz_editor.hip: editor_shade), which shows how
far float32 arithmetic alone moves a colour."""
import numpy as np

AMBIENT = (0.03, 0.03, 0.03)            # uAmbientColor (main.cpp:1269)
CLEAR = (0.05, 0.05, 0.07, 1.0)         # glClearColor (main.cpp:260)


def _lit(x, f):
    """A GLSL float literal (binary32) in the evaluation type."""
    return f(np.float32(x))


def _normalize(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def shade(points, normals, mat_index, materials, lights, cam_pos, num_lights, ambient=AMBIENT, dtype=np.float64):
    """Colour (n, 3) of editor_fragment.glsl for n surface points (world position, world normal, material index)."""
    with np.errstate(invalid="ignore", divide="ignore"):        # (a light the shader skips may make 0 / 0 in the masked lanes)
        return _shade(points, normals, mat_index, materials, lights, cam_pos, num_lights, ambient, dtype)


def _shade(points, normals, mat_index, materials, lights, cam_pos, num_lights, ambient, dtype):
    f = dtype
    p = np.asarray(points, np.float64).reshape(-1, 3).astype(f)
    n = np.asarray(normals, np.float64).reshape(-1, 3).astype(f)
    mats = np.asarray(materials)
    lights = np.asarray(lights)
    mi = np.clip(np.asarray(mat_index, np.int64).reshape(-1), 0, len(mats) - 1)       # clamp(materialIndex, 0, length - 1)
    albedo = np.asarray(mats["albedo"], np.float64)[mi].astype(f)
    metallic = np.asarray(mats["metallic"], np.float64)[mi].astype(f)[:, None]
    roughness = np.asarray(mats["roughness"], np.float64)[mi].astype(f)
    transparency = np.asarray(mats["transparency"], np.float64)[mi].astype(f)

    N = _normalize(n)
    V = _normalize(np.asarray(cam_pos, np.float64).astype(f)[None, :] - p)
    NdotV = np.maximum(np.sum(N * V, -1), f(0.0))
    F0 = _lit(0.04, f) * (f(1.0) - metallic) + albedo * metallic                            # mix(vec3(0.04), albedo, metallic)
    color = np.asarray(ambient, np.float32).astype(f)[None, :] * albedo            # (a float uniform)
    rough = np.clip(roughness, _lit(0.05, f), f(1.0))
    a = rough * rough
    a2 = a * a
    r = rough + f(1.0)
    k = (r * r) / f(8.0)

    def g1(x):
        return x / (x * (f(1.0) - k) + k + _lit(1e-6, f))

    for i in range(min(int(num_lights), len(lights))):
        L_ = lights[i]
        pd = np.asarray(L_["positionOrDirection"], np.float64).astype(f)
        if pd[3] == 1.0:                                                                 # point light
            lv = pd[None, :3] - p
            dist = np.maximum(np.sqrt(np.sum(lv * lv, -1)), _lit(0.001, f))
            L = lv / dist[:, None]
            att = f(L_["power"]) / (dist * dist)
        else:                                                                            # directional
            L = np.broadcast_to(_normalize(pd[:3]), p.shape)
            att = np.full(len(p), f(L_["power"]), f)
        NdotL = np.maximum(np.sum(N * L, -1), f(0.0))
        lit = NdotL > 0.0                                                                # NdotL <= 0: continue
        H = _normalize(V + L)
        NdotH = np.maximum(np.sum(N * H, -1), f(0.0))
        VdotH = np.maximum(np.sum(V * H, -1), f(0.0))
        denom = (NdotH * NdotH) * (a2 - f(1.0)) + f(1.0)
        D = a2 / np.maximum(_lit(3.14159, f) * denom * denom, _lit(1e-4, f))
        G = g1(NdotV) * g1(NdotL)
        F = F0 + (f(1.0) - F0) * ((f(1.0) - VdotH) ** 5)[:, None]
        spec = F * (D * G)[:, None] / np.maximum(f(4.0) * NdotV * NdotL, _lit(1e-4, f))[:, None]
        kD = (f(1.0) - F) * (f(1.0) - metallic)
        diffuse = kD * albedo / _lit(3.14159, f)
        add = (diffuse + spec) * np.asarray(L_["color"], np.float64).astype(f)[None, :] * att[:, None] * NdotL[:, None]
        color = color + np.where(lit[:, None], add, f(0.0))
    t = (np.clip(transparency, f(0.0), f(1.0)) * f(0.5))[:, None]
    mixed = color * (f(1.0) - t) + albedo * t                                           # mix(color, albedo, t)
    return np.where((transparency > 0.0)[:, None], mixed, color).astype(f)


def quantise(rgb):
    """rz_present's RGBA8 quantisation: rint(clamp(c, 0, 1) * 255), alpha 255."""
    c = np.asarray(rgb, np.float32)
    q = np.rint(np.clip(c, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], -1)

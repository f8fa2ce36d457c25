"""The editor preview's reading of RayZen's raster pass, held to RayZen's own shaders (tests/golden/glref_editor_*.npz, made by
oracle/glref's editor mode; the comparison is tests/editor_glref.py).  CPU suite: the oracle's closest hits, clipped as
rz_render_editor clips them and shaded by editor_ref.py, against the fixtures; live (where the reference and Mesa are): the
fixtures are what llvmpipe renders now, and editor_ref.py at llvmpipe's own interpolated inputs is llvmpipe's colour; and the
comparison fails for each of six small misreadings of the shader or of the clipping."""
import numpy as np
import pytest

import editor_glref as EG
import editor_ref as ER
from helpers import oracle_scene
from oracle import rzo
from rayzen_amd import scene as S
from rayzen_amd.renderer import editor_rays

F32 = np.float32


def _local_triangles(sc, inst, point, d):
    """The mesh-local triangle of each oracle hit (rzo.trace does not return it): of the triangles of the instance's mesh that
    the ray, taken to object space in float64, meets (barycentric tolerance 1e-6), the one that it meets nearest the oracle's
    hit point -- not the first one along the ray: the shader's hit test skips a triangle it meets at a grazing angle."""
    tri = np.full(len(inst), -1, np.int64)
    I, T = sc.arrays[S.BIND_INSTANCES], sc.arrays[S.BIND_TRIANGLES]
    offs = sorted(set(int(g) for g in I["globalTriOffset"])) + [len(T)]
    cam = np.asarray(sc.camera.position, np.float64)
    for i in np.unique(inst[inst >= 0]):
        sel = np.flatnonzero(inst == i)
        g = int(I["globalTriOffset"][i])
        t = T[g:offs[offs.index(g) + 1]]
        inv = EG._mat(I["inverseTransform"][i])
        lo = inv[:3, :3] @ cam + inv[:3, 3]
        ld = d[sel].astype(np.float64) @ inv[:3, :3].T
        lp = point[sel].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
        v0, v1, v2 = (np.asarray(t[k], np.float64) for k in ("v0", "v1", "v2"))
        e1, e2 = v1 - v0, v2 - v0
        for c in range(0, len(sel), 512):
            D = ld[c:c + 512, None, :]
            P = np.cross(D, e2[None])
            det = (e1[None] * P).sum(-1)
            s = lo - v0
            with np.errstate(divide="ignore", invalid="ignore"):
                u = (s[None] * P).sum(-1) / det
                Q = np.cross(s, e1)
                v = (D * Q[None]).sum(-1) / det
                tt = (e2 * Q).sum(-1)[None] / det
                ok = (u >= -1e-6) & (v >= -1e-6) & (u + v <= 1 + 1e-6) & (tt > 0)
                miss = np.linalg.norm(lo + D * tt[..., None] - lp[c:c + 512, None, :], axis=-1)
            miss = np.where(ok, miss, np.inf)
            best = miss.argmin(1)
            assert (miss.min(1) <= 1e-4 * (1 + np.abs(lp[c:c + 512]).max(1))).all(), "an oracle hit on no triangle of its instance"
            tri[sel[c:c + 512]] = best
    return tri


_HITS = {}


def oracle_hits(sc, W, H):
    """rzo.trace's closest hit for every pixel ray: (rays, point, normal, material, instance), kept per scene and frame size
    (the power checks shade the same hits again)."""
    key = (sc.arrays[S.BIND_TRIANGLES].tobytes(), sc.camera.view.tobytes(), sc.camera.proj.tobytes(), W, H)
    if key not in _HITS:
        rays = editor_rays(sc.camera, W, H)
        osc = oracle_scene(sc)
        n = W * H
        point, normal = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        inst, mat = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        for j in range(n):
            h = rzo.trace(osc, rays["origin"][j], rays["dir"][j])
            if h["hit"]:
                point[j], normal[j], mat[j], inst[j] = h["point"], h["normal"], h["material"], h["instance"]
        _HITS[key] = (rays, point, normal, mat, inst)
    return _HITS[key]


def oracle_candidate(sc, render, num_lights=None, materials=None, ambient=ER.AMBIENT, keep_near=False, forward_normals=False,
                     transparency_mix=0.5):
    """The oracle's editor frame: rzo.trace on editor_rays (the rays rz_render_editor casts; test_rays_gpu.py holds rz_trace_rays
    equal to rzo.trace), rz_editor.hip's clip rule in binary32, editor_ref.shade in float64.  Pixels whose first hit lies in
    front of the near plane are skipped (the kernel restarts the query there; the GPU suite covers them).  The keyword arguments
    are the power checks' misreadings.  -> (candidate dict, skip mask: the front pixels the candidate does not decide)"""
    W, H = render["W"], render["H"]
    nl = render["num_lights"] if num_lights is None else num_lights
    rays, point, normal, mat, inst = (a.copy() for a in oracle_hits(sc, W, H))
    n = W * H
    z, w = EG.clip_zw(sc.camera, point)
    hit = inst >= 0
    visible = hit & (-w <= z) & (z <= w)
    front = hit & (z < -w)
    if keep_near:
        visible |= front
    inst[~visible] = -1
    tri = _local_triangles(sc, inst, point, rays["dir"])
    if forward_normals:                 # mat3(model) * n instead of the normal matrix
        T, I = sc.arrays[S.BIND_TRIANGLES], sc.arrays[S.BIND_INSTANCES]
        for j in np.flatnonzero(visible):
            t = T[int(I["globalTriOffset"][inst[j]]) + tri[j]]
            ln = np.cross(np.asarray(t["v1"], np.float64) - t["v0"], np.asarray(t["v2"], np.float64) - t["v0"])
            wn = EG._mat(I["transform"][inst[j]])[:3, :3] @ ln
            normal[j] = wn / np.linalg.norm(wn)
    mats = sc.materials if materials is None else materials
    rgb = np.broadcast_to(np.asarray(ER.CLEAR[:3], F32), (n, 3)).copy()
    if visible.any():
        if transparency_mix == 0.5:
            rgb[visible] = ER.shade(point[visible], normal[visible], mat[visible], mats, sc.lights, sc.camera.position, nl, ambient)
        else:                           # mix(color, albedo, clamp(transparency, 0, 1) * transparency_mix)
            opaque = mats.copy()
            opaque["transparency"] = 0.0
            c = ER.shade(point[visible], normal[visible], mat[visible], opaque, sc.lights, sc.camera.position, nl, ambient)
            m = mats[mat[visible]]
            t = (np.clip(m["transparency"].astype(np.float64), 0, 1) * transparency_mix)[:, None]
            rgb[visible] = np.where((m["transparency"] > 0)[:, None], c * (1 - t) + m["albedo"] * t, c)
    shape = (H, W)
    cand = dict(instance=inst.reshape(shape), triangle=tri.reshape(shape), point=point.reshape(H, W, 3),
                normal=normal.reshape(H, W, 3), material=mat.reshape(shape), rgb=rgb.reshape(H, W, 3),
                rgba8=ER.quantise(rgb).reshape(H, W, 4), front=front.reshape(shape))
    return cand, (front & ~visible).reshape(shape)


CASES = EG.cases()
IDS = [f"{n}-{k}" for n, k in CASES]

# upper bounds per class, measured ("Editor mode"): fixture-only candidate (the oracle's hits; the pixels whose
# first hit lies in front of the near plane are skipped)
ORACLE_BOUNDS = {
    ("clip", 0): dict(edge=1, skipped=25584),
    ("cornell", 0): dict(),
    ("coverage", 0): dict(edge=26),
    ("coverage", 1): dict(edge=26),
    ("coverage", 2): dict(edge=26),
    ("rayzen_main", 0): dict(edge=2),
    ("skewed", 0): dict(edge=10),
}


def assert_report(rep, bounds, what):
    msg = f"{what}: {EG.summary(rep)}"
    assert rep["counts"]["unclassified"] == 0, msg
    for c in ("edge", "near", "tie", "skipped"):
        assert rep["counts"][c] <= bounds.get(c, 0), f"{c}: {msg}"
    assert rep["worst"] <= 1.0, msg
    return msg


@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_oracle_editor_frame_matches_rayzens_raster_pass(name, k):
    sc, renders, outs, _ = EG.load(name)
    cand, skip = oracle_candidate(sc, renders[k])
    rep = EG.classify(sc, renders[k], outs[k], cand, skip)
    print(assert_report(rep, ORACLE_BOUNDS[(name, k)], f"oracle vs RayZen's raster pass, {name}[{k}]"))


def test_the_editor_fixtures_cover_the_listed_scenes():
    assert {"cornell", "rayzen_main", "coverage", "skewed", "clip"} <= set(EG.NAMES)
    sc, renders, outs, gl = EG.load("coverage")
    assert [r["num_lights"] for r in renders] == [0, 4, 9] and len(sc.lights) == 4
    assert "llvmpipe" in gl
    for name in EG.NAMES:
        sc, renders, outs, _ = EG.load(name)
        for r, o in zip(renders, outs):
            assert r["W"] * r["H"] <= 256 * 192
            bg = o["object"] < 0
            assert (o["depth"][bg] == 0xFFFFFF).all() and (o["depth"][~bg] < 0xFFFFFF).all() and (~bg).mean() > 0.3
    # the skewed instances are rotated AND scaled non-uniformly: the forward transform is not a normal matrix there
    inst = EG.load("skewed")[0].arrays[S.BIND_INSTANCES]
    m3 = [EG._mat(t)[:3, :3] for t in inst["transform"]]
    assert any(np.ptp(np.linalg.svd(m, compute_uv=False)) > 0.5 and abs(m[0, 1]) > 0.1 for m in m3)
    # the clip frame: surfaces cross the near plane and the far plane inside the view
    sc, renders, outs, _ = EG.load("clip")
    cand, skip = oracle_candidate(sc, renders[0])
    assert skip.sum() > 1000 and (outs[0]["object"][skip] >= 0).any()
    _, point, _, _, inst = oracle_hits(sc, renders[0]["W"], renders[0]["H"])
    z, w = EG.clip_zw(sc.camera, point)
    far = (inst >= 0) & (z > w)                         # hits beyond the far plane: background in RayZen's frame
    assert far.sum() > 100 and (outs[0]["object"].reshape(-1)[far] < 0).all()


# ---- power: each misreading of the shader or of the clipping fails the comparison ----

def _clamp_055(sc):
    m = sc.materials.copy()
    m["roughness"] = np.maximum(m["roughness"], F32(0.055))            # clamp(roughness, 0.055, 1)
    return dict(materials=m)


POWER = {
    "ambient 0.0305": ("cornell", 0, lambda sc, r: dict(ambient=(0.0305,) * 3)),
    "roughness clamp 0.055": ("coverage", 1, lambda sc, r: _clamp_055(sc)),
    "forward transform for normals": ("skewed", 0, lambda sc, r: dict(forward_normals=True)),
    "transparency mix 0.45": ("coverage", 1, lambda sc, r: dict(transparency_mix=0.45)),
    "numLights - 1": ("coverage", 1, lambda sc, r: dict(num_lights=r["num_lights"] - 1)),
    "numLights + 1": ("coverage", 0, lambda sc, r: dict(num_lights=r["num_lights"] + 1)),
    "near-plane surfaces kept": ("clip", 0, lambda sc, r: dict(keep_near=True)),
}


@pytest.mark.parametrize("what", sorted(POWER))
def test_the_comparison_fails_for_a_misreading(what):
    name, k, kw = POWER[what]
    sc, renders, outs, _ = EG.load(name)
    cand, skip = oracle_candidate(sc, renders[k], **kw(sc, renders[k]))
    rep = EG.classify(sc, renders[k], outs[k], cand, skip)
    print(what, EG.summary(rep))
    assert rep["counts"]["unclassified"] >= 20, (what, EG.summary(rep))


# ---- live: only where the reference and Mesa's software driver are ----

def _glref():
    from oracle.glref import glref
    ok, why = glref.usable()
    if not ok:
        pytest.skip(f"RayZen's shaders cannot be run here (the GPU box has neither the reference nor its Mesa): {why}")
    return glref


@pytest.mark.parametrize("name", EG.NAMES)
def test_the_editor_fixtures_are_what_llvmpipe_renders_here(name):
    glref = _glref()
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_glref
    _, _, _, gl = EG.load(name)
    if glref.usable()[1] != gl:
        pytest.skip(f"another llvmpipe than the fixtures' ({glref.usable()[1]} vs {gl})")
    z = np.load(os.path.join(EG.GOLDEN, f"glref_editor_{name}.npz"))
    now = make_glref.editor_fixture(name)
    assert sorted(now) == sorted(z.files)
    for key in z.files:
        a, b = np.asarray(now[key]), z[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_the_restatement_at_llvmpipes_own_inputs(name, k):
    """editor_ref.shade in float64 at llvmpipe's own interpolated worldPos / normal / flat material (the ID pass) against
    llvmpipe's colour, with the per-pixel bound of the comparison: pins editor_ref.py apart from any geometry."""
    glref = _glref()
    sc, renders, outs, _ = EG.load(name)
    r = renders[k]
    live = glref.render_editor(sc.arrays, sc.camera.view, sc.camera.proj, sc.camera.position, r["W"], r["H"], r["num_lights"])
    assert (live["object"] == outs[k]["object"]).all() or live["gl"] != EG.load(name)[3]
    hit = live["object"] >= 0
    clear = np.asarray(ER.CLEAR[:3], F32)
    assert (live["rgb"][~hit] == clear).all() and (live["rgba8"][~hit] == ER.quantise(clear[None])[0]).all()
    p, n, m = live["world_pos"][hit], live["normal"][hit], live["material"][hit]
    want = ER.shade(p, n, m, sc.materials, sc.lights, sc.camera.position, r["num_lights"])
    sp = EG.sensitivity(sc, p, n, m, r["num_lights"])
    g = live["rgb"][hit].astype(np.float64)
    ratio = (np.abs(want - g) / (EG.A + EG.R * np.abs(g) + EG.K * sp)).max(-1)
    print(f"{name}[{k}]: {hit.sum()} pixels, worst {ratio.max():.3g} x bound")
    assert (ratio <= 1.0).all(), f"{int((ratio > 1).sum())} pixels beyond the bound, worst {ratio.max():.3g}"
    assert (np.abs(ER.quantise(want.astype(F32)).astype(int) - live["rgba8"][hit].astype(int)) <= 1).all()


def test_clip_polygon_tags_its_cuts():
    """editor_glref._clip_poly: an edge that runs along the near (far) plane is tagged 1 (2), every other edge 0 -- the near
    class of the comparison measures the distance to the tag-1 edges only."""
    import types
    near, far = 1.0, 10.0
    proj = np.zeros(16)
    proj[0] = proj[5] = 1.0
    proj[10], proj[11], proj[14] = -(far + near) / (far - near), -1.0, -2.0 * far * near / (far - near)
    cam = types.SimpleNamespace(view=np.eye(4).reshape(16), proj=proj)
    sc = types.SimpleNamespace(camera=cam)
    cases = [
        (np.array([[0.0, 0.0, -0.5], [-1.0, 0.0, -3.0], [1.0, 0.0, -3.0]]), 1, near, 4),  # apex in front of the near plane
        (np.array([[-1.0, 0.0, -0.5], [1.0, 0.0, -0.5], [0.0, 0.0, -3.0]]), 1, near, 3),  # two vertices in front of it
        (np.array([[0.0, 0.0, -20.0], [-1.0, 0.0, -3.0], [1.0, 0.0, -3.0]]), 2, far, 4),  # apex beyond the far plane
    ]
    for verts, want, depth, corners in cases:
        poly = EG._clip_poly(sc, verts)
        assert len(poly) == corners
        for i, (p, tag) in enumerate(poly):
            q = poly[(i + 1) % len(poly)][0]
            on_cut = np.isclose(p[3], depth) and np.isclose(q[3], depth)        # w = -z_eye: both ends on that plane
            assert tag == (want if on_cut else 0), (verts, i, p, q, tag)
        assert sum(tag == want for _, tag in poly) == 1

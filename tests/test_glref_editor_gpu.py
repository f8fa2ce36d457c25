"""rz_render_editor against RayZen's own raster pass (tests/golden/glref_editor_*.npz; the comparison is tests/editor_glref.py):
every pixel of every fixture frame agrees -- the same triangle and a colour within its bound, or background in both -- or lies
in a named deviation class within its measured count: a raster edge, the near-plane cut, a depth tie.  The fixtures only:
nothing here needs the reference or Mesa."""
import numpy as np
import pytest

import editor_glref as EG
from rayzen_amd.renderer import Renderer, editor_rays

pytestmark = pytest.mark.gpu

CASES = EG.cases()
IDS = [f"{n}-{k}" for n, k in CASES]

# upper bounds per class, measured on an MI355X ("Editor mode")
BOUNDS = {
    ("clip", 0): dict(edge=1, near=1, tie=0),
    ("cornell", 0): dict(edge=0, near=0, tie=0),
    ("coverage", 0): dict(edge=26, near=0, tie=0),
    ("coverage", 1): dict(edge=26, near=0, tie=0),
    ("coverage", 2): dict(edge=26, near=0, tie=0),
    ("rayzen_main", 0): dict(edge=2, near=0, tie=0),
    ("skewed", 0): dict(edge=10, near=0, tie=0),
}


def _candidate(rgba8, rgb, hits, front):
    return dict(instance=hits["instance"], triangle=hits["triangle"], point=hits["point"], normal=hits["normal"],
                material=hits["material"], rgb=rgb, rgba8=rgba8, front=front)


def _render(sc, r, **kw):
    """rz_render_editor's frame, and where the first hit along each pixel ray (rz_trace_rays on the same rays: the editor's
    first query, bit for bit) lies in front of the near plane, by the kernel's own clip rule."""
    R = Renderer(0)
    try:
        R.upload_scene(sc)
        out = R.render_editor(sc.camera, r["W"], r["H"], num_lights=r["num_lights"], rgb32f=True, hits=True, **kw)
        rays = editor_rays(sc.camera, r["W"], r["H"])
        first = R.trace_rays(rays["origin"], rays["dir"])
    finally:
        R.close()
    z, w = EG.clip_zw(sc.camera, first["point"])
    front = ((first["instance"] >= 0) & (z < -w)).reshape(r["H"], r["W"])
    return out, front


@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_hip_editor_frame_matches_rayzens_raster_pass(name, k):
    sc, renders, outs, _ = EG.load(name)
    r = renders[k]
    (rgba8, rgb, hits), front = _render(sc, r)
    rep = EG.classify(sc, r, outs[k], _candidate(rgba8, rgb, hits, front))
    msg = f"HIP vs RayZen's raster pass, {name}[{k}]: {EG.summary(rep)}"
    print(msg)
    assert rep["counts"]["unclassified"] == 0 and rep["counts"]["skipped"] == 0, msg
    for c in ("edge", "near", "tie"):
        assert rep["counts"][c] <= BOUNDS[(name, k)][c], f"{c}: {msg}"
    assert rep["worst"] <= 1.0, msg
    # the lane-by-lane walk: the same bytes
    (e2, c2, h2), _ = _render(sc, r, incoherent=True)
    assert e2.tobytes() == rgba8.tobytes() and c2.tobytes() == rgb.tobytes() and h2.tobytes() == hits.tobytes()


@pytest.mark.parametrize("name", ["cornell", "rayzen_main"])
def test_hip_editor_comparison_has_power(name):
    """uAmbientColor 0.0305 instead of 0.03: the comparison fails."""
    sc, renders, outs, _ = EG.load(name)
    r = renders[0]
    (rgba8, rgb, hits), front = _render(sc, r, ambient=(0.0305,) * 3)
    rep = EG.classify(sc, r, outs[0], _candidate(rgba8, rgb, hits, front))
    print(name, EG.summary(rep))
    assert rep["counts"]["unclassified"] >= 100, EG.summary(rep)

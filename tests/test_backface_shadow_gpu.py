"""The opaque kernels do not trace the shadow ray of a light that lies behind the surface (rz_path.h: RZ_BACKFACE_SKIP): the
term of such a light is zeros whether it is lit or occluded -- unless it is NaN or the accumulator is -0, in which case the guard
in advance() has the query traced after all.  Every frame here is compared with the oracle, which traces every query, bit for bit:
terminator pixels through every launch shape, a light exactly tangent to a face, inputs chosen to make the guard refuse, the
counting launches' tallies (they keep tracing everything), and the compacting claims with their cross-claim pools."""
import numpy as np
import pytest

from rayzen_amd import scene as S
from helpers import hip_render, oracle_render, mismatch_report

pytestmark = pytest.mark.gpu

CAMERA = (0.0, 1.5, 7.0)


def floor_transform():
    return S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0))      # the reference's floor (main.cpp:378)


def blob_scene(width, height, materials=None, lights=None, blob=True):
    """make_blob(6, 2.0, 0) at (0, 1, 0) over the reference floor under the reference's two lights, seen from (0, 1.5, 7): the
    point light stands to the right of and above the blob, so a crescent of first hits on its left and lower side faces away
    from one light or from both."""
    s = S.Scene(materials=materials, lights=lights, camera=S.Camera(position=CAMERA, aspect=width / height))
    s.add_object(s.add_mesh(S.make_cube(4)), floor_transform())
    if blob:
        s.add_object(s.add_mesh(S.make_blob(6, 2.0, 0)), S.translate(S.identity(), (0.0, 1.0, 0.0)))
    return s.build()


_refs = {}


def reference(key, scene, width, height, spp, bounces, want_counters=False):
    """The oracle's frame (and tallies) of a case: computed once, shared by the tests that need it, never written to."""
    k = (key, width, height, spp, bounces)
    if k not in _refs:
        img, cnt = oracle_render(scene, width, height, spp, bounces, nthreads=16, want_counters=True)
        img.setflags(write=False)
        _refs[k] = (img, cnt)
    return _refs[k] if want_counters else _refs[k][0]


def assert_same_bits(gpu, ref, what):
    assert (gpu.view(np.uint32) == ref.view(np.uint32)).all(), f"{what}: " + mismatch_report(gpu, ref)


# ---- 1. the terminator --------------------------------------------------------------------------------------------------

def test_terminator_case_is_not_vacuous():
    """On the CPU, with the oracle's closest-hit query through the pixel centres: the frame of the terminator cases has both
    kinds of first hit in numbers (measured: 161 with a light behind, 1 241 with every light in front, of 1 402)."""
    from backface_ref import census
    c = census(blob_scene(64, 48), 64, 48)
    print(f"terminator census: {c}")
    assert c["any_behind"] >= 100, c
    assert c["all_front"] >= 100, c


@pytest.mark.parametrize("backend", ["auto", "pixel"])
@pytest.mark.parametrize("spp", [1, 16, 64, 130])      # the group code | several pixels per wave | one batch through claims | several batches, not a divisor
def test_terminator(spp, backend):
    W, H, B = 64, 48, 4
    sc = blob_scene(W, H)
    gpu = hip_render(sc, W, H, spp, B, backend=backend)
    assert_same_bits(gpu, reference("terminator", sc, W, H, spp, B), f"{spp} spp, backend {backend}")


# ---- 2. a light tangent to a face -----------------------------------------------------------------------------------------

def tangent_scene(width, height):
    """The floor alone.  A directional light along +x: dot(n, l) is exactly 0 on the top face (and negative on the face that
    looks down -x, positive on its opposite).  A point light at the height of the top face: there the dot is a rounding
    error of either sign, from pixel to pixel."""
    cube = S.make_cube(4)
    m = np.asarray(floor_transform(), np.float32).reshape(4, 4).T
    ys = [float((m @ np.append(cube[k][i], np.float32(1.0)))[1]) for k in ("v0", "v1", "v2") for i in range(len(cube))]
    top = max(ys)
    lights = np.zeros(2, S.LIGHT)
    lights[0] = ((1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2.0)
    lights[1] = ((3.0, top, 2.0, 1.0), (1.0, 0.9, 0.8), 40.0)
    return blob_scene(width, height, lights=lights, blob=False)


@pytest.mark.parametrize("spp", [2, 64])
def test_tangent_light(spp):
    W, H, B = 48, 32, 4
    sc = tangent_scene(W, H)
    gpu = hip_render(sc, W, H, spp, B)
    assert_same_bits(gpu, reference("tangent", sc, W, H, spp, B), f"{spp} spp")


# ---- 3. inputs for which the guard must refuse ----------------------------------------------------------------------------

def _materials(**fields):
    m = S.reference_materials()
    for i in (0, 4):        # the blob's material and the floor's
        for k, v in fields.items():
            m[i][k] = v
    return m


def _lights(li, **fields):
    l = S.reference_lights()
    for k, v in fields.items():
        l[li][k] = v
    return l


# Finite inputs that make the term of a light behind the surface NaN, or the accumulator -0: "lit" and "occluded" then differ
# in bits and the query has to be traced.
VARIATIONS = {
    "roughness_0": dict(materials=_materials(roughness=0.0)),                       # D = 0 / 0 where n . h is 1
    "roughness_2.5": dict(materials=_materials(roughness=2.5)),                     # k > 1: G's denominator crosses 0
    "albedo_minus_0": dict(materials=_materials(albedo=(-0.0, 0.5, 0.5))),          # the ambient term is -0, and -0 + 0 is +0
    "negative_light_colour": dict(lights=_lights(0, color=(1.0, -0.5, 1.0))),
    "power_0": dict(lights=_lights(1, power=0.0)),                                  # 0 * inf
}


@pytest.mark.parametrize("spp", [4, 64])
@pytest.mark.parametrize("variation", sorted(VARIATIONS))
def test_guard_must_refuse(variation, spp):
    W, H, B = 64, 48, 4
    sc = blob_scene(W, H, **VARIATIONS[variation])
    gpu = hip_render(sc, W, H, spp, B)
    assert_same_bits(gpu, reference(variation, sc, W, H, spp, B), f"{variation}, {spp} spp")


# ---- 4. the counting launches trace every query -----------------------------------------------------------------------------

@pytest.mark.parametrize("spp", [16, 64])
def test_tallies_are_the_reference_algorithms(spp):
    W, H, B = 64, 48, 4
    sc = blob_scene(W, H)
    img, cnt = hip_render(sc, W, H, spp, B, counted=True)
    ref, rc = reference("terminator", sc, W, H, spp, B, want_counters=True)
    assert_same_bits(img, ref, f"counted, {spp} spp")
    assert set(cnt) == set(rc), (sorted(cnt), sorted(rc))
    for field in sorted(rc):
        assert cnt[field] == rc[field], f"{field}: HIP {cnt[field]}, oracle {rc[field]}"


# ---- 5. through claims and cross-claim pools ----------------------------------------------------------------------------------

def test_through_claims_and_pools(monkeypatch):
    W, H, spp, B = 96, 64, 64, 6
    sc = blob_scene(W, H)
    monkeypatch.setenv("RZ_GROUPS_PER_CLAIM", "4")
    monkeypatch.setenv("RZ_CROSS_CLAIM_POOL", "1")
    monkeypatch.setenv("RZ_WPOOL_CHUNK", "64")
    from rayzen_amd.renderer import Renderer
    r = Renderer(0)
    gpu = hip_render(sc, W, H, spp, B, renderer=r)
    name = r.last_kernel_name()
    r.close()
    assert name == "rz_render_samples+pool", name
    assert_same_bits(gpu, reference("claims", sc, W, H, spp, B), "claims of 4 with cross-claim pools")

"""What the cases of tests/test_tlas_entry_gpu.py are made of: small scenes of cubes, the oracle's frame of each
(computed once, never written to), and a render on a context that stays open between frames -- on the launch the plan picks
for a frame this small (the group code) or on the flagship's persistent, compacting claims."""
import numpy as np

from rayzen_amd import scene as S
from helpers import oracle_render, mismatch_report

f32 = np.float32


def cube_at(s, mesh, pos, half=1.0, angle=0.0, axis=(0.0, 1.0, 0.0)):
    """An instance of the cube mesh `mesh` ([-1, 1]^3) scaled to `half` (a number or three), turned and moved to pos."""
    h = (half, half, half) if np.isscalar(half) else half
    m = S.translate(S.identity(), pos)
    if angle:
        m = S.rotate(m, angle, axis)
    return s.add_object(mesh, S.scale(m, h))


def cube_xf(pos, half=1.0, angle=0.0, axis=(0.0, 1.0, 0.0)):
    h = (half, half, half) if np.isscalar(half) else half
    m = S.translate(S.identity(), pos)
    if angle:
        m = S.rotate(m, angle, axis)
    return np.asarray(S.scale(m, h), f32).reshape(16)


def light(posdir, power, color=(1.0, 1.0, 1.0)):
    l = np.zeros(1, S.LIGHT)
    l[0] = (posdir, color, power)
    return l


_refs = {}


def reference(key, scene, width, height, spp, bounces):
    """The oracle's frame of (key, size, spp, bounces); `key` names the scene AND its state (a moved instance, a moved camera)."""
    k = (key, width, height, spp, bounces)
    if k not in _refs:
        img = oracle_render(scene, width, height, spp, bounces, nthreads=16)
        img.setflags(write=False)
        _refs[k] = img
    return _refs[k]


def claims_env(monkeypatch, claims):
    """claims: None, or the groups per claim of the persistent, compacting launch with its cross-claim pools."""
    if claims is not None:
        monkeypatch.setenv("RZ_GROUPS_PER_CLAIM", str(claims))
        monkeypatch.setenv("RZ_CROSS_CLAIM_POOL", "1")
        monkeypatch.setenv("RZ_WPOOL_CHUNK", "64")


def frame(r, scene, width, height, spp, bounces, claims, sample_chunk=None, tile_rank=0, tile_nranks=1):
    """One frame on the open context r (the scene is uploaded already), from sample 0; the launch is checked to be the one asked for."""
    from rayzen_amd.renderer import frame_params
    r.set_frame(frame_params(scene.camera, width, height, len(scene.lights), bounces, spp, 0, tile_rank, tile_nranks))
    r.clear_accum()
    r.render_scene(scene, width, height, spp, bounces, None, tile_rank, tile_nranks, sample_chunk)
    img = r.read_accum()
    kernel, plan = r.last_kernel_name(), r.debug_last_plan()
    assert kernel.startswith("rz_render_samples"), kernel
    if claims is not None:
        assert plan["per_claim"] > 0 and plan["claim_units"] > 0, plan
    return img


def same_bits(gpu, ref, what):
    assert (gpu.view(np.uint32) == ref.view(np.uint32)).all(), f"{what}: " + mismatch_report(gpu, ref)

"""rz_present's overlays against the oracle on the cases of tests/present_cases.py (tests/test_present_cases.py shows with the
oracle alone that they bite): boxes that cross the camera plane, corners that project 2^27 px off the frame or to infinity,
the branch walk on shared meshes, overlapping and clipped light markers, FPS values up to the ends of the int range, frames
smaller than the FPS box.  Renderer.present against rzo.present on the same accumulation -- 1 spp, bounce budget 1, read
back -- the float output bit for bit and the 8-bit output byte for byte.

A MatrixCamera case is path-traced with the scene's own camera and presented with the hand-made matrices (the presenting calls
read the two matrices alone; rz_set_frame at an unchanged size keeps the accumulation); the stage puts its own camera back
after every present, so nothing is ever traced through a MatrixCamera's identity inverses."""
import numpy as np
import pytest

import present_cases as P
from oracle import rzo
from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer, frame_params

pytestmark = pytest.mark.gpu

ORDER = (S.BIND_TRIANGLES, S.BIND_MATERIALS, S.BIND_LIGHTS, S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES, S.BIND_BLAS_NODES,
         S.BIND_BLAS_INDICES, S.BIND_INSTANCES)


class Stage:
    """A renderer with a scene uploaded (and, per `way`, changed on the device), one sample accumulated and read back, and the
    oracle's view of the bindings as the device holds them."""

    def __init__(self, name, width, height, way="fresh", render=True):
        scene = {"box": P.box_scene, "branch": P.branch_scene, "deep": P.deep_scene}[name]()
        self.scene, self.width, self.height = scene, width, height
        self.num_lights = min(P.NUM_LIGHTS, len(scene.lights))
        r = self.r = Renderer(0)
        r.upload_scene(scene)
        if way == "transforms":
            r.update_transforms(P.branch_transforms(name))
        elif way == "refit":
            r.refit_geometry(P.moved_triangles(scene.arrays[S.BIND_TRIANGLES]))
        self.camera = S.Camera(aspect=width / height, position=scene.camera.position, target=scene.camera.target)
        r.set_frame(frame_params(self.camera, width, height, self.num_lights, 1, 1))
        if render:
            r.render()
        self.acc = r.read_accum()
        self.acc.setflags(write=False)
        self.oracle = rzo.Scene(*[r.read_binding(b) for b in ORDER])

    def present(self, case, call="present"):
        """(got rgb, got rgba8, want rgb, want rgba8)"""
        assert (case.width, case.height) == (self.width, self.height)
        self.r.set_frame(frame_params(case.camera, self.width, self.height, self.num_lights, 1, 1))
        got = getattr(self.r, call)(**case.kw)
        self.r.set_frame(frame_params(self.camera, self.width, self.height, self.num_lights, 1, 1))     # a camera one can trace with
        want = rzo.present(self.oracle, self.acc, case.camera.view, case.camera.proj, self.num_lights, **case.kw)
        return got + want


_stage = {}


def stage(*key, **kw):
    """One stage at a time: the tests come grouped by stage."""
    if _stage.get("key") != (key, tuple(sorted(kw.items()))):
        if "stage" in _stage:
            _stage.pop("stage").r.close()
        _stage["stage"], _stage["key"] = Stage(*key, **kw), (key, tuple(sorted(kw.items())))
    return _stage["stage"]


@pytest.fixture(scope="module", autouse=True)
def _close_the_last_stage():
    yield
    if "stage" in _stage:
        _stage.pop("stage").r.close()
    _stage.clear()


def same(got_rgb, got_rgba8, want_rgb, want_rgba8):
    diff = (got_rgb.view(np.uint32) != want_rgb.view(np.uint32)).any(axis=-1)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} pixels differ; first (y, x): {np.argwhere(diff)[:6].tolist()}"
    assert (got_rgba8 == want_rgba8).all()


@pytest.mark.parametrize("name", P.BOX_CASES)
def test_box_cases_match_the_oracle(name):
    case = P.box_case(name)
    got = stage("box", P.W, P.H).present(case)
    same(*got)
    plain = rzo.present(stage("box", P.W, P.H).oracle, stage("box", P.W, P.H).acc, case.camera.view, case.camera.proj, P.NUM_LIGHTS,
                        **dict(case.kw, show_bvh=False))[0]
    assert ((got[0] != plain).any() == (name != "behind"))              # the wire is there (and behind the camera it is not)


def test_a_grazing_case_through_present_display():
    same(*stage("box", P.W, P.H).present(P.box_case("grazing-left"), call="present_display"))


def test_lights_match_the_oracle():
    same(*stage("box", P.W, P.H).present(P.light_case()))


@pytest.mark.parametrize("fps", P.FPS_DEFINED + P.FPS_UNDEFINED, ids=lambda f: repr(float(f)))
def test_fps_values_match_the_oracle(fps):
    got = stage("box", P.W, P.H).present(P.fps_case(fps))
    same(*got)
    if fps in P.FPS_UNDEFINED or fps != fps:
        zero = stage("box", P.W, P.H).present(P.fps_case(0.0))
        assert (got[1] == zero[1]).all()                                 # the rule of rz_present_params.fps: drawn as 000.0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_overlays_at_small_sizes(size, mode):
    same(*stage("box", *size).present(P.combined_case(*size, bvh_mode=mode)))


def test_presented_before_any_render():
    """The sample count is 0 everywhere: the resolve divides by 1 and every overlay is drawn over black."""
    st = stage("box", P.W, P.H, render=False)
    assert not st.acc.any()
    got = st.present(P.combined_case(P.W, P.H))
    same(*got)
    assert got[0].any()


def _id(k):
    c = P.BRANCH_CASES[k]
    return f"{c[0]}-{c[1]}-{c[2]}"


@pytest.mark.parametrize("k", range(len(P.BRANCH_CASES)), ids=_id)
@pytest.mark.parametrize("way", ["fresh", "transforms", "refit"])
def test_branch_walk_matches_the_oracle(way, k):
    """fresh: as uploaded.  transforms: after rz_update_transforms (the device owns the TLAS and the instances).  refit: after
    rz_refit_geometry moved every vertex (the path boxes must be the refitted ones).  The oracle walks the bindings read back.
    The deep cases (trees of 34 and 35 levels: the walk's 32 levels and its 32-entry stack) go the same three ways."""
    case = P.branch_case(k)
    st = stage(P.BRANCH_CASES[k][0], P.W, P.H, way=way)
    got = st.present(case)
    same(*got)
    path, _ = rzo.bvh_branch(st.oracle, case.kw["selected_blas"], case.kw["selected_tri"])
    assert len(path) == P.BRANCH_CASES[k][3]                         # neither change touches the topology
    if way != "fresh":
        before = rzo.Scene(*[case.scene.arrays[b] for b in ORDER])
        moved = rzo.present(before, st.acc, case.camera.view, case.camera.proj, st.num_lights, **case.kw)[0]
        assert (moved != got[2]).any() == (len(path) > 0)               # the change shows in the path's boxes


def test_a_branch_case_through_present_display():
    same(*stage("branch", P.W, P.H, way="refit").present(P.branch_case(4), call="present_display"))

"""The C++ front end (rayzen_amd/csrc/host/Renderer.h) held to the Python binding, the CPU oracle and the host library,
method by method.  tests/cpp/frontend_driver.cpp calls every public method of rayzen::Renderer on one small scene and writes
every input and output as raw files; here the same calls are replayed from those files and every byte is compared:

  python  a fresh Renderer(0) is given the dumped initial bindings and replays the calls with the dumped inputs; every output
          and every read_binding at every step equals the driver's dump
  oracle  every dumped frame equals rzo.render on the bindings dumped at that step, every traceRays / shadowRays result the
          oracle's trace, every pick the brute-force loop of tests/test_rays_gpu.py
  host    after each deforming step the bindings equal those of the host library's byte partner (Scene.refit_mesh,
          skin_triangles, Scene.rebuild_mesh, Scene.update_dynamic); in `sequence` the two per-frame update routes leave the
          same bindings and the same frame

No comparison has a tolerance.  The driver runs once per (scenario, route), in a child process; after a run that ends in a
signal or a timeout nothing more is started in this module."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import rzo
from rayzen_amd import _lib
from rayzen_amd import scene as S
from rayzen_amd.renderer import HIT_DTYPE, MESH_QUALITY, RAY_DTYPE, VISIBILITY_DTYPE, RayZenError, Renderer, make_rays, pick_ray
from helpers import sync_oracle_flavour

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "rayzen_amd", "csrc", "host", "Renderer.h")
DRIVER = os.path.join(ROOT, "tests", "cpp", "frontend_driver.cpp")

# Every public method of rayzen::Renderer -> the driver scenario(s) that execute it (a name with "::" is a test elsewhere in the
# suite that already compares the method's output with another binding).
COVERAGE = {
    "useDeviceBlasBuilder": "frame, sequence (route devblas)",
    "initializeSSBOs": "frame, sequence (routes host, copies, devblas)",
    "initializeSSBOsOnDevice": "frame, sequence, deform (route device)",
    "updateDynamicBVHAndSSBOs": "sequence",
    "updateDynamicBVHAndSSBOsOnDevice": "frame, post, deform, sequence",
    "refitMesh": "deform, sequence",
    "refitAll": "deform, sequence",
    "createRig": "deform, sequence, errors",
    "poseRig": "deform, sequence, errors",
    "destroyRig": "deform, errors",
    "meshQuality": "deform",
    "rebuildDegraded": "deform, sequence",
    "sendSceneDataToShader": "frame",
    "draw": "frame",
    "finish": "frame",
    "readAccum": "frame",
    "resolveRGBA8": "frame",
    "traceRays": "queries, deform",
    "shadowRays": "queries",
    "pickRay": "queries",
    "pick": "queries, errors",
    "renderEditor": "test_editor_gpu.py::test_cpp_render_editor_equals_python",
    "denoise": "post, errors",
    "presentDenoised": "post",
    "denoiseTemporal": "post",
    "presentTemporal": "post",
    "resetTemporal": "post",
    "presentDisplay": "post, errors",
    "presentUpscaled": "post, errors",
    "resetDisplay": "post",
    "lastRenderMs": "frame",
    "context": "deform",
    "buffers": "deform",
}
SCENARIOS = ("frame", "queries", "post", "deform", "sequence", "errors")
ALL_ROUTES = ("host", "copies", "devblas", "device")
BINDINGS = tuple(S.BINDING_DTYPES)
PRESENT = np.dtype([("fps", "<f4"), ("show_fps", "<i4"), ("show_lights", "<i4"), ("show_bvh", "<i4"), ("bvh_mode", "<i4"),
                    ("selected_blas", "<i4"), ("selected_tri", "<i4")])
DENOISE = np.dtype([("iterations", "<i4"), ("sigma_color", "<f4"), ("sigma_normal", "<f4"), ("sigma_plane", "<f4"), ("demodulate", "<i4"),
                    ("reserved", "<i4", 3)])
TEMPORAL = np.dtype([("alpha", "<f4"), ("alpha_moments", "<f4"), ("max_history", "<i4"), ("normal_cos", "<f4"), ("plane_tol", "<f4"),
                     ("iterations", "<i4"), ("sigma_l", "<f4"), ("sigma_normal", "<f4"), ("sigma_plane", "<f4"), ("demodulate", "<i4"),
                     ("reserved", "<i4", 6)])
DISPLAY = np.dtype([("exposure_mode", "<i4"), ("exposure", "<f4"), ("key", "<f4"), ("min_exposure", "<f4"), ("max_exposure", "<f4"),
                    ("adapt", "<f4"), ("low_permille", "<i4"), ("high_permille", "<i4"), ("curve", "<i4"), ("white", "<f4"),
                    ("transfer", "<i4"), ("reserved", "<i4", 5)])
UPSCALE = np.dtype([("factor", "<i4"), ("sigma_normal", "<f4"), ("sigma_plane", "<f4"), ("demodulate", "<i4"), ("reserved", "<i4", 4)])
SOURCES = {v: k for k, v in _lib.DISPLAY_SOURCES.items()}


# ---------------------------------------------------------------------------------------------------------------------
# running the driver

class Run:
    """One finished driver run: the parsed steps.txt and the files next to it."""

    def __init__(self, directory):
        self.dir = str(directory)
        self.steps = []
        for line in open(os.path.join(self.dir, "steps.txt")):
            n, name, *rest = line.rstrip("\n").split(" ", 2)
            text = rest[0] if rest else ""
            kv = {}
            if name == "error":                      # "... message=<free text to the end of the line>"
                head, kv["message"] = text.split(" message=", 1)
                text = head
            kv.update(p.split("=", 1) for p in text.split() if "=" in p)
            self.steps.append((int(n), name, kv))
        assert self.steps and self.steps[-1][1] == "end", "the driver did not reach its end"

    def has(self, n, tag):
        return os.path.exists(os.path.join(self.dir, f"{n}.{tag}.bin"))

    def raw(self, n, tag):
        with open(os.path.join(self.dir, f"{n}.{tag}.bin"), "rb") as f:
            return f.read()

    def arr(self, n, tag, dtype):
        return np.frombuffer(self.raw(n, tag), dtype).copy()

    def opt(self, n, tag, dtype):
        """A params file that exists only when the driver passed a struct (absent: it passed NULL); an empty vector: None."""
        if not self.has(n, tag):
            return None
        a = self.arr(n, tag, dtype)
        return a if len(a) else None

    def bindings(self, n):
        return {b: self.arr(n, f"b{b}", S.BINDING_DTYPES[b]) for b in BINDINGS} if self.has(n, "b0") else None

    def frame(self, n):
        return _lib.FrameParams.from_buffer_copy(self.raw(n, "fp"))


_RUNS = {}          # (scenario, route) -> Run, or the text of a failed run
_FAULT = []         # the reason nothing more is started


@pytest.fixture(scope="module")
def frontend(tmp_path_factory):
    """Compiles the driver once; returns get(scenario, route) -> Run (each pair runs once, in a child process)."""
    sync_oracle_flavour()
    lib = os.path.join(ROOT, "rayzen_amd", "lib")
    exe = str(tmp_path_factory.mktemp("frontend_driver") / "frontend_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(HEADER), DRIVER,
                           "-L", lib, "-lrayzen_host", "-lrayzen_hip", f"-Wl,-rpath,{lib}", "-o", exe])

    def get(scenario, route):
        key = (scenario, route)
        if key not in _RUNS:
            if _FAULT:
                pytest.skip(_FAULT[0])
            out = tmp_path_factory.mktemp(f"{scenario}_{route}")
            try:
                p = subprocess.run([exe, str(out), scenario, route], capture_output=True, text=True, timeout=120)
            except subprocess.TimeoutExpired:
                _FAULT.append(f"frontend_driver {scenario} {route} did not finish in 120 s: nothing more is started")
                _RUNS[key] = _FAULT[0]
                pytest.fail(_FAULT[0])
            if p.returncode in (134, 139) or p.returncode < 0:
                _FAULT.append(f"frontend_driver {scenario} {route} ended with status {p.returncode}: nothing more is started\n{p.stderr[-2000:]}")
                _RUNS[key] = _FAULT[0]
                pytest.fail(_FAULT[0])
            _RUNS[key] = Run(out) if p.returncode == 0 else f"frontend_driver {scenario} {route} returned {p.returncode}: {p.stderr[-2000:]}"
        if _FAULT and _RUNS[key] != _FAULT[0]:
            pytest.skip(_FAULT[0])
        if isinstance(_RUNS[key], str):
            pytest.fail(_RUNS[key])
        return _RUNS[key]

    return get


# ---------------------------------------------------------------------------------------------------------------------
# (a) the Python binding

class _Cam:
    def __init__(self, fp):
        self.inv_view, self.inv_proj = np.array(fp.inv_view, np.float32), np.array(fp.inv_proj, np.float32)
        self.view, self.proj = np.array(fp.view, np.float32), np.array(fp.proj, np.float32)
        self.position = np.array(fp.cam_pos, np.float32)


def _present_kw(pp):
    p = pp[0]
    return dict(fps=float(p["fps"]), show_fps=int(p["show_fps"]), show_lights=int(p["show_lights"]), show_bvh=int(p["show_bvh"]),
                bvh_mode=int(p["bvh_mode"]), selected_blas=int(p["selected_blas"]), selected_tri=int(p["selected_tri"]))


def _denoise_kw(dp):
    if dp is None:
        return {}
    p = dp[0]
    assert not p["reserved"].any()
    return dict(iterations=int(p["iterations"]), sigma_color=float(p["sigma_color"]), sigma_normal=float(p["sigma_normal"]),
                sigma_plane=float(p["sigma_plane"]), demodulate=int(p["demodulate"]))


def _temporal_kw(tp):
    if tp is None:
        return {}
    p = tp[0]
    assert not p["reserved"].any()
    return {k: (int(p[k]) if isinstance(v, int) else float(p[k])) for k, v in _lib.TEMPORAL_DEFAULTS.items()}


def _display_kw(dp):
    if dp is None:
        return {}
    p = dp[0]
    assert not p["reserved"].any()
    curves = {v: k for k, v in _lib.DISPLAY_CURVES.items()}
    transfers = {v: k for k, v in _lib.DISPLAY_TRANSFERS.items()}
    return dict(auto=bool(p["exposure_mode"]), exposure=float(p["exposure"]), key=float(p["key"]), min_exposure=float(p["min_exposure"]),
                max_exposure=float(p["max_exposure"]), adapt=float(p["adapt"]), low=int(p["low_permille"]) / 1000, high=int(p["high_permille"]) / 1000,
                curve=curves[int(p["curve"])], white=float(p["white"]), transfer=transfers[int(p["transfer"])])


def _upscale_kw(up):
    if up is None:
        return {}
    p = up[0]
    assert not p["reserved"].any()
    return dict(factor=int(p["factor"]), sigma_normal=float(p["sigma_normal"]), sigma_plane=float(p["sigma_plane"]), demodulate=int(p["demodulate"]))


def _filter_kw(run, n, source):
    if not run.has(n, "filter"):
        return None
    return _denoise_kw(run.arr(n, "filter", DENOISE)) if source == 1 else _temporal_kw(run.arr(n, "filter", TEMPORAL))


def _differing(got, want, item):
    """How many elements of `item` bytes differ (pixels of a frame, records of an array); -1: another length."""
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if g.size != w.size:
        return -1
    return int((g.reshape(-1, item) != w.reshape(-1, item)).any(axis=1).sum())


def _replay_python(run):
    """Replays every step on the Python binding.  Returns the mismatches as (step, name, what, elements that differ)."""
    bad = []
    r, fp, rigs = None, None, {}

    def same(n, name, what, got, want, item=1):
        got = np.ascontiguousarray(got).tobytes()
        if got != want:
            bad.append((n, name, what, _differing(got, want, item)))

    try:
        for n, name, kv in run.steps:
            if name == "init":
                if r is not None:
                    r.close()
                r, fp, rigs = Renderer(0), None, {}
                for b, a in run.bindings(n).items():
                    r.upload(b, a)
            elif name == "set_frame":
                fp = run.frame(n)
                r.set_frame(fp)
            elif name == "draw":
                r.render()
                same(n, name, "accum (pixels)", r.read_accum(), run.raw(n, "accum"), 16)
            elif name == "resolve":
                same(n, name, "rgba8 (pixels)", r.resolve_rgba8(), run.raw(n, "rgba8"), 4)
            elif name == "last_render_ms":
                if not float.fromhex(kv["ms"]) > 0:
                    bad.append((n, name, "lastRenderMs() is not positive", 1))
            elif name == "update":                    # either route of the front end: the Python side always lets the device do it
                r.update_transforms(run.arr(n, "xf", np.float32).reshape(-1, 16))
            elif name == "trace":
                rays = run.arr(n, "rays", RAY_DTYPE)
                want = run.arr(n, "hits", HIT_DTYPE)
                h = r.trace_rays(rays["origin"], rays["dir"], incoherent=bool(int(kv["incoherent"])))
                for k in h:
                    same(n, name, f"hits.{k} (rays)", h[k], np.ascontiguousarray(want[k]).tobytes(), want[k].dtype.itemsize * max(1, want[k][0].size))
                if want["reserved"].any():
                    bad.append((n, name, "hits.reserved is not zero", int((want["reserved"] != 0).sum())))
            elif name == "shadow":
                rays = run.arr(n, "rays", RAY_DTYPE)
                want = run.arr(n, "vis", VISIBILITY_DTYPE)
                lit, vis = r.shadow_rays(rays["origin"], rays["dir"], rays["max_dist"], incoherent=bool(int(kv["incoherent"])))
                same(n, name, "visibility (rays)", vis, np.ascontiguousarray(want["visibility"]).tobytes(), 4)
                same(n, name, "lit (rays)", lit.astype(np.int32), np.ascontiguousarray(want["lit"]).tobytes(), 4)
            elif name == "pick_ray":
                o, d = pick_ray(float.fromhex(kv["mx"]), float.fromhex(kv["my"]), int(kv["w"]), int(kv["h"]), _Cam(fp))
                same(n, name, "the ray's 28 bytes", np.frombuffer(make_rays(o[None], d[None]).tobytes()[:28], np.uint8), run.raw(n, "ray")[:28], 28)
            elif name == "pick":
                got = r.pick(float.fromhex(kv["mx"]), float.fromhex(kv["my"]), int(kv["w"]), int(kv["h"]), _Cam(fp))
                if (got or (-1, -1)) != (int(kv["instance"]), int(kv["triangle"])):
                    bad.append((n, name, f"pick {got} != {kv['instance']}, {kv['triangle']}", 1))
                if (fp.width, fp.height) != (int(kv["w"]), int(kv["h"])):
                    bad.append((n, name, "the driver's screen is not the frame last set", 1))
            elif name == "denoise":
                same(n, name, "rgb (pixels)", r.denoise(**_denoise_kw(run.opt(n, "dp", DENOISE))), run.raw(n, "rgb"), 12)
            elif name == "present_denoised":
                _, px = r.present_denoised(**_present_kw(run.arr(n, "pp", PRESENT)), **_denoise_kw(run.opt(n, "dp", DENOISE)))
                same(n, name, "rgba8 (pixels)", px, run.raw(n, "rgba8"), 4)
            elif name == "denoise_temporal":
                got = r.denoise_temporal(keep=bool(int(kv["keep"])), **_temporal_kw(run.opt(n, "tp", TEMPORAL)))
                same(n, name, "rgb (pixels)", got, run.raw(n, "rgb"), 12)
            elif name == "present_temporal":
                _, px = r.present_temporal(**_present_kw(run.arr(n, "pp", PRESENT)), **_temporal_kw(run.opt(n, "tp", TEMPORAL)))
                same(n, name, "rgba8 (pixels)", px, run.raw(n, "rgba8"), 4)
            elif name == "reset_temporal":
                r.temporal_reset()
            elif name == "reset_display":
                r.display_reset()
            elif name == "present_display":
                src = int(kv["source"])
                _, px = r.present_display(source=SOURCES[src], filter=_filter_kw(run, n, src), **_present_kw(run.arr(n, "pp", PRESENT)),
                                          **_display_kw(run.opt(n, "disp", DISPLAY)))
                same(n, name, "rgba8 (pixels)", px, run.raw(n, "rgba8"), 4)
            elif name == "present_upscaled":
                src = int(kv["source"])
                _, px = r.present_upscaled(source=SOURCES[src], filter=_filter_kw(run, n, src), **_upscale_kw(run.opt(n, "up", UPSCALE)),
                                           **_present_kw(run.arr(n, "pp", PRESENT)), **_display_kw(run.opt(n, "disp", DISPLAY)))
                same(n, name, "rgba8 (pixels)", px, run.raw(n, "rgba8"), 4)
            elif name == "refit":
                r.refit_geometry(run.arr(n, "tris", S.TRIANGLE), int(kv["first"]))
            elif name == "refit_all":
                r.update(S.BIND_TRIANGLES, run.arr(n, "tris", S.TRIANGLE), int(kv["first"]) * 64)
                r.refit_geometry()
            elif name == "create_rig":
                rigs[int(kv["rig"])] = r.skin_create(int(kv["first"]), run.arr(n, "rest", S.TRIANGLE), run.opt(n, "skin", S.SKIN_TRIANGLE),
                                                     int(kv["bones"]), run.opt(n, "morphs", S.MORPH_TRIANGLE))
            elif name == "pose":
                bones = run.opt(n, "bones", np.float32)
                r.skin_pose(rigs[int(kv["rig"])], None if bones is None else bones.reshape(-1, 16), run.opt(n, "weights", np.float32))
            elif name == "destroy_rig":
                r.skin_destroy(rigs.pop(int(kv["rig"])))
            elif name == "quality":
                same(n, name, "records", r.geometry_quality(), run.raw(n, "quality"), 64)
            elif name == "rebuild":
                same(n, name, "records", r.rebuild_geometry(float.fromhex(kv["ratio"])), run.raw(n, "quality"), 64)
            elif name not in ("begin", "bind", "end", "error", "outside_old_box"):
                raise AssertionError(f"step {n}: unknown step {name}")
            if name != "init" and run.has(n, "b0"):
                for b, want in run.bindings(n).items():
                    same(n, name, f"binding {b} (elements)", r.read_binding(b), want.tobytes(), want.dtype.itemsize)
    finally:
        if r is not None:
            r.close()
    return bad


def _assert_selection(records, max_ratio):
    """rz_rebuild_geometry's rule on its own records: rebuilt are exactly the meshes for which cost <= max_ratio * built is false."""
    want = ~(records["sah_cost_before"] <= max_ratio * records["sah_cost_built"])
    assert ((records["flags"] & _lib.QUALITY_REBUILT != 0) == want).all(), records
    assert (records["sah_cost_before"] > 0).all() and (records["reserved"] == 0).all()


def _report(bad):
    return f"{len(bad)} comparisons differ: " + "; ".join(f"step {n} {name}: {what}: {k}" for n, name, what, k in bad[:12])


# ---------------------------------------------------------------------------------------------------------------------
# (b) the CPU oracle

def _oracle_scene(a):
    return rzo.Scene(a[S.BIND_TRIANGLES], a[S.BIND_MATERIALS], a[S.BIND_LIGHTS], a[S.BIND_TLAS_NODES], a[S.BIND_TLAS_INDICES],
                     a[S.BIND_BLAS_NODES], a[S.BIND_BLAS_INDICES], a[S.BIND_INSTANCES])


class _View:
    def __init__(self, arrays):
        self.arrays = arrays


def _world_pick(arrays, o, d):
    """main.cpp:515-547 per instance (test_rays_gpu._brute_pick on one instance at a time: within an instance the object-local
    t orders hits as the world distance does), then the closest instance by WORLD distance (binary64), as Renderer::pick
    documents it -- this scene has a scaled floor and a skewed cube, where object-local t of different instances do not
    compare.  Returns (instance, triangle) or None, and whether the choice is clear (no runner-up within 1e-4, |a| >= 1e-4)."""
    from test_rays_gpu import _brute_pick
    tris, inst = arrays[S.BIND_TRIANGLES], arrays[S.BIND_INSTANCES]
    starts = sorted(set(int(g) for g in inst["globalTriOffset"])) + [len(tris)]
    found, clear = [], True
    for k in range(len(inst)):
        g = int(inst[k]["globalTriOffset"])
        one = dict(arrays)
        one[S.BIND_INSTANCES] = inst[k:k + 1]
        one[S.BIND_TRIANGLES] = tris[:starts[starts.index(g) + 1]]
        w = _brute_pick(_View(one), o, d)
        if w is None:
            continue
        _, tri, t, runner, a = w
        clear = clear and runner - t > 1e-4 and a >= 1e-4
        m = np.asarray(inst[k]["inverseTransform"], np.float64).reshape(4, 4).T
        f = np.asarray(inst[k]["transform"], np.float64).reshape(4, 4).T
        lo, ld = m[:3, :3] @ o.astype(np.float64) + m[:3, 3], m[:3, :3] @ d.astype(np.float64)
        p = f[:3, :3] @ (lo + ld / np.linalg.norm(ld) * t) + f[:3, 3]
        found.append((float(np.linalg.norm(p - o)), k, tri))
    if not found:
        return None, True
    found.sort()
    if len(found) > 1 and found[1][0] - found[0][0] <= 1e-4:
        clear = False
    return (found[0][1], found[0][2]), clear


def _check_oracle(run):
    from test_rays_gpu import _assert_trace_matches_oracle, _bits
    arrays = osc = fp = None
    frames = traces = shadows = picks = pick_hits = pick_misses = 0
    for n, name, kv in run.steps:
        if run.has(n, "b0"):
            arrays = run.bindings(n)
            osc = _oracle_scene(arrays)
        if name == "set_frame":
            fp = run.frame(n)
        elif name == "draw":
            # sample_base > 0 continues the frame: the accumulation is the frame of sample_base + spp samples from 0
            fr = rzo.make_frame(fp.width, fp.height, np.array(fp.inv_view), np.array(fp.inv_proj), np.array(fp.cam_pos), fp.num_lights,
                                fp.bounce_budget, fp.sample_base + fp.spp, 0)
            ref = rzo.render(osc, fr, nthreads=8)
            got = run.arr(n, "accum", np.float32).reshape(fp.height, fp.width, 4)
            diff = int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
            assert diff == 0, f"step {n}: {diff} of {fp.width * fp.height} pixels differ from the oracle's frame"
            assert got[..., 3].min() == fp.sample_base + fp.spp and got[..., :3].std() > 0
            frames += 1
        elif name == "trace":
            rays, hits = run.arr(n, "rays", RAY_DTYPE), run.arr(n, "hits", HIT_DTYPE)
            _assert_trace_matches_oracle(osc, rays["origin"], rays["dir"], {k: hits[k] for k in ("t", "point", "normal", "material", "instance", "triangle", "prim")})
            sel = hits["instance"] >= 0
            assert (hits["prim"][sel] - arrays[S.BIND_INSTANCES]["globalTriOffset"][hits["instance"][sel]] == hits["triangle"][sel]).all()
            assert sel.any() and not sel.all()
            traces += 1
        elif name == "shadow":
            rays, vis = run.arr(n, "rays", RAY_DTYPE), run.arr(n, "vis", VISIBILITY_DTYPE)
            wrong = []
            for i in range(len(rays)):
                wl, wv = rzo.shadow(osc, rays["origin"][i], rays["dir"][i], float(rays["max_dist"][i]))
                if wl != bool(vis["lit"][i]) or _bits([wv])[0] != _bits(vis["visibility"][i:i + 1])[0]:
                    wrong.append((i, wl, wv, vis[i]))
            assert not wrong, f"step {n}: {len(wrong)} of {len(rays)} shadow rays differ from the oracle; first: {wrong[0]}"
            v = vis["visibility"]
            assert ((v > 0) & (v < 1)).any() and (v == 0).any() and (v == 1).any()       # through glass, blocked, free
            shadows += 1
        elif name == "pick":
            o, d = pick_ray(float.fromhex(kv["mx"]), float.fromhex(kv["my"]), int(kv["w"]), int(kv["h"]), _Cam(fp))
            want, clear = _world_pick(arrays, o, d)
            got = None if int(kv["instance"]) < 0 else (int(kv["instance"]), int(kv["triangle"]))
            if clear:
                assert got == want, f"step {n}: pick({kv['mx']}, {kv['my']}) = {got}, the brute-force loop finds {want}"
                picks += 1
                pick_hits += want is not None
                pick_misses += want is None
    return dict(frames=frames, traces=traces, shadows=shadows, picks=picks, pick_hits=pick_hits, pick_misses=pick_misses)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the host library

def _host_scene(arrays):
    """An S.Scene (librayzen_host) of the dumped arrays: one mesh per distinct triangle range, the instances' transforms."""
    tris, inst = arrays[S.BIND_TRIANGLES], arrays[S.BIND_INSTANCES]
    starts = sorted(set(int(g) for g in inst["globalTriOffset"]))
    ranges = {g: (g, (starts + [len(tris)])[i + 1]) for i, g in enumerate(starts)}
    sc = S.Scene(materials=arrays[S.BIND_MATERIALS], lights=arrays[S.BIND_LIGHTS])
    ids = {g: sc.add_mesh(tris[a:b]) for g, (a, b) in ranges.items()}
    for it in inst:
        sc.add_object(ids[int(it["globalTriOffset"])], it["transform"])
    sc.build(share_meshes=True)
    return sc, ranges, ids


def _check_host_partner(run):
    """After every step that changes the geometry, the host library's partner gives the dumped bytes."""
    sc = ranges = ids = None
    rigs, compared = {}, 0

    def refit(first, new):
        cur = sc.arrays[S.BIND_TRIANGLES].copy()
        cur[first:first + len(new)] = new
        for g, (a, b) in ranges.items():
            if a < first + len(new) and first < b:
                sc.refit_mesh(ids[g], cur[a:b])

    for n, name, kv in run.steps:
        if name == "init":
            sc, ranges, ids = _host_scene(run.bindings(n))
        elif name in ("refit", "refit_all"):
            refit(int(kv["first"]), run.arr(n, "tris", S.TRIANGLE))
        elif name == "create_rig":
            rigs[int(kv["rig"])] = (int(kv["first"]), run.arr(n, "rest", S.TRIANGLE), run.opt(n, "skin", S.SKIN_TRIANGLE),
                                    run.opt(n, "morphs", S.MORPH_TRIANGLE))
        elif name == "pose":
            first, rest, skin, morphs = rigs[int(kv["rig"])]
            bones = run.opt(n, "bones", np.float32)
            refit(first, S.skin_triangles(rest, skin, None if bones is None else bones.reshape(-1, 16), morphs, run.opt(n, "weights", np.float32)))
        elif name == "rebuild":
            for q in run.arr(n, "quality", MESH_QUALITY):
                if q["flags"] & _lib.QUALITY_REBUILT:
                    sc.rebuild_mesh(ids[int(q["tri_offset"])])
        elif name == "update":
            for i, xf in enumerate(run.arr(n, "xf", np.float32).reshape(-1, 16)):
                sc.set_transform(i, xf)
            sc.update_dynamic()
        if run.has(n, "b0"):
            want = run.bindings(n)
            for b in S.GEOMETRY_BINDINGS:
                k = _differing(np.ascontiguousarray(sc.arrays[b]).tobytes(), want[b].tobytes(), want[b].dtype.itemsize)
                assert k == 0, f"step {n} {name}: {k} elements of binding {b} differ from the host library's"
            compared += 1
    return compared


def _subruns(run):
    """`sequence`: {D: {device flag: [(step name, tag, bytes), ...]}} of every file each sub-run wrote after its hand-over."""
    out, cur = {}, None
    for n, name, kv in run.steps:
        if name == "begin":
            cur = out.setdefault(kv["D"], {}).setdefault(int(kv["device"]), [])
        elif cur is not None and name != "init":
            for f in sorted(os.listdir(run.dir)):
                if f.startswith(f"{n}."):
                    cur.append((name, f.split(".")[1], run.raw(n, f.split(".")[1])))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the tests: one per (scenario, route, aspect)

ROUTES = {"frame": ALL_ROUTES, "sequence": ALL_ROUTES, "deform": ("host", "device"), "queries": ("host",), "post": ("host",),
          "errors": ("host",)}
PAIRS = [(s, r) for s in SCENARIOS for r in ROUTES[s]]


@pytest.mark.parametrize("scenario,route", [p for p in PAIRS if p[0] != "errors"])
def test_python_binding_replays_the_same_bytes(frontend, scenario, route):
    run = frontend(scenario, route)
    bad = _replay_python(run)
    assert not bad, _report(bad)
    names = {name for _, name, _ in run.steps}
    if scenario == "post":
        sizes = [int(kv["bytes"]) for _, name, kv in run.steps if name == "present_upscaled"]
        assert sizes == [66 * 34 * 4, 33 * 17 * 4, 99 * 51 * 4, 99 * 51 * 4, 66 * 34 * 4]
        assert {"denoise", "present_denoised", "denoise_temporal", "present_temporal", "reset_temporal", "present_display", "reset_display"} <= names
    if scenario == "deform":
        assert [name for _, name, _ in run.steps].count("refit") == 3            # whole, partial, and spanning two meshes
        assert {"refit_all", "create_rig", "pose", "destroy_rig", "quality", "rebuild"} <= names
        first, second = [run.arr(n, "quality", MESH_QUALITY) for n, name, _ in run.steps if name == "rebuild"]
        _assert_selection(first, 1.0)
        _assert_selection(second, 1e9)
        assert not (second["flags"] & _lib.QUALITY_REBUILT).any()                # ratio 1e9 rebuilds nothing
    if scenario == "sequence":
        rebuilds = [n for n, name, _ in run.steps if name == "rebuild"]
        assert len(rebuilds) == 4                                                # two rounds on either update route
        for n in rebuilds:
            _assert_selection(run.arr(n, "quality", MESH_QUALITY), 1.0)


@pytest.mark.parametrize("scenario,route", [p for p in PAIRS if p[0] != "errors"])
def test_frames_and_queries_equal_the_oracle(frontend, scenario, route):
    run = frontend(scenario, route)
    seen = _check_oracle(run)
    want_frames = {"frame": 3, "queries": 0, "post": 3, "deform": 13, "sequence": 16}[scenario]
    assert seen["frames"] == want_frames, seen
    if scenario == "queries":
        assert seen["traces"] == 2 and seen["shadows"] == 2, seen
        # 126 cursor positions; the brute-force loop decides the clear ones, hits and misses (the sky) among them
        assert seen["picks"] >= 60 and seen["pick_hits"] >= 20 and seen["pick_misses"] >= 10, seen


@pytest.mark.parametrize("route", ROUTES["deform"])
def test_deform_bindings_equal_the_host_library(frontend, route):
    run = frontend("deform", route)
    assert _check_host_partner(run) == 13           # the hand-over and the twelve steps that change a binding


@pytest.mark.parametrize("route", ROUTES["deform"])
def test_deform_leaves_the_old_boxes(frontend, route):
    """The scenario cannot pass vacuously: after the first refit at least 20 pixels of the 40 x 24 frame show a surface
    outside the world box its instance had before (what a stale box would cull)."""
    run = frontend("deform", route)
    counts = [int(kv["pixels"]) for _, name, kv in run.steps if name == "outside_old_box"]
    assert counts and min(counts) >= 20, counts


@pytest.mark.parametrize("route", ROUTES["sequence"])
def test_sequence_both_update_routes_agree(frontend, route):
    """After refitMesh, refitAll, poseRig or rebuildDegraded, updateDynamicBVHAndSSBOs and updateDynamicBVHAndSSBOsOnDevice
    leave the same bindings -- the deformed geometry's -- and the same frame, in the first round and in the second."""
    subs = _subruns(frontend("sequence", route))
    assert sorted(subs) == ["poseRig", "rebuildDegraded", "refitAll", "refitMesh"]
    bad = []
    for D, pair in sorted(subs.items()):
        host, dev = pair[0], pair[1]
        assert [x[:2] for x in host] == [x[:2] for x in dev] and sum(x[1] == "accum" for x in dev) == 2
        for (name, tag, a), (_, _, b) in zip(host, dev):
            if a != b:
                item = 16 if tag == "accum" else S.BINDING_DTYPES[int(tag[1:])].itemsize if tag[0] == "b" and tag[1:].isdigit() else 1
                bad.append(f"{D}: {name}.{tag}: {_differing(a, b, item)} {'pixels' if tag == 'accum' else 'elements'}")
    assert not bad, "updateDynamicBVHAndSSBOs differs from updateDynamicBVHAndSSBOsOnDevice: " + "; ".join(bad)


@pytest.mark.parametrize("route", ("host", "device"))
def test_sequence_bindings_equal_the_host_library(frontend, route):
    run = frontend("sequence", route)
    assert _check_host_partner(run) >= 8 * 4


ERRORS = {      # call -> what the message starts with, a word the library's (or the header's) text carries
    "denoise_no_frame": ("rz_denoise: ", "rz_set_frame"),
    "pick_no_frame": ("pick: ", "sendSceneDataToShader"),
    "present_display_no_frame": ("rz_present_display: ", "rz_set_frame"),
    "present_upscaled_factor_0": ("rz_present_upscaled: ", "factor"),
    "present_upscaled_factor_5": ("rz_present_upscaled: ", "factor"),
    "pose_destroyed_rig": ("rz_skin_pose: ", "rig"),
    "refit_past_the_end": ("rz_refit_geometry: ", "binding 0"),
    "create_rig_short_skin": ("createRig: ", "skin"),
    "create_rig_ragged_morphs": ("createRig: ", "morphs"),
}


def test_errors_throw_and_leave_the_renderer_usable(frontend):
    run = frontend("errors", "host")
    seen = {kv["call"]: (int(kv["threw"]), kv["message"]) for _, name, kv in run.steps if name == "error"}
    assert sorted(seen) == sorted(ERRORS)
    for call, (start, word) in ERRORS.items():
        threw, msg = seen[call]
        assert threw == 1, f"{call} did not throw std::runtime_error"
        assert msg.startswith(start) and word in msg and len(msg) > len(start) + 8, (call, msg)
    # the library's own words: the Python binding gets the same message for the same mistake
    init = next(n for n, name, _ in run.steps if name == "init")
    arrays = run.bindings(init)
    fp = run.frame(next(n for n, name, _ in run.steps if name == "set_frame"))
    blob = int(arrays[S.BIND_INSTANCES]["globalTriOffset"][1])
    r = Renderer(0)
    for b, a in arrays.items():
        r.upload(b, a)

    def message(fn):
        with pytest.raises(RayZenError) as e:
            fn()
        return str(e.value).split("): ", 1)[1]

    def library(call):
        return seen[call][1].split(": ", 1)[1]

    assert message(lambda: r.denoise()) == library("denoise_no_frame")
    assert message(lambda: r.present_display()) == library("present_display_no_frame")
    r.set_frame(fp)
    r.render()
    assert message(lambda: r.present_upscaled(factor=0)) == library("present_upscaled_factor_0")
    assert message(lambda: r.present_upscaled(factor=5)) == library("present_upscaled_factor_5")
    rig = r.skin_create(blob, 432, None, 0, np.zeros((1, 432), S.MORPH_TRIANGLE))
    r.skin_destroy(rig)
    assert message(lambda: r.skin_pose(rig, None, np.zeros(1, np.float32))) == library("pose_destroyed_rig")
    n = len(arrays[S.BIND_TRIANGLES])
    assert message(lambda: r.refit_geometry(arrays[S.BIND_TRIANGLES][:4], n - 3)) == library("refit_past_the_end")
    r.close()
    # the renderer stayed usable and unchanged: the bindings are those handed over, the frame after equals the frame before
    after = next(n for n, name, _ in run.steps if name == "bind")
    for b in BINDINGS:
        assert run.raw(after, f"b{b}") == run.raw(init, f"b{b}"), b
    frames = [run.raw(n, "accum") for n, name, _ in run.steps if name == "draw"]
    assert len(frames) == 2 and frames[0] == frames[1]


def test_coverage_table_names_every_public_method():
    """A plain text scan of Renderer.h: every public method of class Renderer is in COVERAGE, with a scenario of the driver
    that calls it (or the test elsewhere that holds it)."""
    text = open(HEADER).read()
    body = text[text.index("class Renderer {"):text.index("class GroupRenderer")]
    public = body[body.index("public:"):body.index("private:")]
    methods = set()
    for line in public.splitlines():
        m = re.match(r"^    (?![ /}])[^(]*?(\w+)\(", line)
        if m and m.group(1) != "Renderer":
            methods.add(m.group(1))
    assert len(methods) >= 30
    assert methods == set(COVERAGE), (sorted(methods - set(COVERAGE)), sorted(set(COVERAGE) - methods))
    driver = open(DRIVER).read()
    for method, where in COVERAGE.items():
        if "::" in where:
            name = where.split("::")[1]
            assert name in open(os.path.join(ROOT, "tests", where.split("::")[0])).read()
            continue
        assert set(re.findall(r"[a-z]+", where.split("(")[0])) <= set(SCENARIOS), where
        assert re.search(rf"(\.|::){method}\(", driver), f"the driver never calls {method}"

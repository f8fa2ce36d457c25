"""The table of non-geometry edits -- materials, lights, instances -- that tests/test_scene_edits_gpu.py applies to a live
context and tests/test_scene_edits_cases.py shows to bite.  Plain data and small builders, no GPU.

A context is its eight bindings: after any rz_upload / rz_update every call must answer as a fresh context holding the same
arrays would.  A case names a base scene and gives `edit(arrays) -> [Call, ...]`: the calls that edit a context holding
`arrays` (the base's, or what a prior state left: an edit of an instance record reads the offsets and transforms in force).
`apply(calls, arrays)` is the specification of those calls on the arrays themselves; its result is what the fresh context is
given.  Every case states why it is in the table, whether the frame changes, and what rz_debug_last_plan().transparent must be.

Nothing here is drawn at random and nothing models the context: the reference is always a fresh context (and the oracle) on
the final arrays."""
import collections
import functools

import numpy as np

import refit_ref as R
from rayzen_amd import _lib
from rayzen_amd import scene as S

W, H, SPP, BOUNCES = 64, 48, 2, 4
ASPECT = W / H
MAT, LIGHT, INST = S.BIND_MATERIALS, S.BIND_LIGHTS, S.BIND_INSTANCES
TLAS = (S.BIND_TLAS_NODES, S.BIND_TLAS_INDICES)
OFFSETS = ("blasNodeOffset", "blasTriOffset", "globalTriOffset")
AT_LEAST_FRESH = "at least fresh"
F32 = np.float32

# kind: "upload" (rz_upload), "update" (rz_update at `offset` bytes) or "frame" (a frame is rendered here, between two edits)
Call = collections.namedtuple("Call", "kind binding array offset", defaults=(None, None, 0))
FRAME = Call("frame")


class View:
    """Eight arrays and a camera: what helpers.oracle_render and test_refit_gpu._frame read of a scene.  `lights` is read for
    its length only, the frame's num_lights: the lights uploaded, or as many as `num_lights` says."""

    def __init__(self, arrays, camera, num_lights=None):
        self.arrays, self.camera, self.materials = arrays, camera, arrays[MAT]
        self.lights = arrays[LIGHT] if num_lights is None else range(num_lights)


class Base:
    """A base scene: its arrays, its camera, its parts for rz_build_geometry (meshes in the order of binding 0; objects as
    (mesh, transform)), where each mesh lies in binding 0, and the mesh the prior states deform (index into `ranges`)."""

    def __init__(self, name, arrays, camera, meshes, objects, deform):
        self.name, self.arrays, self.camera, self.meshes, self.objects, self.deform = name, arrays, camera, meshes, objects, deform
        first, self.ranges = 0, []
        for m in meshes:
            self.ranges.append((first, len(m)))
            first += len(m)

    def view(self, arrays=None, num_lights=None):
        return View(self.arrays if arrays is None else arrays, self.camera, num_lights)


def copy_arrays(arrays):
    return {b: a.copy() for b, a in arrays.items()}


def apply(calls, arrays):
    """What the calls leave in the eight bindings (the frames among them leave nothing)."""
    out = copy_arrays(arrays)
    for c in calls:
        if c.kind == "upload":
            out[c.binding] = np.ascontiguousarray(c.array).copy()
        elif c.kind == "update":
            raw = out[c.binding].view(np.uint8).copy()
            patch = np.ascontiguousarray(c.array).view(np.uint8).reshape(-1)
            assert c.offset + patch.size <= raw.size
            raw[c.offset:c.offset + patch.size] = patch
            out[c.binding] = raw.view(out[c.binding].dtype)
    return out


def steps(calls, arrays):
    """The arrays at every "frame" among the calls, then the final arrays."""
    out, cur, pending = [], arrays, []
    for c in calls:
        if c.kind == "frame":
            cur, pending = apply(pending, cur), []
            out.append(cur)
        else:
            pending.append(c)
    return out + [apply(pending, cur)]


# ---- the TLAS of an instance array, with the host library's own steps (SceneBuffers::build) ------------------------------

def tlas_for(arrays):
    inst, nodes = arrays[INST], arrays[S.BIND_BLAS_NODES]
    roots = np.zeros(len(inst), S.BVH_NODE)
    for i, it in enumerate(inst):
        r1 = nodes[int(it["blasNodeOffset"]):int(it["blasNodeOffset"]) + 1].copy()
        xf = np.ascontiguousarray(it["transform"], F32)
        mn, mx = np.zeros(3, F32), np.zeros(3, F32)
        _lib.host().rzh_world_bounds(r1.ctypes.data, xf.ctypes.data, mn.ctypes.data, mx.ctypes.data)
        roots[i] = r1[0]
        roots["boundsMin"][i], roots["boundsMax"][i] = mn, mx
    return S.build_tlas(roots)


def with_tlas(arrays):
    out = dict(arrays)
    out[S.BIND_TLAS_NODES], out[S.BIND_TLAS_INDICES] = tlas_for(arrays)
    return out


def instance_edit(arrays, k, transform=None, offsets_of=None, offsets=None):
    """The calls that replace instance record k -- its transform (and inverse), or its three offsets (those of instance
    `offsets_of`, or given) -- by rz_update at byte 144 * k, and upload the TLAS that follows."""
    inst = arrays[INST].copy()
    if transform is not None:
        xf = np.ascontiguousarray(transform, F32).reshape(16)
        inst["transform"][k], inst["inverseTransform"][k] = xf, S.inverse(xf)
    if offsets_of is not None:
        offsets = tuple(int(inst[offsets_of][f]) for f in OFFSETS)
    if offsets is not None:
        for f, v in zip(OFFSETS, offsets):
            inst[f][k] = v
    after = dict(arrays)
    after[INST] = inst
    tn, ti = tlas_for(after)
    return [Call("update", INST, inst[k:k + 1].copy(), 144 * k), Call("upload", TLAS[0], tn), Call("upload", TLAS[1], ti)]


# ---- base scenes ---------------------------------------------------------------------------------------------------------

def _split(tris, counts):
    return [a.copy() for a in np.split(tris, np.cumsum(counts)[:-1])]


def _from_scene(name, sc, counts, mesh_of_object, deform, arrays=None):
    arrays = copy_arrays(sc.arrays if arrays is None else arrays)
    inst = sc.arrays[INST]
    objects = [(m, np.asarray(inst[i]["transform"], F32).copy()) for i, m in enumerate(mesh_of_object)]
    return Base(name, arrays, sc.camera, _split(sc.arrays[S.BIND_TRIANGLES], counts), objects, deform)


GLASS_T = S.translate(S.identity(), (3.5, 0.6, 4.5))        # where the spare scene's third instance stands


def _spare_glass():
    """An opaque scene that HOLDS a glass mesh no instance names: bindings 0, 7 and 8 are those of the host library's build of
    (glass, floor, bunny) -- the glass first, so that it lies in front of every named mesh and rz_rebuild_geometry keeps it --
    and the instances are floor, bunny, and a second bunny at GLASS_T, written by hand with the TLAS that follows."""
    cam = S.Camera(position=(0.0, 2.5, 10.0), aspect=ASPECT)
    s = S.Scene(camera=cam)
    meshes = [S.make_blob(6, 1.2, 3, seed=7), S.make_cube(4), S.make_blob(12, 2.8, 0)]
    glass, floor, bunny = (s.add_mesh(m) for m in meshes)
    xf = [S.translate(S.scale(S.identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)), S.translate(S.identity(), (0.0, 2.0, 0.0)), GLASS_T]
    s.add_object(glass, GLASS_T)
    s.add_object(floor, xf[0])
    s.add_object(bunny, xf[1])
    s.build(share_meshes=True)
    named = s.arrays[INST]
    assert tuple(int(named[0][f]) for f in OFFSETS) == (0, 0, 0)
    inst = np.zeros(3, S.BVH_INSTANCE)
    for i, src in enumerate((1, 2, 2)):
        inst[i] = named[src]
        inst["meshIndex"][i] = i
        inst["transform"][i], inst["inverseTransform"][i] = xf[i], S.inverse(xf[i])
    arrays = copy_arrays(s.arrays)
    arrays[INST] = inst
    return Base("spare_glass", with_tlas(arrays), cam, meshes, [(1, xf[0]), (2, xf[1]), (2, xf[2])], 2)


def _opaque(arrays):
    out = copy_arrays(arrays)
    out[MAT]["transparency"][3] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def base(name):
    """The base scenes, all rendered at 64 x 48, 2 spp, bounce budget 4.  Treat what this returns as read-only."""
    if name in ("reference", "reference_opaque"):
        sc = S.reference_scene(aspect=ASPECT, mesh_n=9)       # 4 872 triangles, 7 instances each with its own mesh, material 3 glass
        arrays = _opaque(sc.arrays) if name == "reference_opaque" else None
        return _from_scene(name, sc, [12, 972, 972, 0, 972, 972, 972], range(7), 2, arrays)
    if name == "bunny":
        sc = S.bunny_scene(n=24, extras=True, aspect=ASPECT)  # floor (4), bunny (0), glass blob (3), mirror cube (2)
        return _from_scene(name, sc, [12, 6912, 432, 12], range(4), 1)
    if name == "instanced":
        sc = S.instanced_scene(n=24, aspect=ASPECT)           # 16 instances of one view
        return _from_scene(name, sc, [12, 6912], [0] + [1] * 16, 1)
    if name == "spare_glass":
        return _spare_glass()
    raise KeyError(name)


BASES = ("reference", "reference_opaque", "bunny", "instanced", "spare_glass")


# ---- the cases ------------------------------------------------------------------------------------------------------------

def _record(arrays, binding, k, **fields):
    rec = arrays[binding][k:k + 1].copy()
    for f, v in fields.items():
        rec[f][0] = v
    return rec


def _update(arrays, binding, k, **fields):
    return Call("update", binding, _record(arrays, binding, k, **fields), 32 * k)


def _m3(a):
    mats = a[MAT].copy()
    mats["transparency"][3], mats["transparency"][0] = 0.0, 0.9
    return [Call("upload", MAT, mats)]


def _m7a(a):
    grown = np.concatenate([a[MAT], a[MAT][:1]])
    return [Call("upload", MAT, grown), _update({MAT: grown}, MAT, len(grown) - 1, transparency=0.9, albedo=(0.1, 0.2, 0.9))]


def _m7b(a):
    mats = a[MAT][:-1].copy()
    mats["albedo"][0] = (0.2, 0.3, 0.9)
    return [Call("upload", MAT, mats)]


def _l3b(a):
    lights = np.concatenate([a[LIGHT], a[LIGHT][:1]])
    lights[2] = ((-4.0, 6.0, 2.0, 1.0), (1.0, 0.6, 0.3), 200.0)
    return [Call("upload", LIGHT, lights)]


I1_T = S.scale(S.rotate(S.translate(S.identity(), (-1.0, 1.5, 3.0)), 0.7, (0.0, 1.0, 0.0)), (0.7, 0.7, 0.7))

Case = collections.namedtuple("Case", "base edit changes_frame transparent why num_lights oracle", defaults=(None, True))

CASES = {
    # -- materials
    "M1": Case("reference_opaque", lambda a: [_update(a, MAT, 1, transparency=0.9)], True, 1,
               "an opaque scene's used material turns to glass by rz_update of its one record: the kernel variant must follow"),
    "M2": Case("bunny", lambda a: [_update(a, MAT, 3, transparency=0.0)], True, 0,
               "the only glass material turns opaque: the variant, its LDS plan and its scratch go back"),
    "M3": Case("reference", _m3, True, 1,
               "glass moves from material 3 to material 0 in one rz_upload: every per-view hint of layout time is wrong, both ways"),
    "M4": Case("reference_opaque", lambda a: [_update(a, MAT, 1, transparency=0.9), FRAME,
                                               _update(a, MAT, 1, transparency=0.0, albedo=(0.2, 0.2, 0.9), metallic=0.0)], True, 0,
               "a second material edit under one layout: matChangedSinceLayout is already set, no instance rebuild is asked for"),
    "M5": Case("reference", lambda a: [_update(a, MAT, 0, albedo=(0.2, 0.8, 0.9), roughness=0.3, metallic=0.5),
                                        _update(a, MAT, 1, reflectivity=1.0)], True, 1,
               "no transparency change: albedo, roughness, metallic; a second material becomes a perfect mirror for the see-through chains"),
    "M6": Case("reference_opaque", lambda a: [_update(a, MAT, 1, transparency=np.nan, albedo=(0.9, 0.6, 0.1))], True, 1,
               "transparency = NaN counts as transparent on the host (!(x == x)); the device re-check must agree (recoloured too: NaN alone moves no pixel)",
               None, False),
    "M7a": Case("reference_opaque", _m7a, False, 0,
                "the material array grows by an unused record, which then turns to glass: dMat grows, nothing laid out is glass"),
    "M7b": Case("reference", _m7b, True, 1,
                "the material array loses its last, unused record (and material 0 its colour): K.nMaterials moves under the guides' clamp"),
    # -- lights
    "L1": Case("reference", lambda a: [_update(a, LIGHT, 1, positionOrDirection=(-0.6, 1.0, 0.8, 0.0), color=(1.0, 0.5, 0.2), power=3.5)],
               True, 1, "rz_update of light 1 at byte 32: direction, colour, power"),
    "L2": Case("reference", lambda a: [_update(a, LIGHT, 0, positionOrDirection=(5.0, 5.0, 5.0, 0.0))], True, 1,
               "a point light becomes directional (w 1 -> 0)"),
    "L3a": Case("reference", lambda a: [Call("upload", LIGHT, a[LIGHT][1:2].copy())], True, 1,
                "the light array re-uploaded shorter than frame.num_lights, light 1 now first: the clamp at launch", 2),
    "L3b": Case("reference", _l3b, True, 1, "the light array re-uploaded longer, num_lights following", 3),
    "L4": Case("reference", lambda a: [_update(a, LIGHT, 0, power=0.0), FRAME, _update(a, LIGHT, 0)], False, 1,
               "a light's power goes to 0 and comes back: what the shadow-query skip was written for"),
    # -- instances / TLAS
    "I1": Case("instanced", lambda a: instance_edit(a, 5, transform=I1_T), True, 0,
               "rz_update of one instance record at a non-zero offset (transform and inverse), TLAS re-uploaded"),
    "I2": Case("instanced", lambda a: instance_edit(a, 14, offsets_of=0), True, 0,
               "an instance re-pointed to another mesh that is already laid out: its three offsets change"),
    "I3": Case("spare_glass", lambda a: instance_edit(a, 2, offsets=(0, 0, 0)), True, 1,
               "an instance re-pointed to the glass mesh nobody named: the view is laid out lazily, glass arrives by an instance edit alone"),
    "I4": Case("spare_glass", lambda a: instance_edit(a, 2, offsets=(0, 0, 0)) + [FRAME] + instance_edit(a, 2, offsets_of=1), False,
               AT_LEAST_FRESH, "I3 undone: a fresh context never lays the glass view out; the flag may stay, the pixels may not differ"),
}

MAX_UNCHANGED = 3           # cases whose final frame equals the base's: M7a, I4, L4

# what also runs in the prior states S1 .. S5 of tests/test_scene_edits_gpu.py, and what a geometry call follows
IN_PRIOR_STATES = ("M1", "M2", "L1", "I1", "I3")
BEFORE_GEOMETRY_CALLS = ("M2", "M4", "I3")
AFTER_A_READ_BACK = ("M1", "I1", "I3")          # in S1 .. S4, once rz_read_binding has refreshed every host copy


def case_arrays(name, arrays=None):
    """(base, calls, before, [arrays at each frame among the calls ..., final])."""
    c = CASES[name]
    b = base(c.base)
    before = b.arrays if arrays is None else arrays
    calls = c.edit(before)
    return b, calls, before, steps(calls, before)


def num_lights(name, before):
    n = CASES[name].num_lights
    return len(before[LIGHT]) if n is None else n


# ---- what the prior states do to a base scene ------------------------------------------------------------------------------

AMPLITUDE = 0.1             # of refit_ref.wobble, on meshes 1.4 to 2.8 units in radius


def moved_transforms(b, again=False):
    """The transforms S1 hands to rz_update_transforms: every object but the floor moves a little, away from the camera.
    `again`: other ones, for a second rz_update_transforms (the objects move the other way, and further)."""
    d = (-0.5, 0.25, -0.4) if again else (0.3, 0.1, 0.2)
    out = []
    for k, (_, xf) in enumerate(b.objects):
        out.append(np.asarray(xf, F32) if k == 0 else S.translate(xf, (d[0], d[1] + 0.02 * k, d[2])))
    return np.stack(out)


def moved_arrays(b, again=False):
    """Scene.set_transform of every object and Scene.update_dynamic, on arrays."""
    out = copy_arrays(b.arrays)
    for k, xf in enumerate(moved_transforms(b, again)):
        out[INST]["transform"][k], out[INST]["inverseTransform"][k] = xf, S.inverse(xf)
    return with_tlas(out)


def deformed(b, again=False):
    """(first triangle, moved triangles) of the mesh S3 and S4 refit.  `again`: another deformation of it, for a second refit."""
    return b.ranges[b.deform][0], R.wobble(b.meshes[b.deform], -1.5 * AMPLITUDE if again else AMPLITUDE)


# ---- the host partners of the geometry calls, on arrays ------------------------------------------------------------------

def _named(arrays):
    """The distinct (node offset, index offset, triangle offset) among the instances, ascending, with each one's node extent."""
    keys = sorted(set(tuple(int(i[f]) for f in OFFSETS) for i in arrays[INST]))
    ends = [k[0] for k in keys[1:]] + [len(arrays[S.BIND_BLAS_NODES])]
    return [(k, e) for k, e in zip(keys, ends)]


def refit_arrays(arrays, first, moved):
    """Scene.refit_mesh on arrays: `moved` replace the mesh that starts at triangle `first`; its boxes follow (rzh_refit_blas),
    then the world boxes and the TLAS."""
    out = copy_arrays(arrays)
    n = len(moved)
    out[S.BIND_TRIANGLES][first:first + n] = moved
    for (off, t0, g0), end in _named(arrays):
        if g0 == first and end - off > 1:
            out[S.BIND_BLAS_NODES][off:end] = S.refit_blas(moved, arrays[S.BIND_BLAS_NODES][off:end], arrays[S.BIND_BLAS_INDICES][t0:t0 + n])
    return with_tlas(out)


def rebuild_arrays(b, arrays):
    """Scene.rebuild_mesh of every mesh with triangles, on arrays: a fresh BLAS each (rzh_build_blas), later meshes moved in
    binding 7, the instances' node offsets patched, then the world boxes and the TLAS."""
    out = copy_arrays(arrays)
    nodes, idx = arrays[S.BIND_BLAS_NODES], out[S.BIND_BLAS_INDICES]
    named = _named(arrays)
    parts, moved, at = [nodes[:named[0][0][0]]], {}, named[0][0][0]
    for (off, t0, g0), end in named:
        n = dict(b.ranges)[g0] if end - off > 1 else 0
        moved[off] = at
        if n:
            fresh, order, _ = S.build_blas(arrays[S.BIND_TRIANGLES][g0:g0 + n])
            idx[t0:t0 + n] = order
        else:
            fresh = nodes[off:end]
        parts.append(fresh)
        at += len(fresh)
    out[S.BIND_BLAS_NODES] = np.concatenate(parts)
    out[INST]["blasNodeOffset"] = [moved[int(o)] for o in arrays[INST]["blasNodeOffset"]]
    return with_tlas(out)

"""Host-side scene assembly (Python view of rayzen_amd/csrc/host).

Mirrors how RayZen's main.cpp builds its scene (RayZen/src/main.cpp:327-388):
materials, lights, camera, meshes, GameObjects with a transform each, then
`build()` = initializeSSBOs (main.cpp:941-1035) producing the six geometry
arrays, and `update_dynamic()` = updateDynamicBVHAndSSBOs (main.cpp:1138-1194).
All geometry work happens in librayzen_host.so (C++); this module only moves
numpy arrays in and out.
"""
import ctypes as C

import numpy as np

from . import _lib

# SSBO element types (include/rayzen_hip.h; RayZen/include/{Mesh,BVH,Material,Light}.h)
TRIANGLE = np.dtype([("v0", "<f4", 3), ("pad0", "<f4"), ("v1", "<f4", 3), ("pad1", "<f4"),
                     ("v2", "<f4", 3), ("pad2", "<f4"), ("materialIndex", "<i4"), ("tail_pad", "<i4", 3)])
SKIN_TRIANGLE = np.dtype([("bones", "<u4", 3), ("pad", "<u4"), ("weights", "<f4", (3, 4))])      # rz_skin_triangle
MORPH_TRIANGLE = np.dtype([("d", "<f4", (3, 4))])                                                   # rz_morph_triangle
BVH_NODE = np.dtype([("boundsMin", "<f4", 3), ("leftFirst", "<i4"), ("boundsMax", "<f4", 3), ("count", "<i4")])
BVH_INSTANCE = np.dtype([("blasNodeOffset", "<i4"), ("blasTriOffset", "<i4"), ("meshIndex", "<i4"),
                         ("globalTriOffset", "<i4"), ("transform", "<f4", 16), ("inverseTransform", "<f4", 16)])
MATERIAL = np.dtype([("albedo", "<f4", 3), ("metallic", "<f4"), ("roughness", "<f4"),
                     ("reflectivity", "<f4"), ("transparency", "<f4"), ("ior", "<f4")])
LIGHT = np.dtype([("positionOrDirection", "<f4", 4), ("color", "<f4", 3), ("power", "<f4")])

BIND_TRIANGLES, BIND_MATERIALS, BIND_LIGHTS = 0, 1, 2
BIND_TLAS_NODES, BIND_TLAS_INDICES, BIND_BLAS_NODES, BIND_BLAS_INDICES, BIND_INSTANCES = 5, 6, 7, 8, 9
BINDING_DTYPES = {BIND_TRIANGLES: TRIANGLE, BIND_MATERIALS: MATERIAL, BIND_LIGHTS: LIGHT,
                  BIND_TLAS_NODES: BVH_NODE, BIND_TLAS_INDICES: np.dtype("<i4"), BIND_BLAS_NODES: BVH_NODE,
                  BIND_BLAS_INDICES: np.dtype("<i4"), BIND_INSTANCES: BVH_INSTANCE}
GEOMETRY_BINDINGS = (BIND_TRIANGLES, BIND_TLAS_NODES, BIND_TLAS_INDICES, BIND_BLAS_NODES, BIND_BLAS_INDICES,
                     BIND_INSTANCES)


def _p(a):
    return a.ctypes.data


def identity():
    return np.eye(4, dtype=np.float32).reshape(16).copy()   # column-major == row-major for I


def _mat_op(fn, m, *args):
    m = np.ascontiguousarray(m, np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    fn(_p(m), *args, _p(out))
    return out


def translate(m, v):
    """glm::translate(m, v) = m * T(v); column-major 16 floats."""
    v = np.asarray(v, np.float32).copy()
    return _mat_op(_lib.host().rzh_mat_translate, m, _p(v))


def scale(m, v):
    v = np.asarray(v, np.float32).copy()
    return _mat_op(_lib.host().rzh_mat_scale, m, _p(v))


def rotate(m, angle, axis):
    axis = np.asarray(axis, np.float32).copy()
    m = np.ascontiguousarray(m, np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    _lib.host().rzh_mat_rotate(_p(m), float(angle), _p(axis), _p(out))
    return out


def inverse(m):
    m = np.ascontiguousarray(m, np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    _lib.host().rzh_mat_inverse(_p(m), _p(out))
    return out


def load_obj(path, material_index):
    """Mesh::loadFromOBJ (RayZen/src/Mesh.cpp:6-50)."""
    import os
    L = _lib.host()
    p = os.fsencode(path)
    n = L.rzh_load_obj(p, material_index, None, 0)
    if n < 0:
        raise FileNotFoundError(path)
    tris = np.zeros(n, TRIANGLE)
    L.rzh_load_obj(p, material_index, _p(tris), n)
    return tris


def make_cube(material_index):
    tris = np.zeros(12, TRIANGLE)
    _lib.host().rzh_make_cube(material_index, _p(tris), 12)
    return tris


def make_blob(n, radius, material_index, seed=1):
    """Closed 12*n*n-triangle 'bunny' stand-in (include/rayzen_host.h)."""
    total = 12 * n * n
    tris = np.zeros(total, TRIANGLE)
    got = _lib.host().rzh_make_blob(n, float(radius), seed, material_index, _p(tris), total)
    assert got == total
    return tris


def make_quad(p0, p1, p2, p3, material_index):
    """Two triangles (p0,p1,p2), (p0,p2,p3)."""
    t = np.zeros(2, TRIANGLE)
    t["v0"][0], t["v1"][0], t["v2"][0] = p0, p1, p2
    t["v0"][1], t["v1"][1], t["v2"][1] = p0, p2, p3
    t["materialIndex"] = material_index
    return t


def build_blas(tris):
    """BVH::buildBLAS (RayZen/src/BVH.cpp:99-175). Returns (nodes, indices, depth)."""
    tris = np.ascontiguousarray(tris)
    assert tris.dtype.itemsize == 64
    n = tris.shape[0]
    nodes = np.zeros(2 * max(n, 1) + 1, BVH_NODE)
    idx = np.zeros(max(n, 1), np.int32)
    depth = C.c_int(0)
    nn = _lib.host().rzh_build_blas(_p(tris) if n else None, n, _p(nodes), _p(idx), C.byref(depth))
    if nn < 0:
        raise RuntimeError("rzh_build_blas failed")
    return nodes[:nn].copy(), idx[:n].copy(), depth.value


def refit_blas(tris, nodes, idx):
    """BVH::refit (librayzen_host.so: rzh_refit_blas): the boxes of `nodes` recomputed bottom-up from the moved `tris` (the
    mesh's triangles in their original order); topology and `idx` kept.  Returns the refitted copy of `nodes`."""
    tris = np.ascontiguousarray(tris)
    assert tris.dtype.itemsize == 64
    out = np.ascontiguousarray(nodes, BVH_NODE).copy()
    idx = np.ascontiguousarray(idx, np.int32)
    n = tris.shape[0]
    if _lib.host().rzh_refit_blas(_p(tris) if n else None, n, _p(out), out.shape[0], _p(idx) if n else None) != 0:
        raise RuntimeError("rzh_refit_blas failed (inconsistent arrays)")
    return out


def sah_cost(nodes):
    """BVH::sahCost (librayzen_host.so: rzh_blas_sah_cost): the SAH cost of one BLAS over the nodes its root reaches, as
    include/rayzen_hip.h states it for rz_geometry_quality.  The host partner of Renderer.geometry_quality."""
    nodes = np.ascontiguousarray(nodes, BVH_NODE)
    cost = _lib.host().rzh_blas_sah_cost(_p(nodes) if nodes.shape[0] else None, nodes.shape[0])
    if cost < 0:
        raise RuntimeError("rzh_blas_sah_cost failed (the nodes do not form a tree)")
    return cost


def pack_bones(indices):
    """Four 8-bit bone indices per corner -> the words of SKIN_TRIANGLE["bones"]: indices[..., j] goes to bits 8j..8j+7."""
    b = np.asarray(indices).astype(np.uint32)
    assert b.shape[-1] == 4 and (b < 256).all()
    return (b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (b[..., 3] << 24)).astype(np.uint32)


def skin_triangles(rest, skin=None, bones=None, morphs=None, morph_weights=None):
    """Mesh::skin (librayzen_host.so: rzh_skin_triangles): `rest` posed by linear-blend skinning (skin: SKIN_TRIANGLE per
    triangle, bones: n_bones x 16 column-major) and / or morph targets (morphs: MORPH_TRIANGLE [n_morphs, n], morph_weights).
    The byte partner of Renderer.skin_pose; its result is what Scene.refit_mesh takes."""
    rest = np.ascontiguousarray(rest, TRIANGLE)
    n = rest.shape[0]
    out = np.zeros(n, TRIANGLE)
    sk = bn = mo = mw = None
    n_bones = n_morphs = 0
    if skin is not None:
        sk = np.ascontiguousarray(skin, SKIN_TRIANGLE)
        bn = np.ascontiguousarray(bones, np.float32).reshape(-1, 16)
        n_bones = bn.shape[0]
        assert sk.shape == (n,)
    if morphs is not None and len(morphs):
        mo = np.ascontiguousarray(morphs, MORPH_TRIANGLE).reshape(-1, n)
        mw = np.ascontiguousarray(morph_weights, np.float32).reshape(-1)
        n_morphs = mo.shape[0]
        assert mw.shape[0] == n_morphs
    rc = _lib.host().rzh_skin_triangles(_p(rest) if n else None, None if sk is None else _p(sk), n, None if bn is None else _p(bn), n_bones,
                                        None if mo is None or not n else _p(mo), None if mw is None else _p(mw), n_morphs, _p(out) if n else None)
    if rc != 0:
        raise RuntimeError("rzh_skin_triangles: " + ("a kept influence names a bone outside the table" if rc == -2 else "inconsistent arguments"))
    return out


def build_tlas(world_roots):
    r = np.ascontiguousarray(world_roots)
    assert r.dtype.itemsize == 32
    n = r.shape[0]
    nodes = np.zeros(2 * max(n, 1), BVH_NODE)
    idx = np.zeros(max(n, 1), np.int32)
    ni = C.c_int(0)
    nn = _lib.host().rzh_build_tlas(_p(r) if n else None, n, _p(nodes), _p(idx), C.byref(ni))
    if nn < 0:
        raise RuntimeError("rzh_build_tlas failed")
    return nodes[:nn].copy(), idx[:ni.value].copy()


# RayZen's materials (main.cpp:342-353) and lights (main.cpp:356-357)
def reference_materials():
    m = np.zeros(5, MATERIAL)
    rows = [((0.8, 0.3, 0.3), 0.0, 1.0, 0.0, 0.0, 1.5),      # 0 red matte
            ((0.1, 0.7, 0.1), 1.0, 0.35, 0.3, 0.0, 1.5),     # 1 green metallic
            ((1.0, 1.0, 1.0), 1.0, 0.05, 1.0, 0.0, 1.5),     # 2 mirror
            ((0.85, 0.95, 1.0), 0.0, 0.02, 0.05, 0.94, 1.5),  # 3 glass
            ((0.6, 0.4, 0.2), 0.0, 0.9, 0.2, 0.0, 1.5)]      # 4 rough
    for i, (alb, met, rough, refl, transp, ior) in enumerate(rows):
        m[i] = (alb, met, rough, refl, transp, ior)
    return m


def reference_lights():
    l = np.zeros(2, LIGHT)
    l[0] = ((5.0, 5.0, 5.0, 1.0), (1.0, 1.0, 1.0), 300.0)   # point light
    l[1] = ((0.8, 1.4, 0.3, 0.0), (1.0, 1.0, 1.0), 2.0)     # directional
    return l


class Camera:
    """include/Camera.h: position, target (a direction), up, fov in degrees."""

    def __init__(self, position=(0.0, 0.0, 3.0), target=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=70.0,
                 aspect=800.0 / 600.0, near=0.1, far=100.0):
        self.position = np.asarray(position, np.float32).copy()
        self.target = np.asarray(target, np.float32).copy()
        self.up = np.asarray(up, np.float32).copy()
        self.fov, self.aspect, self.near, self.far = float(fov), float(aspect), float(near), float(far)
        self.update()

    def update(self):
        self.view, self.proj = np.zeros(16, np.float32), np.zeros(16, np.float32)
        self.inv_view, self.inv_proj = np.zeros(16, np.float32), np.zeros(16, np.float32)
        _lib.host().rzh_camera_matrices(_p(self.position), _p(self.target), _p(self.up), self.fov, self.aspect,
                                        self.near, self.far, _p(self.view), _p(self.proj), _p(self.inv_view),
                                        _p(self.inv_proj))


class Scene:
    """Scene + its SSBO arrays.  `arrays` maps binding index -> numpy array."""

    def __init__(self, materials=None, lights=None, camera=None):
        self._h = _lib.host().rzh_scene_create()
        if not self._h:
            raise MemoryError("rzh_scene_create")
        self.materials = reference_materials() if materials is None else np.ascontiguousarray(materials)
        self.lights = reference_lights() if lights is None else np.ascontiguousarray(lights)
        self.camera = camera or Camera()
        self.arrays = {}
        self.max_blas_depth = self.tlas_depth = 0
        self.name = ""

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.host().rzh_scene_destroy(h)

    def add_mesh(self, tris):
        tris = np.ascontiguousarray(tris)
        assert tris.dtype.itemsize == 64
        mid = _lib.host().rzh_scene_add_mesh(self._h, _p(tris) if tris.shape[0] else None, tris.shape[0])
        if mid < 0:
            raise RuntimeError("rzh_scene_add_mesh failed")
        return mid

    def add_object(self, mesh_id, transform=None):
        t = identity() if transform is None else np.ascontiguousarray(transform, np.float32).reshape(16)
        oid = _lib.host().rzh_scene_add_object(self._h, mesh_id, _p(t))
        if oid < 0:
            raise RuntimeError("rzh_scene_add_object failed")
        return oid

    def set_transform(self, object_id, transform):
        t = np.ascontiguousarray(transform, np.float32).reshape(16)
        if _lib.host().rzh_scene_set_transform(self._h, object_id, _p(t)) != 0:
            raise RuntimeError("rzh_scene_set_transform failed")

    def _pull(self, bindings):
        L = _lib.host()
        for b in bindings:
            nbytes = C.c_size_t(0)
            ptr = L.rzh_scene_buffer(self._h, b, C.byref(nbytes))
            dt = BINDING_DTYPES[b]
            n = nbytes.value // dt.itemsize
            if n:
                buf = (C.c_char * nbytes.value).from_address(ptr)
                self.arrays[b] = np.frombuffer(buf, dtype=dt, count=n).copy()
            else:
                self.arrays[b] = np.zeros(0, dt)
        self.arrays[BIND_MATERIALS] = self.materials
        self.arrays[BIND_LIGHTS] = self.lights
        bd, td = C.c_int(0), C.c_int(0)
        L.rzh_scene_depths(self._h, C.byref(bd), C.byref(td))
        self.max_blas_depth, self.tlas_depth = bd.value, td.value

    def set_blas_builder(self, renderer):
        """Build every BLAS of build() with renderer's device builder (rz_build_blas; same bytes as the host builder).
        None restores the host builder.  The renderer must outlive the scene's build() calls."""
        if renderer is None:
            fn, ctx = None, None
        else:
            fn, ctx = C.cast(renderer._L.rz_build_blas, C.c_void_p), renderer._c
        if _lib.host().rzh_scene_set_blas_builder(self._h, fn, ctx) != 0:
            raise RuntimeError("rzh_scene_set_blas_builder failed")

    def build(self, share_meshes=False):
        rc = _lib.host().rzh_scene_build(self._h, 1 if share_meshes else 0)
        if rc == -2:
            raise RuntimeError("rzh_scene_build: the device BLAS builder failed")
        if rc != 0:
            raise RuntimeError("rzh_scene_build failed")
        self._pull(GEOMETRY_BINDINGS)
        return self

    def save_cache(self, directory):
        """Write RayZen's ssbo_v2_*.bin cache files (main.cpp:1037-1043)."""
        import os
        os.makedirs(directory, exist_ok=True)
        if _lib.host().rzh_scene_save_cache(self._h, os.fsencode(directory)) != 0:
            raise OSError(f"cannot write the scene cache to {directory}")

    def load_cache(self, directory):
        """Read RayZen's ssbo_v2_*.bin cache files (main.cpp:914-939) in place of build()."""
        import os
        if _lib.host().rzh_scene_load_cache(self._h, os.fsencode(directory)) != 0:
            raise OSError(f"no usable scene cache in {directory}")
        self._pull(GEOMETRY_BINDINGS)
        return self

    def build_cached(self, directory, force_rebuild=False):
        """initializeSSBOs with RayZen's whole disk cache (main.cpp:897-1060): `directory` stands for bvh_cache/v2/.
        Returns what was found: dict(ssbo_loaded, ssbo_invalidated, blas_loaded, blas_built, tlas_loaded)."""
        import os
        rep = (C.c_int * 5)()
        rc = _lib.host().rzh_scene_build_cached(self._h, os.fsencode(directory), 1 if force_rebuild else 0, C.byref(rep))
        if rc != 0:
            raise RuntimeError(f"rzh_scene_build_cached failed ({rc})")
        self._pull(GEOMETRY_BINDINGS)
        self.cache_report = dict(ssbo_loaded=bool(rep[0]), ssbo_invalidated=bool(rep[1]), blas_loaded=rep[2],
                                 blas_built=rep[3], tlas_loaded=bool(rep[4]))
        return self

    def refit_mesh(self, mesh_id, tris):
        """A mesh's vertices moved: `tris` replace its triangles (same count), every stored copy is refitted (BVH::refit), and
        the world boxes and the TLAS are rebuilt with the transforms in force.  The host partner of Renderer.refit_geometry."""
        tris = np.ascontiguousarray(tris)
        assert tris.dtype.itemsize == 64
        if _lib.host().rzh_scene_refit_mesh(self._h, int(mesh_id), _p(tris) if tris.shape[0] else None, tris.shape[0]) != 0:
            raise RuntimeError("rzh_scene_refit_mesh failed (unknown mesh, or its triangle count changed)")
        self._pull(GEOMETRY_BINDINGS)
        return self

    def rebuild_mesh(self, mesh_id):
        """A refitted mesh gets a fresh BLAS of its current triangles in every stored copy; bindings 7, 8 and 9 are patched (a
        rebuilt tree has another node count, so later meshes move) and the world boxes and the TLAS are rebuilt with the
        transforms in force.  The host partner of Renderer.rebuild_geometry."""
        if _lib.host().rzh_scene_rebuild_mesh(self._h, int(mesh_id)) != 0:
            raise RuntimeError("rzh_scene_rebuild_mesh failed (unknown mesh)")
        self._pull(GEOMETRY_BINDINGS)
        return self

    def update_dynamic(self):
        if _lib.host().rzh_scene_update_dynamic(self._h) != 0:
            raise RuntimeError("rzh_scene_update_dynamic failed")
        self._pull((BIND_INSTANCES, BIND_TLAS_NODES, BIND_TLAS_INDICES))
        return self


# --------------------------------------------------------------------------
# The benchmark / parity configurations of BASELINE.json.
# No asset file is needed: the "bunny" is the procedural blob of rzh_make_blob.
# --------------------------------------------------------------------------

def cornell_scene():
    """C1: floor quad + back-wall quad + cube = 16 triangles, 3 instances."""
    s = Scene(camera=Camera(position=(0.0, 0.5, 4.5), aspect=1.0))
    floor = s.add_mesh(make_quad((-4, -1.5, 4), (4, -1.5, 4), (4, -1.5, -4), (-4, -1.5, -4), 4))
    wall = s.add_mesh(make_quad((-4, -1.5, -3), (4, -1.5, -3), (4, 4.5, -3), (-4, 4.5, -3), 1))
    cube = s.add_mesh(make_cube(0))
    s.add_object(floor)
    s.add_object(wall)
    s.add_object(cube, rotate(translate(identity(), (0.3, -0.5, 0.0)), 0.6, (0.0, 1.0, 0.0)))
    s.name = "cornell16"
    return s.build()


def fit_mesh(tris, radius):
    """Centre an OBJ mesh on the origin and scale its VERTICES so that its largest half-extent is `radius`.  The scale
    has to go into the vertices, not the instance transform: the shader's determinant cull |a| < 1e-4 (FS:396) works in
    object space, and a raw Stanford bunny (0.15 units across) would be culled triangle by triangle."""
    t = tris.copy()
    v = np.stack([t["v0"], t["v1"], t["v2"]], axis=1).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    centre = ((lo + hi) * np.float32(0.5)).astype(np.float32)
    k = np.float32(radius) / np.float32(max(float((hi - lo).max()) * 0.5, 1e-20))
    for f in ("v0", "v1", "v2"):
        t[f] = ((t[f] - centre) * k).astype(np.float32)
    return t


def bunny_scene(n=76, aspect=16.0 / 9.0, bunny_material=0, floor_material=4, extras=False, radius=2.8, blas_builder=None,
                obj_path=None, camera_position=(0.0, 2.5, 10.0)):
    """C2/C3: ~69k-triangle closed mesh over the reference's floor: the procedural 'bunny' stand-in (12*n*n triangles)
    or, with obj_path, a real OBJ (e.g. the Stanford bunny dropped into assets/bunny.obj) read
    with RayZen's loader quirks (Mesh.cpp:6-50) and fitted to the same radius.

    extras adds a glass blob and a mirror cube so every material branch is exercised.
    camera_position: the default frames the whole mesh from 10 units away (64 % of the camera paths see only sky);
    CLOSE_CAMERA stands 0.9 units outside the mesh, which then covers most of the frame (bench_configs.py: c2close)."""
    s = Scene(camera=Camera(position=tuple(camera_position), aspect=aspect))
    floor = s.add_mesh(make_cube(floor_material))
    if obj_path:
        mesh = fit_mesh(load_obj(obj_path, bunny_material), radius)
    else:
        mesh = make_blob(n, radius, bunny_material)
    bunny = s.add_mesh(mesh)
    # main.cpp:378: translate(scale(I, (8, .5, 8)), (0, -3, 0))
    s.add_object(floor, translate(scale(identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.add_object(bunny, translate(identity(), (0.0, 2.0, 0.0)))
    if extras:
        glass = s.add_mesh(make_blob(max(4, n // 4), 1.2, 3, seed=7))
        mirror = s.add_mesh(make_cube(2))
        s.add_object(glass, translate(identity(), (4.5, 0.6, 3.0)))
        s.add_object(mirror, rotate(translate(identity(), (-5.0, 0.0, 1.5)), 0.5, (0.0, 1.0, 0.0)))
    s.name = (f"obj:{len(mesh)}" if obj_path else f"bunny{12 * n * n}") + ("+glass+mirror" if extras else "")
    s.set_blas_builder(blas_builder)        # a Renderer: BLAS built on the device (same bytes); None: host builder
    return s.build()


CLOSE_CAMERA = (0.0, 2.2, 3.7)     # looks down -z like the default camera (RayZen's conventions: main.cpp:331-339)


def instanced_transforms(frame, count=16, spacing=3.0, obj_scale=0.4):
    """C4: 4x4 grid, transform_i(frame) = translate * rotateY(0.1*frame + i) * scale."""
    side = int(round(count ** 0.5))
    out = []
    for i in range(count):
        gx, gz = i % side, i // side
        t = translate(identity(), ((gx - (side - 1) / 2.0) * spacing, 0.4, (gz - (side - 1) / 2.0) * spacing))
        t = rotate(t, 0.1 * frame + i, (0.0, 1.0, 0.0))
        out.append(scale(t, (obj_scale, obj_scale, obj_scale)))
    return out


def instanced_scene(n=76, count=16, aspect=16.0 / 9.0, share_meshes=True):
    """C4: `count` instances of the bunny mesh over the floor; per-frame TLAS rebuild via set_transform + update_dynamic."""
    s = Scene(camera=Camera(position=(0.0, 5.0, 12.0), target=(0.0, -0.35, -1.0), aspect=aspect))
    floor = s.add_mesh(make_cube(4))
    bunny = s.add_mesh(make_blob(n, 2.8, 0))
    s.add_object(floor, translate(scale(identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.instance_ids = [s.add_object(bunny, t) for t in instanced_transforms(0, count)]
    s.name = f"instanced{count}x{12 * n * n}"
    return s.build(share_meshes=share_meshes)


def stress_scene(n=289, aspect=16.0 / 9.0, blas_builder=None):
    """C5: ~1M-triangle blob, radius 10."""
    s = Scene(camera=Camera(position=(0.0, 6.0, 34.0), aspect=aspect))
    floor = s.add_mesh(make_cube(4))
    blob = s.add_mesh(make_blob(n, 10.0, 0))
    s.add_object(floor, translate(scale(identity(), (40.0, 0.5, 40.0)), (0.0, -28.0, 0.0)))
    s.add_object(blob, identity())
    s.name = f"stress{12 * n * n}"
    s.set_blas_builder(blas_builder)
    return s.build()


SUZANNE_HALF_EXTENTS = (1.367188, 0.984375, 0.851563)     # the AABB of RayZen/meshes/monkey.obj (507 vertices, 968 triangles), symmetric about 0


def fit_to_box(tris, half_extents):
    """Scale a mesh per axis so that its AABB is exactly +-half_extents about its own centre, moved to the origin."""
    t = tris.copy()
    pts = np.stack([t["v0"], t["v1"], t["v2"]]).reshape(-1, 3).astype(np.float64)
    lo, hi = pts.min(0), pts.max(0)
    c, k = (lo + hi) / 2.0, np.asarray(half_extents, np.float64) / ((hi - lo) / 2.0)
    for f in ("v0", "v1", "v2"):
        t[f] = ((t[f].astype(np.float64) - c) * k).astype(np.float32)
    return t


def camera_clearance(scene):
    """Distance from the camera to the nearest instance WORLD box (main.cpp:974-993), 0 if it lies inside one.  RayZen's
    camera stands outside every object of its scene; a stand-in mesh that swallows it renders a different frame (round 4's
    `ref` rows did: VERDICT r4)."""
    inst, nodes = scene.arrays[BIND_INSTANCES], scene.arrays[BIND_BLAS_NODES]
    cam = np.asarray(scene.camera.position, np.float64)
    best = np.inf
    for it in inst:
        root = nodes[int(it["blasNodeOffset"])]
        if int(root["count"]) == 0 and int(root["leftFirst"]) == 0 and not np.all(np.isfinite(root["boundsMin"])):
            continue
        lo, hi = np.asarray(root["boundsMin"], np.float64), np.asarray(root["boundsMax"], np.float64)
        if np.any(lo > hi):             # the empty mesh's inverted root box (BVH.cpp:115-118)
            continue
        m = np.asarray(it["transform"], np.float64).reshape(4, 4).T      # column-major -> row-major
        corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]) @ m.T
        wlo, whi = corners[:, :3].min(0), corners[:, :3].max(0)
        d = np.maximum(np.maximum(wlo - cam, cam - whi), 0.0)
        best = min(best, float(np.sqrt((d * d).sum())))
    return best


def reference_scene(aspect=800.0 / 600.0, mesh_n=9, include_empty=True, monkey_obj=None):
    """RayZen's own scene (RayZen/src/main.cpp:331-384): camera (0, 0, 3) looking down -z, fov 70; the five materials and
    two lights of main.cpp:342-357; seven GameObjects, each with its OWN mesh (main.cpp:360-374 loads one Mesh per object,
    so nothing is shared): the cube floor scaled (8, .5, 8) at y = -3, five ~1 k-triangle meshes -- materials 1 (green
    metal), 2 (mirror), 0, 0 and 3 (GLASS, scaled 1.2) -- and one EMPTY mesh (`car.obj` is absent from the reference's
    meshes/, Mesh.cpp:8-11 logs an error and leaves the mesh empty).  monkey.obj (968 triangles) cannot travel to the GPU
    box, so the stand-in is the 12 * mesh_n^2 = 972-triangle blob scaled per axis to SUZANNE'S EXTENTS (+-1.367, +-0.984,
    +-0.852): the camera at z = 3 then stands 0.148 in front of the mesh at (0, 0, 4) and looks AWAY from it, as in RayZen's
    frame -- half sky above a 16 x 16 floor, two meshes left and right, one ahead.  (Rounds 3-4 used a radius-1.0 blob whose
    surface reaches 1.05: the camera sat INSIDE mesh D and every `ref` number described a closed room.  Retracted.)
    include_empty=False leaves the empty `car` object out: its BLAS root (count 0, inverted box) sends RayZen's shader into an
    unbounded push loop over a 64-entry stack (FS:426-452: undefined behaviour), so a run of the REAL shader (the tests'
    Mesa harness) can only be compared without it.  monkey_obj: path of the reference's own meshes/monkey.obj (build
    container only) in place of the stand-ins."""
    s = Scene(camera=Camera(position=(0.0, 0.0, 3.0), target=(0.0, 0.0, -1.0), aspect=aspect))
    I = identity()
    floor = s.add_mesh(make_cube(0))
    if monkey_obj is None:
        monkey = lambda mat, seed: s.add_mesh(fit_to_box(make_blob(mesh_n, 1.0, mat, seed=seed), SUZANNE_HALF_EXTENTS))
    else:
        monkey = lambda mat, seed: s.add_mesh(load_obj(monkey_obj, mat))
    a, b = monkey(1, 1), monkey(2, 2)
    car = s.add_mesh(np.zeros(0, TRIANGLE)) if include_empty else None
    c, d, glass = monkey(0, 3), monkey(0, 4), monkey(3, 5)
    s.add_object(floor, translate(scale(I, (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.add_object(a, translate(I, (-4.0, 0.0, 0.0)))
    s.add_object(b, translate(I, (4.0, 0.0, 0.0)))
    if include_empty:
        s.add_object(car, translate(I, (0.0, 0.0, 0.0)))
    s.add_object(c, translate(I, (0.0, 0.0, -4.0)))
    s.add_object(d, translate(I, (0.0, 0.0, 4.0)))
    s.add_object(glass, translate(scale(I, (1.2, 1.2, 1.2)), (2.5, 0.8, 2.5)))
    s.name = f"rayzen-main-scene(7 objects, 12+5x{12 * mesh_n * mesh_n} tris, Suzanne-sized stand-ins)"
    s = s.build()
    clear = camera_clearance(s)
    assert clear > 0.1, f"reference_scene: the camera lies inside (or {clear:.3f} from) an instance's world box"
    return s


def hidden_glass_scene(n=76, aspect=16.0 / 9.0):
    """C2's scene plus ONE transparent triangle far behind the camera: no path ever meets it, but the scene "has a transparent
    material", so the launch takes the transparent-scene kernels -- what they cost a frame that never needs them."""
    s = Scene(camera=Camera(position=(0.0, 2.5, 10.0), aspect=aspect))
    floor = s.add_mesh(make_cube(4))
    bunny = s.add_mesh(make_blob(n, 2.8, 0))
    s.add_object(floor, translate(scale(identity(), (8.0, 0.5, 8.0)), (0.0, -3.0, 0.0)))
    s.add_object(bunny, translate(identity(), (0.0, 2.0, 0.0)))
    t = np.zeros(1, TRIANGLE)
    t["v0"], t["v1"], t["v2"] = (0, 0, 0), (0.01, 0, 0), (0, 0.01, 0)
    t["materialIndex"] = 3
    s.add_object(s.add_mesh(t), translate(identity(), (0.0, 50.0, 60.0)))
    s.name = f"bunny{12 * n * n}+hidden-glass-triangle"
    return s.build()


# The named workloads of the measurement scripts (bench_configs.py, profiles/scripts/*): BASELINE.json's configurations on one
# GPU and their companions.  name -> (scene factory, width, height, spp, bounces).
NAMED_CONFIGS = {
    "c1": (lambda: cornell_scene(), 256, 256, 4, 1),
    "c2": (lambda: bunny_scene(n=76, aspect=16 / 9), 1920, 1080, 64, 4),                     # BASELINE configs[1], the bench workload
    # ... the same mesh, frame, spp and bounces with the camera 0.9 units outside the mesh: most camera paths hit geometry
    # (configs[1] fixes size / spp / bounces / triangles, not the camera; at the bench camera 64 % of the paths see only sky)
    "c2close": (lambda: bunny_scene(n=76, aspect=16 / 9, camera_position=CLOSE_CAMERA), 1920, 1080, 64, 4),
    "c2g": (lambda: bunny_scene(n=76, aspect=16 / 9, extras=True), 1920, 1080, 64, 4),       # + a glass blob and a mirror cube
    "glassbunny": (lambda: bunny_scene(n=76, aspect=16 / 9, bunny_material=3), 1920, 1080, 64, 4),
    "c2hidden": (lambda: hidden_glass_scene(n=76, aspect=16 / 9), 1920, 1080, 64, 4),           # the transparent kernels' pure overhead
    "mirror": (lambda: bunny_scene(n=76, aspect=16 / 9, bunny_material=2, floor_material=2), 1920, 1080, 64, 8),
    "c3": (lambda: bunny_scene(n=76, aspect=16 / 9), 1920, 1080, 256, 4),                    # configs[2]'s frame, whole on one GPU
    "c4": (lambda: instanced_scene(n=76, count=16, aspect=16 / 9), 1920, 1080, 16, 4),
    "c5": (lambda: stress_scene(n=289, aspect=16 / 9), 3840, 2160, 32, 8),                   # C5's scene at 32 spp
    "c5full": (lambda: stress_scene(n=289, aspect=16 / 9), 3840, 2160, 128, 8),              # configs[4] as stated
    "ref": (lambda: reference_scene(aspect=800 / 600), 800, 600, 1, 5),                      # RayZen's own workload (main.cpp:35-36, 356-384, 600)
    # ... RayZen's own scene where a launch has claims to compact: 16 samples per launch at its window size, and a 1080p / 64-spp frame
    "ref16": (lambda: reference_scene(aspect=800 / 600), 800, 600, 16, 5),
    "ref64": (lambda: reference_scene(aspect=16 / 9), 1920, 1080, 64, 5),
}


def named_config(name):
    """(scene, width, height, spp, bounces) of one of NAMED_CONFIGS."""
    make, w, h, spp, b = NAMED_CONFIGS[name]
    return make(), w, h, spp, b

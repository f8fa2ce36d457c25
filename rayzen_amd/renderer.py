"""Python view of the render C-ABI (include/rayzen_hip.h).

`Renderer` is the analogue of what RayZen's main.cpp does around its draw
call: upload the SSBO arrays (main.cpp:1072-1119), refresh the dynamic ones
(main.cpp:1196-1207), send the per-frame uniforms (main.cpp:1356-1379), draw
(main.cpp:637).  Everything it calls lives in librayzen_hip.so; there is no
fallback path.
"""
import ctypes as C

import numpy as np

from . import _lib
from .scene import BINDING_DTYPES, BIND_INSTANCES, BIND_TLAS_INDICES, BIND_TLAS_NODES, MORPH_TRIANGLE, SKIN_TRIANGLE


class RayZenError(RuntimeError):
    def __init__(self, what, code, message):
        super().__init__(f"{what} failed ({code}): {message}")
        self.code = code


def frame_params(camera, width, height, num_lights, bounce_budget, spp, sample_base=0, tile_rank=0, tile_nranks=1):
    p = _lib.FrameParams()
    p.width, p.height = int(width), int(height)
    p.inv_view[:] = camera.inv_view.tolist()
    p.inv_proj[:] = camera.inv_proj.tolist()
    p.view[:] = camera.view.tolist()
    p.proj[:] = camera.proj.tolist()
    p.cam_pos[:] = camera.position.tolist()
    p.num_lights, p.bounce_budget = int(num_lights), int(bounce_budget)
    p.spp, p.sample_base = int(spp), int(sample_base)
    p.tile_rank, p.tile_nranks = int(tile_rank), int(tile_nranks)
    return p


RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("max_dist", "<f4"), ("dir", "<f4", 3), ("reserved", "<u4")])   # rz_ray
HIT_DTYPE = np.dtype([("t", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3), ("material", "<i4"), ("instance", "<i4"),
                      ("triangle", "<i4"), ("prim", "<i4"), ("reserved", "<i4")])                                # rz_hit
VISIBILITY_DTYPE = np.dtype([("visibility", "<f4"), ("lit", "<i4")])                                         # rz_visibility
MESH_QUALITY = np.dtype([("node_offset", "<i4"), ("index_offset", "<i4"), ("tri_offset", "<i4"), ("node_offset_before", "<i4"),
                         ("n_triangles", "<i4"), ("n_nodes", "<i4"), ("depth", "<i4"), ("flags", "<u4"), ("sah_cost", "<f8"),
                         ("sah_cost_built", "<f8"), ("sah_cost_before", "<f8"), ("reserved", "<f8")])        # rz_mesh_quality
PIXEL_COST_DTYPE = _lib.PIXEL_COST_DTYPE # rz_pixel_cost (32 B): what render_cost returns
INSTANCE_COVERAGE_DTYPE = _lib.INSTANCE_COVERAGE_DTYPE   # rz_instance_coverage (32 B): what coverage returns
CHAIN_DTYPE = _lib.CHAIN_DTYPE           # rz_chain (16 B): what upscale(see_through=..., chains=True) returns
LINE_DTYPE = _lib.LINE_DTYPE             # rz_line (32 B): what draw_lines takes (rayzen_amd.lines makes them)


def make_rays(origins, dirs, max_dist=1e30):
    """An rz_ray array from (n, 3) origins and directions (float32) and a scalar or (n,) max_dist."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f"origins {o.shape} and dirs {d.shape} differ")
    rays = np.zeros(o.shape[0], RAY_DTYPE)
    rays["origin"], rays["dir"] = o, d
    rays["max_dist"] = np.broadcast_to(np.asarray(max_dist, np.float32), (o.shape[0],))
    return rays


def _glm_mul(m, v):
    """GLM 0.9.9's mat4 * vec4 in float32: (m0 x + m1 y) + (m2 z + m3 w), m column-major (16 floats)."""
    c = np.asarray(m, np.float32).reshape(4, 4)
    x, y, z, w = (np.float32(a) for a in v)
    return (c[0] * x + c[1] * y) + (c[2] * z + c[3] * w)


def pick_ray(mouse_x, mouse_y, screen_w, screen_h, camera):
    """RayZen's picking ray (main.cpp:505-513), step by step in float32: the cursor in NDC, the clip-space point
    (ndcX, ndcY, -1, 1) through the inverse projection, made a direction (x, y, -1, 0) in eye space, through the inverse view
    and normalised (glm::normalize: v * (1 / sqrt(dot(v, v)))).  Returns (origin, dir), each (3,) float32; origin is the camera
    position.  Host-only, no GPU."""
    f32 = np.float32
    ndc_x = f32(2.0) * f32(mouse_x) / f32(screen_w) - f32(1.0)
    ndc_y = f32(1.0) - f32(2.0) * f32(mouse_y) / f32(screen_h)
    ray_eye = _glm_mul(camera.inv_proj, (ndc_x, ndc_y, f32(-1.0), f32(1.0)))
    v = _glm_mul(camera.inv_view, (ray_eye[0], ray_eye[1], f32(-1.0), f32(0.0)))[:3]
    dot = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    direction = (v * (f32(1.0) / np.sqrt(dot))).astype(np.float32)
    return np.asarray(camera.position, np.float32).copy(), direction


def editor_rays(camera, width, height):
    """The rays rz_render_editor casts (rz_path.h: camera_ray_centre), one per pixel centre, step by step in float32: uv =
    (px + 0.5) / width, (py + 0.5) / height; (u * 2 - 1, v * 2 - 1, -1, 1) through the inverse projection, made a direction
    (x, y, -1, 0) through the inverse view and normalised as v / sqrt(dot(v, v)).  Returns (height * width,) rz_ray records in
    pixel order (row 0 = the bottom row) with origin = the camera position and max_dist = 1e30.  Host-only, no GPU."""
    f32 = np.float32
    px = np.arange(width, dtype=f32)
    py = np.arange(height, dtype=f32)
    ux = ((px + f32(0.5)) / f32(width))[None, :]
    uy = ((py + f32(0.5)) / f32(height))[:, None]
    cx = ux * f32(2.0) - f32(1.0)
    cy = uy * f32(2.0) - f32(1.0)
    ip = np.asarray(camera.inv_proj, f32)
    iv = np.asarray(camera.inv_view, f32)
    ex = ((ip[0] * cx + ip[4] * cy) + ip[8] * f32(-1.0)) + ip[12] * f32(1.0)
    ey = ((ip[1] * cx + ip[5] * cy) + ip[9] * f32(-1.0)) + ip[13] * f32(1.0)
    w = [(iv[r] * ex + iv[4 + r] * ey) + iv[8 + r] * f32(-1.0) for r in range(3)]
    dot = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    s = np.sqrt(dot)
    d = np.stack([c / s for c in w], -1).astype(f32).reshape(-1, 3)
    return make_rays(np.broadcast_to(np.asarray(camera.position, f32), d.shape), d)


def ao_directions():
    """The 256 unit directions rz_ambient_occlusion samples (rz_ao_directions): (256, 3) float32.  Host-only, no GPU."""
    out = np.empty((_lib.AO_DIRECTIONS, 3), np.float32)
    rc = _lib.hip().rz_ao_directions(out.ctypes.data, out.nbytes)
    if rc != 0:
        raise RayZenError("rz_ao_directions", rc, _lib.hip().rz_last_error(None).decode())
    return out


def adaptive_plan(active, current, merge_gap=8, max_runs=1):
    """The runs of tiles rz_render_adaptive's next batch renders (rz_adaptive_plan), from one flag per tile in row-major tile
    order: an (n, 2) int32 array of (first, len).  merge_gap and max_runs are taken as given.  Host-only, no GPU."""
    a = np.ascontiguousarray(np.asarray(active) != 0, np.uint8).reshape(-1)
    c = np.ascontiguousarray(np.asarray(current) != 0, np.uint8).reshape(-1)
    if a.size != c.size:
        raise ValueError("adaptive_plan: active and current differ in length")
    runs = np.empty(a.size // 2 + 1, _lib.TILE_RUN_DTYPE)
    n = C.c_size_t(0)
    rc = _lib.hip().rz_adaptive_plan(a.ctypes.data, c.ctypes.data, a.size, int(merge_gap), int(max_runs), runs.ctypes.data, runs.size,
                                     C.byref(n))
    if rc != 0:
        raise RayZenError("rz_adaptive_plan", rc, _lib.hip().rz_last_error(None).decode())
    return runs[:n.value].view(np.int32).reshape(-1, 2).copy()


class Renderer:
    def __init__(self, device=0, flags=0):
        self._L = _lib.hip()
        self._c = self._L.rz_create(int(device), int(flags))
        if not self._c:
            raise RayZenError("rz_create", -2, self._L.rz_last_error(None).decode())
        self.width = self.height = 0
        self._frame = None      # a copy of the last set_frame's params: what coverage(frame=None) casts through

    def close(self):
        c, self._c = getattr(self, "_c", None), None
        if c:
            self._L.rz_destroy(c)

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise RayZenError(what, rc, self._L.rz_last_error(self._c).decode())

    # -- glBufferData / glBufferSubData ------------------------------------
    def upload(self, binding, array):
        a = np.ascontiguousarray(array)
        self._check(self._L.rz_upload(self._c, int(binding), a.ctypes.data if a.nbytes else None, a.nbytes), "rz_upload")

    def update(self, binding, array, offset_bytes=0):
        a = np.ascontiguousarray(array)
        self._check(self._L.rz_update(self._c, int(binding), int(offset_bytes), a.ctypes.data if a.nbytes else None,
                                      a.nbytes), "rz_update")

    def upload_scene(self, scene):
        """initializeSSBOs' eight uploads (main.cpp:1072-1119)."""
        for b in BINDING_DTYPES:
            self.upload(b, scene.arrays[b])

    def update_dynamic(self, scene):
        """The part of updateDynamicBVHAndSSBOs that changes per frame: instances + TLAS."""
        for b in (BIND_INSTANCES, BIND_TLAS_NODES, BIND_TLAS_INDICES):
            self.update(b, scene.arrays[b])

    def update_transforms(self, transforms):
        """Device-side updateDynamicBVHAndSSBOs: transforms = (n, 16) float32, column-major."""
        t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 16)
        self._check(self._L.rz_update_transforms(self._c, t.ctypes.data, t.shape[0]), "rz_update_transforms")

    def refit_geometry(self, triangles=None, first=0):
        """rz_refit_geometry from host memory: `triangles` (TRIANGLE dtype) replace binding 0 from element `first` on and every
        mesh they touch is refitted on the device -- boxes recomputed, topology kept, everything derived patched in place,
        world boxes and TLAS rebuilt with the transforms in force.  triangles=None: refit every mesh from binding 0 as it
        stands (what makes a preceding update() of binding 0 correct)."""
        from .scene import TRIANGLE as TRIANGLE_DTYPE
        if triangles is None:
            self._check(self._L.rz_refit_geometry(self._c, None, 0, 0, 0), "rz_refit_geometry")
            return
        t = np.ascontiguousarray(triangles, TRIANGLE_DTYPE)
        self._check(self._L.rz_refit_geometry(self._c, t.ctypes.data if t.shape[0] else None, int(first), t.shape[0], _lib.REFIT_HOST),
                    "rz_refit_geometry")

    def refit_geometry_device(self, ptr, first, n):
        """rz_refit_geometry on device memory (rz_triangle[n], 16-B aligned), enqueued on the context's stream."""
        self._check(self._L.rz_refit_geometry(self._c, C.c_void_p(ptr), int(first), int(n), 0), "rz_refit_geometry")

    def skin_create(self, first, rest, skin, n_bones, morphs=None):
        """rz_skin_create: a rig for the triangles [first, first + n) of binding 0.  rest: their rest pose (TRIANGLE dtype), or
        an int n -- then binding 0's current content of that range is the rest pose; skin: SKIN_TRIANGLE per triangle, or None
        for a morph-only rig (n_bones 0); morphs: MORPH_TRIANGLE [n_morphs, n] or None.  Everything is copied to the device.
        Returns the rig id."""
        if isinstance(rest, (int, np.integer)):
            n, rest_ptr = int(rest), None
        else:
            rest = np.ascontiguousarray(rest)
            assert rest.dtype.itemsize == 64
            n, rest_ptr = rest.shape[0], rest.ctypes.data
        skin_ptr = None
        if skin is not None:
            skin = np.ascontiguousarray(skin, SKIN_TRIANGLE)
            assert skin.shape == (n,)
            skin_ptr = skin.ctypes.data
        n_morphs, morph_ptr = 0, None
        if morphs is not None and len(morphs):
            morphs = np.ascontiguousarray(morphs, MORPH_TRIANGLE).reshape(-1, n)
            n_morphs, morph_ptr = morphs.shape[0], morphs.ctypes.data
        rig = C.c_int(-1)
        self._check(self._L.rz_skin_create(self._c, int(first), n, rest_ptr, skin_ptr, int(n_bones), morph_ptr, n_morphs, C.byref(rig)),
                    "rz_skin_create")
        return rig.value

    def skin_pose(self, rig, bones=None, morph_weights=None):
        """rz_skin_pose from host memory: the rig's mesh is posed on the device (bones: n_bones x 16 column-major floats,
        morph_weights: n_morphs floats) and refitted as rz_refit_geometry refits it, TLAS included."""
        b = None if bones is None else np.ascontiguousarray(bones, np.float32).reshape(-1)
        w = None if morph_weights is None else np.ascontiguousarray(morph_weights, np.float32).reshape(-1)
        self._check(self._L.rz_skin_pose(self._c, int(rig), None if b is None else b.ctypes.data, None if w is None else w.ctypes.data, 0),
                    "rz_skin_pose")

    def skin_pose_device(self, rig, bones_ptr, weights_ptr):
        """rz_skin_pose with RZ_SKIN_DEVICE_ARGS: bones (16-B aligned) and morph weights are device memory, read on the stream."""
        self._check(self._L.rz_skin_pose(self._c, int(rig), C.c_void_p(bones_ptr), C.c_void_p(weights_ptr), _lib.SKIN_DEVICE_ARGS),
                    "rz_skin_pose")

    def skin_destroy(self, rig):
        self._check(self._L.rz_skin_destroy(self._c, int(rig)), "rz_skin_destroy")

    def skin_last_kernel_ms(self):
        """Device time of the skinning kernel of the last skin_pose (synchronises on it)."""
        ms = C.c_float(0)
        self._check(self._L.rz_skin_last_kernel_ms(self._c, C.byref(ms)), "rz_skin_last_kernel_ms")
        return ms.value

    def geometry_quality(self):
        """rz_geometry_quality: one MESH_QUALITY record per mesh (a distinct offset triple among the instances), in ascending
        order of the triple: its SAH cost as the tree stands, the cost it had when it was last handed over or built, its
        triangle and node counts and its depth.  Measured on the device; synchronises."""
        n = C.c_size_t(0)
        self._check(self._L.rz_geometry_quality(self._c, None, 0, C.byref(n)), "rz_geometry_quality")
        out = np.zeros(n.value, MESH_QUALITY)
        self._check(self._L.rz_geometry_quality(self._c, out.ctypes.data if n.value else None, n.value, C.byref(n)), "rz_geometry_quality")
        return out[:n.value]

    def rebuild_geometry(self, max_ratio=0.0):
        """rz_rebuild_geometry: every mesh whose SAH cost exceeds max_ratio times the cost it was built with gets a fresh BLAS
        on the device from binding 0 as it stands there; later meshes move in binding 7, the instances' offsets are patched
        and the TLAS follows with the transforms in force.  max_ratio = 0 rebuilds every mesh with a non-zero cost.  Returns
        the MESH_QUALITY records (flags & QUALITY_REBUILT: rebuilt by this call; both costs are reported)."""
        n = C.c_size_t(0)
        self._check(self._L.rz_geometry_quality(self._c, None, 0, C.byref(n)), "rz_geometry_quality")
        out = np.zeros(n.value, MESH_QUALITY)
        self._check(self._L.rz_rebuild_geometry(self._c, float(max_ratio), out.ctypes.data if n.value else None, n.value, C.byref(n), 0),
                    "rz_rebuild_geometry")
        return out[:n.value]

    def build_blas(self, triangles):
        """BVH::buildBLAS (BVH.cpp:99-175, SAH) on the device.  triangles: TRIANGLE_DTYPE array.
        Returns (nodes, indices, depth, device_ms); byte-identical to the reference builder's output."""
        from .scene import BVH_NODE as NODE_DTYPE, TRIANGLE as TRIANGLE_DTYPE
        t = np.ascontiguousarray(triangles, TRIANGLE_DTYPE)
        n = t.shape[0]
        nodes = np.zeros(max(2 * n - 1, 1), NODE_DTYPE)
        idx = np.zeros(n, np.int32)
        nn, depth, ms = C.c_size_t(0), C.c_int(0), C.c_float(0)
        self._check(self._L.rz_build_blas(self._c, t.ctypes.data if n else None, n, nodes.ctypes.data, nodes.shape[0],
                                          idx.ctypes.data if n else None, C.byref(nn), C.byref(depth), C.byref(ms)),
                    "rz_build_blas")
        return nodes[:nn.value].copy(), idx, depth.value, ms.value

    def build_geometry(self, triangles, ranges):
        """rz_build_geometry: triangles = all meshes back to back (TRIANGLE dtype), ranges = [(first, count), ...].
        Builds every BLAS on the device, leaves nodes / indices there as bindings 7 / 8 (and the triangles as binding 0).
        Returns one dict per mesh: node_offset, index_offset, n_nodes, depth, root (a BVH_NODE record)."""
        from .scene import BVH_NODE as NODE_DTYPE, TRIANGLE as TRIANGLE_DTYPE
        t = np.ascontiguousarray(triangles, TRIANGLE_DTYPE)
        arr = (_lib.MeshBuild * len(ranges))()
        for k, (first, count) in enumerate(ranges):
            arr[k].first_triangle, arr[k].n_triangles = int(first), int(count)
        self._check(self._L.rz_build_geometry(self._c, t.ctypes.data if t.shape[0] else None, t.shape[0], arr, len(ranges)),
                    "rz_build_geometry")
        out = []
        for m in arr:
            root = np.zeros(1, NODE_DTYPE)
            C.memmove(root.ctypes.data, C.addressof(m.root), 32)
            out.append(dict(node_offset=m.node_offset, index_offset=m.index_offset, n_nodes=m.n_nodes, depth=m.depth, root=root[0]))
        return out

    def upload_scene_built_on_device(self, meshes, objects, materials, lights):
        """initializeSSBOs with the geometry half on the device: meshes = list of TRIANGLE arrays, objects = list of
        (mesh index, 16-float column-major transform).  One BLAS per distinct mesh (true instancing).  Instances, world
        boxes and the TLAS are assembled with librayzen_host exactly as SceneBuffers::build does; returns the arrays
        uploaded for bindings 5, 6 and 9 as a dict (nodes / indices stay on the device: read_binding fetches them)."""
        from . import scene as S
        ranges, first = [], 0
        for m in meshes:
            ranges.append((first, len(m)))
            first += len(m)
        tris = np.concatenate([np.ascontiguousarray(m, S.TRIANGLE) for m in meshes]) if meshes else np.zeros(0, S.TRIANGLE)
        built = self.build_geometry(tris, ranges)
        inst = np.zeros(len(objects), S.BVH_INSTANCE)
        roots = np.zeros(len(objects), S.BVH_NODE)
        for i, (mi, xf) in enumerate(objects):
            xf = np.ascontiguousarray(xf, np.float32).reshape(16)
            b = built[mi]
            inst[i] = (b["node_offset"], b["index_offset"], i, ranges[mi][0], xf, S.inverse(xf))
            mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
            r1 = np.zeros(1, S.BVH_NODE)
            r1[0] = b["root"]
            _lib.host().rzh_world_bounds(r1.ctypes.data, xf.ctypes.data, mn.ctypes.data, mx.ctypes.data)
            roots[i] = b["root"]
            roots[i]["boundsMin"], roots[i]["boundsMax"] = mn, mx
        tn, ti = S.build_tlas(roots)
        self.upload(S.BIND_INSTANCES, inst)
        self.upload(S.BIND_TLAS_NODES, tn)
        self.upload(S.BIND_TLAS_INDICES, ti)
        self.upload(S.BIND_MATERIALS, materials)
        self.upload(S.BIND_LIGHTS, lights)
        return {S.BIND_INSTANCES: inst, S.BIND_TLAS_NODES: tn, S.BIND_TLAS_INDICES: ti, S.BIND_TRIANGLES: tris}

    def read_binding(self, binding):
        """The binding's current content in RayZen's layout (what the device built, after update_transforms)."""
        need = C.c_size_t(0)
        self._check(self._L.rz_read_binding(self._c, int(binding), None, 0, C.byref(need)), "rz_read_binding")
        dt = BINDING_DTYPES[int(binding)]
        out = np.zeros(need.value // dt.itemsize, dt)
        self._check(self._L.rz_read_binding(self._c, int(binding), out.ctypes.data if out.nbytes else None, out.nbytes,
                                            C.byref(need)), "rz_read_binding")
        return out

    # -- uniforms + draw -----------------------------------------------------
    def set_frame(self, params):
        self._check(self._L.rz_set_frame(self._c, C.byref(params)), "rz_set_frame")
        self.width, self.height = params.width, params.height
        self._frame = _lib.FrameParams.from_buffer_copy(params)

    def set_stream(self, hip_stream):
        self._check(self._L.rz_set_stream(self._c, C.c_void_p(hip_stream)), "rz_set_stream")

    def bind_accum(self, device_ptr, nbytes):
        self._check(self._L.rz_bind_accum(self._c, C.c_void_p(device_ptr), int(nbytes)), "rz_bind_accum")

    def render(self):
        self._check(self._L.rz_render(self._c), "rz_render")

    def render_counted(self):
        cnt = _lib.Counters()
        self._check(self._L.rz_render_counted(self._c, C.byref(cnt)), "rz_render_counted")
        return {n: int(getattr(cnt, n)) for n in _lib.COUNTER_FIELDS}

    def sync(self):
        self._check(self._L.rz_sync(self._c), "rz_sync")

    def clear_accum(self):
        self._check(self._L.rz_clear_accum(self._c), "rz_clear_accum")

    def read_accum(self):
        """(H, W, 4) float32; row 0 = bottom row; rgb = sum of per-sample radiance, a = sample count."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.rz_read_accum(self._c, out.ctypes.data, out.nbytes), "rz_read_accum")
        return out

    def resolve_rgba8(self):
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rz_resolve_rgba8(self._c, out.ctypes.data, out.nbytes), "rz_resolve_rgba8")
        return out

    def present(self, fps=0.0, show_fps=True, show_lights=False, show_bvh=False, bvh_mode=0, selected_blas=0,
                selected_tri=0):
        """fragment_shader.glsl:772-819: resolve + overlays.  Returns (rgb float32 (H,W,3), rgba8 uint8 (H,W,4))."""
        p = _lib.PresentParams(float(fps), int(bool(show_fps)), int(bool(show_lights)), int(bool(show_bvh)),
                               int(bvh_mode), int(selected_blas), int(selected_tri))
        rgb = np.empty((self.height, self.width, 3), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rz_present(self._c, C.byref(p), rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data,
                                       rgb.nbytes), "rz_present")
        return rgb, rgba8

    def last_render_ms(self):
        ms, n = C.c_float(0), C.c_int(0)
        self._check(self._L.rz_last_render_ms(self._c, C.byref(ms), C.byref(n)), "rz_last_render_ms")
        return float(ms.value), int(n.value)

    def render_history_ms(self, cap=64):
        """GPU durations (ms) of the render launches issued since the previous call (oldest first)."""
        buf = (C.c_float * cap)()
        n = self._L.rz_render_history_ms(self._c, buf, cap)
        if n < 0:
            self._check(n, "rz_render_history_ms")
        return [float(buf[k]) for k in range(n)]

    def last_kernel_name(self):
        return self._L.rz_last_kernel_name(self._c).decode()

    def debug_fail_alloc(self, nth):
        """Test hook: the nth host allocation site reached from now on throws std::bad_alloc inside the library."""
        self._check(self._L.rz_debug_fail_alloc(self._c, int(nth)), "rz_debug_fail_alloc")

    def debug_last_plan(self):
        """Test hook: how the last render call was launched (rz_launch_plan as a dict)."""
        lp = _lib.LaunchPlan()
        self._check(self._L.rz_debug_last_plan(self._c, C.byref(lp)), "rz_debug_last_plan")
        return {n: int(getattr(lp, n)) for n, _ in _lib.LaunchPlan._fields_}

    def debug_read_layout(self, which):
        """Test hook: the device scene layout as raw bytes (0: DevPair[], 1: DevTri[], 2: TlasDfs[], the TLAS in pop order)."""
        need = C.c_size_t(0)
        self._check(self._L.rz_debug_read_layout(self._c, int(which), None, 0, C.byref(need)), "rz_debug_read_layout")
        out = np.zeros(need.value, np.uint8)
        self._check(self._L.rz_debug_read_layout(self._c, int(which), out.ctypes.data if need.value else None, out.nbytes, C.byref(need)),
                    "rz_debug_read_layout")
        return out

    def accum_device_ptr(self):
        return self._L.rz_accum_device_ptr(self._c)

    # -- ray queries (rz_trace_rays / rz_shadow_rays) ---------------------------
    def trace_rays(self, origins, dirs, incoherent=False):
        """Closest hits of (n, 3) float32 rays on the uploaded scene (host memory; returns when done).  Returns a dict of numpy
        arrays: t, point, normal, material, instance, triangle, prim (a miss: t = 1e30, ids -1, point / normal zero)."""
        rays = make_rays(origins, dirs)
        hits = np.zeros(rays.shape[0], HIT_DTYPE)
        flags = _lib.RAYS_HOST | (_lib.RAYS_INCOHERENT if incoherent else 0)
        self._check(self._L.rz_trace_rays(self._c, rays.ctypes.data if rays.size else None, hits.ctypes.data if hits.size else None,
                                          rays.shape[0], flags), "rz_trace_rays")
        return {k: hits[k].copy() for k in ("t", "point", "normal", "material", "instance", "triangle", "prim")}

    def trace_rays_device(self, rays_ptr, hits_ptr, n, incoherent=False):
        """rz_trace_rays on device memory (rz_ray[n] in, rz_hit[n] out, 16-B aligned): enqueued on the context's stream,
        asynchronous -- the hits are valid after sync() or the caller's own synchronisation of that stream."""
        self._check(self._L.rz_trace_rays(self._c, C.c_void_p(rays_ptr), C.c_void_p(hits_ptr), int(n),
                                          _lib.RAYS_INCOHERENT if incoherent else 0), "rz_trace_rays")

    def shadow_rays(self, origins, dirs, max_dist, incoherent=False):
        """FS:507-528 for (n, 3) float32 rays with a scalar or (n,) max_dist (host memory).  Returns (lit bool (n,),
        visibility float32 (n,))."""
        rays = make_rays(origins, dirs, max_dist)
        out = np.zeros(rays.shape[0], VISIBILITY_DTYPE)
        flags = _lib.RAYS_HOST | (_lib.RAYS_INCOHERENT if incoherent else 0)
        self._check(self._L.rz_shadow_rays(self._c, rays.ctypes.data if rays.size else None, out.ctypes.data if out.size else None,
                                           rays.shape[0], flags), "rz_shadow_rays")
        return out["lit"] != 0, out["visibility"].copy()

    def shadow_rays_device(self, rays_ptr, out_ptr, n, incoherent=False):
        """rz_shadow_rays on device memory (rz_ray[n] in, rz_visibility[n] out, 16-B aligned); asynchronous."""
        self._check(self._L.rz_shadow_rays(self._c, C.c_void_p(rays_ptr), C.c_void_p(out_ptr), int(n),
                                           _lib.RAYS_INCOHERENT if incoherent else 0), "rz_shadow_rays")

    def pick(self, mouse_x, mouse_y, screen_w, screen_h, camera):
        """What RayZen's BLAS debug mode picks under the cursor (main.cpp:501-552), by one closest-hit query of the picking
        ray (pick_ray) on the uploaded scene.  Returns (instance, triangle) -- exactly what present(show_bvh=True, bvh_mode=1,
        selected_blas=instance, selected_tri=triangle) takes -- or None on a miss.  The reference KEEPS its previous selection
        when nothing is hit (main.cpp:548); a caller that wants that behaviour keeps its own on None.
        Unlike the reference's brute-force loop it compares world distances (as the shader does), rejects at |a| < 1e-4 (the
        shader's bound, not 1e-6) and never hits an empty or invalid BLAS: it picks what the frame shows."""
        o, d = pick_ray(mouse_x, mouse_y, screen_w, screen_h, camera)
        h = self.trace_rays(o[None], d[None])
        if h["instance"][0] < 0:
            return None
        return int(h["instance"][0]), int(h["triangle"][0])

    # -- editor preview (rz_render_editor) ---------------------------------------
    @staticmethod
    def _editor_args(camera, width, height, num_lights, ambient, clear):
        # num_lights=None: every light uploaded (the call loops over min(num_lights, lights uploaded))
        fp = frame_params(camera, width, height, 0x7fffffff if num_lights is None else num_lights, 0, 1)
        if ambient is None and clear is None:
            return fp, None
        ep = _lib.EditorParams()
        ep.ambient[:] = [0.03] * 3 if ambient is None else [float(a) for a in ambient]
        ep.clear[:] = [0.05, 0.05, 0.07, 1.0] if clear is None else [float(a) for a in clear]
        return fp, C.byref(ep)

    def render_editor(self, camera, width, height, num_lights=None, ambient=None, clear=None, rgb32f=False, hits=False,
                      incoherent=False):
        """RayZen's editor preview (main.cpp:1210-1322) of the uploaded scene, by a ray cast (host memory; returns when done).
        Returns (rgba8 uint8 (H, W, 4), rgb float32 (H, W, 3) or None, hits HIT_DTYPE (H, W) or None); row 0 = bottom row.
        ambient (3) and clear (4) default to RayZen's 0.03 and (0.05, 0.05, 0.07, 1)."""
        fp, ep = self._editor_args(camera, width, height, num_lights, ambient, clear)
        out8 = np.empty((height, width, 4), np.uint8)
        rgb = np.empty((height, width, 3), np.float32) if rgb32f else None
        hh = np.empty((height, width), HIT_DTYPE) if hits else None
        flags = _lib.EDITOR_HOST | (_lib.EDITOR_INCOHERENT if incoherent else 0)
        self._check(self._L.rz_render_editor(self._c, C.byref(fp), ep, out8.ctypes.data, out8.nbytes,
                                             None if rgb is None else rgb.ctypes.data, 0 if rgb is None else rgb.nbytes,
                                             None if hh is None else hh.ctypes.data, 0 if hh is None else hh.nbytes, flags),
                    "rz_render_editor")
        return out8, rgb, hh

    def render_editor_device(self, camera, width, height, rgba8_ptr=None, rgb32f_ptr=None, hits_ptr=None, num_lights=None,
                             ambient=None, clear=None, incoherent=False):
        """rz_render_editor into device memory (each output optional; hits 16-B aligned, the others 4-B): enqueued on the
        context's stream, asynchronous -- the outputs are valid after sync() or the caller's own synchronisation of that
        stream.  Sizes: rgba8 W*H*4 B, rgb32f W*H*12 B, hits W*H*48 B."""
        fp, ep = self._editor_args(camera, width, height, num_lights, ambient, clear)
        n = int(width) * int(height)
        self._check(self._L.rz_render_editor(self._c, C.byref(fp), ep, C.c_void_p(rgba8_ptr), n * 4 if rgba8_ptr else 0,
                                             C.c_void_p(rgb32f_ptr), n * 12 if rgb32f_ptr else 0, C.c_void_p(hits_ptr),
                                             n * 48 if hits_ptr else 0, _lib.EDITOR_INCOHERENT if incoherent else 0),
                    "rz_render_editor")

    # -- denoiser (rz_denoise / rz_present_denoised) -------------------------------
    @staticmethod
    def _denoise_params(iterations, sigma_color, sigma_normal, sigma_plane, demodulate):
        # all None: the library's defaults (params NULL)
        if iterations is None and sigma_color is None and sigma_normal is None and sigma_plane is None and demodulate is None:
            return None
        p = _lib.DenoiseParams()
        p.iterations = 5 if iterations is None else int(iterations)
        p.sigma_color = 0.5 if sigma_color is None else float(sigma_color)
        p.sigma_normal = 128.0 if sigma_normal is None else float(sigma_normal)
        p.sigma_plane = 1.0 if sigma_plane is None else float(sigma_plane)
        p.demodulate = 1 if demodulate is None else int(bool(demodulate))
        return C.byref(p)

    def denoise(self, rgba_in=None, iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None, demodulate=None,
                guides=False):
        """The a-trous denoiser (include/rayzen_hip.h: rz_denoise) on the accumulation, or on rgba_in ((H, W, 4) float32 in
        the accumulation's sum-and-count form), for the size and camera of the last set_frame (host memory; returns when done).
        Returns the denoised linear colour (H, W, 3) float32, unclamped, and with guides=True also the guide as (H, W) HIT_DTYPE
        records (what trace_rays returns for the pixel-centre rays of editor_rays); row 0 = bottom row.  Parameters left None
        take the library's defaults (K = 5, sigma_color 0.5, sigma_normal 128, sigma_plane 1, demodulate on)."""
        dp = self._denoise_params(iterations, sigma_color, sigma_normal, sigma_plane, demodulate)
        src = None if rgba_in is None else np.ascontiguousarray(rgba_in, np.float32)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        hh = np.empty((self.height, self.width), HIT_DTYPE) if guides else None
        self._check(self._L.rz_denoise(self._c, dp, None if src is None else src.ctypes.data, 0 if src is None else src.nbytes,
                                       rgb.ctypes.data, rgb.nbytes, None if hh is None else hh.ctypes.data,
                                       0 if hh is None else hh.nbytes, _lib.DENOISE_HOST), "rz_denoise")
        return (rgb, hh) if guides else rgb

    def denoise_device(self, rgb32f_ptr=None, guides_ptr=None, rgba_in_ptr=None, iterations=None, sigma_color=None,
                       sigma_normal=None, sigma_plane=None, demodulate=None):
        """rz_denoise on device memory (rgba_in and guides 16-B aligned, rgb32f 4-B; each optional): enqueued on the context's
        stream, asynchronous -- the outputs are valid after sync() or the caller's own synchronisation of that stream.
        Sizes: rgba_in W*H*16 B, rgb32f W*H*12 B, guides W*H*48 B."""
        dp = self._denoise_params(iterations, sigma_color, sigma_normal, sigma_plane, demodulate)
        n = self.width * self.height
        self._check(self._L.rz_denoise(self._c, dp, C.c_void_p(rgba_in_ptr), n * 16 if rgba_in_ptr else 0,
                                       C.c_void_p(rgb32f_ptr), n * 12 if rgb32f_ptr else 0, C.c_void_p(guides_ptr),
                                       n * 48 if guides_ptr else 0, 0), "rz_denoise")

    def present_denoised(self, fps=0.0, show_fps=True, show_lights=False, show_bvh=False, bvh_mode=0, selected_blas=0,
                         selected_tri=0, iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None, demodulate=None):
        """present() with the denoised colour in place of the resolve: the overlays are drawn on top.  Returns (rgb float32
        (H,W,3), rgba8 uint8 (H,W,4)); iterations=0 gives present()'s bytes."""
        p = _lib.PresentParams(float(fps), int(bool(show_fps)), int(bool(show_lights)), int(bool(show_bvh)),
                               int(bvh_mode), int(selected_blas), int(selected_tri))
        dp = self._denoise_params(iterations, sigma_color, sigma_normal, sigma_plane, demodulate)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rz_present_denoised(self._c, C.byref(p), dp, rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data,
                                                rgb.nbytes), "rz_present_denoised")
        return rgb, rgba8

    # -- temporal accumulation (rz_denoise_temporal / rz_present_temporal) ---------
    @staticmethod
    def _temporal_params(kw):
        # nothing given: the library's defaults (params NULL)
        unknown = set(kw) - set(_lib.TEMPORAL_DEFAULTS)
        if unknown:
            raise TypeError(f"unknown temporal parameter(s): {sorted(unknown)}")
        if all(v is None for v in kw.values()):
            return None
        p = _lib.TemporalParams()
        for name, default in _lib.TEMPORAL_DEFAULTS.items():
            v = kw.get(name)
            v = default if v is None else v
            setattr(p, name, int(v) if isinstance(default, int) else float(v))
        return C.byref(p)

    def denoise_temporal(self, rgba_in=None, guides=False, stats=False, keep=False, **params):
        """Temporal accumulation by reprojection plus the variance-guided a-trous filter (include/rayzen_hip.h:
        rz_denoise_temporal) on the accumulation, or on rgba_in ((H, W, 4) float32, sum and count), for the size and camera of the
        last set_frame (host memory; returns when done).  Every call blends the frame into the history the context keeps; keep=True
        computes the outputs and leaves the history as it was.  Returns the colour (H, W, 3) float32, then -- where asked -- the
        guide as (H, W) HIT_DTYPE and the stats (H, W, 2) float32 (history length N, variance); row 0 = bottom row.
        params: alpha, alpha_moments, max_history, normal_cos, plane_tol, iterations, sigma_l, sigma_normal, sigma_plane,
        demodulate (those left out take the library's defaults)."""
        tp = self._temporal_params(params)
        src = None if rgba_in is None else np.ascontiguousarray(rgba_in, np.float32)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        hh = np.empty((self.height, self.width), HIT_DTYPE) if guides else None
        st = np.empty((self.height, self.width, 2), np.float32) if stats else None
        flags = _lib.TEMPORAL_HOST | (_lib.TEMPORAL_KEEP if keep else 0)
        self._check(self._L.rz_denoise_temporal(self._c, tp, None if src is None else src.ctypes.data, 0 if src is None else src.nbytes,
                                                rgb.ctypes.data, rgb.nbytes, None if hh is None else hh.ctypes.data,
                                                0 if hh is None else hh.nbytes, None if st is None else st.ctypes.data,
                                                0 if st is None else st.nbytes, flags), "rz_denoise_temporal")
        out = (rgb,) + ((hh,) if guides else ()) + ((st,) if stats else ())
        return out if len(out) > 1 else rgb

    def denoise_temporal_device(self, rgb32f_ptr=None, guides_ptr=None, stats_ptr=None, rgba_in_ptr=None, keep=False, **params):
        """rz_denoise_temporal on device memory (rgba_in and guides 16-B aligned, rgb32f and stats 4-B; each optional): enqueued
        on the context's stream, asynchronous.  Sizes: rgba_in W*H*16 B, rgb32f W*H*12 B, guides W*H*48 B, stats W*H*8 B."""
        tp = self._temporal_params(params)
        n = self.width * self.height
        self._check(self._L.rz_denoise_temporal(self._c, tp, C.c_void_p(rgba_in_ptr), n * 16 if rgba_in_ptr else 0,
                                                C.c_void_p(rgb32f_ptr), n * 12 if rgb32f_ptr else 0, C.c_void_p(guides_ptr),
                                                n * 48 if guides_ptr else 0, C.c_void_p(stats_ptr), n * 8 if stats_ptr else 0,
                                                _lib.TEMPORAL_KEEP if keep else 0), "rz_denoise_temporal")

    def present_temporal(self, fps=0.0, show_fps=True, show_lights=False, show_bvh=False, bvh_mode=0, selected_blas=0,
                         selected_tri=0, **params):
        """present() with the temporally accumulated, filtered colour in place of the resolve (the history advances): the
        overlays are drawn on top.  Returns (rgb float32 (H,W,3), rgba8 uint8 (H,W,4))."""
        p = _lib.PresentParams(float(fps), int(bool(show_fps)), int(bool(show_lights)), int(bool(show_bvh)),
                               int(bvh_mode), int(selected_blas), int(selected_tri))
        tp = self._temporal_params(params)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rz_present_temporal(self._c, C.byref(p), tp, rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data,
                                                rgb.nbytes), "rz_present_temporal")
        return rgb, rgba8

    def temporal_reset(self):
        """Drops the history: the next temporal call starts every pixel at N = 1."""
        self._check(self._L.rz_temporal_reset(self._c), "rz_temporal_reset")

    def debug_read_temporal(self, which):
        """Test hook: the stored history (0: colour | N float32 (H, W, 4); 1: moments (H, W, 2); 2: the guide, HIT_DTYPE (H, W);
        3: view, proj, inv_proj, cam_pos as 51 floats; 4: per instance inverseTransform and transform, (n, 2, 4, 3) -- columns
        0..3, rows 0..2).  An empty history: None."""
        need = C.c_size_t(0)
        self._check(self._L.rz_debug_read_temporal(self._c, int(which), None, 0, C.byref(need)), "rz_debug_read_temporal")
        if need.value == 0:
            return None
        raw = np.zeros(need.value, np.uint8)
        self._check(self._L.rz_debug_read_temporal(self._c, int(which), raw.ctypes.data, raw.nbytes, C.byref(need)),
                    "rz_debug_read_temporal")
        if which == 2:
            return raw.view(HIT_DTYPE).reshape(self.height, self.width)
        f = raw.view(np.float32)
        if which == 0:
            return f.reshape(self.height, self.width, 4)
        if which == 1:
            return f.reshape(self.height, self.width, 2)
        return f.reshape(-1, 2, 4, 3) if which == 4 else f

    # -- display transform (rz_display / rz_present_display) -------------------------
    @staticmethod
    def _display_params(auto=False, exposure=1.0, key=0.18, min_exposure=1 / 64, max_exposure=64.0, adapt=1.0, low=0.0,
                        high=0.0, curve="clamp", white=4.0, transfer="linear"):
        """rz_display_params from the keyword arguments of display() / present_display(), every field checked here (ValueError)
        whatever the mode; None (params NULL: the reference's display) when nothing departs from the defaults."""
        def positive(name, v):
            v = float(v)
            if not (0.0 < v < float("inf")):
                raise ValueError(f"{name} = {v!r}: must be finite and > 0")
            return v

        if curve not in _lib.DISPLAY_CURVES:
            raise ValueError(f"curve = {curve!r}: one of {sorted(_lib.DISPLAY_CURVES)}")
        if transfer not in _lib.DISPLAY_TRANSFERS:
            raise ValueError(f"transfer = {transfer!r}: one of {sorted(_lib.DISPLAY_TRANSFERS)}")
        p = _lib.DisplayParams()
        p.exposure_mode = int(bool(auto))
        p.exposure = positive("exposure", exposure)
        p.key = positive("key", key)
        p.min_exposure, p.max_exposure = positive("min_exposure", min_exposure), positive("max_exposure", max_exposure)
        if not p.min_exposure <= p.max_exposure:
            raise ValueError(f"min_exposure {min_exposure!r} > max_exposure {max_exposure!r}")
        if not 0.0 <= float(adapt) <= 1.0:
            raise ValueError(f"adapt = {adapt!r}: outside [0, 1]")
        p.adapt = float(adapt)
        if not (float(low) >= 0.0 and float(high) >= 0.0):
            raise ValueError(f"low = {low!r}, high = {high!r}: shares must be >= 0")
        p.low_permille, p.high_permille = int(round(float(low) * 1000)), int(round(float(high) * 1000))
        if p.low_permille + p.high_permille >= 1000:
            raise ValueError(f"low + high = {float(low) + float(high)!r}: must leave something to count (< 1)")
        p.curve = _lib.DISPLAY_CURVES[curve]
        p.white = positive("white", white)
        p.transfer = _lib.DISPLAY_TRANSFERS[transfer]
        d = _lib.DisplayParams(0, 1.0, 0.18, 1 / 64, 64.0, 1.0, 0, 0, 0, 4.0, 0)
        return None if bytes(p) == bytes(d) else p

    def display(self, rgb=None, *, keep=False, **params):
        """The display stage (include/rayzen_hip.h: rz_display) on rgb ((H, W, 3) float32 linear colour, what denoise() and
        denoise_temporal() return) or, with rgb None, on the accumulation; host memory, returns when done.  params: auto=False,
        exposure=1.0, key=0.18, min_exposure=1/64, max_exposure=64.0, adapt=1.0, low=0.0, high=0.0 (the darkest / brightest share
        of the metered pixels left out), curve="clamp"|"reinhard"|"aces", white=4.0, transfer="linear"|"srgb"; with none of them
        it is the reference's display (clamp, linear).  keep=True leaves the adaptation state as it was.  Returns (rgb32f (H, W, 3)
        float32: the encoded colour; rgba8 (H, W, 4) uint8); row 0 = bottom row."""
        dp = self._display_params(**params)
        src = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
        out = np.empty((self.height, self.width, 3), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8)
        flags = _lib.DISPLAY_HOST | (_lib.DISPLAY_KEEP if keep else 0)
        self._check(self._L.rz_display(self._c, None if dp is None else C.byref(dp), None if src is None else src.ctypes.data,
                                       0 if src is None else src.nbytes, out.ctypes.data, out.nbytes, rgba8.ctypes.data,
                                       rgba8.nbytes, flags), "rz_display")
        return out, rgba8

    def display_device(self, rgb_in_ptr=None, rgb32f_ptr=None, rgba8_ptr=None, *, keep=False, **params):
        """rz_display on device memory (4-byte aligned; each optional): enqueued on the context's stream, asynchronous -- the
        exposure is metered, adapted and applied without visiting the host.  Sizes: rgb_in and rgb32f W*H*12 B, rgba8 W*H*4 B."""
        dp = self._display_params(**params)
        n = self.width * self.height
        self._check(self._L.rz_display(self._c, None if dp is None else C.byref(dp), C.c_void_p(rgb_in_ptr),
                                       n * 12 if rgb_in_ptr else 0, C.c_void_p(rgb32f_ptr), n * 12 if rgb32f_ptr else 0,
                                       C.c_void_p(rgba8_ptr), n * 4 if rgba8_ptr else 0, _lib.DISPLAY_KEEP if keep else 0),
                    "rz_display")

    def present_display(self, source="accum", fps=0.0, show_fps=True, show_lights=False, show_bvh=False, bvh_mode=0,
                        selected_blas=0, selected_tri=0, filter=None, **params):
        """present() behind the display stage: the colour of `source` ("accum", "denoise": denoise()'s, "temporal":
        denoise_temporal()'s, whose history advances) is exposed, toned and encoded (params: as display()), and the overlays are
        drawn on top.  filter: a dict of the denoiser's own parameters (present_denoised's / present_temporal's).  Returns (rgb
        float32 (H,W,3), rgba8 uint8 (H,W,4)); with no display parameters, present()'s / present_denoised()'s /
        present_temporal()'s bytes."""
        if source not in _lib.DISPLAY_SOURCES:
            raise ValueError(f"source = {source!r}: one of {sorted(_lib.DISPLAY_SOURCES)}")
        if source == "accum" and filter:
            raise ValueError("filter parameters need source 'denoise' or 'temporal'")
        p = _lib.PresentParams(float(fps), int(bool(show_fps)), int(bool(show_lights)), int(bool(show_bvh)),
                               int(bvh_mode), int(selected_blas), int(selected_tri))
        dp = self._display_params(**params)
        fp = None
        if source == "denoise":
            f = dict(filter or {})
            fp = self._denoise_params(*(f.pop(k, None) for k in ("iterations", "sigma_color", "sigma_normal", "sigma_plane", "demodulate")))
            if f:
                raise TypeError(f"unknown denoise parameter(s): {sorted(f)}")
        elif source == "temporal":
            fp = self._temporal_params(dict(filter or {}))
        rgb = np.empty((self.height, self.width, 3), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rz_present_display(self._c, C.byref(p), None if dp is None else C.byref(dp),
                                               _lib.DISPLAY_SOURCES[source], fp, rgba8.ctypes.data, rgba8.nbytes,
                                               rgb.ctypes.data, rgb.nbytes), "rz_present_display")
        return rgb, rgba8

    def display_state(self):
        """rz_display_state (synchronises): dict(exposure, target, log2_mean, counted, below, above, histogram (128,) uint32) --
        the exposure last applied and what the last metered call saw.  A fresh state: exposure = target = 1."""
        info = _lib.DisplayInfo()
        self._check(self._L.rz_display_state(self._c, C.byref(info)), "rz_display_state")
        return dict(exposure=np.float32(info.exposure), target=np.float32(info.target), log2_mean=np.float32(info.log2_mean),
                    counted=int(info.counted), below=int(info.below), above=int(info.above),
                    histogram=np.array(info.histogram, np.uint32))

    def display_reset(self):
        """Drops the adapted exposure: the next metered call jumps to its target."""
        self._check(self._L.rz_display_reset(self._c), "rz_display_reset")

    # -- glare (rz_bloom / rz_present_bloomed) -------------------------
    @staticmethod
    def _bloom_params(threshold=1.0, knee=0.5, limit=64.0, intensity=0.25, spread=1.0, levels=6):
        """rz_bloom_params from the keyword arguments of bloom() / present_bloomed(), every field checked here (ValueError);
        None (params NULL) when nothing departs from the defaults."""
        def finite0(name, v):
            v = float(v)
            if not (0.0 <= v < float("inf")):
                raise ValueError(f"{name} = {v!r}: must be finite and >= 0")
            return v

        p = _lib.BloomParams()
        p.threshold, p.knee, p.intensity = finite0("threshold", threshold), finite0("knee", knee), finite0("intensity", intensity)
        if not float(limit) > 0.0:
            raise ValueError(f"limit = {limit!r}: must be > 0 (inf: none)")
        p.limit = float(limit)
        if not 0.0 < float(spread) <= 4.0:
            raise ValueError(f"spread = {spread!r}: outside (0, 4]")
        p.spread = float(spread)
        if not 1 <= int(levels) <= _lib.BLOOM_MAX_LEVELS:
            raise ValueError(f"levels = {levels!r}: outside 1..{_lib.BLOOM_MAX_LEVELS}")
        p.levels = int(levels)
        return None if bytes(p) == bytes(_lib.BloomParams(**_lib.BLOOM_DEFAULTS)) else p

    def bloom(self, rgb=None, glare=False, **params):
        """HDR glare (include/rayzen_hip.h: rz_bloom) on rgb ((H, W, 3) float32 linear colour) or, with rgb None, on the
        accumulation; host memory, returns when done.  params: threshold=1.0, knee=0.5, limit=64.0, intensity=0.25, spread=1.0,
        levels=6.  Returns the frame with glare ((H, W, 3) float32, linear, unclamped: what display() takes), or with glare=True
        (frame, the normalised glare alone); row 0 = bottom row."""
        bp = self._bloom_params(**params)
        src = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
        out = np.empty((self.height, self.width, 3), np.float32)
        gl = np.empty((self.height, self.width, 3), np.float32) if glare else None
        self._check(self._L.rz_bloom(self._c, None if bp is None else C.byref(bp), None if src is None else src.ctypes.data,
                                     0 if src is None else src.nbytes, out.ctypes.data, out.nbytes,
                                     None if gl is None else gl.ctypes.data, 0 if gl is None else gl.nbytes, _lib.BLOOM_HOST),
                    "rz_bloom")
        return (out, gl) if glare else out

    def bloom_device(self, rgb_in_ptr=None, rgb32f_ptr=None, glare_ptr=None, **params):
        """rz_bloom on device memory (4-byte aligned; rgb_in None: the accumulation; each output optional, at least one; rgb32f
        may be rgb_in): enqueued on the context's stream, asynchronous.  Sizes: W*H*12 B each."""
        bp = self._bloom_params(**params)
        n = self.width * self.height * 12
        self._check(self._L.rz_bloom(self._c, None if bp is None else C.byref(bp), C.c_void_p(rgb_in_ptr), n if rgb_in_ptr else 0,
                                     C.c_void_p(rgb32f_ptr), n if rgb32f_ptr else 0, C.c_void_p(glare_ptr), n if glare_ptr else 0, 0),
                    "rz_bloom")

    def present_bloomed(self, source="accum", bloom=None, filter=None, fps=0.0, show_fps=True, show_lights=False, show_bvh=False,
                        bvh_mode=0, selected_blas=0, selected_tri=0, **params):
        """present_display() with the glare between the source's colour and the display stage, which runs -- metering included --
        on the bloomed colour.  bloom: a dict of bloom()'s parameters (None: the defaults); filter and params: present_display()'s.
        Returns (rgb float32 (H,W,3), rgba8 uint8 (H,W,4)); with bloom=dict(intensity=0), present_display()'s bytes."""
        if source not in _lib.DISPLAY_SOURCES:
            raise ValueError(f"source = {source!r}: one of {sorted(_lib.DISPLAY_SOURCES)}")
        if source == "accum" and filter:
            raise ValueError("filter parameters need source 'denoise' or 'temporal'")
        p = _lib.PresentParams(float(fps), int(bool(show_fps)), int(bool(show_lights)), int(bool(show_bvh)),
                               int(bvh_mode), int(selected_blas), int(selected_tri))
        dp = self._display_params(**params)
        bp = self._bloom_params(**dict(bloom or {}))
        fp = None
        if source == "denoise":
            f = dict(filter or {})
            fp = self._denoise_params(*(f.pop(k, None) for k in ("iterations", "sigma_color", "sigma_normal", "sigma_plane", "demodulate")))
            if f:
                raise TypeError(f"unknown denoise parameter(s): {sorted(f)}")
        elif source == "temporal":
            fp = self._temporal_params(dict(filter or {}))
        rgb = np.empty((self.height, self.width, 3), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rz_present_bloomed(self._c, C.byref(p), None if dp is None else C.byref(dp),
                                               None if bp is None else C.byref(bp), _lib.DISPLAY_SOURCES[source], fp,
                                               rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data, rgb.nbytes), "rz_present_bloomed")
        return rgb, rgba8

    # -- guided upsampling (rz_upscale / rz_present_upscaled) -------------------------
    @staticmethod
    def _upscale_params(factor, sigma_normal, sigma_plane, demodulate):
        # all None: the library's defaults (params NULL)
        if factor is None and sigma_normal is None and sigma_plane is None and demodulate is None:
            return None
        d = _lib.UPSCALE_DEFAULTS
        p = _lib.UpscaleParams()
        p.factor = d["factor"] if factor is None else int(factor)
        p.sigma_normal = d["sigma_normal"] if sigma_normal is None else float(sigma_normal)
        p.sigma_plane = d["sigma_plane"] if sigma_plane is None else float(sigma_plane)
        p.demodulate = d["demodulate"] if demodulate is None else int(bool(demodulate))
        return p

    @staticmethod
    def _seethrough_params(see_through):
        # True: the library's default depth; an int: max_depth (the library checks the range)
        p = _lib.SeethroughParams()
        p.max_depth = _lib.SEETHROUGH_DEFAULTS["max_depth"] if see_through is True else int(see_through)
        return p

    def upscale(self, rgb=None, factor=None, sigma_normal=None, sigma_plane=None, demodulate=None, guides=False, see_through=None,
                chains=False):
        """Guided upsampling (include/rayzen_hip.h: rz_upscale) of rgb ((h, w, 3) float32 linear colour, what denoise() and
        denoise_temporal() return) or, with rgb None, of the accumulation: the frame of the last set_frame is the LOW frame w x h,
        the result is (factor * h, factor * w, 3) float32, reconstructed from a G-buffer cast at that size (host memory; returns
        when done).  With guides=True also that G-buffer as (H, W) HIT_DTYPE records (what trace_rays returns for the pixel-centre
        rays of editor_rays at W x H); row 0 = bottom row.  Parameters left None take the library's defaults (factor 2,
        sigma_normal 128, sigma_plane 1, demodulate on).
        see_through = 0..8 (or True: 8) takes rz_upscale_seethrough instead: the guide follows glass and perfect mirrors for at
        most that many steps; the guides are then the FINAL hits with t = the length of the chain, and chains=True appends the
        (H, W) CHAIN_DTYPE records (throughput, k | (m_first + 1) << 8).  None is rz_upscale."""
        up = self._upscale_params(factor, sigma_normal, sigma_plane, demodulate)
        s = _lib.UPSCALE_DEFAULTS["factor"] if up is None else up.factor
        src = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
        out = np.empty((max(s, 0) * self.height, max(s, 0) * self.width, 3), np.float32)
        hh = np.empty(out.shape[:2], HIT_DTYPE) if guides else None
        if see_through is not None:
            st = self._seethrough_params(see_through)
            ch = np.empty(out.shape[:2], CHAIN_DTYPE) if chains else None
            self._check(self._L.rz_upscale_seethrough(
                self._c, None if up is None else C.byref(up), C.byref(st), None if src is None else src.ctypes.data,
                0 if src is None else src.nbytes, out.ctypes.data, out.nbytes, None if hh is None else hh.ctypes.data,
                0 if hh is None else hh.nbytes, None if ch is None else ch.ctypes.data, 0 if ch is None else ch.nbytes,
                _lib.UPSCALE_HOST), "rz_upscale_seethrough")
            res = (out,) + ((hh,) if guides else ()) + ((ch,) if chains else ())
            return res if len(res) > 1 else out
        if chains:
            raise ValueError("chains=True needs see_through")
        self._check(self._L.rz_upscale(self._c, None if up is None else C.byref(up), None if src is None else src.ctypes.data,
                                       0 if src is None else src.nbytes, out.ctypes.data, out.nbytes,
                                       None if hh is None else hh.ctypes.data, 0 if hh is None else hh.nbytes, _lib.UPSCALE_HOST),
                    "rz_upscale")
        return (out, hh) if guides else out

    def upscale_device(self, rgb_in_ptr=None, rgb32f_ptr=None, guides_ptr=None, factor=None, sigma_normal=None, sigma_plane=None,
                       demodulate=None, see_through=None, chains_ptr=None):
        """rz_upscale on device memory (guides 16-B aligned, rgb_in and rgb32f 4-B; each optional): enqueued on the context's
        stream, asynchronous.  Sizes: rgb_in w*h*12 B, rgb32f W*H*12 B, guides W*H*48 B, with W x H = factor * (w x h).
        see_through = 0..8 (or True): rz_upscale_seethrough, with chains_ptr (W*H*16 B, 16-B aligned) optional."""
        up = self._upscale_params(factor, sigma_normal, sigma_plane, demodulate)
        s = _lib.UPSCALE_DEFAULTS["factor"] if up is None else up.factor
        n = self.width * self.height
        N = n * s * s
        if see_through is not None:
            st = self._seethrough_params(see_through)
            self._check(self._L.rz_upscale_seethrough(
                self._c, None if up is None else C.byref(up), C.byref(st), C.c_void_p(rgb_in_ptr), n * 12 if rgb_in_ptr else 0,
                C.c_void_p(rgb32f_ptr), N * 12 if rgb32f_ptr else 0, C.c_void_p(guides_ptr), N * 48 if guides_ptr else 0,
                C.c_void_p(chains_ptr), N * 16 if chains_ptr else 0, 0), "rz_upscale_seethrough")
            return
        if chains_ptr:
            raise ValueError("chains_ptr needs see_through")
        self._check(self._L.rz_upscale(self._c, None if up is None else C.byref(up), C.c_void_p(rgb_in_ptr), n * 12 if rgb_in_ptr else 0,
                                       C.c_void_p(rgb32f_ptr), N * 12 if rgb32f_ptr else 0, C.c_void_p(guides_ptr),
                                       N * 48 if guides_ptr else 0, 0), "rz_upscale")

    def present_upscaled(self, source="accum", factor=None, sigma_normal=None, sigma_plane=None, demodulate=None, fps=0.0,
                         show_fps=True, show_lights=False, show_bvh=False, bvh_mode=0, selected_blas=0, selected_tri=0,
                         filter=None, see_through=None, **params):
        """present_display() at display size: the colour of `source` (as present_display: the denoisers run at the low size
        w x h of the last set_frame) is upsampled by `factor`, then exposed, toned and encoded (params: as display()), and the
        overlays are drawn at the high size.  Returns (rgb float32 (H,W,3), rgba8 uint8 (H,W,4)) with H x W = factor * (h x w);
        factor=1 gives present_display()'s bytes.  see_through = 0..8 (or True): rz_present_upscaled_seethrough, the upscale with
        guides that follow glass and perfect mirrors (the denoisers keep their first-hit guides)."""
        if source not in _lib.DISPLAY_SOURCES:
            raise ValueError(f"source = {source!r}: one of {sorted(_lib.DISPLAY_SOURCES)}")
        if source == "accum" and filter:
            raise ValueError("filter parameters need source 'denoise' or 'temporal'")
        p = _lib.PresentParams(float(fps), int(bool(show_fps)), int(bool(show_lights)), int(bool(show_bvh)),
                               int(bvh_mode), int(selected_blas), int(selected_tri))
        up = self._upscale_params(factor, sigma_normal, sigma_plane, demodulate)
        s = _lib.UPSCALE_DEFAULTS["factor"] if up is None else up.factor
        dp = self._display_params(**params)
        fp = None
        if source == "denoise":
            f = dict(filter or {})
            fp = self._denoise_params(*(f.pop(k, None) for k in ("iterations", "sigma_color", "sigma_normal", "sigma_plane", "demodulate")))
            if f:
                raise TypeError(f"unknown denoise parameter(s): {sorted(f)}")
        elif source == "temporal":
            fp = self._temporal_params(dict(filter or {}))
        rgb = np.empty((max(s, 0) * self.height, max(s, 0) * self.width, 3), np.float32)
        rgba8 = np.empty(rgb.shape[:2] + (4,), np.uint8)
        if see_through is not None:
            st = self._seethrough_params(see_through)
            self._check(self._L.rz_present_upscaled_seethrough(
                self._c, C.byref(p), None if up is None else C.byref(up), C.byref(st), None if dp is None else C.byref(dp),
                _lib.DISPLAY_SOURCES[source], fp, rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data, rgb.nbytes),
                "rz_present_upscaled_seethrough")
            return rgb, rgba8
        self._check(self._L.rz_present_upscaled(self._c, C.byref(p), None if up is None else C.byref(up),
                                                None if dp is None else C.byref(dp), _lib.DISPLAY_SOURCES[source], fp,
                                                rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data, rgb.nbytes), "rz_present_upscaled")
        return rgb, rgba8

    # -- anti-aliased edges (rz_antialias / rz_present_antialiased) -------------------
    @staticmethod
    def _antialias_params(factor, sigma_normal, sigma_plane, demodulate, edge_normal, edge_plane):
        # all None: the library's defaults (params NULL)
        given = dict(factor=factor, sigma_normal=sigma_normal, sigma_plane=sigma_plane, demodulate=demodulate,
                     edge_normal=edge_normal, edge_plane=edge_plane)
        if all(v is None for v in given.values()):
            return None
        p = _lib.AntialiasParams()
        for k, v in given.items():
            d = _lib.ANTIALIAS_DEFAULTS[k]
            setattr(p, k, d if v is None else (int(bool(v)) if k == "demodulate" else type(d)(v)))
        return p

    def antialias(self, rgb=None, factor=None, sigma_normal=None, sigma_plane=None, demodulate=None, edge_normal=None,
                  edge_plane=None, guides=False, edges=False, see_through=None, chains=False):
        """Edge anti-aliasing (include/rayzen_hip.h: rz_antialias) of rgb ((h, w, 3) float32 linear colour) or, with rgb None, of
        the accumulation, at the size of the last set_frame: a pixel with a geometric edge in its 3 x 3 neighbourhood becomes the
        mean of factor x factor sub-pixel reconstructions, every other pixel keeps its colour bit for bit (host memory; returns
        when done).  guides=True appends the frame-size G-buffer as (h, w) HIT_DTYPE records, edges=True the (h, w) bool edge
        mask; row 0 = bottom row.  Parameters left None take the library's defaults (factor 2, sigma_normal 128, sigma_plane 1,
        demodulate on, edge_normal 0.9, edge_plane 1).
        see_through = 0..8 (or True: 8) takes rz_antialias_seethrough instead: the pass classifies and reconstructs on guides
        that follow glass and perfect mirrors for at most that many steps, so edges seen through them are smoothed too; the
        guides are then the FINAL hits with t = the length of the chain, and chains=True appends the (h, w) CHAIN_DTYPE records
        after the guides.  None is rz_antialias."""
        ap = self._antialias_params(factor, sigma_normal, sigma_plane, demodulate, edge_normal, edge_plane)
        src = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
        out = np.empty((self.height, self.width, 3), np.float32)
        hh = np.empty(out.shape[:2], HIT_DTYPE) if guides else None
        ee = np.empty(out.shape[:2], np.uint8) if edges else None
        if see_through is not None:
            st = self._seethrough_params(see_through)
            ch = np.empty(out.shape[:2], CHAIN_DTYPE) if chains else None
            self._check(self._L.rz_antialias_seethrough(
                self._c, None if ap is None else C.byref(ap), C.byref(st), None if src is None else src.ctypes.data,
                0 if src is None else src.nbytes, out.ctypes.data, out.nbytes, None if hh is None else hh.ctypes.data,
                0 if hh is None else hh.nbytes, None if ch is None else ch.ctypes.data, 0 if ch is None else ch.nbytes,
                None if ee is None else ee.ctypes.data, 0 if ee is None else ee.nbytes, _lib.ANTIALIAS_HOST), "rz_antialias_seethrough")
            res = (out,) + ((hh,) if guides else ()) + ((ch,) if chains else ()) + ((ee.astype(bool),) if edges else ())
            return res if len(res) > 1 else out
        if chains:
            raise ValueError("chains=True needs see_through")
        self._check(self._L.rz_antialias(self._c, None if ap is None else C.byref(ap), None if src is None else src.ctypes.data,
                                         0 if src is None else src.nbytes, out.ctypes.data, out.nbytes,
                                         None if hh is None else hh.ctypes.data, 0 if hh is None else hh.nbytes,
                                         None if ee is None else ee.ctypes.data, 0 if ee is None else ee.nbytes,
                                         _lib.ANTIALIAS_HOST), "rz_antialias")
        res = (out,) + ((hh,) if guides else ()) + ((ee.astype(bool),) if edges else ())
        return res if len(res) > 1 else out

    def antialias_device(self, rgb_in_ptr=None, rgb32f_ptr=None, guides_ptr=None, edges_ptr=None, factor=None, sigma_normal=None,
                         sigma_plane=None, demodulate=None, edge_normal=None, edge_plane=None, see_through=None, chains_ptr=None):
        """rz_antialias on device memory (guides 16-B aligned, rgb_in and rgb32f 4-B and distinct; each optional): enqueued on
        the context's stream, asynchronous.  Sizes: rgb_in and rgb32f w*h*12 B, guides w*h*48 B, edges w*h B.
        see_through = 0..8 (or True): rz_antialias_seethrough, with chains_ptr (w*h*16 B, 16-B aligned) optional."""
        ap = self._antialias_params(factor, sigma_normal, sigma_plane, demodulate, edge_normal, edge_plane)
        n = self.width * self.height
        if see_through is not None:
            st = self._seethrough_params(see_through)
            self._check(self._L.rz_antialias_seethrough(
                self._c, None if ap is None else C.byref(ap), C.byref(st), C.c_void_p(rgb_in_ptr), n * 12 if rgb_in_ptr else 0,
                C.c_void_p(rgb32f_ptr), n * 12 if rgb32f_ptr else 0, C.c_void_p(guides_ptr), n * 48 if guides_ptr else 0,
                C.c_void_p(chains_ptr), n * 16 if chains_ptr else 0, C.c_void_p(edges_ptr), n if edges_ptr else 0, 0),
                "rz_antialias_seethrough")
            return
        if chains_ptr:
            raise ValueError("chains_ptr needs see_through")
        self._check(self._L.rz_antialias(self._c, None if ap is None else C.byref(ap), C.c_void_p(rgb_in_ptr),
                                         n * 12 if rgb_in_ptr else 0, C.c_void_p(rgb32f_ptr), n * 12 if rgb32f_ptr else 0,
                                         C.c_void_p(guides_ptr), n * 48 if guides_ptr else 0, C.c_void_p(edges_ptr),
                                         n if edges_ptr else 0, 0), "rz_antialias")

    def present_antialiased(self, source="accum", factor=None, sigma_normal=None, sigma_plane=None, demodulate=None,
                            edge_normal=None, edge_plane=None, fps=0.0, show_fps=True, show_lights=False, show_bvh=False,
                            bvh_mode=0, selected_blas=0, selected_tri=0, filter=None, see_through=None, **params):
        """present_display() with the anti-aliasing pass between the source and the display stage: the colour of `source` (as
        present_display) is anti-aliased, then exposed, toned and encoded (params: as display()), and the overlays are drawn on
        top.  Returns (rgb float32 (H,W,3), rgba8 uint8 (H,W,4)); factor=1 gives present_display()'s bytes.  see_through = 0..8
        (or True): rz_present_antialiased_seethrough, the pass on guides that follow glass and perfect mirrors (the denoisers
        keep their first-hit guides)."""
        if source not in _lib.DISPLAY_SOURCES:
            raise ValueError(f"source = {source!r}: one of {sorted(_lib.DISPLAY_SOURCES)}")
        if source == "accum" and filter:
            raise ValueError("filter parameters need source 'denoise' or 'temporal'")
        p = _lib.PresentParams(float(fps), int(bool(show_fps)), int(bool(show_lights)), int(bool(show_bvh)),
                               int(bvh_mode), int(selected_blas), int(selected_tri))
        ap = self._antialias_params(factor, sigma_normal, sigma_plane, demodulate, edge_normal, edge_plane)
        dp = self._display_params(**params)
        fp = None
        if source == "denoise":
            f = dict(filter or {})
            fp = self._denoise_params(*(f.pop(k, None) for k in ("iterations", "sigma_color", "sigma_normal", "sigma_plane", "demodulate")))
            if f:
                raise TypeError(f"unknown denoise parameter(s): {sorted(f)}")
        elif source == "temporal":
            fp = self._temporal_params(dict(filter or {}))
        rgb = np.empty((self.height, self.width, 3), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8)
        if see_through is not None:
            st = self._seethrough_params(see_through)
            self._check(self._L.rz_present_antialiased_seethrough(
                self._c, C.byref(p), None if ap is None else C.byref(ap), C.byref(st), None if dp is None else C.byref(dp),
                _lib.DISPLAY_SOURCES[source], fp, rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data, rgb.nbytes),
                "rz_present_antialiased_seethrough")
            return rgb, rgba8
        self._check(self._L.rz_present_antialiased(self._c, C.byref(p), None if ap is None else C.byref(ap),
                                                   None if dp is None else C.byref(dp), _lib.DISPLAY_SOURCES[source], fp,
                                                   rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data, rgb.nbytes),
                    "rz_present_antialiased")
        return rgb, rgba8

    # -- where a frame is expensive (rz_render_cost / rz_cost_view / rz_present_cost) ------
    @staticmethod
    def _cost_params(spp):
        if spp is None:
            return None
        p = _lib.CostParams()
        p.spp = int(spp)
        return C.byref(p)

    @staticmethod
    def _cost_view_params(metric, curve, scale):
        p = _lib.CostViewParams()
        p.metric = _lib.COST_METRICS[metric] if isinstance(metric, str) else int(metric)
        p.curve = _lib.COST_CURVES[curve] if isinstance(curve, str) else int(curve)
        p.scale = float(scale)
        return p

    def render_cost(self, spp=None, totals=False):
        """The per-pixel traversal cost map (include/rayzen_hip.h: rz_render_cost) of the frame of the last set_frame: (H, W)
        PIXEL_COST_DTYPE records, row 0 = bottom row -- what the reference shader would touch for samples 0 .. spp-1 of each pixel
        (spp None: the frame's).  Touches no render state; the context keeps the map for cost_view / present_cost.  With
        totals=True also the frame's counters as render_counted returns them at sample_base 0."""
        out = np.empty((self.height, self.width), PIXEL_COST_DTYPE)
        cnt = _lib.Counters() if totals else None
        self._check(self._L.rz_render_cost(self._c, self._cost_params(spp), out.ctypes.data, out.nbytes,
                                           None if cnt is None else C.byref(cnt), _lib.COST_HOST), "rz_render_cost")
        return (out, {n: int(getattr(cnt, n)) for n in _lib.COUNTER_FIELDS}) if totals else out

    def render_cost_device(self, ptr=None, spp=None, totals=False):
        """rz_render_cost on device memory (ptr: W*H*32 B, 16-B aligned, or None to keep the context's copy only): enqueued on the
        context's stream.  totals=True waits for the kernel and returns the counters."""
        cnt = _lib.Counters() if totals else None
        self._check(self._L.rz_render_cost(self._c, self._cost_params(spp), C.c_void_p(ptr), self.width * self.height * 32 if ptr else 0,
                                           None if cnt is None else C.byref(cnt), 0), "rz_render_cost")
        return {n: int(getattr(cnt, n)) for n in _lib.COUNTER_FIELDS} if totals else None

    def cost_view(self, cost=None, metric="bytes", curve="linear", scale=0.0, stats=False):
        """A cost map as a false colour (rz_cost_view): (H, W, 3) float32, black - blue - green - yellow - red from 0 to `scale`
        (0: the frame's maximum), white above a caller's scale.  cost None: the context's last map.  metric: "bytes", "nodes",
        "triangles", "traversals" or "instances"; curve: "linear" or "log".  With stats=True also a dict of max_value, sum_value,
        max_x, max_y (the lowest pixel index among the maxima; row 0 = bottom) and scale_used."""
        vp = self._cost_view_params(metric, curve, scale)
        src = None if cost is None else np.ascontiguousarray(cost, PIXEL_COST_DTYPE)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        st = _lib.CostStats() if stats else None
        self._check(self._L.rz_cost_view(self._c, C.byref(vp), None if src is None else src.ctypes.data,
                                         0 if src is None else src.nbytes, rgb.ctypes.data, rgb.nbytes,
                                         None if st is None else C.addressof(st), _lib.COST_HOST), "rz_cost_view")
        if not stats:
            return rgb
        return rgb, dict(max_value=int(st.max_value), sum_value=int(st.sum_value), max_x=int(st.max_x), max_y=int(st.max_y),
                         scale_used=float(st.scale_used))

    def cost_view_device(self, rgb32f_ptr=None, stats_ptr=None, cost_ptr=None, metric="bytes", curve="linear", scale=0.0):
        """rz_cost_view on device memory (cost 16-B, stats 8-B, rgb32f 4-B aligned; each optional): enqueued on the context's
        stream.  Sizes: cost W*H*32 B, rgb32f W*H*12 B, stats 32 B."""
        vp = self._cost_view_params(metric, curve, scale)
        n = self.width * self.height
        self._check(self._L.rz_cost_view(self._c, C.byref(vp), C.c_void_p(cost_ptr), n * 32 if cost_ptr else 0,
                                         C.c_void_p(rgb32f_ptr), n * 12 if rgb32f_ptr else 0, C.c_void_p(stats_ptr), 0),
                    "rz_cost_view")

    def present_cost(self, metric="bytes", curve="linear", scale=0.0, fps=0.0, show_fps=True, show_lights=False, show_bvh=False,
                     bvh_mode=0, selected_blas=0, selected_tri=0):
        """present() with the heat map of the context's last cost map in place of the resolve: the overlays are drawn on top.
        Returns (rgb float32 (H,W,3), rgba8 uint8 (H,W,4))."""
        p = _lib.PresentParams(float(fps), int(bool(show_fps)), int(bool(show_lights)), int(bool(show_bvh)),
                               int(bvh_mode), int(selected_blas), int(selected_tri))
        vp = self._cost_view_params(metric, curve, scale)
        rgb = np.empty((self.height, self.width, 3), np.float32)
        rgba8 = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rz_present_cost(self._c, C.byref(p), C.byref(vp), rgba8.ctypes.data, rgba8.nbytes, rgb.ctypes.data,
                                            rgb.nbytes), "rz_present_cost")
        return rgb, rgba8

    # -- selecting what is on screen (rz_coverage / rz_outline) ---------------------------
    def _coverage_args(self, frame, rect):
        fp = self._frame if frame is None else frame
        if fp is None:
            raise ValueError("coverage: no frame given and set_frame has not been called")
        if rect is None:
            return fp, None
        p = _lib.CoverageParams()
        p.x0, p.y0, p.x1, p.y1 = (int(v) for v in rect)
        return fp, C.byref(p)

    def n_instances(self):
        """How many instances binding 9 holds: coverage returns one record more."""
        need = C.c_size_t(0)
        self._check(self._L.rz_read_binding(self._c, int(BIND_INSTANCES), None, 0, C.byref(need)), "rz_read_binding")
        return need.value // BINDING_DTYPES[BIND_INSTANCES].itemsize

    def coverage(self, frame=None, rect=None, want_ids=False):
        """Which instances the screen shows, where and how near (include/rayzen_hip.h: rz_coverage), for the pixel-centre rays of
        `frame` (frame_params(...); None: the frame of the last set_frame) inside rect = (x0, y0, x1, y1), pixels [x0, x1) x
        [y0, y1) with row 0 = the bottom row (None: the whole frame).  Returns n + 1 INSTANCE_COVERAGE_DTYPE records -- record i
        is instance i, the last one the misses -- and with want_ids=True also the id image (H, W) int32: the instance of every
        pixel inside the rectangle, -1 for a miss and for the pixels outside it.  Host memory; returns when done."""
        fp, cp = self._coverage_args(frame, rect)
        rec = np.empty(self.n_instances() + 1, INSTANCE_COVERAGE_DTYPE)
        ids = np.full((fp.height, fp.width), -1, np.int32) if want_ids else None
        self._check(self._L.rz_coverage(self._c, C.byref(fp), cp, rec.ctypes.data, rec.nbytes, None if ids is None else ids.ctypes.data,
                                        0 if ids is None else ids.nbytes, _lib.COVERAGE_HOST), "rz_coverage")
        return (rec, ids) if want_ids else rec

    def coverage_device(self, coverage_ptr=None, coverage_bytes=0, ids_ptr=None, frame=None, rect=None):
        """rz_coverage on device memory (coverage: (n + 1) * 32 B, 16-B aligned; ids: W*H*4 B, 4-B aligned; either may be None):
        enqueued on the context's stream, asynchronous.  Pixels of ids outside the rectangle are not written."""
        fp, cp = self._coverage_args(frame, rect)
        self._check(self._L.rz_coverage(self._c, C.byref(fp), cp, C.c_void_p(coverage_ptr), int(coverage_bytes) if coverage_ptr else 0,
                                        C.c_void_p(ids_ptr), fp.width * fp.height * 4 if ids_ptr else 0, 0), "rz_coverage")

    def select_rect(self, rect, min_pixels=1, frame=None):
        """The marquee: [(instance, pixels), ...] of the instances that are the closest hit of at least min_pixels pixels of rect,
        the most pixels first, ties by the lower index."""
        px = self.coverage(frame, rect)["pixels"][:-1]
        hit = np.flatnonzero(px >= max(int(min_pixels), 1))
        order = np.lexsort((hit, -px[hit].astype(np.int64)))
        return [(int(hit[k]), int(px[hit[k]])) for k in order]

    @staticmethod
    def selection_bits(selected, n_instances=None):
        """rz_outline's bit set of an iterable of instance indices: (words uint32, n_instances) with bit i & 31 of word i >> 5
        set for every i; n_instances None: the largest index + 1."""
        sel = sorted({int(i) for i in selected})
        if sel and sel[0] < 0:
            raise ValueError(f"selection_bits: negative instance index {sel[0]}")
        n = (sel[-1] + 1 if sel else 0) if n_instances is None else int(n_instances)
        words = np.zeros((n + 31) // 32, np.uint32)
        for i in sel:
            if i < n:
                words[i >> 5] |= np.uint32(1 << (i & 31))
        return words, n

    @staticmethod
    def _outline_params(width, height, radius, color, alpha):
        p = _lib.OutlineParams()
        p.width, p.height, p.radius = int(width), int(height), int(radius)
        p.color[:] = [float(v) for v in color]
        p.alpha = float(alpha)
        return p

    def outline(self, ids, selected, rgba8=None, rgb32f=None, radius=2, color=(1.0, 0.6, 0.0), alpha=1.0):
        """Marks the instances of `selected` (an iterable of instance indices) on an image (rz_outline): the pixels within
        `radius` of a selected pixel of ids ((H, W) int32: coverage's id image, or the instance field of a hit buffer) that are
        not selected themselves are blended towards `color` by `alpha`.  rgba8 (H, W, 4) uint8 and rgb32f (H, W, 3) float32, each
        optional, are not modified: returns (rgba8, rgb32f) as blended copies, None for the one not given.  Needs no scene."""
        idm = np.ascontiguousarray(ids, np.int32)
        h, w = idm.shape
        words, n = self.selection_bits(selected)
        out8 = None if rgba8 is None else np.array(rgba8, np.uint8, order="C").reshape(h, w, 4)
        out32 = None if rgb32f is None else np.array(rgb32f, np.float32, order="C").reshape(h, w, 3)
        p = self._outline_params(w, h, radius, color, alpha)
        self._check(self._L.rz_outline(self._c, C.byref(p), idm.ctypes.data, idm.nbytes, words.ctypes.data if n else None, n,
                                       None if out8 is None else out8.ctypes.data, 0 if out8 is None else out8.nbytes,
                                       None if out32 is None else out32.ctypes.data, 0 if out32 is None else out32.nbytes,
                                       _lib.OUTLINE_HOST), "rz_outline")
        return out8, out32

    def outline_device(self, width, height, ids_ptr, selected_ptr, n_instances, rgba8_ptr=None, rgb32f_ptr=None, radius=2,
                       color=(1.0, 0.6, 0.0), alpha=1.0):
        """rz_outline on device memory, in place (4-B aligned; ids W*H*4 B, selected (n_instances + 31) // 32 words, rgba8 W*H*4 B,
        rgb32f W*H*12 B): enqueued on the context's stream, asynchronous."""
        p = self._outline_params(width, height, radius, color, alpha)
        n = int(width) * int(height)
        self._check(self._L.rz_outline(self._c, C.byref(p), C.c_void_p(ids_ptr), n * 4, C.c_void_p(selected_ptr), int(n_instances),
                                       C.c_void_p(rgba8_ptr), n * 4 if rgba8_ptr else 0, C.c_void_p(rgb32f_ptr),
                                       n * 12 if rgb32f_ptr else 0, 0), "rz_outline")

    # -- drawing into the scene (rz_draw_lines) -------------------------------------------
    def _lines_args(self, frame, width, near_w, depth_bias, hidden_alpha, smooth):
        fp = self._frame if frame is None else frame
        if fp is None:
            raise ValueError("draw_lines: no frame given and set_frame has not been called")
        p = _lib.LinesParams()
        p.width, p.near_w, p.depth_bias, p.hidden_alpha, p.smooth = float(width), float(near_w), float(depth_bias), float(hidden_alpha), int(smooth)
        return fp, p

    def draw_lines(self, lines, rgba8=None, rgb32f=None, hits=None, frame=None, width=1.5, near_w=0.01, depth_bias=2.0 ** -8,
                   hidden_alpha=0.0, smooth=False):
        """Blends `lines` (LINE_DTYPE records: rayzen_amd.lines makes them) over an image as seen through `frame`
        (frame_params(...); None: the frame of the last set_frame), include/rayzen_hip.h: rz_draw_lines.  hits: (H, W) HIT_DTYPE,
        render_editor's hits or a denoiser's guides, the depth the lines are tested against; None: no depth test.  rgba8
        (H, W, 4) uint8 and rgb32f (H, W, 3) float32, each optional, are not modified: returns (rgba8, rgb32f) as blended
        copies, None for the one not given.  A scene is needed only if a line names an instance."""
        fp, p = self._lines_args(frame, width, near_w, depth_bias, hidden_alpha, smooth)
        h, w = fp.height, fp.width
        ln = np.ascontiguousarray(lines, _lib.LINE_DTYPE).reshape(-1)
        ht = None if hits is None else np.ascontiguousarray(hits, HIT_DTYPE).reshape(h, w)
        out8 = None if rgba8 is None else np.array(rgba8, np.uint8, order="C").reshape(h, w, 4)
        out32 = None if rgb32f is None else np.array(rgb32f, np.float32, order="C").reshape(h, w, 3)
        self._check(self._L.rz_draw_lines(self._c, C.byref(fp), C.byref(p), ln.ctypes.data if len(ln) else None, len(ln),
                                          None if ht is None else ht.ctypes.data, 0 if ht is None else ht.nbytes,
                                          None if out8 is None else out8.ctypes.data, 0 if out8 is None else out8.nbytes,
                                          None if out32 is None else out32.ctypes.data, 0 if out32 is None else out32.nbytes,
                                          _lib.LINES_HOST), "rz_draw_lines")
        return out8, out32

    def draw_lines_device(self, lines_ptr, n, rgba8_ptr=None, rgb32f_ptr=None, hits_ptr=None, frame=None, width=1.5, near_w=0.01,
                          depth_bias=2.0 ** -8, hidden_alpha=0.0, smooth=False):
        """rz_draw_lines on device memory, in place (lines n * 32 B and hits W*H*48 B, 16-B aligned; rgba8 W*H*4 B and rgb32f
        W*H*12 B, 4-B aligned): enqueued on the context's stream."""
        fp, p = self._lines_args(frame, width, near_w, depth_bias, hidden_alpha, smooth)
        npx = fp.width * fp.height
        self._check(self._L.rz_draw_lines(self._c, C.byref(fp), C.byref(p), C.c_void_p(lines_ptr), int(n), C.c_void_p(hits_ptr),
                                          npx * 48 if hits_ptr else 0, C.c_void_p(rgba8_ptr), npx * 4 if rgba8_ptr else 0,
                                          C.c_void_p(rgb32f_ptr), npx * 12 if rgb32f_ptr else 0, 0), "rz_draw_lines")

    # -- ambient occlusion for previews (rz_ambient_occlusion) ---------------------------
    def _ao_args(self, frame, samples, radius, smooth, strength, normal_cos, plane_tol):
        fp = self._frame if frame is None else frame
        if fp is None:
            raise ValueError("ambient_occlusion: no frame given and set_frame has not been called")
        p = _lib.AoParams()
        p.samples, p.radius, p.smooth, p.strength = int(samples), float(radius), int(smooth), float(strength)
        p.normal_cos, p.plane_tol = float(normal_cos), float(plane_tol)
        return fp, p

    def ambient_occlusion(self, frame=None, rgb=None, samples=4, radius=1.0, smooth=True, strength=1.0, normal_cos=0.9,
                          plane_tol=2.0, want=("ao",)):
        """Distance-limited ambient occlusion of the pixel-centre hits of `frame` (frame_params(...); None: the frame of the last
        set_frame), include/rayzen_hip.h: rz_ambient_occlusion.  rgb: an (H, W, 3) float32 image to darken (render_editor's
        rgb32f), None: white.  want: which of "ao" ((H, W) float32), "rgb32f" ((H, W, 3) float32) and "rgba8" ((H, W, 4) uint8)
        to return; a dict of them.  Host memory; returns when done."""
        fp, p = self._ao_args(frame, samples, radius, smooth, strength, normal_cos, plane_tol)
        h, w = fp.height, fp.width
        src = None if rgb is None else np.ascontiguousarray(rgb, np.float32).reshape(h, w, 3)
        shapes = {"ao": ((h, w), np.float32), "rgb32f": ((h, w, 3), np.float32), "rgba8": ((h, w, 4), np.uint8)}
        unknown = set(want) - set(shapes)
        if unknown:
            raise ValueError(f"ambient_occlusion: unknown outputs {sorted(unknown)}")
        out = {k: np.empty(*shapes[k]) for k in shapes if k in want}
        ptr = {k: (out[k].ctypes.data, out[k].nbytes) if k in out else (None, 0) for k in shapes}
        self._check(self._L.rz_ambient_occlusion(self._c, C.byref(fp), C.byref(p), None if src is None else src.ctypes.data,
                                                 0 if src is None else src.nbytes, *ptr["ao"], *ptr["rgb32f"], *ptr["rgba8"],
                                                 _lib.AO_HOST), "rz_ambient_occlusion")
        return out

    def ambient_occlusion_device(self, frame=None, rgb_in_ptr=None, ao_ptr=None, rgb32f_ptr=None, rgba8_ptr=None, samples=4,
                                 radius=1.0, smooth=True, strength=1.0, normal_cos=0.9, plane_tol=2.0):
        """rz_ambient_occlusion on device memory (4-B aligned; rgb_in and rgb32f W*H*12 B, ao and rgba8 W*H*4 B; each may be None,
        not all three outputs): enqueued on the context's stream, asynchronous."""
        fp, p = self._ao_args(frame, samples, radius, smooth, strength, normal_cos, plane_tol)
        n = fp.width * fp.height
        self._check(self._L.rz_ambient_occlusion(self._c, C.byref(fp), C.byref(p), C.c_void_p(rgb_in_ptr), n * 12 if rgb_in_ptr else 0,
                                                 C.c_void_p(ao_ptr), n * 4 if ao_ptr else 0, C.c_void_p(rgb32f_ptr),
                                                 n * 12 if rgb32f_ptr else 0, C.c_void_p(rgba8_ptr), n * 4 if rgba8_ptr else 0, 0),
                    "rz_ambient_occlusion")

    # -- adaptive sampling (rz_render_adaptive) -------------------------------------------
    @staticmethod
    def _adaptive_args(batch_spp, min_batches, max_batches, threshold, luminance_floor, merge_gap, max_runs, flags):
        p = _lib.AdaptiveParams()
        p.batch_spp, p.min_batches, p.max_batches = int(batch_spp or 0), int(min_batches or 0), int(max_batches or 0)
        p.threshold, p.luminance_floor = float(threshold or 0.0), float(luminance_floor or 0.0)
        # (0 tiles: the header's -1; None: the default)
        p.merge_gap = 0 if merge_gap is None else (-1 if int(merge_gap) == 0 else int(merge_gap))
        p.max_runs, p.flags = int(max_runs or 0), flags
        return p

    @staticmethod
    def _adaptive_info(info):
        n = info.batches
        return dict(batches=n, n_tiles=info.n_tiles, samples_traced=int(info.samples_traced), samples_uniform=int(info.samples_uniform),
                    render_ms=float(info.render_ms), meter_ms=float(info.meter_ms), tiles_active=list(info.tiles_active[:n]),
                    tiles_rendered=list(info.tiles_rendered[:n]), runs=list(info.runs[:n]))

    def render_adaptive(self, batch_spp=None, min_batches=None, max_batches=None, threshold=None, luminance_floor=None, merge_gap=None,
                        max_runs=None):
        """The frame of the last set_frame in batches of batch_spp samples, sampling on only the 8 x 8 tiles whose estimated error
        is above `threshold` (include/rayzen_hip.h: rz_render_adaptive; None: the default).  The result is the accumulation
        (read_accum, present, ...: a is each pixel's own sample count).  Returns (info, tile_batches, tile_error): a dict of
        rz_adaptive_info's fields with the per-batch lists cut to the batches run, the batches every tile received ((tilesY,
        tilesX) int32, row 0 = bottom) and its last error E (float32).  The frame's spp and sample_base are ignored.  Returns
        when the frame is complete.  A zero stands for the default in every field of rz_adaptive_params, so threshold=0.0 is the
        default 0.02, not "retire at E = 0" (pass a negative threshold to retire nothing); merge_gap is the exception here:
        merge_gap=0 means what it says, no merging across gaps (the header's -1), and None the default."""
        p = self._adaptive_args(batch_spp, min_batches, max_batches, threshold, luminance_floor, merge_gap, max_runs, _lib.ADAPTIVE_HOST)
        ty, tx = (self.height + 7) // 8, (self.width + 7) // 8
        batches, error = np.empty((ty, tx), np.int32), np.empty((ty, tx), np.float32)
        info = _lib.AdaptiveInfo()
        self._check(self._L.rz_render_adaptive(self._c, C.byref(p), C.byref(info), batches.ctypes.data, batches.nbytes,
                                               error.ctypes.data, error.nbytes), "rz_render_adaptive")
        return self._adaptive_info(info), batches, error

    def render_adaptive_device(self, tile_batches_ptr=None, tile_error_ptr=None, batch_spp=None, min_batches=None, max_batches=None,
                               threshold=None, luminance_floor=None, merge_gap=None, max_runs=None):
        """rz_render_adaptive with the per-tile outputs in device memory (4-B aligned, tiles * 4 B each; each may be None).  The
        call still returns when the frame is complete: the plan of every batch is made on the host.  Returns the info dict."""
        p = self._adaptive_args(batch_spp, min_batches, max_batches, threshold, luminance_floor, merge_gap, max_runs, 0)
        n = ((self.height + 7) // 8) * ((self.width + 7) // 8) * 4
        info = _lib.AdaptiveInfo()
        self._check(self._L.rz_render_adaptive(self._c, C.byref(p), C.byref(info), C.c_void_p(tile_batches_ptr),
                                               n if tile_batches_ptr else 0, C.c_void_p(tile_error_ptr), n if tile_error_ptr else 0),
                    "rz_render_adaptive")
        return self._adaptive_info(info)

    # -- convenience -----------------------------------------------------------
    def render_scene(self, scene, width, height, spp, bounce_budget, num_lights=None, tile_rank=0, tile_nranks=1,
                     chunk=None):
        """Upload-free helper: set the frame for `scene.camera` and render spp samples (optionally in
        chunks of `chunk` samples -- bit-identical to one call)."""
        nl = len(scene.lights) if num_lights is None else num_lights
        chunk = spp if not chunk else chunk
        base = 0
        while base < spp:
            k = min(chunk, spp - base)
            self.set_frame(frame_params(scene.camera, width, height, nl, bounce_budget, k, base, tile_rank, tile_nranks))
            self.render()
            base += k


def algorithmic_bytes(c):
    """the bytes RayZen's shader touches for these counts
    (its SSBO element sizes: 32-B node, 4-B TLAS index, 144-B instance, 64-B triangle + 4-B index,
    32-B material, 32-B light, 16-B RGBA32F pixel)."""
    return (32 * c["tlas_nodes"] + 4 * c["tlas_leaf_indices"] + 144 * c["instances"] + 32 * c["blas_nodes"]
            + 68 * c["triangles"] + 32 * c["materials"] + 32 * c["light_fetches"] + 16 * c["pixels"])

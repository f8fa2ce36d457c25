/*
 * rayzen_hip.h -- C-ABI of the MI355X (gfx950) path-tracing render loop.
 *
 * This is the drop-in boundary for RayZen's render hot path.  RayZen (the
 * reference, cited as file:line relative to /root/reference/RayZen) has no
 * FFI of its own for this path: its frontend talks to the GPU through raw
 * OpenGL calls.  Every entry point below replaces one group of those calls,
 * and every struct is byte-for-byte the element type of one of RayZen's
 * SSBOs (C++ layout == std430 layout), so a frontend hands over the very
 * same std::vector<T>::data() pointers it gives to glBufferData today.
 *
 * Plain C, plain pointers and sizes.  No C++ exception crosses this ABI:
 * every call returns RZ_OK (0) or a negative rz_status and records a message
 * readable through rz_last_error().  A context is externally synchronised
 * (one thread at a time), like the single GL context of the reference.
 */
#ifndef RAYZEN_HIP_H
#define RAYZEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* SSBO element types (the data contract).                                   */
/* ------------------------------------------------------------------------ */

/* include/Mesh.h:9-17, shaders/fragment_shader.glsl:30-38.  64 B, align 16.
 * Vertices are in OBJECT space (src/main.cpp:971-972). */
typedef struct rz_triangle {
    float v0[3]; float pad0;
    float v1[3]; float pad1;
    float v2[3]; float pad2;
    int32_t materialIndex;
    int32_t tail_pad[3];
} rz_triangle;

/* include/BVH.h:7-12, fragment_shader.glsl:40-45.  32 B.
 * internal: count == -1, children at leftFirst and leftFirst+1;
 * leaf:     count in [1,4] (0 for an empty mesh), leftFirst = first slot in
 *           the index array (src/BVH.cpp:115-118,166-171). */
typedef struct rz_bvh_node {
    float boundsMin[3]; int32_t leftFirst;
    float boundsMax[3]; int32_t count;
} rz_bvh_node;

/* include/BVH.h:14-21, fragment_shader.glsl:86-93.  144 B.
 * mat4 are column-major (GLM / GLSL convention). */
typedef struct rz_bvh_instance {
    int32_t blasNodeOffset;
    int32_t blasTriOffset;
    int32_t meshIndex;
    int32_t globalTriOffset;
    float   transform[16];
    float   inverseTransform[16];
} rz_bvh_instance;

/* include/Material.h:6-18, fragment_shader.glsl:15-22.  32 B. */
typedef struct rz_material {
    float albedo[3];
    float metallic;
    float roughness;
    float reflectivity;
    float transparency;
    float ior;
} rz_material;

/* include/Light.h:6-13, fragment_shader.glsl:24-28.  32 B.
 * positionOrDirection.w == 1 -> point light, otherwise directional. */
typedef struct rz_light {
    float positionOrDirection[4];
    float color[3];
    float power;
} rz_light;

/* Binding points: the numeric values ARE the GL SSBO binding indices of the
 * reference (fragment_shader.glsl:47-96, src/main.cpp:1072-1119).  Bindings
 * 3 and 4 are dead in the reference and do not exist here. */
typedef enum rz_binding {
    RZ_BIND_TRIANGLES    = 0,  /* rz_triangle[]      */
    RZ_BIND_MATERIALS    = 1,  /* rz_material[]      */
    RZ_BIND_LIGHTS       = 2,  /* rz_light[]         */
    RZ_BIND_TLAS_NODES   = 5,  /* rz_bvh_node[]      */
    RZ_BIND_TLAS_INDICES = 6,  /* int32[] instance ids */
    RZ_BIND_BLAS_NODES   = 7,  /* rz_bvh_node[] (all meshes concatenated) */
    RZ_BIND_BLAS_INDICES = 8,  /* int32[] mesh-local triangle ids */
    RZ_BIND_INSTANCES    = 9   /* rz_bvh_instance[]  */
} rz_binding;

typedef enum rz_status {
    RZ_OK                 =  0,
    RZ_ERR_INVALID_ARG    = -1,
    RZ_ERR_NO_DEVICE      = -2,
    RZ_ERR_HIP            = -3,  /* a HIP runtime call failed */
    RZ_ERR_OUT_OF_RANGE   = -4,  /* rz_update past the end of a binding */
    RZ_ERR_NOT_READY      = -5,  /* render before all bindings / frame set */
    RZ_ERR_BAD_SCENE      = -6,  /* uploaded arrays are inconsistent */
    RZ_ERR_BUFFER_SIZE    = -7,  /* caller buffer too small */
    RZ_ERR_NO_MEMORY      = -8,  /* a host allocation failed inside the library (std::bad_alloc never crosses the ABI) */
    RZ_ERR_INTERNAL       = -9   /* a render kernel (or a ray query) reached one of its "cannot happen" bounds: pixels may be missing (rz_sync reports it) */
} rz_status;

/* Per-frame parameters = the uniforms of sendSceneDataToShader
 * (src/main.cpp:1356-1379; fragment_shader.glsl:4-13,100,105) plus the three
 * knobs the reference hard-codes (spp: `numSamples = 1`, fragment_shader.glsl:675)
 * or does not have (sample_base, tile sharding).  Matrices are column-major.
 * The traced radiance reads only inv_view, inv_proj and cam_pos
 * (fragment_shader.glsl:208-211,714); view/proj ride along for the
 * resolve/overlay stage. */
typedef struct rz_frame_params {
    int32_t width, height;      /* `resolution` */
    float   inv_view[16];
    float   inv_proj[16];
    float   view[16];
    float   proj[16];
    float   cam_pos[3];
    int32_t num_lights;         /* `numLights` */
    int32_t bounce_budget;      /* `uniformBounceBudget`; <= 0 means 5 (glsl:673) */
    int32_t spp;                /* samples per pixel rendered by one rz_render */
    int32_t sample_base;        /* first sample index; 0 resets per-pixel state */
    int32_t tile_rank;          /* this context renders tiles t with          */
    int32_t tile_nranks;        /*   t % tile_nranks == tile_rank (1 => all)  */
} rz_frame_params;

#define RZ_TILE_W 8             /* pixel tile = one wavefront: 8 x 8 pixels */
#define RZ_TILE_H 8

/* Counters of the REFERENCE algorithm's memory touches (what the fragment
 * shader would read from its SSBOs), used to price the roofline. Filled by
 * rz_render_counted().  bytes = 32*tlas_nodes + 4*tlas_leaf_indices +
 * 144*instances + 32*blas_nodes + 68*triangles + 32*materials +
 * 32*light_fetches + 16*pixels  (SURVEY.md section 8d). */
typedef struct rz_counters {
    uint64_t samples;           /* camera paths started                      */
    uint64_t traversals;        /* traverseTLAS calls (primary+shadow+bounce) */
    uint64_t tlas_nodes;        /* tlasNodes[] elements popped               */
    uint64_t tlas_leaf_indices; /* tlasTriIndices[] elements read            */
    uint64_t instances;         /* bvhInstances[] elements entered           */
    uint64_t blas_nodes;        /* blasNodes[] elements popped               */
    uint64_t triangles;         /* hitTriangle calls (index + triangle read) */
    uint64_t materials;         /* materials[] fetches                       */
    uint64_t light_fetches;     /* lights[] fetches                          */
    uint64_t pixels;            /* accumulation-buffer pixels written        */
    /* units of the shading side (round 4: the work model of bench.py prices them instead of bounding them) */
    uint64_t scatters;          /* FS:720-761 executed (a segment that hit)   */
    uint64_t diffuse_scatters;  /* ... of them through FS:755 (hemisphere)    */
    uint64_t hemi_draws;        /* ... of those with a non-zero seed (FS:193-195 evaluated; bounce 0 draws a constant) */
    uint64_t lit_lights;        /* (point, light) pairs whose BRDF term was evaluated (FS:589-607 / 636-659) */
    uint64_t triangles_past_u;  /* hitTriangle calls that pass FS:396-401 (|a|, u range) and run the second half */
} rz_counters;

typedef struct rz_ctx rz_ctx;

/* glfwCreateWindow/MakeContextCurrent (main.cpp:228-241) / teardown (681-686).
 * device = HIP device ordinal.  flags: RZ_FLAG_* below.  Returns NULL on
 * failure (query rz_last_error(NULL)). */
#define RZ_FLAG_NONE          0u  /* default: one lane per sample (rz_render_samples)                         */
#define RZ_FLAG_MEGAKERNEL    1u  /* one lane per pixel, samples in sequence (rz_render_pixels): cross-check  */
#define RZ_FLAG_HOST_RELAYOUT 4u  /* re-lay the scene out on the host instead of on the device (same bytes; cross-check) */
rz_ctx*     rz_create(int device, unsigned flags);
void        rz_destroy(rz_ctx* ctx);
const char* rz_last_error(const rz_ctx* ctx);

/* glGenBuffers + glBufferData + glBindBufferBase (main.cpp:1072-1119).
 * Allocates device storage for the binding and copies `bytes` from host
 * memory; the host pointer is not retained. `bytes` must be a multiple of
 * the binding's element size; 0 is allowed (empty binding). */
int rz_upload(rz_ctx* ctx, rz_binding binding, const void* data, size_t bytes);

/* glBufferSubData (main.cpp:1196-1207): in-place refresh of
 * [offset, offset+bytes) of a binding uploaded before. */
int rz_update(rz_ctx* ctx, rz_binding binding, size_t offset,
              const void* data, size_t bytes);

/* updateDynamicBVHAndSSBOs (main.cpp:1138-1194) done ON THE DEVICE: hand over only the per-instance transforms
 * (n x 16 floats, column-major, n == number of uploaded instances); the library inverts them, recomputes the world
 * AABBs (main.cpp:1168-1191) and rebuilds the TLAS (BVH.cpp:178-240) in one small kernel.  The result is byte-identical
 * to what the host library (SceneBuffers::updateDynamic, librayzen_host.so) produces and rz_read_binding returns it.
 * Inverses and world boxes follow GLM 0.9.9's evaluation order, which is what RayZen's own code executes at
 * main.cpp:974-1001 and 1150-1191: glm::inverse = compute_inverse<4, 4> (the eighteen 2x2 sub-determinants, cofactor
 * columns with alternating signs, the determinant from the cofactors' first row summed pairwise, every cofactor times
 * its reciprocal) and mat4 * vec4 = (m0 x + m1 y) + (m2 z + m3 w).  GLM is not vendored with the reference and is absent
 * from this image, so this is a RESTATEMENT of its published algorithm (rz_linalg.h on the host, rz_tlas_device.hip on
 * the device; the CPU checker states it a third time), pinned by hand-derived known answers in tests/test_linalg_glm.py -- not a run of
 * GLM.  Synchronises the context's stream (the TLAS depth sizes the next launch). */
int rz_update_transforms(rz_ctx* ctx, const float* transforms, size_t n);

/* BVH::buildBLAS (RayZen/src/BVH.cpp:99-175 with the full-sweep SAH of :22-97; called per mesh from main.cpp:954-958)
 * on the device.  Output is byte-identical to the reference builder's `nodes` / `triIndices`: nodes_out receives
 * *n_nodes <= 2n-1 nodes (nodes_cap >= 2n-1, or 1 for n == 0), indices_out n triangle indices.  depth and device_ms
 * (device time, host<->device copies excluded) may be NULL.  tris / outputs are host pointers.
 * Supported: n up to 2^30 (more: RZ_ERR_INVALID_ARG) and finite coordinates only -- no NaN and no infinity: the reference's
 * std::sort is undefined on a NaN centroid; magnitudes whose box areas overflow binary32 are fine and take the reference's
 * midpoint fallback.  The tree may be of ANY depth: the builder has no level bound of its own, so n identical triangles
 * build to the n - 3 levels the reference gives them (one level costs one small round trip to the device: 4200
 * zero-area triangles, 4197 levels, take half a second).  rz_build_geometry and rz_rebuild_geometry run the same builder
 * under the same terms; rz_render rejects a scene whose BLAS is too deep for its stack (RZ_ERR_BAD_SCENE), which is
 * a limit of the traversal, not of the build. */
int rz_build_blas(rz_ctx* ctx, const rz_triangle* tris, size_t n, rz_bvh_node* nodes_out, size_t nodes_cap,
                  int32_t* indices_out, size_t* n_nodes, int* depth, float* device_ms);

/* initializeSSBOs' geometry half (main.cpp:951-972, 1030-1035) without the host in the middle: builds the BLAS of every
 * mesh on the device (the builder of rz_build_blas), concatenates nodes and indices THERE, and makes the results the
 * context's bindings 0, 7 and 8 -- equivalent to BVH::buildBLAS per mesh + rz_upload of the three concatenated arrays,
 * same bytes, but the node / index arrays never visit the host (rz_read_binding fetches them if asked; at 1 M triangles
 * the round trip was 28 of rz_build_blas's 36 ms).  `triangles` holds all meshes' triangles back to back; mesh i is
 * triangles[first_triangle .. +n_triangles).  Per mesh the call returns what an instance of it needs: blasNodeOffset,
 * blasTriOffset (globalTriOffset is first_triangle) and the BLAS root node, whose box main.cpp:974-993 turns into the
 * instance's world box for the TLAS.  The frontend then uploads instances, TLAS, materials and lights as usual. */
typedef struct rz_mesh_build {
    size_t  first_triangle;  /* in  */
    size_t  n_triangles;     /* in  */
    int32_t node_offset;     /* out: blasNodeOffset */
    int32_t index_offset;    /* out: blasTriOffset  */
    int32_t n_nodes;         /* out */
    int32_t depth;           /* out */
    rz_bvh_node root;        /* out */
} rz_mesh_build;
int rz_build_geometry(rz_ctx* ctx, const rz_triangle* triangles, size_t n_triangles, rz_mesh_build* meshes, size_t n_meshes);

/* Deforming meshes: a BLAS REFIT on the device.  (No counterpart in the reference: RayZen re-uploads the triangle array
 * every frame, main.cpp:1196-1201, but builds each BLAS once, main.cpp:1125-1136, so moved vertices are culled by stale
 * boxes there -- and here too after rz_update on binding 0 alone.)
 *
 * Replaces elements [first_triangle, first_triangle + n_triangles) of binding 0 with `triangles` (all 64 bytes of each,
 * materialIndex included), then refits every mesh whose triangle range intersects that interval -- the whole mesh, not
 * only the touched leaves.  A mesh is a distinct (blasNodeOffset, blasTriOffset, globalTriOffset) among the uploaded
 * instances; its triangle range is [globalTriOffset, globalTriOffset + the slots its leaves name).  n_triangles == 0
 * (`triangles` may be NULL): every mesh is refitted from binding 0 as it stands -- what makes a preceding rz_update on
 * binding 0 correct.
 *
 * THE RESULT, for each refitted mesh, in binding 7 (leftFirst and count of every node and all of binding 8 unchanged):
 *   - a leaf's box is computeBounds (RayZen/src/BVH.cpp:11-19) over its own slots: start at (+FLT_MAX, -FLT_MAX), slots in
 *     order, bmin = glm::min(bmin, glm::min(v0, glm::min(v1, v2))), bmax likewise with glm::max, where
 *     glm::min(a, b) = (b < a) ? b : a and glm::max(a, b) = (a < b) ? b : a;
 *   - an internal node's box is glm::min(left.min, right.min), glm::max(left.max, right.max), except that a bound which
 *     compares equal to the one the node holds keeps the node's bits.  Only the sign of a zero can differ: BVH::buildBLAS
 *     folds a node's box over its triangles in the order they had before the node's range was sorted for its children
 *     (BVH.cpp:112, 131-133), which the children's union cannot reproduce;
 *   - a leaf with count == 0 (the root of an empty mesh) is left as it is.
 * This fixes every bit given the nodes in place, signs of zero and NaN planes included; BVH::refit / rzh_refit_blas (librayzen_host.so) state the
 * same on the host and the device result is held to their bytes.  A refit of an unmodified mesh reproduces the builder's
 * nodes, RayZen's own included (tests/test_cppref_gpu.py).
 *
 * Everything derived follows on the device, in place, without the re-layout and without a sort: the device copies of
 * the triangles and nodes, the leaf-ordered triangles and their normals, the child boxes of the traversal's node pairs,
 * the root box of every instance of the mesh, and -- with the transforms currently in force -- the world boxes and the
 * TLAS (the kernel of rz_update_transforms).  "A transparent material is in use" and "an irregular child box exists" come
 * out as a fresh upload would derive them.  Afterwards the context is indistinguishable from a fresh one that was given
 * the new binding 0 and the refitted binding 7 with everything else equal: rz_read_binding (host mirrors are fetched on
 * demand) and rz_debug_read_layout return the same bytes, and frames, ray queries, the editor preview, the denoiser's
 * guide and rz_present's wireframe are bit-identical.  No render state is touched (accumulation, currentIor, the frame,
 * pools, rz_debug_last_plan).  The geometry may have come from rz_upload or from rz_build_geometry; a context made with
 * RZ_FLAG_HOST_RELAYOUT patches its host copies and lets the host re-layout run (same bytes).
 *
 * `triangles` is DEVICE memory by default (16-byte aligned); the work is enqueued on the context's stream, ordered with
 * renders and queries on it, and the call synchronises that stream where rz_update_transforms does (the root boxes and
 * the TLAS depth come back).  With RZ_REFIT_HOST it is host memory and the pointer is not retained.
 *
 * RZ_ERR_INVALID_ARG: null context, NULL `triangles` with n_triangles > 0, a misaligned device pointer, unknown flags.
 * RZ_ERR_OUT_OF_RANGE: the interval reaches past the end of binding 0.  RZ_ERR_NOT_READY: a binding is missing.  These
 * launch nothing and leave the context as it was.  RZ_ERR_BAD_SCENE: where a fresh upload of the result would say so (a
 * materialIndex outside the materials: found on the device, so the triangles are in place by then, and every later
 * call reports the same until binding 0 or the materials are corrected).  RZ_ERR_NO_MEMORY as everywhere. */
#define RZ_REFIT_HOST 1u   /* `triangles` is host memory: staged through a context buffer */
int rz_refit_geometry(rz_ctx* ctx, const rz_triangle* triangles, size_t first_triangle, size_t n_triangles, unsigned flags);

/* Skinned meshes: the moved triangles of rz_refit_geometry PRODUCED on the device.  (No counterpart in the reference, which
 * deforms nothing.)  A RIG is context-owned device state for one triangle range of binding 0: a private copy of the range's
 * rest pose, per-corner bone indices and weights (linear-blend skinning) and / or morph targets (blend shapes).
 * rz_skin_create copies everything it is given to the device (`rest` NULL: what binding 0 holds in that range right now);
 * nothing of the caller's is retained, and *rig_out is an id that is never reused within the context.
 *
 * rz_skin_pose runs the skinning kernel (rz_skin.hip) from the rig's rest pose into a triangle buffer of the context and then
 * takes exactly the path of rz_refit_geometry(ctx, that buffer, first_triangle, n_triangles, 0): afterwards the context is
 * indistinguishable from one that was given the same triangles through rz_refit_geometry, and ordering, synchronisation
 * and RZ_ERR_BAD_SCENE (a bad materialIndex in the rest pose) are the refit's.  `bones` is n_bones x 16 floats, column-major
 * like rz_update_transforms; `morph_weights` is n_morphs floats; both are host memory that is not retained, or -- with
 * RZ_SKIN_DEVICE_ARGS -- device memory read on the context's stream (bones 16-byte aligned, morph_weights 4-byte aligned).
 * The rest pose is private to the rig, so posing is never cumulative.  Several rigs may exist on disjoint ranges;
 * rz_skin_destroy frees one, rz_destroy all of them.
 *
 * THE POSED TRIANGLE, bit for bit.  Binary32, one rounding per operation, no fused multiply-add.  All 64 bytes of the output
 * triangle are the rest triangle's -- materialIndex and every pad word included -- except the xyz of the three corners.  Per corner:
 *   morph   p = the rest corner; for k = 0 .. n_morphs-1 in order, per component c: p.c = p.c + w_k * d_k.c, with d_k the
 *           corner's delta in target k (rz_morph_triangle.d, 4th word ignored).  Every target is applied, a zero weight included.
 *   skin    with m the column-major matrix of a bone:  q.x = ((m[0]*p.x + m[4]*p.y) + m[8]*p.z) + m[12],
 *           q.y = ((m[1]*p.x + m[5]*p.y) + m[9]*p.z) + m[13],  q.z = ((m[2]*p.x + m[6]*p.y) + m[10]*p.z) + m[14]; the fourth
 *           row is ignored.  The corner's influences j = 0..3 are taken in order (bone index = bits 8j..8j+7 of the corner's word in
 *           rz_skin_triangle.bones, weight = weights[corner][j]): an influence whose weight compares equal to 0 is skipped and
 *           its bone is not read; the first kept influence gives out = w*q (three products), each later one out = out + w*q;
 *           with no influence kept -- and in a rig without bones -- out = p.
 * Weights are used as given: not normalised, negative and non-finite values flow through, and NaN or Inf in bones or weights
 * gives whatever this arithmetic gives.  rzh_skin_triangles (librayzen_host.so) states the same on the host and the device
 * result is held to its bytes.
 *
 * Every error below launches nothing and leaves the context as it was.  RZ_ERR_INVALID_ARG: a null context, NULL rig_out,
 * n_triangles == 0, n_bones outside 1..256 with `skin` (or != 0 without), skin == NULL with n_morphs == 0, a negative n_morphs,
 * NULL morphs with n_morphs > 0, an unknown (or destroyed) rig id, NULL bones for a rig with bones, NULL morph_weights for a rig
 * with morphs, unknown flags, misaligned device arguments.  RZ_ERR_NOT_READY: binding 0 has not been uploaded (at pose: any
 * binding the refit needs).  RZ_ERR_OUT_OF_RANGE: the range reaches past the end of binding 0 -- checked at create and again at
 * pose, since binding 0 may have been uploaded anew and smaller -- or, at create, the bone index of a kept influence is
 * >= n_bones (validated on the host there, so the kernel indexes without checks).  RZ_ERR_NO_MEMORY as everywhere.
 * rz_skin_last_kernel_ms: device time of the skinning kernel of the context's last successful rz_skin_pose (synchronises on
 * it); RZ_ERR_NOT_READY before the first.
 * (Additive: no existing struct changed, so RZ_ABI_VERSION stays 5.) */
typedef struct rz_skin_triangle {   /* 64 B, one per triangle of the rig; rz_sizeof(17) */
    uint32_t bones[3];              /* per corner v0,v1,v2: four 8-bit bone indices, influence j in bits 8j..8j+7 */
    uint32_t pad;
    float    weights[3][4];         /* per corner: the four weights */
} rz_skin_triangle;

typedef struct rz_morph_triangle {  /* 48 B, one per triangle per target; rz_sizeof(18) */
    float d[3][4];                  /* per corner: delta xyz, 4th word ignored */
} rz_morph_triangle;

#define RZ_SKIN_DEVICE_ARGS 1u   /* bones / morph_weights are device memory, read on the context's stream */
int rz_skin_create(rz_ctx* ctx, size_t first_triangle, size_t n_triangles,
                   const rz_triangle* rest,            /* host; NULL = binding 0's current content of that range */
                   const rz_skin_triangle* skin,       /* host; NULL = a morph-only rig */
                   int n_bones,                        /* 1..256 when skin != NULL, else 0 */
                   const rz_morph_triangle* morphs,    /* host, target-major [n_morphs][n_triangles]; NULL with n_morphs 0 */
                   int n_morphs, int* rig_out);
int rz_skin_pose(rz_ctx* ctx, int rig, const float* bones, const float* morph_weights, unsigned flags);
int rz_skin_destroy(rz_ctx* ctx, int rig);
int rz_skin_last_kernel_ms(rz_ctx* ctx, float* ms);

/* BLAS quality: how far the tree of every mesh has degraded, measured on the device.  (No counterpart in the reference, which
 * deforms nothing.)  rz_refit_geometry and rz_skin_pose keep a tree's topology while its boxes grow; the measure is the tree's
 * SAH cost, the quantity BVH::buildBLAS minimises greedily, next to the cost the same tree had when it was handed over.
 *
 * One record per mesh -- a distinct (blasNodeOffset, blasTriOffset, globalTriOffset) among the uploaded instances, however
 * many instances share it -- in ascending order of (node_offset_before, index_offset, tri_offset).  out == NULL: only
 * *n_meshes is set.  `cap` smaller than the mesh count: RZ_ERR_INVALID_ARG, nothing done.
 *
 * THE COST.  Area of a node's box, from its binary32 bounds in binding 7: d = (double)max - (double)min per axis,
 * A = 2 (dx dy + dy dz + dz dx) in binary64 (the expression of BVH.cpp:32-35); A = 0 when any d fails d >= 0 (an inverted or
 * NaN box, the count == 0 root of an empty mesh).  Over the nodes reachable from the mesh's root, with traversal and
 * intersection cost both 1:
 *     cost = (sum over internal nodes of A(n) + sum over leaves of A(n) * count) / A(root),     cost = 0 when A(root) == 0.
 * Infinities flow through IEEE arithmetic.  The order of the sum is not fixed; the result is within 1e-9 relative of the
 * exactly rounded sum (at most 2^21 non-negative terms x 2^-53 per addition, plus the few roundings per term), and two calls
 * on an unchanged context return identical bytes: the device sums per-workgroup partials that are stored and then added in
 * index order, without floating-point atomics (rz_quality.hip).  BVH::sahCost / rzh_blas_sah_cost (librayzen_host.so)
 * state the same on the host.
 *
 * sah_cost_built is the cost measured the first time the library looks at the mesh after its tree was last handed over or
 * built: after rz_upload / rz_update on binding 7 or 8, after rz_build_geometry, after an instance upload that introduces
 * a new triple.  rz_refit_geometry and rz_skin_pose take that look before they move a box of a mesh, on either of their
 * routes; upload -> refit -> refit -> quality therefore reports the uploaded tree's cost.  That look is one extra pass in the
 * first refit after a hand-over, the only thing existing calls gain, and it changes none of their results.
 *
 * The call needs the bindings the refit needs (else RZ_ERR_NOT_READY), brings a pending layout up to date as the refit
 * does, runs on the context's stream -- ordered with refits and renders on it -- and synchronises it, because the records
 * come back.  It touches no scene, layout or render state: rz_read_binding, rz_debug_read_layout, the accumulation buffer
 * and rz_debug_last_plan are byte-identical before and after.  A context whose layout is host-side (RZ_FLAG_HOST_RELAYOUT,
 * or the fallback) computes the same definition on its host copies.
 * (Additive: no existing struct changed, so RZ_ABI_VERSION stays 5.) */
#define RZ_QUALITY_REBUILT 1u           /* rz_mesh_quality::flags: this call rebuilt the mesh (rz_rebuild_geometry only) */
typedef struct rz_mesh_quality {        /* 64 B; rz_sizeof(20) */
    int32_t  node_offset, index_offset, tri_offset;  /* the mesh = its instances' (blasNodeOffset, blasTriOffset, globalTriOffset), AFTER the call */
    int32_t  node_offset_before;        /* blasNodeOffset before the call (differs only after a rebuild of this or an earlier mesh) */
    int32_t  n_triangles;               /* the slots its leaves name */
    int32_t  n_nodes;                   /* nodes reachable from its root */
    int32_t  depth;                     /* longest root-to-leaf path, in nodes (a root that is a leaf: 1) */
    uint32_t flags;                     /* RZ_QUALITY_REBUILT */
    double   sah_cost;                  /* of the tree as it stands after the call */
    double   sah_cost_built;            /* of the tree when it was last built or handed over (above) */
    double   sah_cost_before;           /* of the tree at entry (== sah_cost unless rebuilt) */
    double   reserved;                  /* 0 */
} rz_mesh_quality;
int rz_geometry_quality(rz_ctx* ctx, rz_mesh_quality* out, size_t cap, size_t* n_meshes);

/* The exit from the refit's steady state: rebuild, on the device, only the meshes whose tree has degraded, from binding 0 as it
 * stands there -- triangles posed by rz_skin_pose never visit the host -- with instances and TLAS following.
 *   1. measures as rz_geometry_quality does (same records, same `out` / `cap` / `n_meshes` rules);
 *   2. selects every mesh for which  sah_cost <= max_ratio * sah_cost_built  is false: max_ratio == 0 selects every mesh with
 *      a non-zero cost.  A greedy SAH rebuild is not always cheaper than the refitted tree, so the call reports both costs
 *      and promises no gain;
 *   3. nothing selected: the context is untouched, RZ_OK, all flags clear;
 *   4. else builds new bindings 7 and 8.  Meshes are taken in ascending blasNodeOffset; a mesh's node extent is
 *      [blasNodeOffset, the next larger distinct blasNodeOffset or the end of binding 7).  A selected mesh contributes
 *      BVH::buildBLAS (the device builder of rz_build_blas: RayZen's bytes) of triangles [globalTriOffset, + n_triangles) of
 *      binding 0, and its n_triangles indices go to [blasTriOffset, + n_triangles) of binding 8, which keeps its size; an
 *      unselected mesh contributes its extent verbatim (leftFirst is mesh-relative), shifted -- a rebuilt tree has another
 *      node count.  Nodes in front of the first mesh stay.  The blasNodeOffset of every instance is patched; nothing else in
 *      binding 9 changes.  Then the re-layout runs and world boxes and TLAS are rebuilt with the transforms in force,
 *      exactly as rz_refit_geometry does.  Where the layout is made on the device, builder and re-layout both read
 *      binding 0 from the device copy as it stands: it is neither fetched to the host nor uploaded again (a context with
 *      RZ_FLAG_HOST_RELAYOUT works on its host copies throughout).
 * Afterwards the context is indistinguishable from a fresh one given binding 0 as it stands and the new 7, 8 and 9, followed
 * by rz_update_transforms with the transforms in force: bindings, layout arrays, frames, ray queries, the editor preview,
 * the denoiser's guide and the wireframe.  (Closest-hit ties depend on visiting order, so frames on the rebuilt tree are
 * bit-identical to that fresh context's, not to frames on the refitted tree.)  Accumulation, currentIor, the frame and the
 * pools are untouched; rigs stay valid (they name triangle ranges) and a later rz_skin_pose refits the new tree;
 * rz_denoise_temporal's history is dropped when something was rebuilt, as after rz_build_geometry; sah_cost_built of a
 * rebuilt mesh becomes its new cost.  SceneBuffers::rebuildMesh / rzh_scene_rebuild_mesh (librayzen_host.so) produce the
 * same bytes on the host: what keeps a host mirror in step.
 * The call builds into fresh buffers and swaps them in last; any failure (RZ_ERR_NO_MEMORY, a HIP error) leaves the context
 * as it was.  RZ_ERR_INVALID_ARG, nothing changed: a negative or NaN max_ratio, flags != 0, a short `cap`, and a scene
 * that is not rebuildable this way -- a mesh's reachable nodes leave its extent, or two distinct triples share a node or
 * index extent (rz_geometry_quality still works there).  RZ_ERR_NOT_READY: a binding the refit needs is missing.
 * Synchronises the context's stream.  (Additive: RZ_ABI_VERSION stays 5.) */
int rz_rebuild_geometry(rz_ctx* ctx, double max_ratio, rz_mesh_quality* out, size_t cap, size_t* n_meshes, unsigned flags /* 0 */);

/* Copy a binding's current content back to the host in RayZen's own layout (after rz_update_transforms: the
 * instances / TLAS nodes / TLAS indices the device built).  out == NULL: only *needed is set. */
int rz_read_binding(rz_ctx* ctx, rz_binding binding, void* out, size_t bytes, size_t* needed);

/* glUniform* in sendSceneDataToShader (main.cpp:1356-1379).  A change of resolution or of the tile assignment
 * (tile_rank / tile_nranks) zeroes the whole accumulation buffer: pixels a context does not own always read as zero. */
int rz_set_frame(rz_ctx* ctx, const rz_frame_params* params);

/* Optional plumbing for a caller that owns the device memory and the stream
 * (e.g. a torch tensor reduced with RCCL): render on `hip_stream` (a
 * hipStream_t; NULL = the context's own stream) and accumulate into
 * `device_rgba` (width*height*4 floats, device memory; NULL = the context's
 * own buffer). */
int rz_set_stream(rz_ctx* ctx, void* hip_stream);
int rz_bind_accum(rz_ctx* ctx, void* device_rgba, size_t bytes);

/* glDrawArrays(GL_TRIANGLE_FAN,0,4) (main.cpp:637): asynchronous launch of
 * one path-tracing frame: params.spp samples for every pixel of the tiles
 * this context owns, ADDED to the accumulation buffer (RGBA32F; rgb = sum of
 * per-sample radiance before the reference's divide and clamp,
 * fragment_shader.glsl:772-773; a = number of samples).  sample_base == 0
 * first clears the owned pixels. */
int rz_render(rz_ctx* ctx);
/* Same frame, and additionally counts the reference algorithm's memory
 * touches (slower; never used for timing). */
int rz_render_counted(rz_ctx* ctx, rz_counters* out);
/* glFinish (main.cpp:1347). */
int rz_sync(rz_ctx* ctx);

/* Zero the whole accumulation buffer (all pixels, owned or not). */
int rz_clear_accum(rz_ctx* ctx);

/* The reference never reads pixels back; this is new.  Copies the RGBA32F
 * accumulation buffer to host.  Row 0 is the BOTTOM row (gl_FragCoord
 * origin).  Synchronises. */
int rz_read_accum(rz_ctx* ctx, float* rgba, size_t bytes);

/* color /= numSamples; clamp(0,1) (fragment_shader.glsl:772-773), then
 * 8-bit quantisation round(c*255) as the default framebuffer would.
 * Row 0 = bottom row.  Synchronises. */
int rz_resolve_rgba8(rz_ctx* ctx, uint8_t* rgba8, size_t bytes);

/* The rest of the shader's main() after the path loop (fragment_shader.glsl:772-819): resolve, then the overlays the
 * reference draws on top -- BVH wireframe (debugShowBVH/debugBVHMode/debugSelectedBLAS/debugSelectedTri,
 * glsl:98-104,214-373), light markers (debugShowLights, glsl:781-803) and the FPS digits (uniformFps, glsl:805-819;
 * the reference always draws them) -- and 8-bit quantisation.  rgba8 (width*height*4 bytes) and rgb32f
 * (width*height*3 floats: the colour before quantisation) may each be NULL.  Row 0 = bottom row.  Synchronises. */
typedef struct rz_present_params {
    float   fps;            /* uniformFps.  The digits are (int)fps and (int)(fract(fps) * 10), as the shader spells them;
                             * where that conversion is undefined -- fps non-finite (1 / dt with dt == 0) or
                             * |fps| >= 2^31 -- the value is taken as 0 and the digits read 000.0.  Every finite
                             * value below 2^31 in magnitude, negative ones included, is drawn as the shader would. */
    int32_t show_fps;       /* 1 = as the reference */
    int32_t show_lights;    /* debugShowLights */
    int32_t show_bvh;       /* debugShowBVH */
    int32_t bvh_mode;       /* debugBVHMode: 0 = TLAS leaves + BLAS roots, 1 = branch to one triangle */
    int32_t selected_blas;  /* debugSelectedBLAS (an instance index) */
    int32_t selected_tri;   /* debugSelectedTri (mesh-local triangle id) */
} rz_present_params;
int rz_present(rz_ctx* ctx, const rz_present_params* params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f,
               size_t rgb32f_bytes);

/* Wall-clock-free timing: milliseconds the render kernels of the LAST
 * rz_render spent on the GPU (HIP events on the stream they ran on), and how
 * many kernel launches that was.  Synchronises. */
int rz_last_render_ms(rz_ctx* ctx, float* ms, int* launches);
/* Every rz_render launch is bracketed by a HIP event pair on its stream (a ring of 64).  Copies the
 * durations (ms, oldest first) of the launches issued since the previous call -- at most `cap`,
 * at most 64 -- and returns how many; negative on error.  Synchronises on those events only, so a
 * timed loop can issue its launches back to back and collect their GPU times afterwards. */
int rz_render_history_ms(rz_ctx* ctx, float* ms, int cap);
/* Name of the render kernel the last rz_render used (the one those event pairs bracket): the library picks
 * "rz_render_samples" (one lane per sample; "rz_render_samples<glass>" when a triangle uses a transparent material
 * and currentIor is speculated) or "rz_render_pixels" (RZ_FLAG_MEGAKERNEL). */
const char* rz_last_kernel_name(const rz_ctx* ctx);

/* Device pointer of the accumulation buffer currently in use. */
void* rz_accum_device_ptr(rz_ctx* ctx);

/* TEST HOOK: make the nth host-side allocation site reached from now on (scene re-layout, upload copies, staging
 * vectors) fail as if memory had run out; the call in progress returns RZ_ERR_NO_MEMORY and the context stays usable.
 * nth <= 0 disarms. */
int rz_debug_fail_alloc(rz_ctx* ctx, int nth);

/* The HIP stream (hipStream_t) the context's work is enqueued on. */
void* rz_stream_handle(rz_ctx* ctx);

/* ------------------------------------------------------------------------ */
/* Multi-GPU group: tile-sharded rendering + ONE exchange step per frame.     */
/* ------------------------------------------------------------------------ */
/* The reference is single-GPU: its context lifetime is glfwCreateWindow / glfwMakeContextCurrent (main.cpp:228-241)
 * and the teardown at main.cpp:681-686.  A group is that lifetime for N GPUs of one node: it owns one rz_ctx per LOCAL
 * device and the RCCL communicator(s), gives member m the tiles t with t % nranks == rank(m) (rz_frame_params.tile_rank
 * / tile_nranks are filled in by the group), and lands the frame on the root rank with ONE exchange step over xGMI,
 * issued on the members' render streams (no host synchronisation between the render kernel and the exchange).  Two
 * exchange steps exist, both bit-identical to a single-GPU frame:
 *   "reduce" (the default; BASELINE.json's "single RCCL reduce on the accumulation buffer"): ONE ncclReduce(SUM) of the
 *            whole RGBA32F accumulation buffers -- tile sets are disjoint and non-owned pixels are zero, so the sum adds
 *            each pixel's single value to zeros;
 *   "gather" (RZ_GROUP_TRANSPORT=gather in the environment when the group is made, or rz_group_set_transport): every
 *            member packs the tiles it owns (1 / N of the frame) and sends them straight to the root (ncclSend /
 *            ncclRecv), which scatters the N sets into the frame; bits are copied, never added.  A gather whose enqueue
 *            fails makes the group fall back to "reduce" for the rest of its life (the frame still lands).
 * Every rank of a group must use the same one.
 *
 * Two ways to form a group:
 *   rz_group_create       one process drives ndev devices (ncclCommInitAll); ranks = 0..ndev-1, all local.
 *   rz_group_create_rank  one process per GPU (the usual launcher layout): every process passes its own device, its
 *                         rank, the group size and the 128-byte id that rank 0 obtained from rz_group_unique_id and
 *                         distributed by whatever channel the launcher has (ncclCommInitRank; blocks until all ranks
 *                         have called it).
 * RCCL is bound at run time, when the first group is created (librayzen_hip.so has no link-time dependency on the
 * 570-MB librccl, so single-GPU users never load it): an RCCL already loaded in the process is reused, else
 * $RZ_RCCL_LIBRARY, else /opt/rocm/lib/librccl.so.1.  rz_group_rccl_version() reports what was bound (no GPU needed). */
typedef struct rz_group rz_group;
#define RZ_GROUP_ID_BYTES 128
/* rz_group_create only, or-ed into `flags`: a REHEARSAL group -- `devices` may name a device more than once (N ranks on
 * one GPU), no communicator is made and device-to-device copies stand in for the links.  Everything else (the dealing
 * of tiles, packing, the root's scatter, stream ordering) is the code an N-GPU group runs. */
#define RZ_GROUP_LOOPBACK 0x10000u
int       rz_group_rccl_version(int* version);                 /* binds RCCL; *version = ncclGetVersion() */
int       rz_group_unique_id(void* id128);                      /* ncclGetUniqueId into RZ_GROUP_ID_BYTES bytes */
rz_group* rz_group_create(int ndev, const int* devices, unsigned flags);        /* devices NULL: 0..ndev-1 */
rz_group* rz_group_create_rank(int device, int rank, int nranks, const void* id128, unsigned flags);
void      rz_group_destroy(rz_group* g);
const char* rz_group_last_error(const rz_group* g);             /* g NULL: the error of a failed create */
int       rz_group_size(const rz_group* g);                     /* ranks in the communicator */
const char* rz_group_transport(const rz_group* g);              /* how rz_group_reduce moves the frame: "rccl-reduce" | "rccl-reduce(fallback: why)" | "tile-gather(...)" */
int       rz_group_set_transport(rz_group* g, const char* name); /* "reduce" | "gather", from the next rz_group_reduce on; the same call on EVERY rank */
int       rz_group_local_count(const rz_group* g);              /* members owned by this process */
int       rz_group_rank(const rz_group* g, int local);          /* global rank of local member `local` */
rz_ctx*   rz_group_ctx(rz_group* g, int local);                 /* the member's context (for per-device calls) */
/* glBufferData / glBufferSubData on every local member (the scene is replicated: <= 88 MB even for configs[4]). */
int rz_group_upload(rz_group* g, rz_binding binding, const void* data, size_t bytes);
int rz_group_update(rz_group* g, rz_binding binding, size_t offset, const void* data, size_t bytes);
/* sendSceneDataToShader for every local member; tile_rank / tile_nranks of *params are ignored and set per member. */
int rz_group_set_frame(rz_group* g, const rz_frame_params* params);
/* glDrawArrays on every local member: asynchronous, each on its own device and stream. */
int rz_group_render(rz_group* g);
/* The frame's exchange step (tile gather or ncclReduce, see above), enqueued on every member's stream behind its render
 * kernel, from the members' accumulation buffers into the root member's frame buffer (out of place: nobody's
 * accumulation buffer is overwritten, so frames can be continued with sample_base > 0). */
int rz_group_reduce(rz_group* g, int root);
int rz_group_sync(rz_group* g);                                 /* glFinish on every local member */
/* GPU time of the last rz_group_reduce, from HIP events recorded on each local member's stream just before and just
 * after its share of the collective was enqueued: *root_ms on the root member (-1 when the root lives in another
 * process), *max_ms the longest over this process's members.  A member's interval starts when its render kernel ends,
 * so it contains the wait for the slowest rank as well as the transfer.  Synchronises the members' streams. */
int rz_group_last_reduce_ms(rz_group* g, float* root_ms, float* max_ms);
/* Copy the reduced frame (RGBA32F, row 0 = bottom) to host memory.  Only valid in the process that owns `root` of the
 * last rz_group_reduce; RZ_ERR_NOT_READY elsewhere.  Synchronises that member's stream. */
int rz_group_read_frame(rz_group* g, float* rgba, size_t bytes);
/* Device pointer of the reduced frame on the root member (NULL in other processes). */
void* rz_group_frame_device_ptr(rz_group* g);

/* TEST HOOK: set bits of the context's backstop word as a render kernel that ran into one of its bounds would; the next
 * rz_sync returns RZ_ERR_INTERNAL naming them and clears the word. */
int rz_debug_poke_backstop(rz_ctx* ctx, unsigned bits);

/* TEST HOOK: the device-side scene layout as built (which = 0: DevPair[] 64 B each, 1: DevTri[] 48 B each, 2: TlasDfs[] 64 B
 * each -- the TLAS in the order the shader's loop pops it, the list every traversal walks, whether the host route made it
 * from bindings 10 / 11 or the device rebuild of rz_update_transforms / rz_refit_geometry / rz_rebuild_geometry /
 * rz_skin_pose did; rayzen_amd/csrc/hip/rz_scene_dev.h).  out NULL: only *needed is set.  Runs the pending re-layout first.
 * RZ_ERR_BUFFER_SIZE: `bytes` is less than the view holds; RZ_ERR_INVALID_ARG: which is not 0, 1 or 2. */
int rz_debug_read_layout(rz_ctx* ctx, int which, void* out, size_t bytes, size_t* needed);

/* TEST HOOK: how the last rz_render / rz_render_counted of this context was launched (rz_kernels.hip:
 * plan_render_samples).  A (pixel, 64-sample batch) pair is one "unit" of work; persistent launches hand their waves
 * `per_claim` pixel groups per atomic, compacting ones work off `claim_units`-unit claims. */
typedef struct rz_launch_plan {
    int64_t groups;             /* pixel groups of the launch (one wave's pixels: 1 pixel when spp >= 64, else 64 / spp) */
    int64_t grid;               /* workgroups launched (one wave each) */
    int32_t per_claim;          /* groups a persistent wave claims per atomic; 0 = one workgroup per group */
    int32_t claim_units;        /* units of a compacting claim (8 or 16); 0 = the launch does not compact */
    int32_t batches_per_pixel;  /* ceil(spp / 64) */
    int32_t pixels_per_wave;    /* 1, or 64 / spp when spp < 64 */
    int32_t lds_stack_entries;  /* BLAS stack entries per lane kept in LDS */
    int32_t overflow_entries;   /* ... and in the global overflow columns (0: the whole stack fits the LDS window) */
    int32_t transparent;        /* 1: the scene has a transparent material (the speculating variant of the kernel) */
    int32_t scratch_mib;        /* MiB of scratch the launch's resident waves own (pools of parked paths + wait slots); 0: none */
} rz_launch_plan;
int rz_debug_last_plan(rz_ctx* ctx, rz_launch_plan* out);

/* ------------------------------------------------------------------------ */
/* Batched ray queries on the uploaded scene (new: the reference has none).  */
/* ------------------------------------------------------------------------ */
/* The closest hit of FS:457-503 (traverseTLAS) and the transparency-aware visibility walk of FS:507-528 (shadowVisibility), for
 * rays of the caller's choosing, by the very traversal a frame uses: a hit is what a camera or shadow ray of the frame would
 * see.  The direction need not be unit.  t is the WORLD distance length(worldHit - origin) (FS:485); a triangle is accepted as
 * the shader accepts it (local t > 1e-4, |a| >= 1e-4: FS:391-416), and an instance whose BLAS is empty or invalid is never hit.
 * rz_ray.max_dist is read by rz_shadow_rays only (FS:517's maxDist; 1e30f for a directional light); rz_trace_rays ignores it.
 * A miss: t = 1e30f (the shader's initial tHit), material = instance = triangle = prim = -1, point and normal zero.
 *   instance  index into binding 9 (rz_bvh_instance)
 *   prim      index into binding 0 (rz_triangle) of the triangle hit
 *   triangle  prim - instances[instance].globalTriOffset: the mesh-local id rz_present_params.selected_tri names
 * Pointers are DEVICE memory (16-byte aligned) by default: the call is enqueued on the context's stream (rz_set_stream) and
 * returns at once; results are valid after rz_sync or the caller's own synchronisation of that stream.  With RZ_RAYS_HOST they
 * are host memory: the call stages them through buffers of the context and returns when the results are written, having read
 * the backstop word itself (RZ_ERR_INTERNAL if a walk was cut short).  A query sees the scene as of the last rz_upload /
 * rz_update / rz_update_transforms issued before it; it needs no rz_set_frame and touches no render state (accumulation,
 * currentIor, pools).  n == 0: RZ_OK, nothing launched.  RZ_ERR_INVALID_ARG: null context, null pointer with n > 0, a device
 * pointer not 16-byte aligned, n > INT32_MAX, unknown flags; RZ_ERR_NOT_READY: no scene uploaded.
 * (Additive: no existing struct changed, so RZ_ABI_VERSION stays 5.) */
typedef struct rz_ray {
    float    origin[3];
    float    max_dist;
    float    dir[3];
    uint32_t reserved;
} rz_ray;                       /* 32 B */
typedef struct rz_hit {
    float   t;
    float   point[3];           /* world-space hit point */
    float   normal[3];          /* world-space geometric normal, unit (FS:489-491) */
    int32_t material, instance, triangle, prim, reserved;
} rz_hit;                       /* 48 B */
typedef struct rz_visibility {
    float   visibility;         /* the product of the transparencies passed (1 when nothing was met, 0 when blocked) */
    int32_t lit;                /* 1: shadowVisibility returned true */
} rz_visibility;                /* 8 B */
#define RZ_RAYS_HOST        1u  /* pointers are host memory: staged through context buffers, returns when results are written */
#define RZ_RAYS_INCOHERENT  2u  /* walk lane by lane (trace_spread): a scheduling hint, identical results */
int rz_trace_rays(rz_ctx* ctx, const rz_ray* rays, rz_hit* hits, size_t n, unsigned flags);
int rz_shadow_rays(rz_ctx* ctx, const rz_ray* rays, rz_visibility* out, size_t n, unsigned flags);

/* ------------------------------------------------------------------------ */
/* Editor preview (main.cpp:1210-1322, shaders/editor_{vertex,fragment}.glsl) */
/* ------------------------------------------------------------------------ */
/* RayZen's editor mode (F1) -- flat-shaded geometry, GGX direct lighting from every light, an ambient term, no shadows -- as a
 * ray cast instead of a raster pass: per pixel, the closest hit of the ray through the pixel centre (the render's camera ray
 * with no jitter, from cam_pos), clipped as the rasteriser clips (the world hit through view then proj: visible iff
 * -w <= z_clip <= w; beyond the far plane the pixel is background; a surface in front of the near plane is skipped and the
 * query restarts where the ray crosses the near plane, at most 4 times), shaded by editor_fragment.glsl:58-112 with the hit's
 * world normal (normalize(mat3(transpose(inverseTransform)) * faceNormal): uNormalMatrix * faceNormal of main.cpp:1299-1301 up
 * to rounding).  No culling: a back face gets NdotV = 0 (diffuse only).  Where nothing visible is hit: the clear colour.
 * From `frame` the call reads width, height, inv_view, inv_proj, view, proj, cam_pos and num_lights (the loop runs over
 * min(num_lights, lights uploaded)); it needs no rz_set_frame and leaves the frame rz_set_frame set, the accumulation,
 * currentIor and rz_debug_last_plan as they were.  Outputs (each optional: NULL is not written), row 0 = the bottom row:
 *   rgba8   width*height*4 B: rint(clamp(colour, 0, 1) * 255), alpha 255 (rz_present's quantisation)
 *   rgb32f  width*height*3 floats: the colour before quantisation
 *   hits    width*height rz_hit: a visible hit exactly as rz_trace_rays returns it for the pixel's ray, except that t counts
 *           from the camera after a near-plane restart; a background pixel gets the miss record (t = 1e30f, ids -1)
 * Pointers are DEVICE memory by default (hits 16-byte aligned, the others 4-byte): the call is enqueued on the context's stream
 * and sees the scene as of the last rz_upload / rz_update / rz_update_transforms issued before it.  With RZ_EDITOR_HOST they
 * are host memory: staged through a buffer of the context, the call returns when they are written and reports a walk cut
 * short at its backstop as rz_trace_rays does (RZ_ERR_INTERNAL).  RZ_ERR_INVALID_ARG: null context or frame, width or
 * height <= 0, more than INT32_MAX pixels, a misaligned device pointer, unknown flags; RZ_ERR_BUFFER_SIZE: a non-NULL output
 * smaller than the above; RZ_ERR_NOT_READY: no scene uploaded, or no materials.
 * (Additive: RZ_ABI_VERSION stays 5.) */
typedef struct rz_editor_params {      /* NULL = RayZen's values */
    float ambient[3];  float pad0;      /* uAmbientColor, main.cpp:1269: 0.03 */
    float clear[4];                     /* glClearColor, main.cpp:260: 0.05 0.05 0.07 1 */
} rz_editor_params;                     /* 32 B; rz_sizeof(10) */
#define RZ_EDITOR_HOST       1u  /* outputs are host memory: staged, returns when written */
#define RZ_EDITOR_INCOHERENT 2u  /* trace_spread: scheduling hint, identical results */
int rz_render_editor(rz_ctx* ctx, const rz_frame_params* frame, const rz_editor_params* params,
                     uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes,
                     rz_hit* hits, size_t hits_bytes, unsigned flags);

/* ------------------------------------------------------------------------ */
/* Denoising the low-sample frame (new: the reference has none)              */
/* ------------------------------------------------------------------------ */
/* An edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) of the resolved frame, guided by a per-pixel G-buffer the
 * call casts itself (rz_denoise.hip).  Per pixel p, row 0 = the bottom row:
 *   colour   c_p = rgba.rgb / n with n = rgba.a > 0 ? rgba.a : 1 (rz_present's divide without the clamp: unclamped HDR)
 *   guide    G_p = the closest hit of the ray through the pixel centre, from cam_pos (the rays rz_render_editor casts, not
 *            clipped; the render's camera ray differs from it only by the shader's 2e-5 uv jitter, FS:205): hit or miss, world
 *            point x_p, unit world normal n_p, world distance t_p, material m_p -- bit for bit what rz_trace_rays returns
 *   demodulate (default on)  alpha_p = materials[clamp(m_p)].albedo for a hit, (1, 1, 1) for a miss; d_p = c_p / max(alpha_p,
 *            1e-3) per channel, and the result of the last pass is multiplied by alpha_p again.  Off: d_p = c_p.
 *   pass i = 0..K-1, step s = 2^i:
 *            d'_p = sum_q w_pq d_q / sum_q w_pq over q = p + s (a, b), a, b in -2..2, q inside the image (taps outside are
 *            dropped, not clamped);
 *            w_pq = h_a h_b [hit_p == hit_q] W_geom exp(-|d_p - d_q|^2 / (sigma_color^2 2^-i)), h = (1/16, 1/4, 3/8, 1/4, 1/16);
 *            W_geom = max(0, n_p.n_q)^sigma_normal exp(-|n_p.(x_q - x_p)| / (sigma_plane t_p f s max(|a|, |b|))) when both
 *            are hits (0^0 = 1), 1 when both are misses and for the centre tap (a = b = 0);
 *            f = 2 |inv_proj[5]| / height, the world size of one pixel at unit distance.
 *            A hit and a miss never mix; different instances may (the normal and plane terms separate them where the geometry
 *            does).  The centre weight 9/64 keeps every sum non-empty.
 *   K = 0: no filtering, the output is exactly c_p.
 *   Non-finite samples.  A pixel p is BAD in a call iff a channel of c_p (after the divide by n) is NaN or +-Inf, decided on
 *            the bit pattern (exponent field all ones).  A bad sample never leaves its pixel: only pass 0 changes, and for an
 *            input without bad pixels every output byte is what it would be without this rule.  In pass 0 a bad tap q is
 *            dropped exactly as a tap outside the image is.  A bad centre p drops its own centre term as well (num and den start
 *            at 0), takes the colour weight of every remaining tap as 1 (h_a h_b, the hit-or-miss rule and W_geom apply as
 *            written), and d'_p = num / den where den > 0, otherwise (0, 0, 0); d_p of a bad pixel is never used in arithmetic.
 *            Pass 0's output is therefore finite, and passes 1..K-1 and the re-modulation are as written.  K = 0 stays "the
 *            output is exactly c_p", bad or not (rz_present_denoised at K = 0 keeps rz_present's bytes).  (n = NaN counts as
 *            n = 1; a finite sum over n = +Inf is c = 0, not bad.)
 * Defaults (params NULL): K = 5, sigma_color = 0.5, sigma_normal = 128, sigma_plane = 1, demodulate = 1 -- chosen by the CPU
 * measurement of tests/test_denoise_abi.py.  Arithmetic is binary32.
 * Camera and size come from the last rz_set_frame (width, height, inv_view, inv_proj, cam_pos), as rz_present takes them.
 * rz_denoise outputs (each optional, NULL = not written):
 *   rgb32f   width*height*3 floats: the denoised linear colour, unclamped
 *   guides   width*height rz_hit: the guide, as rz_trace_rays returns it for the pixel's ray (a miss: t = 1e30f, ids -1)
 * rgba_in NULL reads the context's accumulation; otherwise it is a caller RGBA32F buffer (width*height*16 B) in the same
 * sum-and-count form.  Pointers are DEVICE memory by default (rgba_in and guides 16-byte aligned, rgb32f 4-byte): the call is
 * enqueued on the context's stream and returns at once (a walk cut short at its backstop is reported by rz_sync).  With
 * RZ_DENOISE_HOST they are host memory: staged through buffers of the context, the call returns when the outputs are written
 * and reports a cut walk itself (RZ_ERR_INTERNAL).  It sees the scene as of the last rz_upload / rz_update /
 * rz_update_transforms issued before it.
 * rz_present_denoised is rz_present with the denoised colour in place of the divide: the colour is written as (c_out, 1) to a
 * buffer of the context and rz_present's kernel runs on it, so the overlays are drawn on top (not blurred) and K = 0 gives
 * rz_present's bytes exactly.  Its outputs are host memory, and it synchronises as rz_present does.
 * Neither call touches render state: the accumulation, currentIor, the pools, the frame and rz_debug_last_plan stay as they were.
 * RZ_ERR_NOT_READY: no scene, no materials, or no rz_set_frame.  RZ_ERR_INVALID_ARG: null context, iterations outside 0..10,
 * a sigma that is negative, NaN or infinite (sigma_color and sigma_plane must be > 0), non-zero reserved words, unknown flags,
 * a misaligned device pointer, or a frame with tile_nranks > 1 (the filter needs the whole frame).  RZ_ERR_BUFFER_SIZE: a
 * non-NULL output or input smaller than the above.  RZ_ERR_INTERNAL: a host-path call whose guide walk hit the backstop.
 * (Additive: RZ_ABI_VERSION stays 5.) */
typedef struct rz_denoise_params {      /* NULL = defaults */
    int32_t iterations;                 /* K, 0..10 */
    float   sigma_color, sigma_normal, sigma_plane;
    int32_t demodulate;                 /* 1 = divide by the primary hit's albedo before filtering */
    int32_t reserved[3];                /* must be 0 */
} rz_denoise_params;                    /* 32 B; rz_sizeof(11) */
#define RZ_DENOISE_HOST 1u              /* pointers are host memory: staged, returns when written */
int rz_denoise(rz_ctx* ctx, const rz_denoise_params* params, const float* rgba_in, size_t rgba_in_bytes,
               float* rgb32f, size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, unsigned flags);
int rz_present_denoised(rz_ctx* ctx, const rz_present_params* present, const rz_denoise_params* params,
                        uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes);

/* ------------------------------------------------------------------------ */
/* Temporal accumulation and a variance-guided filter (new: the reference has none) */
/* ------------------------------------------------------------------------ */
/* For the one-sample frame of a camera and instances that move: every call blends the frame into a per-pixel history that is
 * carried to where the pixel's surface was in the previous call's frame (reprojection, through the instance's previous
 * transform), and filters the result with rz_denoise's a-trous guided by the luminance variance (SVGF: Schied et al., HPG 2017;
 * rz_temporal.hip).  Per pixel p = (px, py), row 0 = the bottom row; W, H = the frame's width and height; binary32 throughout,
 * every expression evaluated as written (no fused multiply-add), sums left to right:
 *  1 guide, colour   G_p, c_p, alpha_p exactly as rz_denoise's (the same guide kernel); d_p = c_p / max(alpha_p, 1e-3) for a hit
 *            when demodulate is set, else c_p; l_p = (0.2126 d.r + 0.7152 d.g) + 0.0722 d.b.
 *  2 reprojection    a 3 x 4 transform applies as ((m0 x + m1 y) + m2 z) + m3 per row (m0..m3 its columns); dot(a, b) =
 *            (a.x b.x + a.y b.y) + a.z b.z.
 *            hit on instance i:  o = inverseTransform_i (x_p, 1);  x' = transformPrev_i (o, 1);
 *              n' = b / sqrt(dot(b, b)), b = mat3(transpose(inversePrev_i)) (mat3(transpose(transform_i)) n_p)
 *              (mat3(transpose(M)) v: the dot products of M's columns with v).  If transform_i equals transformPrev_i bit for
 *              bit (the 3 x 4 part), x' = x_p and n' = n_p: the round trip is skipped.  t' = sqrt(dot(x' - cam_prev, x' - cam_prev)).
 *            miss:  x' = the unit direction of the pixel-centre ray (what the guide's ray was cast along), with w = 0.
 *            e = ((view_prev[k] x'.x + view_prev[4+k] x'.y) + view_prev[8+k] x'.z) + view_prev[12+k] w, k = 0..3 (w = 1 for a
 *            hit); clip likewise from proj_prev and e.  No history if clip.w <= 0 (hit or miss alike).
 *            u = (clip.x / clip.w * 0.5 + 0.5) * W - 0.5, v likewise with clip.y and H; no history unless -1 < u < W and
 *            -1 < v < H.
 *            Static shortcut: when view and proj equal the previous call's bit for bit and (for a hit) so does the instance's
 *            transform, (u, v) = (px, py) exactly -- one tap of weight 1.
 *  3 taps    x0 = floor(u), y0 = floor(v), fx = u - x0, fy = v - y0; the taps q = (x0, y0), (x0+1, y0), (x0, y0+1),
 *            (x0+1, y0+1), in this order, with weights (1-fx)(1-fy), fx (1-fy), (1-fx) fy, fx fy.  A tap counts iff its weight
 *            is > 0, it lies inside the image, the previous guide at q has p's hit-or-miss status and, for a hit: the same
 *            instance, dot(n', n_q) >= normal_cos, and |dot(n', x_q - x')| <= plane_tol * t' * f_prev, f_prev =
 *            2 |inv_proj_prev[5]| / H.  S = the sum of the counted weights; history is accepted iff S >= 0.01, and then
 *            D_h, (m1, m2) = (sum of w * value over the counted taps) / S, and N_h = N_0 + (sum of w * (N_q - N_0)) / S with N_0
 *            the first counted tap's N (the same mean; taps of one length give that length exactly).
 *  4 accumulation    N_p = min(N_h + 1, max_history) with history, else 1 (N is carried as a float);  a = max(alpha, 1 / N_p);
 *            D_p = D_h + a * (d_p - D_h);  am = max(alpha_moments, 1 / N_p);  M1 = m1 + am * (l_p - m1);
 *            M2 = m2 + am * (l_p * l_p - m2).  Without history D_p = d_p, (M1, M2) = (l_p, l_p * l_p).
 *  5 variance        N_p >= 4: max(0, M2 - M1 * M1).  Below: max(0, E[l^2] - E[l]^2) * (4 / N_p) over the 7 x 7 window around p
 *            of the luminance of D (this call's), with weights 1 for p itself and, for q = p + (a, b) inside the image,
 *            [hit_p == hit_q] W_geom, W_geom = rz_denoise's at step 1 with tap distance max(|a|, |b|) (1 between two misses).
 *  6 filter  K passes of rz_denoise's a-trous on (D, variance): the same taps, h, W_geom, hit-or-miss rule and border rule; the
 *            colour weight is exp(-|l_p - l_q| / (sigma_l * sqrt(g_p) + 1e-8)) with l the luminance of the pass's input and
 *            g_p the input variance under the 3 x 3 kernel (1/4 centre, 1/8 edges, 1/16 corners) at distance 1, renormalised
 *            over the taps inside the image.  The variance is filtered along: var'_p = sum_q w_pq^2 var_q / (sum_q w_pq)^2.
 *            After the last pass a hit's colour is multiplied by alpha_p again (demodulate).
 *            K = 0: the output is D_p alpha_p (demodulate and a hit; else D_p) where history was accepted and c_p itself where
 *            it was not -- so a call on an empty history returns exactly what rz_denoise returns for K = 0.
 *  Non-finite samples.  p is BAD iff a channel of c_p is NaN or +-Inf (rz_denoise's definition, on the bit pattern).  A bad
 *            sample never outlives its frame: steps 2 and 3 are as written (they never read d_p); then, for a bad p,
 *            d_p := D_h where history was accepted, otherwise (0, 0, 0), and l_p is taken from that d_p.  Step 4 is as written:
 *            with d_p = D_h the blend returns D_h exactly and N counts on; steps 5 and 6 see a finite D.  The K = 0 rule
 *            stays: D_p alpha_p where history was accepted, c_p itself where not -- so a bad pixel shows through at K = 0 on a
 *            pixel without history, and only there.  Consequence: a bad sample without history is stored as black with N = 1
 *            and fades as 1 / N afterwards (it is not filled from its neighbours).  For an input without bad pixels every
 *            output byte is what it would be without this rule.  rz_present_temporal, and rz_present_display with source 1 or
 *            2, run these kernels and follow.
 * The history -- D | N, the moments, the guide (rz_hit records), the frame's view, proj, inv_proj and cam_pos, and every
 * instance's transform and inverseTransform -- lives in the context: allocated by the first call, sized by the frame, freed by
 * rz_destroy.  A call commits what it computed as the new history (two sets of buffers swap roles; no frame is copied) unless
 * RZ_TEMPORAL_KEEP is set, which computes the same outputs and leaves the history as it was.  The history is dropped (the next
 * call starts every pixel at N = 1) by rz_temporal_reset, by a frame of another width or height, by another instance count, by
 * rz_upload on binding 0, 7, 8 or 9, and by rz_build_geometry.  It is KEPT across rz_update, rz_update_transforms and
 * rz_refit_geometry: a deformed mesh reprojects by its instance transform only, and the validity tests of step 3 are what
 * discard the taps that no longer belong to the pixel's surface.
 * Outputs of rz_denoise_temporal (each optional), conventions and errors are rz_denoise's: rgb32f, guides, and
 *   stats    width*height*2 floats: N_p after this call, and the variance of step 5 (what the filter's first pass reads)
 * Device pointers by default (rgba_in and guides 16-byte aligned, rgb32f and stats 4-byte), enqueued on the context's stream;
 * RZ_TEMPORAL_HOST: host memory, staged, returns when written and reports a cut walk itself.  rgba_in NULL reads the context's
 * accumulation.  A call with every output NULL still advances the history.  rz_present_temporal is to this call what
 * rz_present_denoised is to rz_denoise (on an empty history with K = 0: rz_present's bytes).  No render state is touched.
 * RZ_ERR_INVALID_ARG additionally: alpha or alpha_moments outside [0, 1] or NaN, max_history < 1, normal_cos outside [-1, 1],
 * plane_tol or sigma_l not finite and > 0.  Nothing is launched by a call that fails, and the history stays as it was.
 * Defaults (params NULL): alpha = alpha_moments = 0.2, max_history = 32, normal_cos = 0.9, plane_tol = 2, K = 5, sigma_l = 0.5,
 * sigma_normal = 128, sigma_plane = 1, demodulate = 1 -- sigma_l chosen by the CPU measurement of tests/test_temporal_abi.py
 * (the sweep).
 * (Additive: RZ_ABI_VERSION stays 5.) */
typedef struct rz_temporal_params {     /* NULL = defaults */
    float   alpha, alpha_moments;       /* the least weight of the new frame (colour, moments), 0..1 */
    int32_t max_history;                /* the cap of N, >= 1 */
    float   normal_cos, plane_tol;      /* tap validity: the least n'.n_q; the plane distance in previous-frame pixel footprints */
    int32_t iterations;                 /* K, 0..10 */
    float   sigma_l, sigma_normal, sigma_plane;
    int32_t demodulate;
    int32_t reserved[6];                /* must be 0 */
} rz_temporal_params;                   /* 64 B; rz_sizeof(12) */
#define RZ_TEMPORAL_HOST 1u             /* pointers are host memory, as RZ_DENOISE_HOST */
#define RZ_TEMPORAL_KEEP 4u             /* compute the outputs, leave the history as it was */
int rz_denoise_temporal(rz_ctx* ctx, const rz_temporal_params* params, const float* rgba_in, size_t rgba_in_bytes,
                        float* rgb32f, size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes,
                        float* stats, size_t stats_bytes, unsigned flags);
int rz_present_temporal(rz_ctx* ctx, const rz_present_params* present, const rz_temporal_params* params,
                        uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes);
int rz_temporal_reset(rz_ctx* ctx);
/* TEST HOOK: the stored history as raw bytes, in the style of rz_debug_read_layout (out NULL: only *needed is set; an empty
 * history has 0 bytes of everything).  which = 0: D | N, width*height float4;  1: the moments, width*height float2;  2: the
 * guide, width*height rz_hit;  3: view[16], proj[16], inv_proj[16], cam_pos[3] of the frame it was made for (51 floats);
 * 4: per instance 24 floats: inverseTransform then transform, each as columns 0..3, rows 0..2. */
int rz_debug_read_temporal(rz_ctx* ctx, int which, void* out, size_t bytes, size_t* needed);

/* ------------------------------------------------------------------------ */
/* Display transform (new: the reference has none)                           */
/* ------------------------------------------------------------------------ */
/* The reference shows a frame by clamping it (FS:772-773), and so does rz_present.  This stage turns linear HDR colour -- the
 * accumulation, or what rz_denoise / rz_denoise_temporal write -- into display colour on the device: an exposure (manual, or
 * metered from the frame and adapted over calls), a tone curve and a transfer function (rz_display.hip).  Per pixel p, row 0 =
 * the bottom row; binary32, every expression evaluated as written (no fused multiply-add), unless binary64 is said:
 *  1 luminance   l_p = (0.2126 r + 0.7152 g) + 0.0722 b of the input colour (rz_denoise_temporal's expression).
 *  2 metering (auto)  u = the bit pattern of l_p, b = (int)(u >> 21) - 444.  A set sign bit or b < 0 counts in `below`, b > 127
 *            in `above` (a positive NaN or infinity lands there), otherwise histogram[b] is incremented: 128 bins over
 *            [2^-16, 2^16), four per octave, edges at the mantissa quarters (1.0 -> 64, 1.25 -> 65, 2^-16 -> 0).  The counts
 *            are integers added with integer atomics: exact, whatever the scheduling.
 *  3 target      N = the sum of the bins.  N == 0: the exposure stays what it was (1 on a fresh state) and `target` reports it.
 *            Otherwise, in 64-bit integers, lo = N * low_permille / 1000, hi = N - N * high_permille / 1000, C_b the prefix
 *            count, kept_b = max(0, min(C_{b+1}, hi) - max(C_b, lo)), K = hi - lo (> 0), I = sum kept_b * (b >> 2), M_m = the
 *            sum of kept_b over b % 4 == m; in binary64, left to right,
 *              log2_mean = I / K - 16 + (((M_0 g_0 + M_1 g_1) + M_2 g_2) + M_3 g_3) / K,
 *            g_m = (log2(1 + m/4) + log2(1 + (m+1)/4)) / 2, the log2 mid-point of a bin: 0x1.49a784bcd1b8bp-3,
 *            0x1.d053f6d260896p-2, 0x1.646eea247c5c2p-1, 0x1.ceaecfea8085ap-1;
 *              T = clamp((float)(key / exp2(log2_mean)), min_exposure, max_exposure).
 *  4 adaptation  E = E_prev + adapt * (T - E_prev); E = T exactly on a fresh state or when adapt == 1.  Manual mode: E = exposure.
 *  5 tone        per channel x = c * E.  curve 0: y = x.  curve 1 (extended Reinhard): x = max(x, 0),
 *            y = (x * (1 + x / (white * white))) / (1 + x).  curve 2 (the ACES fit of Narkowicz 2015): x = max(x, 0),
 *            y = (x * (2.51 x + 0.03)) / (x * (2.43 x + 0.59) + 0.14).  Then y = clamp(y, 0, 1) (rz_present's clamp).
 *  6 transfer 1  y <= 0.0031308 ? 12.92 y : 1.055 * powf(y, 1 / 2.4f) - 0.055 (the sRGB OETF).
 * With params NULL x = c * 1 = c, so the stage is the reference's clamp.
 *
 * rz_display is the asynchronous building block, with rz_denoise's conventions: device pointers by default (4-byte aligned),
 * the work is enqueued on the context's stream, the call returns at once and the exposure never visits the host; width and
 * height come from the last rz_set_frame (no scene is needed).  rgb_in is width*height*3 floats of linear colour; rgb_in NULL
 * reads the context's accumulation as c = rgb / n, n = a > 0 ? a : 1 (refused for a frame with tile_nranks > 1, as rz_denoise
 * refuses it).  Outputs, each optional:
 *   rgb32f   width*height*3 floats: the encoded colour before quantisation (may be rgb_in itself: in place)
 *   rgba8    width*height*4 B: rint(clamp(c, 0, 1) * 255), alpha 255
 * With RZ_DISPLAY_HOST the pointers are host memory, staged through buffers of the context, and the call returns when the
 * outputs are written.  A call with every output NULL still meters and adapts.
 * rz_present_display is to rz_display what rz_present_denoised is to rz_denoise.  source selects the colour: 0 the accumulation
 * (filter_params must be NULL), 1 rz_denoise's output (filter_params: an rz_denoise_params* or NULL), 2 rz_denoise_temporal's
 * (an rz_temporal_params* or NULL; the history advances exactly as rz_present_temporal advances it).  The stage writes
 * (encoded colour, 1) to a buffer of the context and rz_present's kernel runs on it, so the overlays are drawn on top of the
 * tone-mapped image, not through it.  Outputs are host memory and the call synchronises, as rz_present does.  With display
 * NULL the bytes are rz_present's, rz_present_denoised's or rz_present_temporal's exactly.
 * State: the context carries, on the device, the exposure last applied and whether one exists.  Every call commits its E
 * (a manual call too) unless RZ_DISPLAY_KEEP is set, which computes the same outputs and leaves the state -- rz_display_state's
 * record included -- as it was.  Only rz_display_reset drops it (the next auto call then jumps to its target) and rz_destroy
 * frees it; uploads, frame changes and the denoisers do not touch it.  A fresh state reports exposure = target = 1.  The display
 * calls touch no render state: the accumulation, currentIor, the pools, the frame, rz_debug_last_plan and the temporal history
 * stay as they were (except through source 2).
 * RZ_ERR_INVALID_ARG: null context, exposure_mode, curve or transfer unknown, a field of the mode or curve in use outside its
 * range (manual: exposure; auto: key, min_exposure, max_exposure, adapt, low_permille, high_permille; curve 1: white), non-zero
 * reserved words, unknown flags, a misaligned device pointer, an unknown source, filter_params with source 0.
 * RZ_ERR_BUFFER_SIZE: a buffer that is too small.  RZ_ERR_NOT_READY: no rz_set_frame (sources 1 and 2: what their denoiser
 * says).  A failing call launches nothing and leaves the state as it was.
 * (Additive: RZ_ABI_VERSION stays 5.) */
typedef struct rz_display_params {      /* NULL = the reference's display: manual exposure 1, clamp, linear */
    int32_t exposure_mode;              /* 0 manual, 1 auto (metered from this call's input) */
    float   exposure;                   /* manual: the multiplier, finite, > 0 */
    float   key;                        /* auto: the value the log-average luminance is brought to (0.18); finite, > 0 */
    float   min_exposure, max_exposure; /* auto: clamp of the target, 0 < min <= max, finite */
    float   adapt;                      /* auto: share of the way to the target taken per call, 0..1 (1 = jump) */
    int32_t low_permille, high_permille;/* auto: darkest / brightest share of the counted pixels ignored; >= 0, sum < 1000 */
    int32_t curve;                      /* 0 clamp, 1 extended Reinhard, 2 ACES fit (Narkowicz 2015) */
    float   white;                      /* curve 1: the value mapped to 1; finite, > 0 */
    int32_t transfer;                   /* 0 linear (the reference), 1 sRGB OETF */
    int32_t reserved[5];                /* must be 0 */
} rz_display_params;                    /* 64 B; rz_sizeof(14) */

typedef struct rz_display_info {
    float    exposure;                  /* E applied by the last call */
    float    target;                    /* T of the last auto call (E for a manual call) */
    float    log2_mean;                 /* (float) of step 3's mean; 0 when nothing was counted or manual */
    uint32_t counted, below, above;     /* of the last auto call */
    uint32_t histogram[128];            /* of the last auto call */
} rz_display_info;                      /* 536 B; rz_sizeof(15) */

#define RZ_DISPLAY_HOST 1u              /* pointers are host memory: staged, returns when written */
#define RZ_DISPLAY_KEEP 4u              /* compute the outputs, leave the adaptation state as it was */
int rz_display(rz_ctx* ctx, const rz_display_params* params, const float* rgb_in, size_t rgb_in_bytes,
               float* rgb32f, size_t rgb32f_bytes, uint8_t* rgba8, size_t rgba8_bytes, unsigned flags);
int rz_present_display(rz_ctx* ctx, const rz_present_params* present, const rz_display_params* display,
                       int source, const void* filter_params,
                       uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes);
int rz_display_reset(rz_ctx* ctx);
int rz_display_state(rz_ctx* ctx, rz_display_info* out);   /* synchronises */

/* ------------------------------------------------------------------------ */
/* Rendering below display size: guided upsampling (new: the reference has none) */
/* ------------------------------------------------------------------------ */
/* The path loop is the one cost that scales with pixels x samples.  This stage lets a frame be rendered at 1 / s of the display
 * size and reconstructed at display size from a full-resolution G-buffer, so that silhouettes and material boundaries are as
 * sharp as in a native frame and only the slowly varying, demodulated colour is interpolated (rz_upscale.hip).
 * The frame of the last rz_set_frame is the LOW frame, w x h: the one that was rendered.  The output is W x H = s w x s h; the
 * aspect is unchanged, so inv_view, inv_proj and cam_pos serve both sizes.  Row 0 = the bottom row.  Arithmetic is binary32
 * without fused multiply-add.  The footprint, the bilinear weights, admissibility and the choice of stage are evaluated exactly as
 * written, one rounding per operation; W_geom is evaluated in the form given under "as evaluated", whose exp, exp2 and log2
 * are the device's (not correctly rounded), so the colours are held to the float64 restatement within a tolerance
 * (tests/test_upscale_gpu.py), not bit for bit.
 *  guides    g_q = rz_denoise's guide record of low pixel q at w x h; G_P = the same for high pixel P = (X, Y) at W x H: hit or
 *            miss, world point x, unit world normal n, world distance t, material m -- both cast by rz_denoise's guide kernel,
 *            unchanged, with only the width and height differing.  alpha(m) = materials[clamp(m)].albedo for a hit, (1, 1, 1)
 *            for a miss.
 *  colours   c_q = the low colour; d_q = c_q / max(alpha(m_q), 1e-3) per channel when demodulating, else c_q.  A low pixel is BAD
 *            by rz_denoise's rule: a channel of c_q is NaN or +-Inf, decided on the bit pattern.
 *  footprint, in integers: r_x = 2X + 1 - s, i0 = floor(r_x / 2s) (integer floor division), fx = (float)(r_x - 2s i0) /
 *            (float)(2s); likewise r_y, j0, fy.  No floating-point floor is taken.
 *  a tap q is ADMISSIBLE iff it lies inside the low image, is not bad, and hit_q == hit_P (a hit and a miss never mix).
 *  W_geom    max(0, n_P.n_q)^sigma_normal exp(-|n_P.(x_q - x_P)| / (sigma_plane t_P f)) when both are hits (0^0 = 1), 1 when
 *            both are misses; f = 2 |inv_proj[5]| / h, the world size of one LOW pixel at unit distance.
 *            As evaluated (rz_denoise_atrous's form): k = (float)(1 / (sigma_plane f)), computed in binary64 on the host;
 *            nd = max(0, n_P.n_q); the power is exp2f(sigma_normal * log2f(nd)) for nd > 0, else 1 if sigma_normal == 0, else 0;
 *            W_geom = power * expf(-(|n_P.(x_q - x_P)| * (k / t_P))); dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
 *  stage 1   the taps q = (i0 + a, j0 + b), a, b in {0, 1}, with bilinear weight B = (a ? fx : 1 - fx)(b ? fy : 1 - fy); a tap with
 *            B == 0 is skipped.  w = B max(W_geom, 1e-4) over the admissible taps, b outer, a inner, and
 *            out = alpha(m_P) sum w d_q / sum w when demodulating, else sum w d_q / sum w.  The floor makes the sum non-empty
 *            whenever a tap is admissible, and makes every stage decision a function of exact data: flags, bit patterns, integers.
 *  stage 2   only if stage 1 found no admissible tap (with B > 0): the same with the twelve outer taps of the 4 x 4 window
 *            i0-1..i0+2 x j0-1..j0+2 and w = max(W_geom, 1e-4).
 *  stage 3   only if stage 2 found none either: out = c_q of the nearest low pixel q = (X / s, Y / s) (integer division), not
 *            demodulated; (0, 0, 0) if that pixel is bad.  A bad low pixel therefore reaches no output: it is no tap in stages 1
 *            and 2 and reads as black in stage 3.
 *  s = 1     out = c_p exactly and nothing is cast (unless the guide is asked for), as K = 0 in rz_denoise.
 * KNOWN LIMIT.  The guide is the FIRST hit.  Reflections in the metals and everything seen through glass are upsampled as
 * colour on the reflecting or refracting surface: they are blurred to the low resolution.  (rz_upscale_seethrough below follows
 * glass and perfect mirrors.)
 * Defaults (params NULL): factor 2, sigma_normal = 128, sigma_plane = 1 (rz_denoise's), demodulate = 1.
 * rz_upscale.  rgb_in is w*h*3 floats of linear colour in rz_display's convention (what both denoisers write); rgb_in NULL reads
 * the context's accumulation as c = rgb / n, n = a > 0 ? a : 1.  Outputs, each optional:
 *   rgb32f   W*H*3 floats: the reconstructed linear colour, unclamped
 *   guides   W*H rz_hit: the high-size guide, bit for bit what rz_trace_rays returns for those pixel-centre rays
 * Device pointers by default (guides 16-byte aligned, rgb_in and rgb32f 4-byte): enqueued on the context's stream, returns at
 * once (a walk cut short at its backstop is reported by rz_sync).  With RZ_UPSCALE_HOST they are host memory: staged through
 * buffers of the context, the call returns when the outputs are written and reports a cut walk itself (RZ_ERR_INTERNAL).  No
 * render state, temporal history or display state is touched; the buffers of the high size live in the context, allocated on
 * first use and kept.
 * rz_present_upscaled is rz_present_display at the display size: source and filter_params are rz_present_display's (0 the
 * accumulation, 1 rz_denoise, 2 rz_denoise_temporal, whose history advances as rz_present_temporal advances it) and the
 * denoisers run at w x h; then the upscale; then the display stage at W x H (display NULL: clamp and linear); then rz_present's
 * kernel on (colour, 1) at W x H, with the overlays drawn at the high size.  Outputs are host memory of W x H and the call
 * synchronises.  With factor = 1 the bytes are rz_present_display's exactly, for every source.  Like rz_present_display it
 * commits its exposure to the context's display state (a metered one is metered from the W x H colour); rz_upscale does not.
 * RZ_ERR_INVALID_ARG: null context, factor outside 1..4, a sigma that is negative, NaN or infinite (sigma_plane must be > 0),
 * demodulate other than 0 or 1, non-zero reserved words, unknown flags, a misaligned device pointer, a frame with tile_nranks > 1,
 * more than INT32_MAX high pixels (rz_present_upscaled: also what rz_present_display says).  RZ_ERR_BUFFER_SIZE: a buffer that is
 * too small.  RZ_ERR_NOT_READY: no scene, no materials, or no rz_set_frame.  A failing call launches nothing.
 * (Additive: RZ_ABI_VERSION stays 5.) */
typedef struct rz_upscale_params {      /* NULL = defaults */
    int32_t factor;                     /* s, 1..4 */
    float   sigma_normal, sigma_plane;  /* rz_denoise's: sigma_normal >= 0, sigma_plane > 0, finite */
    int32_t demodulate;                 /* 1 = interpolate the colour divided by the first hit's albedo */
    int32_t reserved[4];                /* must be 0 */
} rz_upscale_params;                    /* 32 B; rz_sizeof(21) */
#define RZ_UPSCALE_HOST 1u              /* pointers are host memory: staged, returns when written */
int rz_upscale(rz_ctx* ctx, const rz_upscale_params* params, const float* rgb_in, size_t rgb_in_bytes,
               float* rgb32f, size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, unsigned flags);
int rz_present_upscaled(rz_ctx* ctx, const rz_present_params* present, const rz_upscale_params* upscale,
                        const rz_display_params* display, int source, const void* filter_params,
                        uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes);

/* ------------------------------------------------------------------------ */
/* See-through guides for the upsampler: glass and mirrors (new)            */
/* ------------------------------------------------------------------------ */
/* rz_upscale's guide is the first hit (its KNOWN LIMIT).  Two events of the path loop are deterministic: a transparent surface
 * always refracts, or reflects on total internal reflection, and a surface with reflectivity >= 1 always mirrors (its test is
 * rand < reflectivity with rand in [0, 1)).  These entry points follow the pixel-centre ray through such surfaces to the first
 * surface that scatters diffusely and interpolate there (rz_seethrough.hip).  Everything of rz_upscale stands as written
 * except the guide, alpha and one more admissibility term.
 *  chain     of a pixel, at either size.  o = cam_pos, d = the direction rz_denoise's guide casts for the pixel centre, ior = 1,
 *            T = (1, 1, 1), L = 0, k = 0.  Repeat: h = the closest hit of (o, d) by rz_trace_rays' query.  A miss ends the chain
 *            with final = miss.  Otherwise L = L + t (binary32, in order) and M = materials[clamp(h.material)]; m_first is the
 *            clamped material of the first hit.  If k == max_depth the chain ends at this hit.  Else if M.transparency > 0: the
 *            dielectric step of the path loop (rz_path.h: scatter) verbatim -- entering = dot(-d, n) > 0, N = entering ? n : -n,
 *            next = entering ? M.ior : 1, eta = ior / next, cosi = clamp(dot(-d, N), 0, 1), F0 = ((ior - next) / (ior + next))^2,
 *            fresnel = F0 + (1 - F0)(1 - cosi)^5 with x^5 = (x^2)^2 x; on total internal reflection d = d - N (2 dot(d, N)) and
 *            T = T * 0.98; else d = the refracted direction, ior = next, tint = mix(1, albedo, transparency) per channel and
 *            T = T * clamp((tint * transparency) * (1 - fresnel), 0, 1).  Else if M.reflectivity >= 1: d = d - n (2 dot(d, n)) and
 *            T = T * 0.95.  Else the chain ends at this hit.  After a step o = hp + (n * (dot(d, n) > 0 ? 1 : -1)) * 0.003 and
 *            k = k + 1.  NaN parameters fail both comparisons and end the chain.  The bounce budget and Russian roulette play no
 *            part: this is a guide, not a sample.  Binary32, one rounding per operation, no fused multiply-add, operands in
 *            scatter()'s order.
 *  guide     G = (hit or miss of the FINAL query; x, n and material of the final hit; t = L).
 *  class     cls = 0 if k == 0, else m_first + 1.
 *  alpha     T * albedo(final material) per channel for a final hit, T for a final miss (a miss is demodulated too).  With
 *            k = 0 this is rz_upscale's alpha bit for bit.
 *  a tap q is ADMISSIBLE iff rz_upscale admits it on these guides AND cls_q == cls_P.  W_geom (on the final hits, t_P = L_P),
 *            the 1e-4 floor, stages 1 to 3, demodulation by max(alpha, 1e-3) and re-modulation by alpha_P are rz_upscale's.
 * So max_depth = 0, or a scene in which no pixel's chain moves, gives rz_upscale's / rz_present_upscaled's bytes exactly, and
 * factor 1 gives c exactly (rz_present_upscaled_seethrough: rz_present_display's bytes).
 * LIMITS.  Surfaces with 0 < reflectivity < 1 are not followed.  The first surface's direct-light term (a highlight on the glass)
 * is interpolated within its class.  The denoisers that run in front of the upscale (sources 1 and 2) keep first-hit guides.
 * rz_upscale_seethrough is rz_upscale with: seethrough (NULL: max_depth 8); guides = the rz_hit of the FINAL hit with t = L (a
 * final miss is the miss record); chains, optional, W*H rz_chain, 16-byte aligned on the device path.  Pointer conventions,
 * RZ_UPSCALE_HOST, the error codes and "a failing call launches nothing" are rz_upscale's; in addition a max_depth outside 0..8
 * or a non-zero reserved word is RZ_ERR_INVALID_ARG and a chains buffer that is too small RZ_ERR_BUFFER_SIZE.  The calls touch no
 * render, temporal or display state beyond what their first-hit twins touch; their guide buffers live in the context beside
 * the first-hit ones, allocated on first use and kept.
 * (Additive: RZ_ABI_VERSION stays 5.) */
typedef struct rz_seethrough_params {   /* NULL = defaults */
    int32_t max_depth;                  /* specular steps followed at most, 0..8 (default 8) */
    int32_t reserved[7];                /* must be 0 */
} rz_seethrough_params;                 /* 32 B; rz_sizeof(23) */
typedef struct rz_chain {
    float   throughput[3];              /* T */
    int32_t word;                       /* k | (m_first + 1) << 8; 0 for a primary miss */
} rz_chain;                             /* 16 B; rz_sizeof(24) */
int rz_upscale_seethrough(rz_ctx* ctx, const rz_upscale_params* params, const rz_seethrough_params* seethrough,
                          const float* rgb_in, size_t rgb_in_bytes, float* rgb32f, size_t rgb32f_bytes,
                          rz_hit* guides, size_t guides_bytes, rz_chain* chains, size_t chains_bytes, unsigned flags);
int rz_present_upscaled_seethrough(rz_ctx* ctx, const rz_present_params* present, const rz_upscale_params* upscale,
                                   const rz_seethrough_params* seethrough, const rz_display_params* display, int source,
                                   const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes,
                                   float* rgb32f, size_t rgb32f_bytes);

/* ------------------------------------------------------------------------ */
/* Anti-aliased edges from sub-pixel guides (new: the reference has none)   */
/* ------------------------------------------------------------------------ */
/* The path loop's camera jitter is rand * 2e-5 in uv (about 0.04 pixel at 1080p), so a frame converges to its pixel-centre sample
 * and its silhouettes stay stair-stepped at any sample count; the denoisers and the upsampler preserve edges, aliased ones
 * included.  This stage shades once per pixel and takes geometry at s x s sub-pixel positions, on the pixels that have an edge
 * only, then averages (sub-pixel reconstruction anti-aliasing; rz_antialias.hip).  The render path does not change.
 * The frame of the last rz_set_frame is the frame that was rendered, w x h, and the output has its size.  c_p is its colour:
 * rgb_in, or the accumulation as rgb / n as in rz_upscale.  g_p = (hit_p, x_p, n_p, t_p, m_p) is rz_denoise's guide record of pixel
 * p (m the clamped material word).  f = 2 |inv_proj[5]| / h.  Row 0 = the bottom row.
 *  DIFFERENT a neighbour q is DIFFERENT from p when any of these holds: hit_q != hit_p; both are hits and m_q != m_p; both are
 *            hits and nd < edge_normal, nd = (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z; both are hits and pd > k_e * t_p, where
 *            pd = |dot(n_p, x_q - x_p)| in the same operand order and k_e = (float)(edge_plane * f), formed in binary64 on the
 *            host.  Binary32, one rounding per operation, no fused multiply-add: every decision is a function of exact data
 *            and tests/antialias_ref.py reproduces it bit for bit.
 *  EDGE      p is an EDGE pixel iff c_p is bad (rz_denoise's bit-pattern rule) or one of its up to eight neighbours inside the
 *            image is DIFFERENT from it.  Neighbours outside the image do not count; a 1 x 1 frame is flat unless it is bad.
 *  flat      out = c_p exactly.
 *  edge      out = (((u_0 + u_1) + ...) + u_{s^2 - 1}) / (float)(s s) per channel, binary32, b outer and a inner, where u_(a, b)
 *            is what rz_upscale defines for high pixel (s x + a, s y + b) of an s w x s h output of THIS frame at factor s: the
 *            high guide is the closest hit of the ray through that high pixel's centre, uv = ((float)X + 0.5f) / (float)(s w),
 *            from cam_pos -- bit for bit what rz_upscale casts -- and the footprint, admissibility, W_geom, the 1e-4 floor,
 *            stages 1 to 3, demodulation and re-modulation are rz_upscale's with this call's sigma_normal, sigma_plane and
 *            demodulate.  A bad pixel is an edge pixel; its sub-samples find no tap in it and stage 3 reads it as black, so the
 *            output is finite for s >= 2 whatever the input.
 *  s = 1     out = c_p exactly and nothing is cast unless guides or edges is asked for; rz_present_antialiased then gives
 *            rz_present_display's bytes for every source.
 * LIMITS.  Classification sees pixel centres only: geometry that lies between the centres of a flat neighbourhood is missed.
 * Guides are first hits, so edges behind glass and in mirrors stay aliased (the reserved words leave room for a see-through
 * variant).  The average is taken in linear HDR, before the tone curve.
 * Defaults (params NULL): factor 2, sigma_normal 128, sigma_plane 1, demodulate 1, edge_normal 0.9, edge_plane 1.
 * rz_antialias.  rgb_in as rz_upscale's.  Outputs, each optional:
 *   rgb32f   w*h*3 floats: the anti-aliased linear colour, unclamped
 *   guides   w*h rz_hit: the frame-size guide, as rz_denoise returns it
 *   edges    w*h bytes, 1 = edge; classified for factor 1 too
 * Pointer, alignment, staging (RZ_ANTIALIAS_HOST), stream, backstop and error conventions are rz_upscale's; edges needs no
 * alignment.  RZ_ERR_INVALID_ARG also covers: edge_normal outside -1..1 or not finite, edge_plane negative or not finite, non-zero
 * reserved words, rgb32f == rgb_in on the device path (an edge pixel reads its neighbours).  A failing call launches nothing.
 * The calls touch no render, temporal or display state; the frame-size guide lives in the upsampler's low-guide buffer.
 * rz_present_antialiased is rz_present_display with the pass between the source and the display stage: source 0 the
 * accumulation, 1 rz_denoise, 2 rz_denoise_temporal (the filter runs first and the history advances as in rz_present_temporal);
 * the overlays are drawn after it.  It commits its exposure as rz_present_display does.
 * (Additive: RZ_ABI_VERSION stays 5.) */
typedef struct rz_antialias_params {    /* NULL = defaults */
    int32_t factor;                     /* s: s x s sub-samples per edge pixel, 1..4 (default 2) */
    float   sigma_normal, sigma_plane;  /* rz_upscale's (128, 1) */
    int32_t demodulate;                 /* rz_upscale's (1) */
    float   edge_normal;                /* default 0.9: finite, -1..1 */
    float   edge_plane;                 /* default 1.0: finite, >= 0 */
    int32_t reserved[2];                /* must be 0 */
} rz_antialias_params;                  /* 32 B; rz_sizeof(26) -- 25 stays unassigned, tests probe it */
#define RZ_ANTIALIAS_HOST 1u            /* pointers are host memory: staged, returns when written */
int rz_antialias(rz_ctx* ctx, const rz_antialias_params* params, const float* rgb_in, size_t rgb_in_bytes,
                 float* rgb32f, size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes,
                 uint8_t* edges, size_t edges_bytes, unsigned flags);
int rz_present_antialiased(rz_ctx* ctx, const rz_present_params* present, const rz_antialias_params* antialias,
                           const rz_display_params* display, int source, const void* filter_params,
                           uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes);

/* ------------------------------------------------------------------------ */
/* Anti-aliased edges seen through glass and in mirrors (new)               */
/* ------------------------------------------------------------------------ */
/* rz_antialias' guides are first hits (its LIMITS): a pixel in the middle of a pane is flat to its classifier, so the silhouette
 * of what stands behind the pane stays stair-stepped, and a pixel on the pane's border is reconstructed with first-hit
 * admissibility, which mixes colour across the edge seen through it.  These entry points classify and reconstruct on the
 * see-through records of rz_upscale_seethrough (rz_antialias_seethrough.hip).  Everything of rz_antialias stands as written
 * except the guide, the DIFFERENT rule and which upsampler defines a sub-pixel.
 *  record    of pixel p: rz_upscale_seethrough's chain record at the frame's own size w x h for this call's max_depth.
 *            G_p = (hit or miss of the FINAL query; x, n and clamped material m of the final hit; t = L), T_p the throughput,
 *            cls_p = 0 if k == 0, else m_first + 1 -- bit for bit what rz_upscale_seethrough at factor 1 returns in guides and
 *            chains.
 *  DIFFERENT q is DIFFERENT from p when rz_antialias' rule holds on these FINAL records (hit status, material, edge_normal,
 *            edge_plane with t_p = L_p, k_e unchanged) or cls_q != cls_p.  Binary32, one rounding per operation, no fused
 *            multiply-add; tests/antialias_seethrough_ref.py reproduces it bit for bit.
 *  EDGE      as in rz_antialias: c_p bad, or any of the up to eight neighbours inside the image DIFFERENT.
 *  flat      out = c_p exactly.
 *  edge      out = the binary32 mean, b outer and a inner, of u_(a, b), where u_(a, b) is what rz_upscale_seethrough defines for
 *            high pixel (s x + a, s y + b) of an s w x s h output of THIS frame at factor s with this call's max_depth, sigmas
 *            and demodulate: the chain of that high pixel, alpha = T * albedo, the class term in admissibility and stages 1 to 3
 *            are stated there.
 * So max_depth = 0, or a scene in which no pixel's chain moves, gives rz_antialias' bytes exactly (colour, edges, guides);
 * factor 1 gives c exactly; rz_present_antialiased_seethrough at factor 1 gives rz_present_display's bytes.
 * LIMITS.  Surfaces with 0 < reflectivity < 1 are not followed.  Classification still sees pixel centres only.  On curved glass
 * neighbouring final hits jump, so much of a glass blob classifies as edge: this is correct, and costs s^2 chains per pixel there.
 * Measured with the restatement on the CPU oracle's frames (tests/test_antialias_seethrough_abi.py; 80 x 60 at 8 spp, 5 bounces,
 * s = 2, against the oracle's frame at twice the size and 64 spp, box-averaged): the mean squared error on the edge pixels whose
 * chain moves drops 18 x (RayZen's own scene) and 2.4 x (bunny_scene with its glass blob and mirror cube) against rz_antialias,
 * and over the whole frame 1.10 x and 1.47 x.  Cost at 1080p, s = 2 (profiles/antialias_seethrough/README.md): 0.40 ms where
 * nothing is specular, 1.4 ms with a glass blob and a mirror cube in view (rz_upscale_seethrough at factor 2: 0.77 and 2.0 ms).
 * rz_antialias_seethrough is rz_antialias with: seethrough (NULL: max_depth 8); guides = the rz_hit of the FINAL hit with t = L;
 * chains, optional, w*h rz_chain, 16-byte aligned on the device path.  Pointers, alignment, RZ_ANTIALIAS_HOST, stream, backstop
 * and "a failing call launches nothing" are rz_antialias'; in addition a max_depth outside 0..8 or a non-zero reserved word of
 * rz_seethrough_params is RZ_ERR_INVALID_ARG and a chains buffer that is too small RZ_ERR_BUFFER_SIZE.  rz_antialias_params.reserved
 * stays must-be-zero.  The calls touch no render, temporal or display state; the frame-size chain records live in the
 * see-through low-guide buffer, and the list of edge pixels between the pass's two kernels in a
 * buffer of its own.  rz_present_antialiased_seethrough is rz_present_antialiased with this pass.
 * (Additive: RZ_ABI_VERSION stays 5; no new struct, rz_sizeof(25) and rz_sizeof(27) stay 0.) */
int rz_antialias_seethrough(rz_ctx* ctx, const rz_antialias_params* params, const rz_seethrough_params* seethrough,
                            const float* rgb_in, size_t rgb_in_bytes, float* rgb32f, size_t rgb32f_bytes,
                            rz_hit* guides, size_t guides_bytes, rz_chain* chains, size_t chains_bytes,
                            uint8_t* edges, size_t edges_bytes, unsigned flags);
int rz_present_antialiased_seethrough(rz_ctx* ctx, const rz_present_params* present, const rz_antialias_params* antialias,
                                      const rz_seethrough_params* seethrough, const rz_display_params* display, int source,
                                      const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes,
                                      float* rgb32f, size_t rgb32f_bytes);

/* ------------------------------------------------------------------------ */
/* Where a frame is expensive: the per-pixel traversal cost map (new)       */
/* ------------------------------------------------------------------------ */
/* rz_render_counted prices a frame in the reference algorithm's memory touches, as totals.  rz_render_cost keeps the attribution:
 * for every pixel, what the reference shader would touch for that pixel's samples (rz_cost.hip).
 * rz_render_cost measures the frame of the last rz_set_frame -- size, camera, num_lights, bounce_budget -- with its own spp
 * (rz_cost_params.spp; 0 = the frame's), always from sample 0: samples 0 .. spp-1 of every pixel, from currentIor 1, exactly the
 * paths rz_render runs at sample_base 0.  The record of a pixel holds the eight traversal-side counts of rz_counters for those
 * paths, so every column summed over the frame is rz_render_counted's total.  `totals` is optional HOST memory whatever the
 * flags say: when given it receives exactly what rz_render_counted returns for the same frame at sample_base 0 (the call then
 * waits for its kernel).  The call sees the scene as the last upload / update / refit / pose / rebuild left it.  It leaves the
 * accumulation, currentIor, the pools, rz_debug_last_plan, rz_last_kernel_name, the ring of render times, and temporal and
 * display state untouched.  The context keeps the last cost buffer with its size and spp; `cost` may be NULL, in which case
 * only that copy is kept.  Row 0 of `cost` is the bottom row, as everywhere.
 * The VALUE v of a pixel is a uint64 and depends on the metric:
 *   0 bytes            32 tlas_nodes + 4 tlas_leaf_indices + 144 instances + 32 blas_nodes + 68 triangles + 32 materials +
 *                      32 light_fetches + 16 (rz_counters' formula with the pixel's own 16 bytes: the frame's sum is that total)
 *   1 node visits      tlas_nodes + blas_nodes
 *   2 triangle tests   triangles
 *   3 traversals       traversals
 *   4 instances        instances
 * rz_cost_view reduces the metric over the frame -- rz_cost_stats: the maximum, the LOWEST pixel index that attains it as
 * (max_x, max_y), the sum; exact integers, the same on every run -- and maps every pixel to a false colour, in binary32 with one
 * rounding per operation and no fused multiply-add:
 *   S = scale > 0 ? scale : (float)max_value, and 1 for a frame whose maximum is 0 (scale_used reports S);
 *   linear u = min((float)v / S, 1); logarithmic u = min(log2(1 + (float)v) / log2(1 + S), 1);
 *   k = min((int)(u * 4), 3), w = u * 4 - (float)k, c = a_k + (a_(k+1) - a_k) * w
 *   with the stops a_0 .. a_4 = (0,0,0), (0,0,1), (0,1,0), (1,1,0), (1,0,0): black, blue, green, yellow, red;
 *   a pixel with (float)v > S is (1,1,1): possible only under a caller's scale, it flags saturation.
 * With cost == NULL it views the context's last cost buffer: RZ_ERR_NOT_READY if there is none or the frame's size has changed
 * since.  A caller's buffer holds width * height records of the frame's size.  rgb32f (width * height * 3 floats) and stats are
 * each optional.  rz_present_cost is rz_present with that colour, as (c, 1), in place of the accumulation's divide, the way
 * rz_present_denoised does it, from the context's last cost buffer: wireframe, light markers and FPS digits are drawn on top of
 * the heat map.  Its buffers are host memory, as rz_present's.
 * Conventions are rz_denoise's.  cost, rgb32f and stats are DEVICE pointers (cost 16-byte, stats 8-byte, rgb32f 4-byte aligned)
 * and the work is queued on the context's stream, a walk cut at its backstop being left to rz_sync; with RZ_COST_HOST they are
 * host memory, staged, the call returns when they are written and reports a cut walk itself as RZ_ERR_INTERNAL.  A failing
 * call launches nothing and leaves its outputs untouched.
 * Errors.  RZ_ERR_NOT_READY: no scene, no materials (rz_render_cost) or no frame.  RZ_ERR_INVALID_ARG: null context; spp outside
 * 0..1024; unknown metric, curve or flags; scale negative or not finite; a non-zero reserved word; a misaligned device pointer;
 * a frame with tile_nranks > 1.  RZ_ERR_BUFFER_SIZE: any buffer too small.
 * Cost (profiles/cost/README.md): the path loop of the one-lane-per-pixel kernel plus 32 B per pixel -- a 1-spp map of a 1080p
 * frame of a 69 k-triangle scene takes 2.3 ms, 0.65 of that kernel's counted render; rz_cost_view 0.035 ms.
 * (Additive: RZ_ABI_VERSION stays 5; rz_sizeof(25) and rz_sizeof(27) stay 0.) */
typedef struct rz_pixel_cost {          /* 32 B; rz_sizeof(28) */
    uint32_t traversals, tlas_nodes, tlas_leaf_indices, instances, blas_nodes, triangles, materials, light_fetches;
} rz_pixel_cost;
typedef struct rz_cost_params {         /* NULL = defaults; 32 B; rz_sizeof(29) */
    int32_t spp;                        /* 0 = the frame's spp; else 1..1024 */
    int32_t reserved[7];                /* must be 0 */
} rz_cost_params;
typedef struct rz_cost_view_params {    /* NULL = defaults; 32 B; rz_sizeof(30) */
    int32_t metric;                     /* 0 bytes (default) 1 node visits 2 triangle tests 3 traversals 4 instances entered */
    int32_t curve;                      /* 0 linear (default), 1 logarithmic */
    float   scale;                      /* value at the top of the ramp; 0 = this frame's maximum */
    int32_t reserved[5];                /* must be 0 */
} rz_cost_view_params;
typedef struct rz_cost_stats {          /* 32 B; rz_sizeof(31) */
    uint64_t max_value, sum_value;
    int32_t  max_x, max_y;              /* lowest pixel index among the maxima; row 0 = bottom row */
    float    scale_used;
    int32_t  reserved;
} rz_cost_stats;
#define RZ_COST_HOST 1u                 /* pointers are host memory, as RZ_DENOISE_HOST */
int rz_render_cost(rz_ctx* ctx, const rz_cost_params* params, rz_pixel_cost* cost, size_t cost_bytes, rz_counters* totals,
                   unsigned flags);
int rz_cost_view(rz_ctx* ctx, const rz_cost_view_params* params, const rz_pixel_cost* cost, size_t cost_bytes,
                 float* rgb32f, size_t rgb32f_bytes, rz_cost_stats* stats, unsigned flags);
int rz_present_cost(rz_ctx* ctx, const rz_present_params* present, const rz_cost_view_params* params,
                    uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes);

/* ------------------------------------------------------------------------ */
/* Selecting what is on screen: coverage, marquee and outlines (new)        */
/* ------------------------------------------------------------------------ */
/* rz_coverage answers "which instances does this rectangle of the screen show, where and how near" on the device
 * (rz_coverage.hip).  Per pixel of the rectangle it casts the ray through the pixel centre from cam_pos, unclipped -- the ray of
 * rz_denoise's guide, so the closest hit of a pixel is what rz_denoise's guides and rz_trace_rays return for it -- and reduces the
 * hits per instance.  `frame` is taken as rz_render_editor takes it: the call reads width, height, inv_view, inv_proj and cam_pos,
 * needs no rz_set_frame and ignores the tile fields.  params NULL: the whole frame; else the pixels [x0, x1) x [y0, y1), row 0 =
 * the bottom row, intersected with the frame.
 * `coverage` holds n + 1 records, n = the instances of binding 9: record i < n is instance i, record n is the misses (pixels and
 * box filled, t_min / t_max as in an empty record).  An empty record is pixels 0, x_min = y_min = INT32_MAX, x_max = y_max = -1,
 * t_min = 1e30f, t_max = 0.  The pixels of all n + 1 records sum to the area of the clipped rectangle; a rectangle that is empty
 * after clipping gives RZ_OK and n + 1 empty records.  `ids` is optional and holds width * height int32 for the frame: every pixel
 * inside the clipped rectangle gets its instance index, -1 for a miss; pixels outside are not written.  Either output may be
 * NULL, not both.  The records are merged with integer operations that commute (add; signed min / max; unsigned min / max on the
 * bit pattern of t, which is positive and finite for a hit), so the bytes are the same on every run.
 * rz_outline marks a set of instances on an image, in place.  ids is width * height int32 (rz_coverage's, or the instance field of
 * a hit buffer); `selected` is a bit set, bit i & 31 of word i >> 5, in (n_instances + 31) / 32 words.  sel(p) = 0 <= ids[p] <
 * n_instances and that bit set (an id out of range is unselected).  Pixel p is an OUTLINE pixel iff sel(p) is false and some
 * pixel q inside the image with max(|dx|, |dy|) <= radius has sel(q) true.  On outline pixels o = in * (1 - alpha) + color * alpha
 * per channel, binary32, one rounding per operation, no fused multiply-add; for rgba8 in = (float)byte / 255.0f and the result is
 * written with rz_present's quantisation, rint(clamp(o, 0, 1) * 255), the alpha byte kept.  Every other pixel keeps its bytes
 * exactly, non-finite floats included.  Each image is optional, at least one must be given.  The call needs no scene and no frame.
 * Conventions are rz_denoise's.  Pointers are DEVICE memory (coverage 16-byte, everything else 4-byte aligned; rgba8 is read
 * and written as 4-byte pixels) and the work is queued on the context's stream, a walk cut at its backstop being left to rz_sync;
 * with RZ_COVERAGE_HOST / RZ_OUTLINE_HOST they are host memory, staged, the call returns when the outputs are written and
 * rz_coverage reports a cut walk itself as RZ_ERR_INTERNAL.  A failing call launches nothing and leaves its outputs untouched.
 * Neither call touches render state: accumulation, currentIor, pools, the frame of rz_set_frame, rz_debug_last_plan,
 * rz_last_kernel_name, the ring of render times, temporal and display state.
 * Errors.  RZ_ERR_NOT_READY: no scene (rz_coverage).  RZ_ERR_INVALID_ARG: null context, frame (rz_coverage), params, ids or
 * selected (rz_outline); a bad frame size; x1 < x0 or y1 < y0; both outputs (rz_coverage) or both images (rz_outline) NULL;
 * width or height <= 0, radius outside 1..4, a colour or alpha that is not finite, alpha outside [0, 1]; a non-zero reserved
 * word; unknown flags; a misaligned device pointer.  RZ_ERR_BUFFER_SIZE: any buffer too small.
 * Cost (profiles/coverage/README.md), 1080p, a 69 k-triangle mesh over a floor: rz_coverage with records and ids 0.157 ms, ids
 * alone 0.140 ms, against 0.158 ms for rz_denoise's guide cast; rz_outline 0.016 ms.  (Additive: RZ_ABI_VERSION stays 5;
 * rz_sizeof(32) stays 0.) */
typedef struct rz_coverage_params {      /* NULL = the whole frame; 32 B; rz_sizeof(33) */
    int32_t x0, y0, x1, y1;              /* pixels [x0, x1) x [y0, y1), row 0 = the bottom row; intersected with the frame */
    int32_t reserved[4];                 /* must be 0 */
} rz_coverage_params;
typedef struct rz_instance_coverage {    /* 32 B; rz_sizeof(34) */
    uint32_t pixels;                     /* pixels of the rectangle whose closest hit is this instance */
    int32_t  x_min, y_min, x_max, y_max; /* inclusive box of those pixels, frame coordinates */
    float    t_min, t_max;               /* smallest / largest rz_hit.t among them, bit for bit */
    uint32_t reserved;                   /* 0 */
} rz_instance_coverage;
typedef struct rz_outline_params {       /* 32 B; rz_sizeof(35) */
    int32_t width, height;               /* of ids and of the images */
    int32_t radius;                      /* line width in pixels, 1..4 */
    float   color[3];
    float   alpha;                       /* 0 <= alpha <= 1, all finite */
    int32_t reserved;                    /* must be 0 */
} rz_outline_params;
#define RZ_COVERAGE_HOST 1u              /* pointers are host memory, as RZ_DENOISE_HOST */
#define RZ_OUTLINE_HOST 1u
int rz_coverage(rz_ctx* ctx, const rz_frame_params* frame, const rz_coverage_params* params, rz_instance_coverage* coverage,
                size_t coverage_bytes, int32_t* ids, size_t ids_bytes, unsigned flags);
int rz_outline(rz_ctx* ctx, const rz_outline_params* params, const int32_t* ids, size_t ids_bytes, const uint32_t* selected,
               size_t n_instances, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes, unsigned flags);

/* ------------------------------------------------------------------------ */
/* Ambient occlusion for previews (new)                                     */
/* ------------------------------------------------------------------------ */
/* rz_ambient_occlusion gives the ray-cast viewport contact and depth: distance-limited ambient occlusion, N short visibility
 * walks per hit pixel over an interleaved 4 x 4 pattern of directions and an edge-aware 4 x 4 gather (rz_ao.hip).  All arithmetic
 * is binary32 with one rounding per operation, no fused multiply-add; `/` and sqrt are correctly rounded.
 * Direction table.  For candidates k = 1, 2, ...: a = (k * 3242174889u) >> 8, b = (k * 2447445414u) >> 8 (uint32, wrapping);
 * x1 = (float)a * 2^-23 - 1, x2 = (float)b * 2^-23 - 1; S = x1*x1 + x2*x2.  The candidate is accepted iff S < 1; the j-th accepted
 * candidate, j = 0..255, gives P_j = ((2*x1)*q, (2*x2)*q, 1 - 2*S) with q = sqrt(1 - S): Marsaglia's sphere point from an R2
 * lattice, no trigonometry.  321 candidates yield the 256 points.  The library builds the table once on the host;
 * rz_ao_directions copies its 256 x 3 floats to `out` and needs no GPU (RZ_ERR_INVALID_ARG: null out; RZ_ERR_BUFFER_SIZE).
 * Per pixel (X, Y), row 0 = the bottom row.  The guide is the closest hit of the pixel-centre ray from cam_pos, unclipped: the ray
 * and the record of rz_denoise's guide.  A miss gives raw = ao = 1.  For a hit with point x, unit normal n and ray direction d:
 * n_f = (n.x*d.x + n.y*d.y) + n.z*d.z > 0 ? -n : n;  o = x + n_f * 0.001f per component;  c = (X & 3) + 4 * (Y & 3).  For sample
 * i = 0..N-1: v = n_f + P[16*i + c], L2 = (v.x*v.x + v.y*v.y) + v.z*v.z.  If !(L2 >= 1e-6f), a_i = 1 and nothing is walked;
 * otherwise v = v / sqrt(L2) and a_i is rz_shadow_rays' answer for the ray (o, v, max_dist = radius): lit ? visibility : 0.
 * Glass attenuates, it does not block.  raw_p = tree(a) * (1.0f / N), tree the pairwise sum s[i] = s[2i] + s[2i+1] applied level
 * by level.  The walk is the shader's: it finds the closest hit in the whole scene and only then compares its distance with radius.
 * Smoothing (smooth = 1).  For a hit p the taps are q = (X + a, Y + b), b = -2..1 the outer loop and a = -2..1 the inner: the
 * window holds each of the 16 patterns once.  A tap counts iff q is inside the image, q is a hit and, for (a, b) != (0, 0),
 * dot(n_p, n_q) >= normal_cos and |dot(n_p, x_q - x_p)| <= ((plane_tol * t_p) * f) * max(|a|, |b|), with n, x, t the guide's
 * normal, point and distance, f = 2 |inv_proj[5]| / height evaluated in binary64 and rounded to binary32, dots and sums left to
 * right.  ao_p = (the sum of raw_q over the counted taps, in loop order) / (float)count.  With smooth = 0, ao_p = raw_p.
 * Outputs, each optional, at least one: ao, width*height floats; rgb32f, rgb_in * m per channel with m = 1.0f - strength *
 * (1.0f - ao_p), a NULL rgb_in standing for (1, 1, 1); rgba8, rz_present's quantisation of that colour, rint(clamp(c, 0, 1) *
 * 255), alpha 255.
 * Conventions are rz_coverage's.  `frame` is read for width, height, inv_view, inv_proj and cam_pos; no rz_set_frame is needed
 * and the tile fields are ignored.  Pointers are DEVICE memory (4-byte aligned), the work is queued on the context's stream and a
 * walk cut at its backstop is left to rz_sync; with RZ_AO_HOST they are host memory, staged, the call returns when the outputs
 * are written and reports a cut walk itself as RZ_ERR_INTERNAL.  A failing call launches nothing and leaves its outputs
 * untouched.  No render, temporal or display state is touched (the guide goes to the scratch rz_denoise casts its own into).
 * Errors.  RZ_ERR_INVALID_ARG: null context or frame; unknown flags; a bad frame size; samples not 1, 2, 4, 8 or 16; radius or
 * plane_tol not finite and > 0; smooth not 0 or 1; strength outside [0, 1]; normal_cos outside [-1, 1]; a non-zero reserved
 * word; no output given; a misaligned device pointer.  RZ_ERR_NOT_READY: no scene, or no materials.  RZ_ERR_BUFFER_SIZE: any
 * buffer too small.  Cost: profiles/ao/README.md.  (Additive: RZ_ABI_VERSION stays 5; rz_sizeof(36) stays 0.) */
typedef struct rz_ao_params {            /* NULL = defaults; 32 B; rz_sizeof(37) */
    int32_t samples;                     /* N: 1, 2, 4, 8, 16; default 4 */
    float   radius;                      /* world units, finite, > 0; default 1 */
    int32_t smooth;                      /* 0 / 1; default 1 */
    float   strength;                    /* 0..1; default 1 */
    float   normal_cos, plane_tol;       /* tap validity; defaults 0.9 and 2 */
    int32_t reserved[2];                 /* must be 0 */
} rz_ao_params;
#define RZ_AO_HOST 1u                    /* pointers are host memory, as RZ_DENOISE_HOST */
int rz_ambient_occlusion(rz_ctx* ctx, const rz_frame_params* frame, const rz_ao_params* params, const float* rgb_in,
                         size_t rgb_in_bytes, float* ao, size_t ao_bytes, float* rgb32f, size_t rgb32f_bytes, uint8_t* rgba8,
                         size_t rgba8_bytes, unsigned flags);
int rz_ao_directions(float* out, size_t bytes);

/* ------------------------------------------------------------------------ */
/* Adaptive sampling (new)                                                  */
/* ------------------------------------------------------------------------ */
/* rz_render_adaptive renders the frame of rz_set_frame in batches of s = batch_spp samples per pixel and stops sampling the
 * 8 x 8 tiles whose estimated error has fallen under a threshold.  The render kernels are rz_render's own, launched over
 * contiguous runs of tiles (row-major tile index, tile (0, 0) at the bottom left); a path's arithmetic does not depend on the
 * launch that runs it, so every pixel ends with exactly the bits rz_render gives at that pixel's own sample count.  The result
 * is the ordinary accumulation: rgb the running sum, a the pixel's own sample count, which every presenting and off-frame call
 * divides by per pixel.  Between batches a metering kernel (rz_adaptive_meter, rz_adaptive.hip) decides which tiles go on.
 * Sequence.  Batch 1 is the whole frame from sample 0.  After batch B = 1, 2, ... the meter runs over the tiles batch B rendered,
 * one byte of flags per tile comes back to the host, rz_adaptive_plan makes the runs of batch B + 1 from them, and batch B + 1
 * is one launch per run from sample B * s.  The call ends when no tile is active or after max_batches; it returns when the
 * frame is complete.  The frame's spp and sample_base are ignored and left as they are.
 * The meter.  All arithmetic is binary32 with one rounding per operation, no fused multiply-add; `/` and sqrt are correctly
 * rounded.  The context keeps per pixel prev (4 floats: the accumulation after the previous batch) and (S1, S2), all zero
 * before batch 1.  Per pixel inside the frame, with I the accumulation after batch B and fs = (float)s, fB = (float)B:
 *   d.c = (I.c - prev.c) / fs for c = r, g, b;  L = (0.2126f * d.r + 0.7152f * d.g) + 0.0722f * d.b;
 *   S1 = S1 + L;  S2 = S2 + L * L;  prev = I;  m = S1 / fB;
 *   B >= 2: x = (S2 - S1 * m) / (float)(B - 1);  v = x > 0 ? x : (x is a NaN ? x : 0);  e = sqrt(v / fB).   B = 1: e = 0.
 * A lane outside the frame contributes e = 0 and |m| = 0.  Per tile, lane = x + 8 * y inside the tile: num = the sum of e and
 * sm = the sum of |m| over the 64 lanes, each by the butterfly t[l] = t[l] + t[l ^ o] for o = 32, 16, 8, 4, 2, 1 in this order;
 * den = sm + luminance_floor * (float)(pixels of the tile inside the frame);  E = num / den.
 * A tile starts active and retires -- for good -- when B >= min_batches and E <= threshold; the comparison is false for a NaN,
 * so a tile with non-finite samples stays active to the end.  A tile is current while it has received every batch so far.  A
 * retired tile that a merged run covers is rendered and metered again (its E and its count follow) and stays retired.
 * The luminance of a batch is the difference of two running sums, so E carries their rounding: about 1e-4 on a tile of constant
 * colour.  Thresholds under about 1e-3 ask for more than the numbers hold.
 * The plan.  rz_adaptive_plan needs no GPU.  active / current: one byte per tile, non-zero = set.  (1) The runs are the maximal
 * intervals of active tiles.  (2) Two neighbouring runs merge when the gap between them is at most merge_gap tiles and every
 * tile of the gap is current; merged runs merge on by the same rule.  (3) While there are more than max_runs runs and two
 * neighbours with an all-current gap between them, whatever its length, the pair with the smallest such gap merges, the lowest
 * tile index first among equals.  (4) If none is left the plan stands with more runs: max_runs is a target.  The runs are
 * written in ascending order and *n_runs is set to their number, also when `cap` is too small for them (RZ_ERR_BUFFER_SIZE,
 * nothing written).  RZ_ERR_INVALID_ARG: null active, current (with n_tiles > 0) or n_runs, null runs with cap > 0, merge_gap
 * < 0, max_runs < 1, n_tiles > 2^30.  Here merge_gap and max_runs are taken as given: 0 merges nothing in step 2.
 * rz_render_adaptive.  params NULL = defaults.  tile_batches / tile_error: one int32 / float per tile, the batches the tile
 * received and its last E; each optional; DEVICE memory (4-byte aligned), or host memory with RZ_ADAPTIVE_HOST.  info, optional,
 * is host memory.  Both backends, a bound accumulation (rz_bind_accum) and the backstop word (left to rz_sync) work as in
 * rz_render; rz_last_kernel_name and rz_debug_last_plan describe the call's last render launch, and the timing ring of
 * rz_last_render_ms is not advanced.  No temporal, display or other state is touched, and a following rz_render from sample 0
 * gives what it gives on a fresh context.  Continuing an adaptive frame with rz_render at sample_base > 0 is not defined: the
 * pixels are at different sample counts.  rz_group_* has no adaptive form.
 * Errors, nothing launched.  RZ_ERR_INVALID_ARG: null context; unknown flags; batch_spp outside 1..1024; min_batches outside
 * 2..64; max_batches outside min_batches..64; a NaN threshold; luminance_floor not finite or < 0; merge_gap < -1; max_runs < 0;
 * a misaligned device pointer; a frame that is one of several tile ranks (tile_nranks > 1).  RZ_ERR_NOT_READY: no rz_set_frame,
 * no scene.  RZ_ERR_BUFFER_SIZE: tile_batches or tile_error too small, or a bound accumulation smaller than the frame.
 * Cost, where it pays and where it loses: profiles/adaptive/README.md.  (Additive: RZ_ABI_VERSION stays 5.) */
typedef struct rz_adaptive_params {      /* a zero field = its default; 32 B; rz_sizeof(38) */
    int32_t  batch_spp;                  /* s, 1..1024; default 8 */
    int32_t  min_batches;                /* 2..64; default 4 */
    int32_t  max_batches;                /* min_batches..64; default 8, or min_batches if that is more */
    float    threshold;                  /* default 0.02; negative: no tile retires; +inf: every finite tile retires at min_batches */
    float    luminance_floor;            /* finite, > 0; default 0.01 */
    int32_t  merge_gap;                  /* tiles; default 8; -1: merge nothing in step 2 */
    int32_t  max_runs;                   /* the target of step 3; default 1: one launch per batch, from the first active tile to the last */
    uint32_t flags;                      /* RZ_ADAPTIVE_HOST */
} rz_adaptive_params;
#define RZ_ADAPTIVE_HOST 1u              /* tile_batches and tile_error are host memory */
#define RZ_ADAPTIVE_MAX_BATCHES 64
typedef struct rz_adaptive_info {        /* 800 B; rz_sizeof(39) */
    int32_t  batches;                    /* batches run */
    int32_t  n_tiles;                    /* tiles of the frame */
    uint64_t samples_traced;             /* s x the pixels inside the frame of every tile rendered, over the batches */
    uint64_t samples_uniform;            /* width x height x max_batches x s */
    float    render_ms, meter_ms;        /* the render launches and the metering launches, from events on the stream */
    int32_t  tiles_active[RZ_ADAPTIVE_MAX_BATCHES];      /* [B - 1]: tiles still active after batch B's metering */
    int32_t  tiles_rendered[RZ_ADAPTIVE_MAX_BATCHES];    /* [B - 1]: tiles batch B rendered, and */
    int32_t  runs[RZ_ADAPTIVE_MAX_BATCHES];              /* [B - 1]: the launches it took */
} rz_adaptive_info;
typedef struct rz_tile_run {             /* 8 B; rz_sizeof(40) */
    int32_t first, len;
} rz_tile_run;
int rz_render_adaptive(rz_ctx* ctx, const rz_adaptive_params* params, rz_adaptive_info* info, int32_t* tile_batches,
                       size_t tile_batches_bytes, float* tile_error, size_t tile_error_bytes);
int rz_adaptive_plan(const uint8_t* active, const uint8_t* current, size_t n_tiles, int merge_gap, int max_runs,
                     rz_tile_run* runs, size_t cap, size_t* n_runs);

/* ------------------------------------------------------------------------ */
/* Drawing into the scene: depth-tested 3D lines (new)                      */
/* ------------------------------------------------------------------------ */
/* rz_draw_lines blends n line segments given in world space, or in the space of an instance, over a presented image, in place,
 * each tested per pixel against the depth of a hit image (rz_lines.hip): a ground grid, gizmo axes, the box of a selection, a
 * camera frustum, the edges of a mesh.  All arithmetic is binary32 with one rounding per operation, no fused multiply-add; `/`
 * and sqrt are correctly rounded.  m4v(M, x, y, z, w) is the column-major product with each row summed left to right,
 * ((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r] * w.  clamp(x, lo, hi) = min(max(x, lo), hi) with minNum / maxNum (a NaN
 * x gives lo).  For line i, in this order:
 *  1 World ends.  instance < 0: a and b, bit for bit.  Otherwise (x, y, z) of m4v(M, a, 1) and of m4v(M, b, 1) with M the
 *    `transform` of that instance of binding 9 as it stands on the device after the last rz_update_transforms.  An instance >=
 *    the instance count is RZ_ERR_INVALID_ARG on the host path; on the device path the line is dropped.
 *  2 Clip space.  VP = proj * view, VP[4 c + r] = ((proj[r] * view[4 c] + proj[4 + r] * view[4 c + 1]) + proj[8 + r] *
 *    view[4 c + 2]) + proj[12 + r] * view[4 c + 3] (rz_present's).  A = m4v(VP, a, 1), B = m4v(VP, b, 1).
 *  3 Near clip on w, n = near_w.  If neither A.w >= n nor B.w >= n the line is dropped (a NaN fails the comparison).  If only A
 *    fails: k = (n - A.w) / (B.w - A.w), A.x = A.x + k * (B.x - A.x), A.y likewise, A.w = n.  If only B fails, the same with the
 *    roles swapped.  There is no far clip.
 *  4 Screen ends.  sx = (x / w * 0.5f + 0.5f) * (float)width, sy likewise with height, for both ends: A_s and B_s.  A line with
 *    a non-finite screen coordinate is dropped.  ia = 1.0f / A.w, ib = 1.0f / B.w.
 *  5 Per pixel p = (px, py), centre (fx, fy) = ((float)px + 0.5f, (float)py + 0.5f), row 0 = the bottom row.  ab = B_s - A_s,
 *    L = ab.x * ab.x + ab.y * ab.y, pa = (fx, fy) - A_s;  t = L == 0 ? 0 : clamp((pa.x * ab.x + pa.y * ab.y) / L, 0, 1);
 *    dx = fx - (A_s.x + t * ab.x), dy likewise, d = sqrt(dx * dx + dy * dy): rz_present's distanceToSegment.  hw = width * 0.5f.
 *    Hard edge (smooth = 0): covered iff d < hw, cov = 1.  Smooth: cov = clamp((hw + 0.5f) - d, 0, 1), covered iff cov > 0.
 *  6 Depth, for a covered pixel.  w_s = 1.0f / (ia + t * (ib - ia)).  If hits is given and the pixel's record is a hit (instance
 *    >= 0): w_h = ((VP[3] * X + VP[7] * Y) + VP[11] * Z) + VP[15] of its point (X, Y, Z), and the line is OCCLUDED at p iff
 *    w_s * (1.0f - depth_bias) > w_h.  alpha = (float)alpha_byte / 255.0f, times hidden_alpha if occluded, then times cov.
 *    alpha == 0: the line does not touch p.
 *  7 Blend, over the lines that touch p in ascending index: o = in * (1.0f - alpha) + c * alpha per channel, c = (float)byte /
 *    255.0f.  rgb32f is blended as it stands.  An rgba8 pixel is converted once, (float)byte / 255.0f, blended by all its lines in
 *    float and quantised once as rz_present does, rint(clamp(o, 0, 1) * 255); its alpha byte is kept.  A pixel no line touches is
 *    not written and keeps its bytes, non-finite floats included.
 * `frame` is read as rz_render_editor reads it -- width, height, view and proj only; no rz_set_frame is needed and the tile
 * fields are ignored.  width and height are at most 2^23 (a pixel centre is exact in binary32).  params NULL: the defaults.
 * hits is optional: NULL means no depth test, every line counts as visible; else width * height rz_hit, rz_render_editor's hits
 * or the guides of rz_denoise and its relatives.  Each image is optional, at least one must be given.  n = 0 is RZ_OK and writes
 * nothing; n is at most 2^20.  A scene is needed only if some line has instance >= 0.
 * Conventions are rz_outline's.  Pointers are DEVICE memory (lines and hits 16-byte, the images 4-byte aligned; rgba8 is read and
 * written as 4-byte pixels) and the work is queued on the context's stream; with RZ_LINES_HOST they are host memory, staged, and
 * the call returns when the images are written.  The lines are binned on the device into lists per 128 x 128 pixels, made with
 * ballots and prefix sums in line order, in a workspace the context keeps and grows on demand: a device-path call whose lists
 * might not fit what it holds (more than 4 MiB if every line met every cell) waits for the count of its entries before it
 * queues the rest.  The bytes are the same on every run.  A failing call launches nothing that writes the images and leaves them
 * untouched; that includes RZ_ERR_NO_MEMORY and RZ_ERR_HIP from growing the workspace.  No render, temporal or display state and
 * not the frame of rz_set_frame is touched.
 * Errors.  RZ_ERR_INVALID_ARG: null context or frame; unknown flags; a bad frame size; width outside [1, 16], near_w not > 0,
 * depth_bias outside [0, 1), hidden_alpha outside [0, 1], any of them not finite, smooth not 0 or 1, a non-zero reserved word;
 * NULL lines with n > 0; n > 2^20; both images NULL; a misaligned device pointer; on the host path a line whose instance is not
 * below the instance count.  RZ_ERR_BUFFER_SIZE: hits or an image too small.  RZ_ERR_NOT_READY: on the host path a line names an
 * instance and no scene has been uploaded (on the device path the lines are not read on the host: without a scene every line
 * that names an instance is dropped).  Cost: profiles/lines/README.md.
 * (Additive: RZ_ABI_VERSION stays 5; rz_sizeof(41) stays 0.) */
typedef struct rz_line {                 /* 32 B; rz_sizeof(42) */
    float    a[3];  uint32_t color;      /* bytes r, g, b, alpha in memory order */
    float    b[3];  int32_t  instance;   /* < 0: a, b are world space; else local to that instance of binding 9 */
} rz_line;
typedef struct rz_lines_params {         /* NULL = defaults; 32 B; rz_sizeof(43) */
    float   width;                       /* full line width in pixels, 1..16; default 1.5 */
    float   near_w;                      /* clip threshold on clip-space w, > 0; default 0.01 */
    float   depth_bias;                  /* relative, 0 <= bias < 1; default 0x1p-8 */
    float   hidden_alpha;                /* 0..1: factor on alpha where the line is behind the hit; 0 = hidden; default 0 */
    int32_t smooth;                      /* 0 hard edge, 1 one-pixel coverage ramp; default 0 */
    int32_t reserved[3];                 /* must be 0 */
} rz_lines_params;
#define RZ_LINES_HOST 1u                 /* pointers are host memory, as RZ_DENOISE_HOST */
int rz_draw_lines(rz_ctx* ctx, const rz_frame_params* frame, const rz_lines_params* params,
                  const rz_line* lines, size_t n, const rz_hit* hits, size_t hits_bytes,
                  uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes, unsigned flags);

/* ------------------------------------------------------------------------ */
/* Glare: light that spills from over-bright pixels (new)                   */
/* ------------------------------------------------------------------------ */
/* The display stage tones every pixel on its own, so a pixel 50 times over white looks like one barely over it.  rz_bloom adds
 * the glare of the over-bright pixels to their neighbours, in linear HDR colour, in front of that stage (rz_bloom.hip): the
 * bright part of the frame is taken down an image pyramid and back up.  All arithmetic is binary32 with one rounding per
 * operation, no fused multiply-add; `/` is correctly rounded; min / max are minNum / maxNum.  Row 0 = the bottom row; the frame
 * is W x H.
 *  1 Level sizes.  (w_0, h_0) = (ceil(W / 2), ceil(H / 2)), (w_{k+1}, h_{k+1}) = (ceil(w_k / 2), ceil(h_k / 2)); levels are
 *    appended until one is 1 x 1 or there are `levels` of them; L is their number (a 1 x 1 frame: L = 1; 1920 x 1080 with 6
 *    levels ends at 30 x 17).
 *  2 Prefilter, per pixel of colour c.  A pixel with a NaN or +-Inf channel (decided on the bit pattern, as rz_denoise decides
 *    it) contributes p = (0, 0, 0).  Otherwise c' = max(c, 0) per channel (+0 for every c <= 0), b = max(max(c'.r, c'.g), c'.b),
 *    d = b - threshold, s = min(max(d + knee, 0), 2 * knee), q = knee > 0 ? (s * s) / (4 * knee) : 0, m = min(max(q, d), limit),
 *    f = m > 0 ? m / max(b, 1e-4f) : 0, p = c' * f: nothing below threshold - knee, m = b - threshold above threshold + knee, a
 *    quadratic onset between them, and no pixel glares with more than `limit`.
 *  3 Down.  D_0 is made from p, D_{k+1} from D_k, by the 4 x 4 filter (1, 3, 3, 1) x (1, 3, 3, 1) / 64 with its taps at 2X - 1 ..
 *    2X + 2 and 2Y - 1 .. 2Y + 2, each index clamped to the source.  Rows first, r_j = ((t_{-1} + 3 * t_0) + 3 * t_1) + t_2; the
 *    four row results are combined the same way in ascending y; the result is multiplied by 0.015625f.
 *  4 Up(S, w, h) resamples a coarse image S to w x h.  For output x: near = x / 2, far = x even ? x / 2 - 1 : x / 2 + 1, both
 *    clamped to S; the same for y.  r = 3 * S[near_x] + S[far_x] on a row, then (3 * r[near_y] + r[far_y]) * 0.0625f.
 *  5 Merge.  U_{L-1} = D_{L-1}; for k = L - 2 down to 0, U_k = D_k + spread * Up(U_{k+1}, w_k, h_k).
 *  6 Combine.  N = the sum of spread^k over k < L in binary64 on the host, ascending k, the powers by repeated multiplication
 *    from (double)spread; n = (float)(1 / N); glare = Up(U_0, W, H) * n; out = c + intensity * glare.  A bad pixel's out is
 *    whatever that expression gives; its neighbours stay finite.  With intensity == 0 out is c bit for bit (a copy, or nothing
 *    when in place) and the pyramid is made only if `glare` is asked for.
 * rz_bloom has rz_display's conventions: device pointers by default (4-byte aligned), the work is queued on the context's stream
 * and the call returns at once; width and height come from the last rz_set_frame (no scene is needed).  rgb_in is W*H*3 floats
 * of linear colour; rgb_in NULL reads the accumulation as c = rgb / n, n = a > 0 ? a : 1 (refused for a frame with tile_nranks
 * > 1, as rz_display refuses it).  Outputs, each optional, at least one:
 *   rgb32f   W*H*3 floats: the frame with glare, linear and unclamped (may be rgb_in itself: in place)
 *   glare    W*H*3 floats: the normalised glare alone (must not alias rgb_in or rgb32f)
 * With RZ_BLOOM_HOST the pointers are host memory, staged through buffers of the context, and the call returns when the outputs
 * are written.  The pyramid (a float4 per texel, 4 / 3 of a quarter frame) lives in a workspace of the context, allocated on
 * first use, kept, and freed with the context.  2 L kernels run, the same bytes on every run.  The call touches no render
 * state, temporal history, display state or frame.
 * rz_present_bloomed is rz_present_display with the pass between the source's colour and the display stage: source and
 * filter_params are rz_present_display's (source 2 advances the temporal history as rz_present_temporal does); the display
 * stage, metering included, runs unchanged on the bloomed colour and commits its exposure as rz_present_display does; the
 * overlays are drawn on top.  bloom NULL: the defaults.  With intensity == 0 the bytes are rz_present_display's exactly.  With
 * source 0 and intensity > 0 it needs the whole frame (tile_nranks == 1), as metering does.
 * Errors.  RZ_ERR_INVALID_ARG: null context; a field outside its range or not finite where it must be; non-zero reserved words;
 * unknown flags; a misaligned device pointer; both outputs NULL; glare aliasing rgb_in or rgb32f; a frame of more than 262140
 * rows (rz_present_bloomed: also what rz_present_display says).  RZ_ERR_BUFFER_SIZE: a buffer that is too small.
 * RZ_ERR_NOT_READY: no rz_set_frame.  RZ_ERR_NO_MEMORY, RZ_ERR_HIP: the workspace could not be allocated.  A failing call
 * launches nothing and writes nothing.  Cost: profiles/bloom/README.md.
 * (Additive: RZ_ABI_VERSION stays 5; rz_sizeof(44) stays 0.) */
typedef struct rz_bloom_params {         /* NULL = defaults; 32 B; rz_sizeof(45) */
    float   threshold;                   /* brightness above which a pixel glares; finite, >= 0; default 1 */
    float   knee;                        /* half-width of the soft onset below / above the threshold; finite, >= 0; default 0.5 */
    float   limit;                       /* cap on a pixel's glaring brightness (fireflies); > 0, +Inf allowed; default 64 */
    float   intensity;                   /* weight of the glare added to the frame; finite, >= 0; default 0.25 */
    float   spread;                      /* weight of each coarser level relative to the finer; finite, 0 < spread <= 4; default 1 */
    int32_t levels;                      /* most pyramid levels, 1..8; default 6 */
    int32_t reserved[2];                 /* must be 0 */
} rz_bloom_params;
#define RZ_BLOOM_HOST 1u                 /* pointers are host memory, as RZ_DISPLAY_HOST */
int rz_bloom(rz_ctx* ctx, const rz_bloom_params* params, const float* rgb_in, size_t rgb_in_bytes,
             float* rgb32f, size_t rgb32f_bytes, float* glare, size_t glare_bytes, unsigned flags);
int rz_present_bloomed(rz_ctx* ctx, const rz_present_params* present, const rz_display_params* display,
                       const rz_bloom_params* bloom, int source, const void* filter_params,
                       uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes);

/* Number of HIP devices visible to the process (0 without a GPU). */
int rz_device_count(void);

/* Library/version probe that needs no GPU. */
const char* rz_version(void);
/* The ABI revision this library was compiled to: bumped whenever a struct of this header changes size or meaning
 * (rz_counters grew in round 4 without one -- a caller built against the older header would have been written past).
 * A binding compares it with RZ_ABI_VERSION of the header it was written against before its first call. */
#define RZ_ABI_VERSION 5
int rz_abi_version(void);
/* Which implementation of the three built-ins GLSL leaves open -- sin, cos, acos; RayZen's hash is fract(sin(x) * 43758.5453)
 * (fragment_shader.glsl:188-190) -- this library was compiled with (rz_device_math.h, RZ_MATH_FLAVOUR): 1 = Mesa llvmpipe's, the
 * OpenGL implementation RayZen's own shader was run on for this project's parity tests (binary32 Cephes sin / cos with fused
 * multiply-adds, Mesa's acos polynomial); 0 = binary64 evaluation rounded once (correctly rounded).  A frame is a function of this
 * choice from the third path segment on.  Needs no GPU. */
int rz_math_flavour(void);
/* sha256 (64 hex digits) of the sources and compiler flags this library was built from (rayzen_amd/build.py:
 * source_hash), or "unstamped": ties the LOADED library to a source tree and to a committed profile.  Needs no GPU. */
const char* rz_source_hash(void);
/* sizeof() of the ABI structs as compiled into the library, for layout
 * checks from other languages: which = 0 triangle, 1 node, 2 instance,
 * 3 material, 4 light, 5 frame_params, 6 counters, 7 ray, 8 hit,
 * 9 visibility, 10 editor_params, 11 denoise_params, 12 temporal_params,
 * 14 display_params, 15 display_info, 17 skin_triangle, 18 morph_triangle, 20 mesh_quality,
 * 21 upscale_params, 23 seethrough_params, 24 chain, 26 antialias_params, 28 pixel_cost, 29 cost_params, 30 cost_view_params,
 * 31 cost_stats, 33 coverage_params, 34 instance_coverage, 35 outline_params, 37 ao_params, 38 adaptive_params, 39 adaptive_info,
 * 40 tile_run, 42 line, 43 lines_params, 45 bloom_params (13, 16, 19, 22, 25, 27, 32, 36, 41 and 44 are unassigned and
 * return 0, as every unknown index does). */
size_t rz_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif /* RAYZEN_HIP_H */

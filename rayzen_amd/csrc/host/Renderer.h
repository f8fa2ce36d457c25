// Renderer.h -- the frontend-side glue: what RayZen's main.cpp does with
// OpenGL, done with the C-ABI of include/rayzen_hip.h instead.  Header-only;
// link the program with librayzen_host.so and librayzen_hip.so.
//
//   initializeSSBOs(scene)             <- main.cpp:897-1120  (build + 8x glBufferData)
//   updateDynamicBVHAndSSBOs(scene)    <- main.cpp:1123-1208 (TLAS rebuild + glBufferSubData)
//   sendSceneDataToShader(scene, ...)  <- main.cpp:1356-1392 (uniforms)
//   draw() / finish()                  <- main.cpp:637 glDrawArrays / :1347 glFinish
//   pick(mouseX, mouseY, scene)        <- main.cpp:501-552 (brute-force picking loop), one ray query instead
//   renderEditor(scene, width, height) <- main.cpp:1210-1322 (renderRasterized + the editor shaders), a ray cast instead
//   denoise() / presentDenoised()      <- new: the a-trous denoiser of the 1-spp frame (rz_denoise / rz_present_denoised)
//   denoiseTemporal() / presentTemporal() / resetTemporal()
//                                      <- new: temporal accumulation + the variance-guided filter (rz_denoise_temporal)
//   presentUpscaled()                  <- new: render below display size, reconstruct at display size (rz_present_upscaled,
//                                         and rz_present_upscaled_seethrough: guides that follow glass and mirrors)
//   presentDisplay() / resetDisplay()  <- new: exposure, tone curve and sRGB encode in front of present (rz_present_display;
//                                         with an rz_antialias_params: rz_present_antialiased, anti-aliased edges; with an
//                                         rz_seethrough_params too: rz_present_antialiased_seethrough)
// Unlike the reference's per-frame path, updateDynamicBVHAndSSBOs re-uploads
// only what changed (instances + TLAS, a few KB), not all geometry.
//
// Deformation and the per-frame update: refitMesh, refitAll, poseRig and rebuildDegraded change the geometry ON THE DEVICE
// and leave the host copies in buffers() as they were handed over.  From then on, until the next initializeSSBOs /
// initializeSSBOsOnDevice, updateDynamicBVHAndSSBOs does its work on the device too (rz_update_transforms, the route of
// updateDynamicBVHAndSSBOsOnDevice): both routes leave the context with identical bindings, and those are the deformed
// geometry's -- world boxes and TLAS from the refitted roots, blasNodeOffset as a rebuild left it.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <optional>
#include <stdexcept>
#include <utility>
#include <string>
#include <vector>

#include "RayZenScene.h"
#include "rayzen_hip.h"

// The first of the three entry points of the front end that are referenced WEAKLY: a program linked against a library from before it, or against
// a stand-in that defines only what it exercises, still links, and presentUpscaled(..., &seeThrough) throws there.
extern "C" int rz_present_upscaled_seethrough(rz_ctx* ctx, const rz_present_params* present, const rz_upscale_params* upscale,
                                              const rz_seethrough_params* seethrough, const rz_display_params* display, int source,
                                              const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f,
                                              size_t rgb32f_bytes) __attribute__((weak));
// ... and rz_present_antialiased, on the same terms: presentDisplay(..., &antialias) throws where it is absent.
extern "C" int rz_present_antialiased(rz_ctx* ctx, const rz_present_params* present, const rz_antialias_params* antialias,
                                      const rz_display_params* display, int source, const void* filter_params, uint8_t* rgba8,
                                      size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) __attribute__((weak));
// ... and rz_present_antialiased_seethrough: presentDisplay(..., &antialias, &seeThrough) throws where it is absent.
extern "C" int rz_present_antialiased_seethrough(rz_ctx* ctx, const rz_present_params* present, const rz_antialias_params* antialias,
                                                 const rz_seethrough_params* seethrough, const rz_display_params* display, int source,
                                                 const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f,
                                                 size_t rgb32f_bytes) __attribute__((weak));

namespace rayzen {

class Renderer {
public:
    explicit Renderer(int device = 0, unsigned flags = RZ_FLAG_NONE) : ctx_(rz_create(device, flags)) {
        if (!ctx_) throw std::runtime_error(std::string("rz_create: ") + rz_last_error(nullptr));
    }
    ~Renderer() { rz_destroy(ctx_); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    // Build every BLAS on the device (rz_build_blas: RayZen's full-sweep SAH, same bytes as BVH::buildBLAS).
    void useDeviceBlasBuilder(bool on = true) {
        if (!on) { buffers_.blasBuilder = nullptr; return; }
        buffers_.blasBuilder = [this](const Mesh& mesh, BVH& out) {
            const size_t n = mesh.triangles.size();
            out.nodes.assign(n ? 2 * n - 1 : 1, BVHNode{});
            out.triIndices.assign(n, 0);
            size_t nn = 0;
            if (rz_build_blas(ctx_, reinterpret_cast<const rz_triangle*>(mesh.triangles.data()), n,
                              reinterpret_cast<rz_bvh_node*>(out.nodes.data()), out.nodes.size(), out.triIndices.data(), &nn,
                              nullptr, nullptr) != RZ_OK) return false;
            out.nodes.resize(nn);
            return true;
        };
    }

    void initializeSSBOs(const Scene& scene, bool shareMeshes = false) {
        if (!buffers_.build(scene, shareMeshes)) throw std::runtime_error(std::string("rz_build_blas: ") + rz_last_error(ctx_));
        up(RZ_BIND_TRIANGLES, buffers_.allTriangles);
        up(RZ_BIND_MATERIALS, scene.materials);
        up(RZ_BIND_LIGHTS, scene.lights);
        up(RZ_BIND_TLAS_NODES, buffers_.tlasNodes);
        up(RZ_BIND_TLAS_INDICES, buffers_.tlasTriIndices);
        up(RZ_BIND_BLAS_NODES, buffers_.allBLASNodes);
        up(RZ_BIND_BLAS_INDICES, buffers_.allBLASTriIndices);
        up(RZ_BIND_INSTANCES, buffers_.meshInstances);
        deviceGeometryNewer_ = false;
    }
    // initializeSSBOs with the geometry half on the GPU (rz_build_geometry): one BLAS per distinct Mesh is built on the
    // device and stays there as bindings 7 / 8; only instances, the TLAS, materials and lights are assembled here and
    // uploaded.  Frames are the same bits as after initializeSSBOs(scene, /*shareMeshes=*/true).
    void initializeSSBOsOnDevice(const Scene& scene) {
        static const Mesh kEmpty;
        std::map<const Mesh*, size_t> index;
        std::vector<rz_mesh_build> built;
        SceneBuffers b;
        std::vector<size_t> meshOf(scene.gameObjects.size());
        for (size_t i = 0; i < scene.gameObjects.size(); ++i) {
            const Mesh* mesh = scene.gameObjects[i].mesh ? scene.gameObjects[i].mesh.get() : &kEmpty;
            auto it = index.find(mesh);
            if (it == index.end()) {
                it = index.emplace(mesh, built.size()).first;
                rz_mesh_build m{};
                m.first_triangle = b.allTriangles.size(); m.n_triangles = mesh->triangles.size();
                built.push_back(m);
                b.allTriangles.insert(b.allTriangles.end(), mesh->triangles.begin(), mesh->triangles.end());
            }
            meshOf[i] = it->second;
        }
        check(rz_build_geometry(ctx_, reinterpret_cast<const rz_triangle*>(b.allTriangles.data()), b.allTriangles.size(), built.data(),
                                built.size()), "rz_build_geometry");
        std::vector<BVHNode> worldRootNodes;
        for (size_t i = 0; i < scene.gameObjects.size(); ++i) {
            const rz_mesh_build& m = built[meshOf[i]];
            BVHNode root;
            std::memcpy(static_cast<void*>(&root), &m.root, sizeof root);
            worldRootNodes.push_back(worldRootNode(root, scene.gameObjects[i].transform));      // main.cpp:974-993
            b.blasRoots.push_back(root);
            BVHInstance inst;
            inst.blasNodeOffset = m.node_offset; inst.blasTriOffset = m.index_offset;
            inst.globalTriOffset = (int)m.first_triangle; inst.meshIndex = (int)i;
            inst.transform = scene.gameObjects[i].transform;
            inst.inverseTransform = inverse(scene.gameObjects[i].transform);
            b.meshInstances.push_back(inst);
            b.maxBLASDepth = std::max(b.maxBLASDepth, (int)m.depth);
        }
        BVH tlas;
        tlas.buildTLAS(b.meshInstances, worldRootNodes);
        b.tlasNodes = tlas.nodes; b.tlasTriIndices = tlas.triIndices; b.tlasDepth = tlas.depth();
        b.blasBuilder = buffers_.blasBuilder;
        buffers_ = std::move(b);
        up(RZ_BIND_MATERIALS, scene.materials);
        up(RZ_BIND_LIGHTS, scene.lights);
        up(RZ_BIND_TLAS_NODES, buffers_.tlasNodes);
        up(RZ_BIND_TLAS_INDICES, buffers_.tlasTriIndices);
        up(RZ_BIND_INSTANCES, buffers_.meshInstances);
        deviceGeometryNewer_ = false;
    }
    // After a deforming call (refitMesh, refitAll, poseRig, rebuildDegraded) the root boxes and node offsets in buffers_ are
    // those of the undeformed geometry: a TLAS built from them would cull what has left the old boxes.  The device has the
    // current ones, so the step is forwarded to it (byte-identical to the host builder on equal inputs).
    void updateDynamicBVHAndSSBOs(const Scene& scene) {
        if (deviceGeometryNewer_) { updateDynamicBVHAndSSBOsOnDevice(scene); return; }
        buffers_.updateDynamic(scene);
        // the TLAS keeps its node count (2*I-1) and index count (I) for a fixed instance count
        upd(RZ_BIND_INSTANCES, buffers_.meshInstances);
        upd(RZ_BIND_TLAS_NODES, buffers_.tlasNodes);
        upd(RZ_BIND_TLAS_INDICES, buffers_.tlasTriIndices);
    }
    // The same per-frame step with the work done on the GPU: only the transforms (64 B per object) are handed over;
    // inverse, world AABBs and the TLAS rebuild run in the library (rz_update_transforms).
    void updateDynamicBVHAndSSBOsOnDevice(const Scene& scene) {
        std::vector<float> xf(scene.gameObjects.size() * 16);
        for (size_t i = 0; i < scene.gameObjects.size(); ++i) std::memcpy(&xf[i * 16], scene.gameObjects[i].transform.m, 64);
        check(rz_update_transforms(ctx_, xf.data(), scene.gameObjects.size()), "rz_update_transforms");
    }
    // Deforming meshes (rz_refit_geometry; the reference has no counterpart): `triangles` replace binding 0 from element
    // firstTriangle on, every mesh they touch is refitted on the device and the TLAS follows with the transforms in force.
    // refitAll: every mesh from binding 0 as it stands (after an rz_update of binding 0).  The host copies in buffers_
    // are NOT updated (rz_read_binding returns the refitted arrays); a later updateDynamicBVHAndSSBOs therefore takes the
    // device route, like updateDynamicBVHAndSSBOsOnDevice, and keeps the refitted boxes.
    void refitMesh(size_t firstTriangle, const std::vector<Triangle>& triangles) {
        deviceGeometryNewer_ = true;
        check(rz_refit_geometry(ctx_, reinterpret_cast<const rz_triangle*>(triangles.data()), firstTriangle, triangles.size(), RZ_REFIT_HOST),
              "rz_refit_geometry");
    }
    void refitAll() { deviceGeometryNewer_ = true; check(rz_refit_geometry(ctx_, nullptr, 0, 0, 0), "rz_refit_geometry"); }
    // Skinned meshes (rz_skin_create / rz_skin_pose; the reference has no counterpart): a rig keeps the rest pose of the
    // triangles [firstTriangle, +rest.size()) of binding 0 on the device with their bone indices / weights (skin, one per
    // triangle; empty: a morph-only rig) and morph targets (target-major, morphs.size() / rest.size() of them).  poseRig
    // skins on the device and refits what moved, TLAS included; nothing but the bones (64 B each) and the morph weights
    // crosses to the device per frame.  As with refitMesh the host copies in buffers_ are NOT updated and a later
    // updateDynamicBVHAndSSBOs takes the device route.  skin holds rest.size() records or none, morphs a whole number of
    // targets of rest.size() records each: anything else throws before the library is given a pointer it would read past.
    int createRig(size_t firstTriangle, const std::vector<Triangle>& rest, const std::vector<rz_skin_triangle>& skin, int nBones,
                  const std::vector<rz_morph_triangle>& morphs = {}) {
        int rig = -1;
        const size_t n = rest.size();
        if (!skin.empty() && skin.size() != n)
            throw std::runtime_error("createRig: skin holds " + std::to_string(skin.size()) + " records for " + std::to_string(n) + " rest triangles");
        if (!morphs.empty() && (n == 0 || morphs.size() % n != 0))
            throw std::runtime_error("createRig: morphs holds " + std::to_string(morphs.size()) + " records, not a multiple of the " +
                                     std::to_string(n) + " rest triangles");
        check(rz_skin_create(ctx_, firstTriangle, n, reinterpret_cast<const rz_triangle*>(rest.data()), skin.empty() ? nullptr : skin.data(),
                             nBones, morphs.empty() ? nullptr : morphs.data(), n ? (int)(morphs.size() / n) : 0, &rig),
              "rz_skin_create");
        return rig;
    }
    void poseRig(int rig, const std::vector<mat4>& bones, const std::vector<float>& morphWeights = {}) {
        deviceGeometryNewer_ = true;
        check(rz_skin_pose(ctx_, rig, bones.empty() ? nullptr : bones[0].m, morphWeights.empty() ? nullptr : morphWeights.data(), 0),
              "rz_skin_pose");
    }
    void destroyRig(int rig) { check(rz_skin_destroy(ctx_, rig), "rz_skin_destroy"); }
    // How far refits have degraded each mesh's tree (rz_geometry_quality): one record per mesh with its SAH cost as it stands
    // and the cost it had when it was last handed over or built.  Measured on the device; synchronises.
    std::vector<rz_mesh_quality> meshQuality() {
        size_t n = 0;
        check(rz_geometry_quality(ctx_, nullptr, 0, &n), "rz_geometry_quality");
        std::vector<rz_mesh_quality> out(n);
        check(rz_geometry_quality(ctx_, out.data(), out.size(), &n), "rz_geometry_quality");
        out.resize(n);
        return out;
    }
    // The exit from the refit's steady state (rz_rebuild_geometry): every mesh whose cost exceeds maxRatio times the cost it
    // was built with is rebuilt on the device from binding 0 as it stands there (posed triangles never visit the host);
    // instances and TLAS follow.  Returns the records; RZ_QUALITY_REBUILT marks what was rebuilt.  As with refitMesh the
    // host copies in buffers_ are NOT updated (SceneBuffers::rebuildMesh is the host partner): their blasNodeOffset values
    // are those from before later meshes moved, so a later updateDynamicBVHAndSSBOs takes the device route.
    std::vector<rz_mesh_quality> rebuildDegraded(double maxRatio) {
        deviceGeometryNewer_ = true;
        size_t n = 0;
        check(rz_geometry_quality(ctx_, nullptr, 0, &n), "rz_geometry_quality");
        std::vector<rz_mesh_quality> out(n);
        check(rz_rebuild_geometry(ctx_, maxRatio, out.data(), out.size(), &n, 0), "rz_rebuild_geometry");
        out.resize(n);
        return out;
    }
    void sendSceneDataToShader(const Scene& scene, int width, int height, int bounceBudget, int spp = 1,
                               int sampleBase = 0, int tileRank = 0, int tileNRanks = 1) {
        rz_frame_params p{};
        p.width = width; p.height = height;
        mat4 iv = inverse(scene.camera.viewMatrix), ip = inverse(scene.camera.projectionMatrix);
        std::memcpy(p.inv_view, iv.m, 64); std::memcpy(p.inv_proj, ip.m, 64);
        std::memcpy(p.view, scene.camera.viewMatrix.m, 64); std::memcpy(p.proj, scene.camera.projectionMatrix.m, 64);
        p.cam_pos[0] = scene.camera.position.x; p.cam_pos[1] = scene.camera.position.y; p.cam_pos[2] = scene.camera.position.z;
        p.num_lights = (int)scene.lights.size();
        p.bounce_budget = bounceBudget; p.spp = spp; p.sample_base = sampleBase;
        p.tile_rank = tileRank; p.tile_nranks = tileNRanks;
        check(rz_set_frame(ctx_, &p), "rz_set_frame");
        width_ = width; height_ = height;
    }
    void draw() { check(rz_render(ctx_), "rz_render"); }
    void finish() { check(rz_sync(ctx_), "rz_sync"); }
    std::vector<float> readAccum() {
        std::vector<float> out((size_t)width_ * height_ * 4);
        check(rz_read_accum(ctx_, out.data(), out.size() * sizeof(float)), "rz_read_accum");
        return out;
    }
    std::vector<uint8_t> resolveRGBA8() {
        std::vector<uint8_t> out((size_t)width_ * height_ * 4);
        check(rz_resolve_rgba8(ctx_, out.data(), out.size()), "rz_resolve_rgba8");
        return out;
    }
    // Batched ray queries on the uploaded scene (rz_trace_rays / rz_shadow_rays), host memory: return when the results are written.
    std::vector<rz_hit> traceRays(const std::vector<rz_ray>& rays, bool incoherent = false) {
        std::vector<rz_hit> hits(rays.size());
        check(rz_trace_rays(ctx_, rays.data(), hits.data(), rays.size(), RZ_RAYS_HOST | (incoherent ? RZ_RAYS_INCOHERENT : 0u)), "rz_trace_rays");
        return hits;
    }
    std::vector<rz_visibility> shadowRays(const std::vector<rz_ray>& rays, bool incoherent = false) {
        std::vector<rz_visibility> out(rays.size());
        check(rz_shadow_rays(ctx_, rays.data(), out.data(), rays.size(), RZ_RAYS_HOST | (incoherent ? RZ_RAYS_INCOHERENT : 0u)), "rz_shadow_rays");
        return out;
    }
    // The picking ray of main.cpp:505-513 (cursor -> NDC -> inverse projection -> eye direction -> inverse view), for a
    // screen of width x height pixels.
    static rz_ray pickRay(double mouseX, double mouseY, int width, int height, const Camera& camera) {
        const float ndcX = 2.0f * float(mouseX) / float(width) - 1.0f;
        const float ndcY = 1.0f - 2.0f * float(mouseY) / float(height);
        vec4 rayEye = inverse(camera.projectionMatrix) * vec4{ndcX, ndcY, -1.0f, 1.0f};
        rayEye = vec4{rayEye.x, rayEye.y, -1.0f, 0.0f};
        const vec4 w = inverse(camera.viewMatrix) * rayEye;
        const vec3 dir = normalize(vec3{w.x, w.y, w.z});
        rz_ray r{};
        r.origin[0] = camera.position.x; r.origin[1] = camera.position.y; r.origin[2] = camera.position.z;
        r.max_dist = 1e30f;
        r.dir[0] = dir.x; r.dir[1] = dir.y; r.dir[2] = dir.z;
        return r;
    }
    // main.cpp:501-552 as one closest-hit query: (instance, mesh-local triangle) under the cursor -- the values
    // rz_present_params.selected_blas / selected_tri take -- or nothing on a miss (the reference then keeps its previous
    // selection: main.cpp:548).  The screen is the frame of the last sendSceneDataToShader.  World distances decide, not the
    // reference's object-local t; |a| < 1e-4 rejects as in the shader; empty BLAS are never hit ("Picking").
    // Before the first sendSceneDataToShader there is no screen to place the cursor on: that throws.
    std::optional<std::pair<int, int>> pick(double mouseX, double mouseY, const Scene& scene) {
        if (width_ <= 0 || height_ <= 0) throw std::runtime_error("pick: no frame has been set (sendSceneDataToShader comes first)");
        const std::vector<rz_ray> ray{pickRay(mouseX, mouseY, width_, height_, scene.camera)};
        const rz_hit h = traceRays(ray)[0];
        if (h.instance < 0) return std::nullopt;
        return std::make_pair(h.instance, h.triangle);
    }
    // Editor mode (F1): renderRasterized (main.cpp:1281-1310) as one rz_render_editor call on the uploaded scene, with the
    // uniforms of sendRasterSceneData (main.cpp:1266-1275): the camera's view, projection and position, numLights =
    // scene.lights.size(), ambient 0.03, clear colour (0.05, 0.05, 0.07, 1).  Returns width x height RGBA8, row 0 = the bottom
    // row (as resolveRGBA8); host memory, returns when written.  Needs no sendSceneDataToShader and leaves its frame alone.
    std::vector<uint8_t> renderEditor(const Scene& scene, int width, int height, bool incoherent = false) {
        rz_frame_params p{};
        p.width = width; p.height = height;
        mat4 iv = inverse(scene.camera.viewMatrix), ip = inverse(scene.camera.projectionMatrix);
        std::memcpy(p.inv_view, iv.m, 64); std::memcpy(p.inv_proj, ip.m, 64);
        std::memcpy(p.view, scene.camera.viewMatrix.m, 64); std::memcpy(p.proj, scene.camera.projectionMatrix.m, 64);
        p.cam_pos[0] = scene.camera.position.x; p.cam_pos[1] = scene.camera.position.y; p.cam_pos[2] = scene.camera.position.z;
        p.num_lights = (int)scene.lights.size();
        std::vector<uint8_t> out((size_t)std::max(width, 0) * (size_t)std::max(height, 0) * 4);    // (a bad size: rz_render_editor says so)
        check(rz_render_editor(ctx_, &p, nullptr, out.data(), out.size(), nullptr, 0, nullptr, 0,
                               RZ_EDITOR_HOST | (incoherent ? RZ_EDITOR_INCOHERENT : 0u)), "rz_render_editor");
        return out;
    }
    // The denoised linear colour of the last frame set (width x height x 3 floats, row 0 = bottom, unclamped); params NULL =
    // the library's defaults.
    std::vector<float> denoise(const rz_denoise_params* params = nullptr) {
        std::vector<float> out((size_t)width_ * (size_t)height_ * 3);
        check(rz_denoise(ctx_, params, nullptr, 0, out.data(), out.size() * sizeof(float), nullptr, 0, RZ_DENOISE_HOST), "rz_denoise");
        return out;
    }
    // rz_present with the denoised colour: RGBA8 (width x height x 4, row 0 = bottom) with the overlays drawn on top.
    std::vector<uint8_t> presentDenoised(const rz_present_params& present, const rz_denoise_params* params = nullptr) {
        std::vector<uint8_t> out((size_t)width_ * (size_t)height_ * 4);
        check(rz_present_denoised(ctx_, &present, params, out.data(), out.size(), nullptr, 0), "rz_present_denoised");
        return out;
    }
    // Temporal accumulation by reprojection plus the variance-guided filter: blends the last frame set into the history the
    // context keeps and returns the colour (width x height x 3 floats, row 0 = bottom, unclamped).  keep: leave the history
    // as it was.  Call once per frame, after draw().
    std::vector<float> denoiseTemporal(const rz_temporal_params* params = nullptr, bool keep = false) {
        std::vector<float> out((size_t)width_ * (size_t)height_ * 3);
        check(rz_denoise_temporal(ctx_, params, nullptr, 0, out.data(), out.size() * sizeof(float), nullptr, 0, nullptr, 0,
                                  RZ_TEMPORAL_HOST | (keep ? RZ_TEMPORAL_KEEP : 0u)), "rz_denoise_temporal");
        return out;
    }
    // rz_present with that colour: RGBA8 (width x height x 4, row 0 = bottom), overlays on top; advances the history.
    std::vector<uint8_t> presentTemporal(const rz_present_params& present, const rz_temporal_params* params = nullptr) {
        std::vector<uint8_t> out((size_t)width_ * (size_t)height_ * 4);
        check(rz_present_temporal(ctx_, &present, params, out.data(), out.size(), nullptr, 0), "rz_present_temporal");
        return out;
    }
    // Drops the history (a cut: the next frame starts every pixel anew).
    void resetTemporal() { check(rz_temporal_reset(ctx_), "rz_temporal_reset"); }
    // present() behind the display stage: exposure (manual, or metered from the frame and adapted from call to call), tone
    // curve, transfer.  source 0: the accumulation; 1: rz_denoise's output (filter: an rz_denoise_params* or null); 2:
    // rz_denoise_temporal's (an rz_temporal_params* or null; the history advances).  display null: present()'s bytes.
    // antialias non-null: rz_present_antialiased, which averages factor x factor sub-pixel reconstructions on the pixels that
    // have a geometric edge, between the source and the display stage (factor 1: the bytes without it); null: rz_present_display.
    // seeThrough non-null: rz_present_antialiased_seethrough, the same pass on guides that follow glass and perfect mirrors for
    // at most max_depth steps, so that edges seen through them are smoothed too (antialias null: its defaults).
    std::vector<uint8_t> presentDisplay(const rz_present_params& present, const rz_display_params* display = nullptr, int source = 0,
                                        const void* filter = nullptr, const rz_antialias_params* antialias = nullptr,
                                        const rz_seethrough_params* seeThrough = nullptr) {
        std::vector<uint8_t> out((size_t)width_ * (size_t)height_ * 4);
        if (seeThrough) {
            if (&rz_present_antialiased_seethrough == nullptr)
                throw std::runtime_error("rz_present_antialiased_seethrough: the linked library does not have it");
            check(rz_present_antialiased_seethrough(ctx_, &present, antialias, seeThrough, display, source, filter, out.data(), out.size(),
                                                    nullptr, 0),
                  "rz_present_antialiased_seethrough");
        } else if (antialias) {
            if (&rz_present_antialiased == nullptr) throw std::runtime_error("rz_present_antialiased: the linked library does not have it");
            check(rz_present_antialiased(ctx_, &present, antialias, display, source, filter, out.data(), out.size(), nullptr, 0),
                  "rz_present_antialiased");
        } else
            check(rz_present_display(ctx_, &present, display, source, filter, out.data(), out.size(), nullptr, 0), "rz_present_display");
        return out;
    }
    // presentDisplay() at display size for a frame rendered below it: the frame last set is the LOW one (width x height), the
    // result is RGBA8 of factor * width x factor * height (row 0 = bottom), reconstructed from a G-buffer cast at that size, with
    // the overlays drawn there.  upscale null: factor 2 and rz_denoise's sigmas; factor 1: presentDisplay()'s bytes.
    // seeThrough non-null: rz_present_upscaled_seethrough, whose guides follow glass and perfect mirrors for at most
    // seeThrough->max_depth steps (0: the first-hit call's bytes); null: rz_present_upscaled.
    std::vector<uint8_t> presentUpscaled(const rz_present_params& present, const rz_upscale_params* upscale = nullptr,
                                         const rz_display_params* display = nullptr, int source = 0, const void* filter = nullptr,
                                         const rz_seethrough_params* seeThrough = nullptr) {
        const size_t s = upscale ? (size_t)std::max(upscale->factor, 0) : 2;
        std::vector<uint8_t> out((size_t)width_ * s * (size_t)height_ * s * 4);
        if (seeThrough) {
            if (&rz_present_upscaled_seethrough == nullptr) throw std::runtime_error("rz_present_upscaled_seethrough: the linked library does not have it");
            check(rz_present_upscaled_seethrough(ctx_, &present, upscale, seeThrough, display, source, filter, out.data(), out.size(), nullptr, 0),
                  "rz_present_upscaled_seethrough");
        } else
            check(rz_present_upscaled(ctx_, &present, upscale, display, source, filter, out.data(), out.size(), nullptr, 0), "rz_present_upscaled");
        return out;
    }
    // Drops the adapted exposure (a cut: the next metered call jumps to its target).
    void resetDisplay() { check(rz_display_reset(ctx_), "rz_display_reset"); }
    float lastRenderMs() { float ms = 0; int n = 0; check(rz_last_render_ms(ctx_, &ms, &n), "rz_last_render_ms"); return ms; }
    rz_ctx* context() { return ctx_; }
    // The geometry as it was last HANDED OVER (initializeSSBOs / initializeSSBOsOnDevice) with the transforms of the last
    // host-side update: deforming calls do not reach it.  rz_read_binding on context() returns what the device holds.
    const SceneBuffers& buffers() const { return buffers_; }

private:
    template <class T> void up(rz_binding b, const std::vector<T>& v) {
        check(rz_upload(ctx_, b, v.data(), v.size() * sizeof(T)), "rz_upload");
    }
    template <class T> void upd(rz_binding b, const std::vector<T>& v) {
        check(rz_update(ctx_, b, 0, v.data(), v.size() * sizeof(T)), "rz_update");
    }
    void check(int rc, const char* what) {
        if (rc != RZ_OK) throw std::runtime_error(std::string(what) + ": " + rz_last_error(ctx_));
    }
    rz_ctx* ctx_;
    SceneBuffers buffers_;
    int width_ = 0, height_ = 0;
    bool deviceGeometryNewer_ = false;      // a deforming call ran since the last hand-over: the device's geometry is newer than buffers_
};

// The same frontend glue for N GPUs of one node driven by ONE process: every device holds the whole scene, renders the
// 8x8-pixel tiles t with t % N == its rank, and one exchange step per frame (a gather of the members' tiles over RCCL) lands the image on rank 0 (rz_group_*).
// A frontend written against Renderer switches by changing the type.
class GroupRenderer {
public:
    explicit GroupRenderer(int ndev, const int* devices = nullptr, unsigned flags = RZ_FLAG_NONE)
        : g_(rz_group_create(ndev, devices, flags)) {
        if (!g_) throw std::runtime_error(std::string("rz_group_create: ") + rz_group_last_error(nullptr));
    }
    ~GroupRenderer() { rz_group_destroy(g_); }
    GroupRenderer(const GroupRenderer&) = delete;
    GroupRenderer& operator=(const GroupRenderer&) = delete;

    int size() const { return rz_group_size(g_); }
    void initializeSSBOs(const Scene& scene, bool shareMeshes = false) {
        if (!buffers_.build(scene, shareMeshes)) throw std::runtime_error("scene build failed");
        up(RZ_BIND_TRIANGLES, buffers_.allTriangles);
        up(RZ_BIND_MATERIALS, scene.materials);
        up(RZ_BIND_LIGHTS, scene.lights);
        up(RZ_BIND_TLAS_NODES, buffers_.tlasNodes);
        up(RZ_BIND_TLAS_INDICES, buffers_.tlasTriIndices);
        up(RZ_BIND_BLAS_NODES, buffers_.allBLASNodes);
        up(RZ_BIND_BLAS_INDICES, buffers_.allBLASTriIndices);
        up(RZ_BIND_INSTANCES, buffers_.meshInstances);
    }
    void updateDynamicBVHAndSSBOs(const Scene& scene) {
        buffers_.updateDynamic(scene);
        upd(RZ_BIND_INSTANCES, buffers_.meshInstances);
        upd(RZ_BIND_TLAS_NODES, buffers_.tlasNodes);
        upd(RZ_BIND_TLAS_INDICES, buffers_.tlasTriIndices);
    }
    void sendSceneDataToShader(const Scene& scene, int width, int height, int bounceBudget, int spp = 1, int sampleBase = 0) {
        rz_frame_params p{};
        p.width = width; p.height = height;
        mat4 iv = inverse(scene.camera.viewMatrix), ip = inverse(scene.camera.projectionMatrix);
        std::memcpy(p.inv_view, iv.m, 64); std::memcpy(p.inv_proj, ip.m, 64);
        std::memcpy(p.view, scene.camera.viewMatrix.m, 64); std::memcpy(p.proj, scene.camera.projectionMatrix.m, 64);
        p.cam_pos[0] = scene.camera.position.x; p.cam_pos[1] = scene.camera.position.y; p.cam_pos[2] = scene.camera.position.z;
        p.num_lights = (int)scene.lights.size();
        p.bounce_budget = bounceBudget; p.spp = spp; p.sample_base = sampleBase;
        p.tile_rank = 0; p.tile_nranks = 1;         // filled in per member by the group
        check(rz_group_set_frame(g_, &p), "rz_group_set_frame");
        width_ = width; height_ = height;
    }
    // glDrawArrays on every device, then the one collective, all asynchronous
    void draw() { check(rz_group_render(g_), "rz_group_render"); check(rz_group_reduce(g_, 0), "rz_group_reduce"); }
    void finish() { check(rz_group_sync(g_), "rz_group_sync"); }
    std::vector<float> readFrame() {
        std::vector<float> out((size_t)width_ * height_ * 4);
        check(rz_group_read_frame(g_, out.data(), out.size() * sizeof(float)), "rz_group_read_frame");
        return out;
    }
    rz_group* group() { return g_; }

private:
    template <class T> void up(rz_binding b, const std::vector<T>& v) {
        check(rz_group_upload(g_, b, v.data(), v.size() * sizeof(T)), "rz_group_upload");
    }
    template <class T> void upd(rz_binding b, const std::vector<T>& v) {
        check(rz_group_update(g_, b, 0, v.data(), v.size() * sizeof(T)), "rz_group_update");
    }
    void check(int rc, const char* what) {
        if (rc != RZ_OK) throw std::runtime_error(std::string(what) + ": " + rz_group_last_error(g_));
    }
    rz_group* g_;
    SceneBuffers buffers_;
    int width_ = 0, height_ = 0;
};

}  // namespace rayzen

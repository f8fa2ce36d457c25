// adaptive_driver.cpp -- a TEST program (tests/test_adaptive_gpu.py compiles and runs it): the free functions of
// rayzen_amd/csrc/host/Adaptive.h called on one small scene, with the scene's bindings, the frame and every output written as raw
// little-endian files, so that the Python binding can replay the same calls and compare bytes.
//
//   g++ -std=c++17 -O2 -Iinclude -Irayzen_amd/csrc/host tests/cpp/adaptive_driver.cpp
//       -Lrayzen_amd/lib -lrayzen_host -lrayzen_hip -Wl,-rpath,$PWD/rayzen_amd/lib -o adaptive_driver
//   ./adaptive_driver OUTDIR
//
// Files: b0, b1, b2, b5 .. b9 (rz_read_binding), frame (rz_frame_params), params (rz_adaptive_params), info (rz_adaptive_info
// with the two times zeroed), batches, error (per tile), accum (rz_read_accum), mask (active then current, one byte per tile) and
// plan (rz_tile_run) -- each OUTDIR/<name>.bin.  A std::exception is printed and ends the program with 1; nothing is retried.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "Adaptive.h"
#include "RayZenScene.h"
#include "Renderer.h"
#include "rayzen_host.h"

using namespace rayzen;

static void put(const std::string& dir, const std::string& name, const void* p, size_t bytes) {
    const std::string path = dir + "/" + name + ".bin";
    FILE* o = std::fopen(path.c_str(), "wb");
    if (!o) throw std::runtime_error("cannot write " + path);
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, o) == bytes;
    std::fclose(o);
    if (!ok) throw std::runtime_error("short write to " + path);
}
template <class T> static void put(const std::string& dir, const std::string& name, const std::vector<T>& v) {
    put(dir, name, v.data(), v.size() * sizeof(T));
}

static std::shared_ptr<Mesh> cubeMesh(int material) {
    auto m = std::make_shared<Mesh>();
    m->triangles.resize(12);
    rzh_make_cube(material, reinterpret_cast<rz_triangle*>(m->triangles.data()), 12);
    return m;
}
static std::shared_ptr<Mesh> blobMesh(int n, float radius, int material) {
    auto m = std::make_shared<Mesh>();
    m->triangles.resize((size_t)12 * n * n);
    rzh_make_blob(n, radius, 1u, material, reinterpret_cast<rz_triangle*>(m->triangles.data()), (int)m->triangles.size());
    return m;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: adaptive_driver OUTDIR\n"); return 2; }
    const std::string dir = argv[1];
    const int W = 37, H = 21, kBounces = 3, kSpp = 2;
    try {
        Scene scene;
        scene.camera = Camera(vec3(0.0f, 2.5f, 10.0f), vec3(0.0f, -0.1f, -1.0f), vec3(0.0f, 1.0f, 0.0f), 70.0f, float(W) / float(H), 0.1f, 100.0f);
        scene.materials = {Material(vec3(0.8f, 0.3f, 0.3f), 0.0f, 1.0f, 0.0f, 0.0f, 1.5f),
                           Material(vec3(0.85f, 0.95f, 1.0f), 0.0f, 0.02f, 0.05f, 0.94f, 1.5f),
                           Material(vec3(0.6f, 0.4f, 0.2f), 0.0f, 0.9f, 0.2f, 0.0f, 1.5f)};
        scene.lights.push_back(Light(vec4{5.0f, 5.0f, 5.0f, 1.0f}, vec3(1.0f), 300.0f));
        scene.lights.push_back(Light(vec4{0.8f, 1.4f, 0.3f, 0.0f}, vec3(1.0f), 2.0f));
        auto floor = cubeMesh(2), blob = blobMesh(6, 1.6f, 0), glass = blobMesh(4, 1.2f, 1);
        scene.gameObjects.push_back(GameObject{floor, translate(scale(mat4(1.0f), vec3(8.0f, 0.5f, 8.0f)), vec3(0.0f, -3.0f, 0.0f))});
        scene.gameObjects.push_back(GameObject{blob, translate(mat4(1.0f), vec3(-2.5f, 1.5f, 0.0f))});
        scene.gameObjects.push_back(GameObject{glass, translate(mat4(1.0f), vec3(0.5f, 0.8f, 4.0f))});

        Renderer r(0);
        r.initializeSSBOs(scene, true);
        r.sendSceneDataToShader(scene, W, H, kBounces, kSpp);
        for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS, RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES,
                      RZ_BIND_BLAS_NODES, RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES}) {
            size_t need = 0;
            if (rz_read_binding(r.context(), (rz_binding)b, nullptr, 0, &need) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
            std::vector<uint8_t> buf(need);
            if (rz_read_binding(r.context(), (rz_binding)b, buf.data(), buf.size(), &need) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
            put(dir, "b" + std::to_string(b), buf);
        }
        // what sendSceneDataToShader handed to rz_set_frame, stated again so that the replay can set the same frame
        rz_frame_params p{};
        p.width = W; p.height = H;
        const mat4 iv = inverse(scene.camera.viewMatrix), ip = inverse(scene.camera.projectionMatrix);
        std::memcpy(p.inv_view, iv.m, 64); std::memcpy(p.inv_proj, ip.m, 64);
        std::memcpy(p.view, scene.camera.viewMatrix.m, 64); std::memcpy(p.proj, scene.camera.projectionMatrix.m, 64);
        p.cam_pos[0] = scene.camera.position.x; p.cam_pos[1] = scene.camera.position.y; p.cam_pos[2] = scene.camera.position.z;
        p.num_lights = (int)scene.lights.size();
        p.bounce_budget = kBounces; p.spp = kSpp; p.sample_base = 0;
        p.tile_rank = 0; p.tile_nranks = 1;
        put(dir, "frame", &p, sizeof p);

        rz_adaptive_params q = adaptiveParams();
        // (this scene's direct light is deterministic and its glass takes few pixels: E is 4e-5 .. 2e-3 after two batches, so the
        //  threshold sits at the rounding floor to make some tiles go on and others retire)
        q.batch_spp = 2; q.min_batches = 2; q.max_batches = 5; q.threshold = 0.0005f; q.merge_gap = 1; q.max_runs = 8;
        put(dir, "params", &q, sizeof q);
        AdaptiveResult res = renderAdaptive(r, W, H, q);
        res.info.render_ms = res.info.meter_ms = 0.0f;
        put(dir, "info", &res.info, sizeof res.info);
        put(dir, "batches", res.tileBatches);
        put(dir, "error", res.tileError);
        std::vector<float> accum((size_t)W * H * 4);
        if (rz_read_accum(r.context(), accum.data(), accum.size() * sizeof(float)) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
        put(dir, "accum", accum);
        std::vector<uint8_t> active(40, 0), current(40, 1);
        for (int t : {0, 1, 5, 6, 20, 21, 39}) active[t] = 1;
        current[3] = 0;
        std::vector<uint8_t> mask(active);
        mask.insert(mask.end(), current.begin(), current.end());
        put(dir, "mask", mask);
        put(dir, "plan", adaptivePlan(active, current, 4, 3));
        r.finish();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "adaptive_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}

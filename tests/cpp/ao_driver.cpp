// ao_driver.cpp -- a TEST program (tests/test_ao_gpu.py compiles and runs it): the free functions of
// rayzen_amd/csrc/host/AmbientOcclusion.h called on one small scene, with the scene's bindings, the frame and every input and
// output written as raw little-endian files, so that the Python binding can replay the same calls and compare bytes.
//
//   g++ -std=c++17 -O2 -Iinclude -Irayzen_amd/csrc/host tests/cpp/ao_driver.cpp
//       -Lrayzen_amd/lib -lrayzen_host -lrayzen_hip -Wl,-rpath,$PWD/rayzen_amd/lib -o ao_driver
//   ./ao_driver OUTDIR
//
// Files: b0, b1, b2, b5 .. b9 (rz_read_binding), frame (rz_frame_params), dirs (the direction table), in32 (the image that is
// darkened), ao, rgb32f, rgba8 (the defaults on in32), raw8 (ao of N = 8, radius 3, smooth = 0), white (rgb32f of a NULL input at
// strength 0.5) -- each OUTDIR/<name>.bin.  A std::exception is printed and ends the program with 1; nothing is retried.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "AmbientOcclusion.h"
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
    if (argc < 2) { std::fprintf(stderr, "usage: ao_driver OUTDIR\n"); return 2; }
    const std::string dir = argv[1];
    const int W = 37, H = 21;
    try {
        Scene scene;
        scene.camera = Camera(vec3(0.0f, 2.5f, 10.0f), vec3(0.0f, -0.1f, -1.0f), vec3(0.0f, 1.0f, 0.0f), 70.0f, float(W) / float(H), 0.1f, 100.0f);
        scene.materials = {Material(vec3(0.8f, 0.3f, 0.3f), 0.0f, 1.0f, 0.0f, 0.0f, 1.5f),
                           Material(vec3(0.85f, 0.95f, 1.0f), 0.0f, 0.02f, 0.05f, 0.94f, 1.5f),
                           Material(vec3(0.6f, 0.4f, 0.2f), 0.0f, 0.9f, 0.2f, 0.0f, 1.5f)};
        scene.lights.push_back(Light(vec4{5.0f, 5.0f, 5.0f, 1.0f}, vec3(1.0f), 300.0f));
        auto floor = cubeMesh(2), blob = blobMesh(6, 1.6f, 0), glass = blobMesh(4, 1.2f, 1);
        scene.gameObjects.push_back(GameObject{floor, translate(scale(mat4(1.0f), vec3(8.0f, 0.5f, 8.0f)), vec3(0.0f, -3.0f, 0.0f))});
        scene.gameObjects.push_back(GameObject{blob, translate(mat4(1.0f), vec3(-2.5f, 0.6f, 0.0f))});      // (it rests on the floor)
        scene.gameObjects.push_back(GameObject{glass, translate(mat4(1.0f), vec3(0.5f, 0.3f, 4.0f))});
        scene.gameObjects.push_back(GameObject{blob, translate(mat4(1.0f), vec3(3.0f, 2.0f, -1.0f))});

        Renderer r(0);
        r.initializeSSBOs(scene, true);
        for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS, RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES,
                      RZ_BIND_BLAS_NODES, RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES}) {
            size_t need = 0;
            if (rz_read_binding(r.context(), (rz_binding)b, nullptr, 0, &need) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
            std::vector<uint8_t> buf(need);
            if (rz_read_binding(r.context(), (rz_binding)b, buf.data(), buf.size(), &need) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
            put(dir, "b" + std::to_string(b), buf);
        }
        // the frame the call casts through: no rz_set_frame is needed
        rz_frame_params p{};
        p.width = W; p.height = H;
        const mat4 iv = inverse(scene.camera.viewMatrix), ip = inverse(scene.camera.projectionMatrix);
        std::memcpy(p.inv_view, iv.m, 64); std::memcpy(p.inv_proj, ip.m, 64);
        std::memcpy(p.view, scene.camera.viewMatrix.m, 64); std::memcpy(p.proj, scene.camera.projectionMatrix.m, 64);
        p.cam_pos[0] = scene.camera.position.x; p.cam_pos[1] = scene.camera.position.y; p.cam_pos[2] = scene.camera.position.z;
        p.num_lights = (int)scene.lights.size();
        p.bounce_budget = 1; p.spp = 1; p.sample_base = 0;
        p.tile_rank = 0; p.tile_nranks = 1;
        put(dir, "frame", &p, sizeof p);

        put(dir, "dirs", aoDirections());
        std::vector<float> img32((size_t)W * H * 3);
        for (size_t i = 0; i < img32.size(); ++i) img32[i] = (float)(i % 97) / 64.0f;
        put(dir, "in32", img32);
        const AmbientOcclusionImages all = ambientOcclusion(r, p, aoParams(), &img32, AO_WANT_AO | AO_WANT_RGB32F | AO_WANT_RGBA8);
        put(dir, "ao", all.ao);
        put(dir, "rgb32f", all.rgb32f);
        put(dir, "rgba8", all.rgba8);
        rz_ao_params q = aoParams();
        q.samples = 8; q.radius = 3.0f; q.smooth = 0;
        put(dir, "raw8", ambientOcclusion(r, p, q).ao);
        q = aoParams();
        q.strength = 0.5f;
        put(dir, "white", ambientOcclusion(r, p, q, nullptr, AO_WANT_RGB32F).rgb32f);
        r.finish();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ao_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}

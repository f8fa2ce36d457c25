// bloom_driver OUTDIR -- the free functions of Bloom.h on one small scene.  Writes the bindings, the frame record and the
// results as raw files into OUTDIR; tests/test_bloom_gpu.py replays the same calls through the Python binding and compares every
// byte.
//   b<k>.bin       the eight bindings as the library holds them
//   fp.bin         the rz_frame_params of the frame
//   out.bin        bloom(r, W, H): the accumulation with glare, the defaults       glare.bin   its glare alone
//   out2.bin       bloom(r, W, H, &out, &wide): `wide` on out.bin's floats
//   plain.bin      presentDisplay(present, &aces)                                   (rz_present_display)
//   zero.bin       presentBloomed(..., &aces, &{intensity 0}): plain.bin's bytes
//   bloomed.bin    presentBloomed(..., &aces): the defaults                         bloomed32.bin   its rgb32f
//   denoised.bin   presentBloomed(..., &aces, &wide, 1, &dn): behind rz_denoise, two passes
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Bloom.h"
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
    if (argc != 2) { std::fprintf(stderr, "usage: bloom_driver OUTDIR\n"); return 2; }
    const std::string dir = argv[1];
    try {
        const int W = 72, H = 40, bounces = 3, spp = 2;
        Scene scene;
        scene.camera = Camera(vec3(0.0f, 2.5f, 10.0f), vec3(0.0f, -0.1f, -1.0f), vec3(0.0f, 1.0f, 0.0f), 70.0f, float(W) / float(H), 0.1f, 100.0f);
        scene.materials = {Material(vec3(0.8f, 0.3f, 0.3f), 0.0f, 1.0f, 0.0f, 0.0f, 1.5f),
                           Material(vec3(0.1f, 0.7f, 0.1f), 1.0f, 0.35f, 0.3f, 0.0f, 1.5f),
                           Material(vec3(0.6f, 0.4f, 0.2f), 0.0f, 0.9f, 0.2f, 0.0f, 1.5f)};
        scene.lights.push_back(Light(vec4{5.0f, 5.0f, 5.0f, 1.0f}, vec3(1.0f), 300.0f));
        scene.lights.push_back(Light(vec4{0.8f, 1.4f, 0.3f, 0.0f}, vec3(1.0f), 2.0f));
        auto floor = cubeMesh(2), blob = blobMesh(6, 1.6f, 0), cube = cubeMesh(1);
        scene.gameObjects.push_back(GameObject{floor, translate(scale(mat4(1.0f), vec3(8.0f, 0.5f, 8.0f)), vec3(0.0f, -3.0f, 0.0f))});
        scene.gameObjects.push_back(GameObject{blob, translate(mat4(1.0f), vec3(-2.5f, 1.5f, 0.0f))});
        scene.gameObjects.push_back(GameObject{cube, rotate(translate(mat4(1.0f), vec3(3.0f, 0.5f, 2.0f)), 0.5f, vec3(0.0f, 1.0f, 0.0f))});

        Renderer r(0);
        r.initializeSSBOs(scene, true);
        r.sendSceneDataToShader(scene, W, H, bounces, spp, 0);
        r.draw();
        r.finish();
        for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS, RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES,
                      RZ_BIND_BLAS_NODES, RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES}) {
            size_t need = 0;
            if (rz_read_binding(r.context(), (rz_binding)b, nullptr, 0, &need) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
            std::vector<uint8_t> buf(need);
            if (rz_read_binding(r.context(), (rz_binding)b, buf.data(), buf.size(), &need) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
            put(dir, "b" + std::to_string(b), buf.data(), buf.size());
        }
        rz_frame_params p{};
        p.width = W; p.height = H;
        const mat4 iv = inverse(scene.camera.viewMatrix), ip = inverse(scene.camera.projectionMatrix);
        std::memcpy(p.inv_view, iv.m, 64); std::memcpy(p.inv_proj, ip.m, 64);
        std::memcpy(p.view, scene.camera.viewMatrix.m, 64); std::memcpy(p.proj, scene.camera.projectionMatrix.m, 64);
        p.cam_pos[0] = scene.camera.position.x; p.cam_pos[1] = scene.camera.position.y; p.cam_pos[2] = scene.camera.position.z;
        p.num_lights = (int)scene.lights.size();
        p.bounce_budget = bounces; p.spp = spp; p.sample_base = 0; p.tile_rank = 0; p.tile_nranks = 1;
        put(dir, "fp", &p, sizeof p);

        const rz_present_params pp = {0.0f, 0, 0, 0, 0, 0, 0};
        const rz_bloom_params wide = {0.5f, 0.25f, 8.0f, 0.5f, 2.0f, 3, {0, 0}}, zero = {1.0f, 0.5f, 64.0f, 0.0f, 1.0f, 6, {0, 0}};
        const rz_denoise_params dn = {2, 0.5f, 128.0f, 1.0f, 1, {0, 0, 0}};
        const rz_display_params aces = {0, 1.5f, 0.18f, 1.0f / 64.0f, 64.0f, 1.0f, 0, 0, 2, 4.0f, 1, {0, 0, 0, 0, 0}};
        std::vector<float> glare;
        const std::vector<float> out = bloom(r, W, H, nullptr, nullptr, &glare);
        put(dir, "out", out.data(), out.size() * sizeof(float));
        put(dir, "glare", glare.data(), glare.size() * sizeof(float));
        const std::vector<float> out2 = bloom(r, W, H, &out, &wide);
        put(dir, "out2", out2.data(), out2.size() * sizeof(float));
        std::vector<uint8_t> px = r.presentDisplay(pp, &aces);
        put(dir, "plain", px.data(), px.size());
        px = presentBloomed(r, W, H, pp, &aces, &zero);
        put(dir, "zero", px.data(), px.size());
        std::vector<float> rgb32f;
        px = presentBloomed(r, W, H, pp, &aces, nullptr, 0, nullptr, &rgb32f);
        put(dir, "bloomed", px.data(), px.size());
        put(dir, "bloomed32", rgb32f.data(), rgb32f.size() * sizeof(float));
        px = presentBloomed(r, W, H, pp, &aces, &wide, 1, &dn);
        put(dir, "denoised", px.data(), px.size());
        // a spread out of range is the library's error, raised as the front end raises every error
        const rz_bloom_params bad = {1.0f, 0.5f, 64.0f, 0.25f, 4.5f, 6, {0, 0}};
        bool threw = false;
        try { bloom(r, W, H, nullptr, &bad); } catch (const std::exception&) { threw = true; }
        if (!threw) throw std::runtime_error("spread 4.5 was accepted");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "bloom_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}

// render_editor.cpp -- RayZen's editor mode (F1) without OpenGL: the scene of examples/render_scene.cpp drawn by
// Renderer::renderEditor, which replaces renderRasterized, buildRasterMeshes, cleanupRasterMeshes and the raster shader
// program of main.cpp:1210-1322 with one rz_render_editor call ("Editor mode").
//
//   g++ -std=c++17 -O2 -Iinclude -Irayzen_amd/csrc/host examples/render_editor.cpp
//       -Lrayzen_amd/lib -lrayzen_host -lrayzen_hip -Wl,-rpath,$PWD/rayzen_amd/lib -o render_editor
//   ./render_editor outdir [width height]
//
// Writes into outdir: editor.ppm (the frame), editor.rgba (its raw RGBA8, row 0 = the bottom row), binding<N>.bin (the eight
// arrays the library holds, rz_read_binding) and frame.f32 (inv_view, inv_proj, view, proj, cam_pos, num_lights as floats):
// everything another binding needs to render the same frame (tests/test_editor_gpu.py does, from Python).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "RayZenScene.h"
#include "Renderer.h"
#include "rayzen_host.h"

using namespace rayzen;

static bool writeFile(const std::string& path, const void* data, size_t bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::perror(path.c_str()); return false; }
    const bool ok = std::fwrite(data, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
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
    const std::string dir = argc > 1 ? argv[1] : ".";
    const int W = argc > 2 ? std::atoi(argv[2]) : 800, H = argc > 3 ? std::atoi(argv[3]) : 600;

    Scene scene;
    scene.camera = Camera(vec3(0.0f, 2.5f, 10.0f), vec3(0.0f, 0.0f, -1.0f), vec3(0.0f, 1.0f, 0.0f), 70.0f,
                          float(W) / float(H), 0.1f, 100.0f);
    scene.materials = {Material(vec3(0.8f, 0.3f, 0.3f), 0.0f, 1.0f, 0.0f, 0.0f, 1.5f),     // main.cpp:342-353
                       Material(vec3(0.1f, 0.7f, 0.1f), 1.0f, 0.35f, 0.3f, 0.0f, 1.5f),
                       Material(vec3(1.0f), 1.0f, 0.05f, 1.0f, 0.0f, 1.5f),
                       Material(vec3(0.85f, 0.95f, 1.0f), 0.0f, 0.02f, 0.05f, 0.94f, 1.5f),
                       Material(vec3(0.6f, 0.4f, 0.2f), 0.0f, 0.9f, 0.2f, 0.0f, 1.5f)};
    scene.lights.push_back(Light(vec4{5.0f, 5.0f, 5.0f, 1.0f}, vec3(1.0f), 300.0f));     // main.cpp:356-357
    scene.lights.push_back(Light(vec4{0.8f, 1.4f, 0.3f, 0.0f}, vec3(1.0f), 2.0f));
    auto floor = cubeMesh(4), bunny = blobMesh(40, 2.8f, 0), glass = blobMesh(12, 1.2f, 3);
    scene.gameObjects.push_back(GameObject{floor, translate(scale(mat4(1.0f), vec3(8.0f, 0.5f, 8.0f)), vec3(0.0f, -3.0f, 0.0f))});
    scene.gameObjects.push_back(GameObject{bunny, translate(mat4(1.0f), vec3(0.0f, 2.0f, 0.0f))});
    scene.gameObjects.push_back(GameObject{glass, translate(mat4(1.0f), vec3(4.5f, 0.6f, 3.0f))});

    try {
        Renderer renderer(0);
        renderer.initializeSSBOs(scene, /*shareMeshes=*/true);            // main.cpp:388
        const std::vector<uint8_t> px = renderer.renderEditor(scene, W, H);   // main.cpp:1320: renderRasterized(scene)

        if (!writeFile(dir + "/editor.rgba", px.data(), px.size())) return 1;
        FILE* f = std::fopen((dir + "/editor.ppm").c_str(), "wb");
        if (!f) { std::perror("editor.ppm"); return 1; }
        std::fprintf(f, "P6\n%d %d\n255\n", W, H);
        for (int y = H - 1; y >= 0; --y)                                   // row 0 is the bottom row
            for (int x = 0; x < W; ++x) std::fwrite(&px[((size_t)y * W + x) * 4], 1, 3, f);
        std::fclose(f);
        for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS, RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES,
                      RZ_BIND_BLAS_NODES, RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES}) {
            size_t need = 0;
            if (rz_read_binding(renderer.context(), (rz_binding)b, nullptr, 0, &need) != RZ_OK) throw std::runtime_error(rz_last_error(renderer.context()));
            std::vector<uint8_t> buf(need);
            if (rz_read_binding(renderer.context(), (rz_binding)b, buf.data(), buf.size(), &need) != RZ_OK) throw std::runtime_error(rz_last_error(renderer.context()));
            if (!writeFile(dir + "/binding" + std::to_string(b) + ".bin", buf.data(), buf.size())) return 1;
        }
        // the matrices renderEditor handed over (sendRasterSceneData's uniforms, main.cpp:1266-1275)
        const mat4 iv = inverse(scene.camera.viewMatrix), ip = inverse(scene.camera.projectionMatrix);
        std::vector<float> fr(68);
        std::memcpy(&fr[0], iv.m, 64); std::memcpy(&fr[16], ip.m, 64);
        std::memcpy(&fr[32], scene.camera.viewMatrix.m, 64); std::memcpy(&fr[48], scene.camera.projectionMatrix.m, 64);
        fr[64] = scene.camera.position.x; fr[65] = scene.camera.position.y; fr[66] = scene.camera.position.z;
        fr[67] = float(scene.lights.size());
        if (!writeFile(dir + "/frame.f32", fr.data(), fr.size() * sizeof(float))) return 1;
        std::printf("wrote %s/editor.ppm\n", dir.c_str());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

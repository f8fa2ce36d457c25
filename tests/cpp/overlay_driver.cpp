// overlay_driver.cpp -- a TEST program (tests/test_lines_gpu.py compiles and runs it): the free functions of
// rayzen_amd/csrc/host/Overlay.h called on one small scene, with the scene's bindings, the frame and every input and output
// written as raw little-endian files, so that the Python binding can replay the same calls and compare bytes.
//
//   g++ -std=c++17 -O2 -Iinclude -Irayzen_amd/csrc/host tests/cpp/overlay_driver.cpp
//       -Lrayzen_amd/lib -lrayzen_host -lrayzen_hip -Wl,-rpath,$PWD/rayzen_amd/lib -o overlay_driver
//   ./overlay_driver OUTDIR
//
// Files: b0, b1, b2, b5 .. b9 (rz_read_binding), frame (rz_frame_params), grid and box (what gridLines and boxLines returned),
// lines (everything drawn: grid, the box of instance 1 in its own space, a world-space box), hits (rz_render_editor's), params
// (rz_lines_params), in8, in32 (the images before), out8, out32 (after, with hits and params), plain8 (rgba8 alone, no hits,
// default params) -- each OUTDIR/<name>.bin.  A std::exception is printed and ends the program with 1; nothing is retried.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "Overlay.h"
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

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: overlay_driver OUTDIR\n"); return 2; }
    const std::string dir = argv[1];
    const int W = 45, H = 27;
    try {
        Scene scene;
        scene.camera = Camera(vec3(0.0f, 2.5f, 10.0f), vec3(0.0f, -0.1f, -1.0f), vec3(0.0f, 1.0f, 0.0f), 70.0f, float(W) / float(H), 0.1f, 100.0f);
        scene.materials = {Material(vec3(0.8f, 0.3f, 0.3f), 0.0f, 1.0f, 0.0f, 0.0f, 1.5f),
                           Material(vec3(0.6f, 0.4f, 0.2f), 0.0f, 0.9f, 0.2f, 0.0f, 1.5f)};
        scene.lights.push_back(Light(vec4{5.0f, 5.0f, 5.0f, 1.0f}, vec3(1.0f), 300.0f));
        auto floor = cubeMesh(1), cube = cubeMesh(0);
        scene.gameObjects.push_back(GameObject{floor, translate(scale(mat4(1.0f), vec3(8.0f, 0.5f, 8.0f)), vec3(0.0f, -3.0f, 0.0f))});
        scene.gameObjects.push_back(GameObject{cube, translate(scale(mat4(1.0f), vec3(2.0f, 3.0f, 2.0f)), vec3(-0.8f, 0.2f, 0.5f))});
        scene.gameObjects.push_back(GameObject{cube, translate(mat4(1.0f), vec3(3.0f, 2.0f, -1.0f))});

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

        std::vector<rz_hit> hits((size_t)W * H);
        if (rz_render_editor(r.context(), &p, nullptr, nullptr, 0, nullptr, 0, hits.data(), hits.size() * sizeof(rz_hit), RZ_EDITOR_HOST) != RZ_OK)
            throw std::runtime_error(rz_last_error(r.context()));
        put(dir, "hits", hits);

        const std::vector<rz_line> grid = gridLines(6.0f, 1.5f, lineColor(160, 160, 160, 200), -1.5f);
        const float lo[3] = {-0.5f, -0.5f, -0.5f}, hi[3] = {0.5f, 0.5f, 0.5f};
        const std::vector<rz_line> box = boxLines(lo, hi, lineColor(255, 160, 0, 255), 1);     // instance 1, in its own space
        const float wlo[3] = {2.0f, 1.0f, -2.0f}, whi[3] = {4.0f, 3.0f, 0.0f};
        const std::vector<rz_line> world = boxLines(wlo, whi, lineColor(0, 200, 255, 128));
        put(dir, "grid", grid);
        put(dir, "box", box);
        std::vector<rz_line> lines(grid);
        lines.insert(lines.end(), box.begin(), box.end());
        lines.insert(lines.end(), world.begin(), world.end());
        put(dir, "lines", lines);

        std::vector<uint8_t> img8((size_t)W * H * 4);
        std::vector<float> img32((size_t)W * H * 3);
        for (size_t i = 0; i < img8.size(); ++i) img8[i] = (uint8_t)((i * 7 + 3) & 255);
        for (size_t i = 0; i < img32.size(); ++i) img32[i] = (float)(i % 97) / 64.0f;
        put(dir, "in8", img8);
        put(dir, "in32", img32);
        std::vector<uint8_t> plain8(img8);
        drawLines(r, p, lines, nullptr, &plain8, nullptr);
        put(dir, "plain8", plain8);
        rz_lines_params lp{};
        lp.width = 2.0f; lp.near_w = 0.01f; lp.depth_bias = 0.01f; lp.hidden_alpha = 0.25f; lp.smooth = 1;
        put(dir, "params", &lp, sizeof lp);
        drawLines(r, p, lines, &hits, &img8, &img32, &lp);
        put(dir, "out8", img8);
        put(dir, "out32", img32);
        r.finish();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "overlay_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}

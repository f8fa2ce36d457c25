// frontend_driver.cpp -- a TEST program (tests/test_cpp_frontend_gpu.py compiles and runs it): every public method of
// rayzen::Renderer (rayzen_amd/csrc/host/Renderer.h) called on one small scene, with every input and every output written
// as raw little-endian files, so that another binding can replay the same calls and compare bytes.
//
//   g++ -std=c++17 -O2 -Iinclude -Irayzen_amd/csrc/host tests/cpp/frontend_driver.cpp
//       -Lrayzen_amd/lib -lrayzen_host -lrayzen_hip -Wl,-rpath,$PWD/rayzen_amd/lib -o frontend_driver
//   ./frontend_driver OUTDIR SCENARIO [ROUTE]
//     SCENARIO  frame | queries | post | deform | sequence | errors
//     ROUTE     host (initializeSSBOs(scene, true), the default) | copies (initializeSSBOs(scene, false)) |
//               devblas (useDeviceBlasBuilder, then host) | device (initializeSSBOsOnDevice)
//
// OUTDIR/steps.txt lists the calls in order, one line each: "<n> <name> key=value ...".  Floating-point values are written
// with %a (exact).  The files of step n are OUTDIR/<n>.<tag>.bin.  Steps "init" and "bind" carry the eight bindings as
// b0, b1, b2, b5 .. b9 (rz_read_binding).  A std::exception is printed and ends the program with 1; nothing is retried.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "RayZenScene.h"
#include "Renderer.h"
#include "rayzen_host.h"

using namespace rayzen;

static std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

struct Log {
    std::string dir;
    FILE* f = nullptr;
    int n = -1;
    explicit Log(const std::string& d) : dir(d) {
        f = std::fopen((d + "/steps.txt").c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + d + "/steps.txt");
    }
    ~Log() { if (f) std::fclose(f); }
    void step(const std::string& name, const std::string& kv = "") {
        ++n;
        std::fprintf(f, "%d %s%s%s\n", n, name.c_str(), kv.empty() ? "" : " ", kv.c_str());
        std::fflush(f);
    }
    void put(const std::string& tag, const void* p, size_t bytes) {
        const std::string path = dir + "/" + std::to_string(n) + "." + tag + ".bin";
        FILE* o = std::fopen(path.c_str(), "wb");
        if (!o) throw std::runtime_error("cannot write " + path);
        const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, o) == bytes;
        std::fclose(o);
        if (!ok) throw std::runtime_error("short write to " + path);
    }
    template <class T> void put(const std::string& tag, const std::vector<T>& v) { put(tag, v.data(), v.size() * sizeof(T)); }
    // the eight arrays the library holds, under the step just written
    void bindings(Renderer& r) {
        for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS, RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES,
                      RZ_BIND_BLAS_NODES, RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES}) {
            size_t need = 0;
            if (rz_read_binding(r.context(), (rz_binding)b, nullptr, 0, &need) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
            std::vector<uint8_t> buf(need);
            if (rz_read_binding(r.context(), (rz_binding)b, buf.data(), buf.size(), &need) != RZ_OK) throw std::runtime_error(rz_last_error(r.context()));
            put("b" + std::to_string(b), buf);
        }
    }
    void bind(Renderer& r) { step("bind"); bindings(r); }
};

// ---------------------------------------------------------------------------------------------------------------------
// the scene

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

static const int kBounces = 3, kSpp = 2;
enum { FLOOR = 0, BLOB_A = 1, BLOB_B = 2, GLASS = 3, SKEW = 4 };

static mat4 skewed(vec3 at) {
    mat4 m = translate(mat4(1.0f), at);
    m.m[4] = 0.4f; m.m[9] = 0.3f; m.m[2] = -0.2f;          // x follows y, y follows z, z follows x: no rotation, no uniform scale
    return m;
}

static void setCamera(Scene& scene, int W, int H) {
    scene.camera = Camera(vec3(0.0f, 2.5f, 10.0f), vec3(0.0f, -0.1f, -1.0f), vec3(0.0f, 1.0f, 0.0f), 70.0f, float(W) / float(H), 0.1f, 100.0f);
}

static Scene makeScene(int W, int H) {
    Scene scene;
    setCamera(scene, W, H);
    scene.materials = {Material(vec3(0.8f, 0.3f, 0.3f), 0.0f, 1.0f, 0.0f, 0.0f, 1.5f),
                       Material(vec3(0.1f, 0.7f, 0.1f), 1.0f, 0.35f, 0.3f, 0.0f, 1.5f),
                       Material(vec3(1.0f), 1.0f, 0.05f, 1.0f, 0.0f, 1.5f),
                       Material(vec3(0.85f, 0.95f, 1.0f), 0.0f, 0.02f, 0.05f, 0.94f, 1.5f),
                       Material(vec3(0.6f, 0.4f, 0.2f), 0.0f, 0.9f, 0.2f, 0.0f, 1.5f)};
    scene.lights.push_back(Light(vec4{5.0f, 5.0f, 5.0f, 1.0f}, vec3(1.0f), 300.0f));      // a point light
    scene.lights.push_back(Light(vec4{0.8f, 1.4f, 0.3f, 0.0f}, vec3(1.0f), 2.0f));        // a directional light
    auto floor = cubeMesh(4), blob = blobMesh(6, 1.6f, 0), glass = blobMesh(4, 1.2f, 3), cube = cubeMesh(1);
    scene.gameObjects.push_back(GameObject{floor, translate(scale(mat4(1.0f), vec3(8.0f, 0.5f, 8.0f)), vec3(0.0f, -3.0f, 0.0f))});
    scene.gameObjects.push_back(GameObject{blob, translate(mat4(1.0f), vec3(-2.5f, 1.5f, 0.0f))});
    scene.gameObjects.push_back(GameObject{blob, rotate(translate(mat4(1.0f), vec3(2.5f, 2.0f, -1.0f)), 0.7f, vec3(0.0f, 1.0f, 0.0f))});
    scene.gameObjects.push_back(GameObject{glass, translate(mat4(1.0f), vec3(0.5f, 0.8f, 4.0f))});
    scene.gameObjects.push_back(GameObject{cube, skewed(vec3(-1.5f, 0.2f, 3.0f))});
    return scene;
}

// two objects move: the second instance of the shared blob and the skewed cube
static void moveObjects(Scene& scene, int k) {
    scene.gameObjects[BLOB_B].transform = rotate(translate(mat4(1.0f), vec3(2.5f - 0.4f * k, 2.0f + 0.15f * k, -1.0f)), 0.7f + 0.2f * k, vec3(0.0f, 1.0f, 0.0f));
    scene.gameObjects[SKEW].transform = skewed(vec3(-1.5f - 0.3f * k, 0.2f, 3.0f + 0.25f * k));
}

static void handOver(Log& L, Renderer& r, const Scene& scene, const std::string& route) {
    if (route == "host") r.initializeSSBOs(scene, true);
    else if (route == "copies") r.initializeSSBOs(scene, false);
    else if (route == "devblas") { r.useDeviceBlasBuilder(); r.initializeSSBOs(scene, true); }
    else if (route == "device") r.initializeSSBOsOnDevice(scene);
    else throw std::runtime_error("unknown route " + route);
    L.step("init", "route=" + route);
    L.bindings(r);
}

// what sendSceneDataToShader hands to rz_set_frame, stated again so that the replay can set the same frame
static rz_frame_params frameRecord(const Scene& scene, int W, int H, int spp, int base) {
    rz_frame_params p{};
    p.width = W; p.height = H;
    const mat4 iv = inverse(scene.camera.viewMatrix), ip = inverse(scene.camera.projectionMatrix);
    std::memcpy(p.inv_view, iv.m, 64); std::memcpy(p.inv_proj, ip.m, 64);
    std::memcpy(p.view, scene.camera.viewMatrix.m, 64); std::memcpy(p.proj, scene.camera.projectionMatrix.m, 64);
    p.cam_pos[0] = scene.camera.position.x; p.cam_pos[1] = scene.camera.position.y; p.cam_pos[2] = scene.camera.position.z;
    p.num_lights = (int)scene.lights.size();
    p.bounce_budget = kBounces; p.spp = spp; p.sample_base = base;
    p.tile_rank = 0; p.tile_nranks = 1;
    return p;
}

static void setFrame(Log& L, Renderer& r, const Scene& scene, int W, int H, int base = 0) {
    r.sendSceneDataToShader(scene, W, H, kBounces, kSpp, base);
    const rz_frame_params p = frameRecord(scene, W, H, kSpp, base);
    L.step("set_frame");
    L.put("fp", &p, sizeof p);
}

static std::vector<float> draw(Log& L, Renderer& r) {
    r.draw();
    r.finish();
    std::vector<float> a = r.readAccum();
    L.step("draw");
    L.put("accum", a);
    return a;
}

static std::vector<float> transformsOf(const Scene& scene) {
    std::vector<float> xf(scene.gameObjects.size() * 16);
    for (size_t i = 0; i < scene.gameObjects.size(); ++i) std::memcpy(&xf[i * 16], scene.gameObjects[i].transform.m, 64);
    return xf;
}

static void update(Log& L, Renderer& r, const Scene& scene, bool onDevice) {
    if (onDevice) r.updateDynamicBVHAndSSBOsOnDevice(scene);
    else r.updateDynamicBVHAndSSBOs(scene);
    L.step("update", fmt("device=%d", (int)onDevice));
    L.put("xf", transformsOf(scene));
    L.bindings(r);
}

// the pixel-centre rays of a W x H frame (row 0 = the bottom row)
static std::vector<rz_ray> cameraRays(const Camera& cam, int W, int H) {
    const mat4 iv = inverse(cam.viewMatrix), ip = inverse(cam.projectionMatrix);
    std::vector<rz_ray> rays;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            vec4 e = ip * vec4{(x + 0.5f) / W * 2.0f - 1.0f, (y + 0.5f) / H * 2.0f - 1.0f, -1.0f, 1.0f};
            const vec4 w = iv * vec4{e.x, e.y, -1.0f, 0.0f};
            const vec3 d = normalize(vec3{w.x, w.y, w.z});
            rz_ray r{};
            r.origin[0] = cam.position.x; r.origin[1] = cam.position.y; r.origin[2] = cam.position.z;
            r.max_dist = 1e30f;
            r.dir[0] = d.x; r.dir[1] = d.y; r.dir[2] = d.z;
            rays.push_back(r);
        }
    return rays;
}

// ---------------------------------------------------------------------------------------------------------------------
// deformation: a shear plus the sine displacement of INTEGRATION.md (x += A sin(3y + phase), z += A cos 2x).  The shear
// (x += 4y) carries the top of a radius-1.6 blob about 6 units sideways: more than its 3.2-unit root box beyond that box.

static std::vector<Triangle> deformed(const std::vector<Triangle>& rest, float phase, float shear = 4.0f, float amp = 0.5f) {
    std::vector<Triangle> out = rest;
    for (Triangle& t : out)
        for (vec3* v : {&t.v0, &t.v1, &t.v2}) {
            const float x = v->x, y = v->y;
            v->x = x + shear * y + amp * std::sin(3.0f * y + phase);
            v->z = v->z + amp * std::cos(2.0f * x);
        }
    return out;
}

// [first, first + count) of the mesh of game object `object` in binding 0, as the hand-over laid it out
static size_t firstTriangleOf(const Renderer& r, int object) { return (size_t)r.buffers().meshInstances[object].globalTriOffset; }

static std::vector<rz_skin_triangle> makeSkin(const std::vector<Triangle>& rest, int nBones) {
    std::vector<rz_skin_triangle> skin(rest.size());
    for (size_t t = 0; t < rest.size(); ++t) {
        rz_skin_triangle& s = skin[t];
        std::memset(&s, 0, sizeof s);
        const vec3* v[3] = {&rest[t].v0, &rest[t].v1, &rest[t].v2};
        for (int c = 0; c < 3; ++c) {
            const float w = 0.5f + 0.3f * std::sin(2.0f * v[c]->y);       // two influences, chosen by height
            const unsigned b0 = v[c]->y > 0.0f ? 1u : 0u, b1 = (unsigned)(nBones - 1);
            s.bones[c] = b0 | (b1 << 8);
            s.weights[c][0] = w; s.weights[c][1] = 1.0f - w;
        }
    }
    return skin;
}
static std::vector<rz_morph_triangle> makeMorphs(const std::vector<Triangle>& rest, int nMorphs) {
    std::vector<rz_morph_triangle> m(rest.size() * nMorphs);
    for (int k = 0; k < nMorphs; ++k)
        for (size_t t = 0; t < rest.size(); ++t) {
            const vec3* v[3] = {&rest[t].v0, &rest[t].v1, &rest[t].v2};
            for (int c = 0; c < 3; ++c) {
                float* d = m[(size_t)k * rest.size() + t].d[c];
                d[0] = (k ? 0.6f : 0.25f) * v[c]->y; d[1] = k ? 0.3f * v[c]->x : 0.0f; d[2] = 0.2f * std::cos(3.0f * v[c]->x + k); d[3] = 7.0f;
            }
        }
    return m;
}
static std::vector<mat4> makeBones(int n, int k) {
    std::vector<mat4> b;
    for (int i = 0; i < n; ++i)
        b.push_back(rotate(translate(mat4(1.0f), vec3(1.5f * i * (k + 1), 0.2f * k, -0.3f * i)), 0.3f * (i + k), vec3(0.0f, 0.0f, 1.0f)));
    return b;
}

// the logged forms of the deforming calls
static void refit(Log& L, Renderer& r, size_t first, const std::vector<Triangle>& tris) {
    r.refitMesh(first, tris);
    L.step("refit", fmt("first=%zu", first));
    L.put("tris", tris);
    L.bindings(r);
}
static void refitAllAfterUpdate(Log& L, Renderer& r, size_t first, const std::vector<Triangle>& tris) {
    if (rz_update(r.context(), RZ_BIND_TRIANGLES, first * sizeof(Triangle), tris.data(), tris.size() * sizeof(Triangle)) != RZ_OK)
        throw std::runtime_error(std::string("rz_update: ") + rz_last_error(r.context()));
    r.refitAll();
    L.step("refit_all", fmt("first=%zu", first));
    L.put("tris", tris);
    L.bindings(r);
}
static int createRig(Log& L, Renderer& r, size_t first, const std::vector<Triangle>& rest, const std::vector<rz_skin_triangle>& skin, int nBones,
                     const std::vector<rz_morph_triangle>& morphs) {
    const int rig = r.createRig(first, rest, skin, nBones, morphs);
    L.step("create_rig", fmt("rig=%d first=%zu bones=%d", rig, first, nBones));
    L.put("rest", rest); L.put("skin", skin); L.put("morphs", morphs);
    return rig;
}
static void pose(Log& L, Renderer& r, int rig, const std::vector<mat4>& bones, const std::vector<float>& weights) {
    r.poseRig(rig, bones, weights);
    L.step("pose", fmt("rig=%d", rig));
    std::vector<float> b(bones.size() * 16);
    for (size_t i = 0; i < bones.size(); ++i) std::memcpy(&b[i * 16], bones[i].m, 64);
    L.put("bones", b); L.put("weights", weights);
    L.bindings(r);
}
static std::vector<rz_mesh_quality> rebuild(Log& L, Renderer& r, double ratio) {
    std::vector<rz_mesh_quality> q = r.rebuildDegraded(ratio);
    L.step("rebuild", fmt("ratio=%a", ratio));
    L.put("quality", q);
    L.bindings(r);
    return q;
}

// ---------------------------------------------------------------------------------------------------------------------
// scenarios

static void scenarioFrame(Log& L, const std::string& route) {
    const int W = 33, H = 17;
    Scene scene = makeScene(W, H);
    Renderer r(0);
    handOver(L, r, scene, route);
    setFrame(L, r, scene, W, H);
    draw(L, r);
    L.step("resolve");
    L.put("rgba8", r.resolveRGBA8());
    setFrame(L, r, scene, W, H, /*sampleBase=*/kSpp);      // two more samples on top of the first two
    draw(L, r);
    L.step("last_render_ms", fmt("ms=%a", (double)r.lastRenderMs()));
    moveObjects(scene, 1);
    update(L, r, scene, /*onDevice=*/true);
    setCamera(scene, 40, 24);
    setFrame(L, r, scene, 40, 24);
    draw(L, r);
}

static void scenarioQueries(Log& L, const std::string& route) {
    const int W = 33, H = 17;
    Scene scene = makeScene(W, H);
    Renderer r(0);
    handOver(L, r, scene, route);
    // 300 rays: every second camera ray, rays from inside the glass blob, rays that miss everything
    std::vector<rz_ray> rays;
    const std::vector<rz_ray> cam = cameraRays(scene.camera, W, H);
    for (size_t i = 0; i < cam.size() && rays.size() < 280; i += 2) rays.push_back(cam[i]);
    for (int i = 0; i < 12; ++i) {
        rz_ray q{};
        q.origin[0] = 0.5f; q.origin[1] = 0.8f; q.origin[2] = 4.0f;
        q.dir[0] = std::cos(0.55f * i); q.dir[1] = 0.4f * std::sin(1.3f * i); q.dir[2] = 2.0f * std::sin(0.55f * i);     // not unit length
        q.max_dist = 1e30f;
        rays.push_back(q);
    }
    for (int i = 0; i < 8; ++i) {
        rz_ray q{};
        q.origin[0] = -3.0f + i; q.origin[1] = 50.0f; q.origin[2] = 0.0f;
        q.dir[0] = 0.1f * i; q.dir[1] = 1.0f; q.dir[2] = -0.2f;
        q.max_dist = 1e30f;
        rays.push_back(q);
    }
    for (size_t i = 0; i < rays.size(); ++i)
        if (i % 3) rays[i].max_dist = 4.0f + 0.05f * i;                   // finite reaches for the shadow queries
    for (int incoherent = 0; incoherent < 2; ++incoherent) {
        const std::vector<rz_hit> hits = r.traceRays(rays, incoherent != 0);
        L.step("trace", fmt("incoherent=%d", incoherent));
        L.put("rays", rays); L.put("hits", hits);
        const std::vector<rz_visibility> vis = r.shadowRays(rays, incoherent != 0);
        L.step("shadow", fmt("incoherent=%d", incoherent));
        L.put("rays", rays); L.put("vis", vis);
    }
    // picking: a 9 x 7 grid with the four corners, fractional positions and positions over the sky (small y = the top)
    int w = W, h = H;
    for (int round = 0; round < 2; ++round) {
        setFrame(L, r, scene, w, h);
        const double fx[9] = {0.0, 0.1, 0.26, 0.39, 0.5, 0.61, 0.74, 0.9, 1.0}, fy[7] = {0.0, 0.15, 0.31, 0.5, 0.69, 0.85, 1.0};
        for (double v : fy)
            for (double u : fx) {
                const double mx = u * w, my = v * h;
                const rz_ray q = Renderer::pickRay(mx, my, w, h, scene.camera);
                L.step("pick_ray", fmt("mx=%a my=%a w=%d h=%d", mx, my, w, h));
                L.put("ray", &q, sizeof q);
                const auto p = r.pick(mx, my, scene);
                L.step("pick", fmt("mx=%a my=%a w=%d h=%d instance=%d triangle=%d", mx, my, w, h, p ? p->first : -1, p ? p->second : -1));
            }
        w = 40; h = 24;                                                  // pick reads the size of the last frame set
        setCamera(scene, w, h);
    }
}

template <class T> static void putParams(Log& L, const char* tag, const T* p) { if (p) L.put(tag, p, sizeof *p); }

static void scenarioPost(Log& L, const std::string& route) {
    const int W = 33, H = 17;
    Scene scene = makeScene(W, H);
    Renderer r(0);
    handOver(L, r, scene, route);
    setFrame(L, r, scene, W, H);
    draw(L, r);

    rz_denoise_params dp{};
    dp.iterations = 3; dp.sigma_color = 0.6f; dp.sigma_normal = 64.0f; dp.sigma_plane = 1.5f; dp.demodulate = 1;
    const rz_present_params on{57.3f, 1, 1, 1, 1, BLOB_A, 5}, off{0.0f, 0, 0, 0, 0, 0, 0};
    for (const rz_denoise_params* p : {(const rz_denoise_params*)nullptr, (const rz_denoise_params*)&dp}) {
        L.step("denoise");
        putParams(L, "dp", p);
        L.put("rgb", r.denoise(p));
    }
    for (const rz_present_params* pp : {&on, &off}) {
        L.step("present_denoised");
        L.put("pp", pp, sizeof *pp); putParams(L, "dp", pp == &on ? &dp : nullptr);
        L.put("rgba8", r.presentDenoised(*pp, pp == &on ? &dp : nullptr));
    }

    rz_temporal_params tp{};
    tp.alpha = 0.3f; tp.alpha_moments = 0.25f; tp.max_history = 8; tp.normal_cos = 0.8f; tp.plane_tol = 3.0f; tp.iterations = 2;
    tp.sigma_l = 0.7f; tp.sigma_normal = 64.0f; tp.sigma_plane = 1.5f; tp.demodulate = 1;
    auto temporal = [&](const rz_temporal_params* p, bool keep) {
        L.step("denoise_temporal", fmt("keep=%d", (int)keep));
        putParams(L, "tp", p);
        L.put("rgb", r.denoiseTemporal(p, keep));
    };
    temporal(nullptr, false);                                            // frame 1
    moveObjects(scene, 1);
    update(L, r, scene, true);
    setFrame(L, r, scene, W, H);
    draw(L, r);
    temporal(&tp, true);                                                 // frame 2: computed, the history stays ...
    temporal(&tp, false);                                                // ... and committed
    moveObjects(scene, 2);
    update(L, r, scene, true);
    setFrame(L, r, scene, W, H);
    draw(L, r);
    temporal(nullptr, false);                                            // frame 3
    L.step("present_temporal");
    L.put("pp", &on, sizeof on); putParams(L, "tp", &tp);
    L.put("rgba8", r.presentTemporal(on, &tp));
    r.resetTemporal();
    L.step("reset_temporal");
    temporal(&tp, false);

    rz_display_params manual{}, autoexp{};
    manual.exposure_mode = 0; manual.exposure = 1.7f; manual.key = 0.18f; manual.min_exposure = 1.0f / 64; manual.max_exposure = 64.0f;
    manual.adapt = 1.0f; manual.curve = 2; manual.white = 4.0f; manual.transfer = 1;
    autoexp = manual;
    autoexp.exposure_mode = 1; autoexp.exposure = 1.0f; autoexp.adapt = 0.4f; autoexp.low_permille = 50; autoexp.high_permille = 20; autoexp.curve = 1;
    auto display = [&](const rz_present_params& pp, const rz_display_params* d, int source, const void* filter, size_t filterBytes) {
        L.step("present_display", fmt("source=%d", source));
        L.put("pp", &pp, sizeof pp); putParams(L, "disp", d);
        if (filter) L.put("filter", filter, filterBytes);
        L.put("rgba8", r.presentDisplay(pp, d, source, filter));
    };
    display(on, nullptr, 0, nullptr, 0);
    display(off, &manual, 1, &dp, sizeof dp);
    display(off, &autoexp, 0, nullptr, 0);                               // jumps to its target
    display(off, &autoexp, 0, nullptr, 0);                               // adapts from there
    display(on, &autoexp, 2, &tp, sizeof tp);
    r.resetDisplay();
    L.step("reset_display");
    display(off, &autoexp, 0, nullptr, 0);
    display(off, &manual, 2, nullptr, 0);

    rz_upscale_params up1{}, up3{};
    up1.factor = 1; up1.sigma_normal = 128.0f; up1.sigma_plane = 1.0f; up1.demodulate = 1;
    up3 = up1; up3.factor = 3; up3.sigma_normal = 32.0f; up3.demodulate = 0;
    auto upscaled = [&](const rz_present_params& pp, const rz_upscale_params* u, const rz_display_params* d, int source, const void* filter,
                        size_t filterBytes) {
        const std::vector<uint8_t> px = r.presentUpscaled(pp, u, d, source, filter);
        L.step("present_upscaled", fmt("source=%d bytes=%zu", source, px.size()));
        L.put("pp", &pp, sizeof pp); putParams(L, "up", u); putParams(L, "disp", d);
        if (filter) L.put("filter", filter, filterBytes);
        L.put("rgba8", px);
    };
    upscaled(on, nullptr, nullptr, 0, nullptr, 0);                       // factor 2: 66 x 34
    upscaled(off, &up1, &manual, 0, nullptr, 0);
    upscaled(on, &up3, &manual, 2, &tp, sizeof tp);
    upscaled(off, &up3, nullptr, 0, nullptr, 0);
    upscaled(off, nullptr, &autoexp, 2, nullptr, 0);
}

// pixels of the W x H frame whose closest hit lies outside the world box its instance had BEFORE the deformation (the box
// Renderer::buffers() still describes): what a stale TLAS would cull
static int pixelsOutsideOldBoxes(Log& L, Renderer& r, const Scene& scene, int W, int H) {
    const std::vector<rz_ray> rays = cameraRays(scene.camera, W, H);
    const std::vector<rz_hit> hits = r.traceRays(rays);
    L.step("trace", "incoherent=0");
    L.put("rays", rays); L.put("hits", hits);
    int outside = 0;
    for (const rz_hit& h : hits) {
        if (h.instance < 0) continue;
        const BVHNode box = worldRootNode(r.buffers().blasRoots[h.instance], scene.gameObjects[h.instance].transform);
        const float lo[3] = {box.boundsMin.x, box.boundsMin.y, box.boundsMin.z}, hi[3] = {box.boundsMax.x, box.boundsMax.y, box.boundsMax.z};
        bool out = false;
        for (int c = 0; c < 3; ++c) out = out || h.point[c] < lo[c] - 1e-3f || h.point[c] > hi[c] + 1e-3f;
        outside += out;
    }
    L.step("outside_old_box", fmt("pixels=%d of=%d", outside, W * H));
    return outside;
}

static void scenarioDeform(Log& L, const std::string& route) {
    const int W = 40, H = 24;
    Scene scene = makeScene(W, H);
    Renderer r(0);
    handOver(L, r, scene, route);
    setFrame(L, r, scene, W, H);
    draw(L, r);
    const std::vector<Triangle>& blob = scene.gameObjects[BLOB_A].mesh->triangles;
    const std::vector<Triangle>& glass = scene.gameObjects[GLASS].mesh->triangles;
    const std::vector<Triangle>& cube = scene.gameObjects[SKEW].mesh->triangles;
    const size_t blobAt = firstTriangleOf(r, BLOB_A), glassAt = firstTriangleOf(r, GLASS), cubeAt = firstTriangleOf(r, SKEW);

    refit(L, r, blobAt, deformed(blob, 0.0f));                           // the whole shared mesh: two instances follow
    draw(L, r);
    pixelsOutsideOldBoxes(L, r, scene, W, H);
    {   // a partial interval inside the mesh
        const std::vector<Triangle> d = deformed(blob, 1.0f, 2.0f);
        refit(L, r, blobAt + 100, std::vector<Triangle>(d.begin() + 100, d.begin() + 171));
        draw(L, r);
    }
    if (glassAt == blobAt + blob.size()) {                               // the end of one mesh and the start of the next
        const std::vector<Triangle> a = deformed(blob, 2.0f, 1.0f), b = deformed(glass, 2.0f, 0.5f);
        std::vector<Triangle> span(a.end() - 5, a.end());
        span.insert(span.end(), b.begin(), b.begin() + 7);
        refit(L, r, glassAt - 5, span);
        draw(L, r);
    }
    refitAllAfterUpdate(L, r, glassAt, deformed(glass, 0.5f, 1.5f, 0.3f));
    draw(L, r);

    // rigs: skin, morph-only, skin + two morph targets; on disjoint ranges
    const int skinRig = createRig(L, r, blobAt, blob, makeSkin(blob, 3), 3, {});
    const int morphRig = createRig(L, r, glassAt, glass, {}, 0, makeMorphs(glass, 1));
    const int bothRig = createRig(L, r, cubeAt, cube, makeSkin(cube, 2), 2, makeMorphs(cube, 2));
    for (int k = 0; k < 3; ++k) {                                        // the pose is not cumulative
        pose(L, r, skinRig, makeBones(3, k), {});
        draw(L, r);
    }
    pose(L, r, morphRig, {}, {0.8f});
    draw(L, r);
    pose(L, r, bothRig, makeBones(2, 1), {0.5f, -0.75f});
    draw(L, r);
    for (int rig : {morphRig, bothRig, skinRig}) {
        r.destroyRig(rig);
        L.step("destroy_rig", fmt("rig=%d", rig));
    }
    L.step("quality");
    L.put("quality", r.meshQuality());
    rebuild(L, r, 1.0);
    draw(L, r);
    rebuild(L, r, 1e9);                                                  // rebuilds nothing
    draw(L, r);
    moveObjects(scene, 1);
    update(L, r, scene, true);
    draw(L, r);
}

static void scenarioSequence(Log& L, const std::string& route) {
    const int W = 40, H = 24;
    for (const char* D : {"refitMesh", "refitAll", "poseRig", "rebuildDegraded"})
        for (int onDevice = 0; onDevice < 2; ++onDevice) {
            Scene scene = makeScene(W, H);
            Renderer r(0);
            L.step("begin", fmt("D=%s device=%d", D, onDevice));
            handOver(L, r, scene, route);
            setFrame(L, r, scene, W, H);
            const std::vector<Triangle>& blob = scene.gameObjects[BLOB_A].mesh->triangles;
            const size_t blobAt = firstTriangleOf(r, BLOB_A);
            int rig = -1;
            if (std::string(D) == "poseRig") rig = createRig(L, r, blobAt, blob, makeSkin(blob, 3), 3, makeMorphs(blob, 1));
            for (int round = 1; round <= 2; ++round) {
                const std::string d = D;
                if (d == "refitMesh") refit(L, r, blobAt, deformed(blob, 0.5f * round));
                else if (d == "refitAll") refitAllAfterUpdate(L, r, blobAt, deformed(blob, 0.5f * round));
                else if (d == "poseRig") pose(L, r, rig, makeBones(3, round), {0.4f * round});
                else {
                    refit(L, r, blobAt, deformed(blob, 0.5f * round, 4.0f * round));
                    rebuild(L, r, 1.0);
                }
                moveObjects(scene, round);
                update(L, r, scene, onDevice != 0);
                draw(L, r);
            }
        }
}

// a call that must throw std::runtime_error: its message goes to steps.txt
template <class F> static void mustThrow(Log& L, const char* name, F call) {
    std::string msg;
    int threw = 0;
    try { call(); } catch (const std::runtime_error& e) { threw = 1; msg = e.what(); }
    for (char& c : msg) if (c == '\n') c = ' ';
    L.step("error", fmt("call=%s threw=%d message=", name, threw) + msg);
}

static void scenarioErrors(Log& L, const std::string& route) {
    const int W = 33, H = 17;
    Scene scene = makeScene(W, H);
    Renderer r(0);
    handOver(L, r, scene, route);
    const rz_present_params off{0.0f, 0, 0, 0, 0, 0, 0};
    mustThrow(L, "denoise_no_frame", [&] { r.denoise(); });
    mustThrow(L, "pick_no_frame", [&] { r.pick(3.0, 4.0, scene); });
    mustThrow(L, "present_display_no_frame", [&] { r.presentDisplay(off); });
    setFrame(L, r, scene, W, H);
    draw(L, r);
    const std::vector<Triangle>& blob = scene.gameObjects[BLOB_A].mesh->triangles;
    const size_t blobAt = firstTriangleOf(r, BLOB_A);
    rz_upscale_params up{};
    up.sigma_normal = 128.0f; up.sigma_plane = 1.0f; up.demodulate = 1;
    up.factor = 0;
    mustThrow(L, "present_upscaled_factor_0", [&] { r.presentUpscaled(off, &up); });
    up.factor = 5;
    mustThrow(L, "present_upscaled_factor_5", [&] { r.presentUpscaled(off, &up); });
    const int rig = r.createRig(blobAt, blob, makeSkin(blob, 3), 3);
    r.destroyRig(rig);
    mustThrow(L, "pose_destroyed_rig", [&] { r.poseRig(rig, makeBones(3, 0)); });
    size_t bytes = 0;
    rz_read_binding(r.context(), RZ_BIND_TRIANGLES, nullptr, 0, &bytes);
    mustThrow(L, "refit_past_the_end", [&] { r.refitMesh(bytes / sizeof(Triangle) - 3, std::vector<Triangle>(blob.begin(), blob.begin() + 4)); });
    std::vector<rz_skin_triangle> shortSkin = makeSkin(blob, 3);
    shortSkin.resize(blob.size() / 2);
    mustThrow(L, "create_rig_short_skin", [&] { r.createRig(blobAt, blob, shortSkin, 3); });
    mustThrow(L, "create_rig_ragged_morphs", [&] { r.createRig(blobAt, blob, {}, 0, std::vector<rz_morph_triangle>(blob.size() + 1)); });
    L.bind(r);
    draw(L, r);                                                          // the renderer is still usable: the same frame again
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s OUTDIR SCENARIO [ROUTE]\n", argv[0]); return 2; }
    const std::string dir = argv[1], scenario = argv[2], route = argc > 3 ? argv[3] : "host";
    try {
        Log L(dir);
        if (scenario == "frame") scenarioFrame(L, route);
        else if (scenario == "queries") scenarioQueries(L, route);
        else if (scenario == "post") scenarioPost(L, route);
        else if (scenario == "deform") scenarioDeform(L, route);
        else if (scenario == "sequence") scenarioSequence(L, route);
        else if (scenario == "errors") scenarioErrors(L, route);
        else throw std::runtime_error("unknown scenario " + scenario);
        L.step("end");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

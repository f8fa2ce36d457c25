// marshalling_check.cpp -- a host-only TEST program (tests/test_cpp_frontend_host.py builds it with -fsanitize=address,undefined
// and runs it; no GPU, no library): rayzen::Renderer against stubs of the C-ABI that read every record the ABI entitles the
// library to read and write every byte it is told it may write -- so that a vector the header passes on too short, or an
// output it sizes too small, is a heap-buffer-overflow under the sanitizer -- and that record the counts, flags and NULL
// conventions they were given.  Held here: createRig (n_triangles of rest and of skin, n_morphs * n_triangles of morphs,
// morphs.size() / n targets, sizes checked before the call) and the flags that change no output byte and therefore cannot be
// seen from a GPU run (RZ_RAYS_INCOHERENT is a scheduling hint), next to the one that does (RZ_TEMPORAL_KEEP).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irayzen_amd/csrc/host
//       tests/cpp/marshalling_check.cpp -o marshalling_check && ./marshalling_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "RayZenScene.h"
#include "Renderer.h"

static struct {
    int calls;
    size_t first, n;
    bool rest, skin, morphs;
    int nBones, nMorphs;
    unsigned sum;
    unsigned flags;         // of the last ray or temporal call
    size_t count, bytes;    // rays of the last query; rgb32f_bytes of the last temporal call
    int width, height;
} g;

template <class T> static unsigned readAll(const T* p, size_t count) {
    unsigned s = 0;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
    for (size_t i = 0; i < count * sizeof(T); ++i) s += b[i];
    return s;
}

extern "C" {
rz_ctx* rz_create(int, unsigned) { return reinterpret_cast<rz_ctx*>(&g); }
void rz_destroy(rz_ctx*) {}
const char* rz_last_error(const rz_ctx*) { return "stub"; }
int rz_skin_create(rz_ctx*, size_t first, size_t n, const rz_triangle* rest, const rz_skin_triangle* skin, int nBones,
                   const rz_morph_triangle* morphs, int nMorphs, int* rigOut) {
    g.calls++;
    g.first = first; g.n = n; g.rest = rest != nullptr; g.skin = skin != nullptr; g.morphs = morphs != nullptr;
    g.nBones = nBones; g.nMorphs = nMorphs;
    g.sum = 0;
    if (rest) g.sum += readAll(rest, n);
    if (skin) g.sum += readAll(skin, n);
    if (morphs) g.sum += readAll(morphs, n * (size_t)nMorphs);
    *rigOut = 40 + g.calls;
    return RZ_OK;
}
int rz_set_frame(rz_ctx*, const rz_frame_params* p) { g.width = p->width; g.height = p->height; return RZ_OK; }
int rz_trace_rays(rz_ctx*, const rz_ray* rays, rz_hit* hits, size_t n, unsigned flags) {
    g.flags = flags; g.count = n; g.sum = readAll(rays, n);
    std::memset(static_cast<void*>(hits), 0, n * sizeof(rz_hit));
    return RZ_OK;
}
int rz_shadow_rays(rz_ctx*, const rz_ray* rays, rz_visibility* out, size_t n, unsigned flags) {
    g.flags = flags; g.count = n; g.sum = readAll(rays, n);
    std::memset(static_cast<void*>(out), 0, n * sizeof(rz_visibility));
    return RZ_OK;
}
int rz_denoise_temporal(rz_ctx*, const rz_temporal_params*, const float* rgbaIn, size_t rgbaInBytes, float* rgb, size_t rgbBytes, rz_hit* guides,
                        size_t guidesBytes, float* stats, size_t statsBytes, unsigned flags) {
    g.flags = flags; g.bytes = rgbBytes;
    if (rgbaIn || rgbaInBytes || guides || guidesBytes || stats || statsBytes) return RZ_ERR_INVALID_ARG;      // the header passes none of them
    std::memset(rgb, 0, rgbBytes);
    return RZ_OK;
}
int rz_present_upscaled(rz_ctx*, const rz_present_params*, const rz_upscale_params* up, const rz_display_params*, int, const void*, uint8_t* rgba8,
                        size_t rgba8Bytes, float* rgb, size_t rgbBytes) {
    const size_t s = up ? (size_t)up->factor : 2, need = s * g.width * s * g.height * 4;      // W x H = s w x s h, RGBA8
    g.bytes = rgba8Bytes;
    if (rgb || rgbBytes) return RZ_ERR_INVALID_ARG;
    if (rgba8Bytes < need) return RZ_ERR_BUFFER_SIZE;
    std::memset(rgba8, 0, need);
    return RZ_OK;
}
}

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "marshalling_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    using namespace rayzen;
    Renderer r(0);
    const size_t n = 37;
    const std::vector<Triangle> rest(n);
    const std::vector<rz_skin_triangle> skin(n);
    const std::vector<rz_morph_triangle> one(n), two(2 * n);

    CHECK(r.createRig(5, rest, skin, 3) == 41);                                  // skin only
    CHECK(g.first == 5 && g.n == n && g.rest && g.skin && !g.morphs && g.nBones == 3 && g.nMorphs == 0);
    CHECK(r.createRig(0, rest, {}, 0, one) == 42);                               // morph-only: skin NULL
    CHECK(g.rest && !g.skin && g.morphs && g.nBones == 0 && g.nMorphs == 1);
    CHECK(r.createRig(7, rest, skin, 2, two) == 43);                             // skin + two targets: morphs.size() / n of them
    CHECK(g.first == 7 && g.skin && g.morphs && g.nBones == 2 && g.nMorphs == 2);

    const int before = g.calls;
    int threw = 0;
    try { r.createRig(0, rest, std::vector<rz_skin_triangle>(n / 2), 3); } catch (const std::runtime_error&) { ++threw; }
    try { r.createRig(0, rest, std::vector<rz_skin_triangle>(n + 1), 3); } catch (const std::runtime_error&) { ++threw; }
    try { r.createRig(0, rest, {}, 0, std::vector<rz_morph_triangle>(n + 1)); } catch (const std::runtime_error&) { ++threw; }
    try { r.createRig(0, rest, {}, 0, std::vector<rz_morph_triangle>(n - 1)); } catch (const std::runtime_error&) { ++threw; }
    try { r.createRig(0, {}, {}, 0, one); } catch (const std::runtime_error&) { ++threw; }
    CHECK(threw == 5 && g.calls == before);                                      // refused before the library saw a pointer

    const std::vector<rz_ray> rays(19);
    CHECK(r.traceRays(rays).size() == 19 && g.count == 19 && g.flags == RZ_RAYS_HOST);
    CHECK(r.traceRays(rays, true).size() == 19 && g.flags == (RZ_RAYS_HOST | RZ_RAYS_INCOHERENT));
    CHECK(r.shadowRays(rays).size() == 19 && g.count == 19 && g.flags == RZ_RAYS_HOST);
    CHECK(r.shadowRays(rays, true).size() == 19 && g.flags == (RZ_RAYS_HOST | RZ_RAYS_INCOHERENT));
    Scene scene;
    r.sendSceneDataToShader(scene, 33, 17, 3, 2);
    CHECK(g.width == 33 && g.height == 17);
    CHECK(r.denoiseTemporal().size() == 33 * 17 * 3 && g.bytes == 33 * 17 * 3 * sizeof(float) && g.flags == RZ_TEMPORAL_HOST);
    CHECK(r.denoiseTemporal(nullptr, true).size() == 33 * 17 * 3 && g.flags == (RZ_TEMPORAL_HOST | RZ_TEMPORAL_KEEP));
    const rz_present_params pp{};
    rz_upscale_params up{};
    CHECK(r.presentUpscaled(pp).size() == 66 * 34 * 4);                          // NULL: factor 2
    for (int f = 1; f <= 4; ++f) {
        up.factor = f;
        CHECK(r.presentUpscaled(pp, &up).size() == (size_t)(33 * f) * (17 * f) * 4 && g.bytes == (size_t)(33 * f) * (17 * f) * 4);
    }
    // pickRay is host arithmetic in binary32: its 28 bytes (origin, max_dist, dir) for the test to compare with pick_ray
    scene.camera = Camera(vec3(0.5f, 2.5f, 10.0f), vec3(0.1f, -0.2f, -1.0f), vec3(0.0f, 1.0f, 0.0f), 70.0f, 33.0f / 17.0f, 0.1f, 100.0f);
    for (double my : {0.0, 4.25, 8.5, 17.0})
        for (double mx : {0.0, 7.75, 16.5, 33.0}) {
            const rz_ray q = Renderer::pickRay(mx, my, 33, 17, scene.camera);
            std::printf("pick_ray %a %a", mx, my);
            for (int i = 0; i < 28; ++i) std::printf("%s%02x", i ? "" : " ", reinterpret_cast<const unsigned char*>(&q)[i]);
            std::printf("\n");
        }
    std::printf("marshalling_check ok\n");
    return 0;
}

// Overlay.h -- drawing into the scene: rz_draw_lines of include/rayzen_hip.h for programs that use the front end of Renderer.h.
// Header-only free functions over Renderer::context().
//
//   drawLines(r, frame, lines, ...) blends the lines over an rgba8 and / or an rgb32f image, in place, as seen through `frame`
//                                   (its width, height, view and proj are read; no rz_set_frame is needed), depth-tested
//                                   against `hits` (width x height rz_hit: rz_render_editor's hits or a denoiser's guides) when
//                                   given.  A scene is needed only if a line names an instance
//   gridLines(size, step, rgba)     a ground grid in the plane y = `y`: what rayzen_amd.lines.grid makes, line for line
//   boxLines(bmin, bmax, rgba)      the 12 edges of an axis-aligned box, in world space or in an instance's (its selection box:
//                                   the root box of its BLAS with instance = its index)
// Nothing here touches the accumulation or any other render state.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "Renderer.h"
#include "rayzen_hip.h"

namespace rayzen {

// colour bytes r, g, b, alpha in memory order
inline uint32_t lineColor(uint8_t r, uint8_t g, uint8_t b, uint8_t a = 255) {
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | ((uint32_t)a << 24);
}

inline rz_line makeLine(float ax, float ay, float az, float bx, float by, float bz, uint32_t color, int32_t instance = -1) {
    rz_line l{};
    l.a[0] = ax; l.a[1] = ay; l.a[2] = az;
    l.b[0] = bx; l.b[1] = by; l.b[2] = bz;
    l.color = color;
    l.instance = instance;
    return l;
}

// The lines x = k * step and z = k * step for |k * step| <= size, each from -size to size: first those along z in ascending x,
// then those along x in ascending z.
inline std::vector<rz_line> gridLines(float size, float step, uint32_t color, float y = 0.0f) {
    if (!(size > 0.0f && step > 0.0f)) throw std::invalid_argument("gridLines: size and step must be positive");
    const int k = (int)std::floor((double)size / (double)step + 1e-6);
    std::vector<rz_line> out;
    out.reserve((size_t)(2 * k + 1) * 2);
    for (int i = -k; i <= k; ++i) {
        const float at = (float)((double)i * (double)step);
        out.push_back(makeLine(at, y, -size, at, y, size, color));
    }
    for (int i = -k; i <= k; ++i) {
        const float at = (float)((double)i * (double)step);
        out.push_back(makeLine(-size, y, at, size, y, at, color));
    }
    return out;
}

// rz_present's corner and edge order; instance >= 0: bmin and bmax are in that instance's space.
inline std::vector<rz_line> boxLines(const float bmin[3], const float bmax[3], uint32_t color, int32_t instance = -1) {
    static const int corner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
    static const int edge[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
    std::vector<rz_line> out;
    out.reserve(12);
    for (const auto& e : edge) {
        const int* p = corner[e[0]];
        const int* q = corner[e[1]];
        out.push_back(makeLine(p[0] ? bmax[0] : bmin[0], p[1] ? bmax[1] : bmin[1], p[2] ? bmax[2] : bmin[2], q[0] ? bmax[0] : bmin[0],
                               q[1] ? bmax[1] : bmin[1], q[2] ? bmax[2] : bmin[2], color, instance));
    }
    return out;
}

// rgba8 (width * height * 4 bytes) and rgb32f (width * height * 3 floats): each optional, at least one; modified in place.
// hits: optional, width * height records.  params null: the library's defaults.
inline void drawLines(Renderer& r, const rz_frame_params& frame, const std::vector<rz_line>& lines, const std::vector<rz_hit>* hits,
                      std::vector<uint8_t>* rgba8, std::vector<float>* rgb32f, const rz_lines_params* params = nullptr) {
    const int rc = rz_draw_lines(r.context(), &frame, params, lines.empty() ? nullptr : lines.data(), lines.size(),
                                 hits ? hits->data() : nullptr, hits ? hits->size() * sizeof(rz_hit) : 0,
                                 rgba8 ? rgba8->data() : nullptr, rgba8 ? rgba8->size() : 0, rgb32f ? rgb32f->data() : nullptr,
                                 rgb32f ? rgb32f->size() * sizeof(float) : 0, RZ_LINES_HOST);
    if (rc != RZ_OK) throw std::runtime_error(std::string("rz_draw_lines: ") + rz_last_error(r.context()));
}

}  // namespace rayzen

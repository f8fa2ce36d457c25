// Selection.h -- selecting what is on screen: rz_coverage and rz_outline of include/rayzen_hip.h for programs that use the front
// end of Renderer.h.  Header-only free functions over Renderer::context().
//
//   coverage(r, frame)              n + 1 rz_instance_coverage records for the pixel-centre rays of `frame` (its width, height,
//                                   inv_view, inv_proj and cam_pos are read; no rz_set_frame is needed): record i is instance i,
//                                   the last one the misses.  Optionally a rectangle, and the id image (width x height int32,
//                                   row 0 = bottom; -1 for a miss and for the pixels outside the rectangle)
//   selectRect(r, frame, rect)      the marquee: (instance, pixels) of the instances that are the closest hit of at least
//                                   minPixels pixels of the rectangle, the most pixels first, ties by the lower index
//   outline(r, w, h, ids, sel, ...) blends `color` into the pixels within `radius` of a selected instance's pixels that are not
//                                   selected themselves, in place, on an rgba8 and / or an rgb32f image; needs no scene
// Nothing here touches the accumulation or any other render state.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "Renderer.h"
#include "rayzen_hip.h"

namespace rayzen {

namespace detail {
inline void selectionCheck(Renderer& r, int rc, const char* what) {
    if (rc != RZ_OK) throw std::runtime_error(std::string(what) + ": " + rz_last_error(r.context()));
}
}  // namespace detail

// rect null: the whole frame.  ids: optional, resized to width * height and filled with -1 before the call.
inline std::vector<rz_instance_coverage> coverage(Renderer& r, const rz_frame_params& frame, const rz_coverage_params* rect = nullptr,
                                                  std::vector<int32_t>* ids = nullptr) {
    size_t bytes = 0;
    detail::selectionCheck(r, rz_read_binding(r.context(), RZ_BIND_INSTANCES, nullptr, 0, &bytes), "rz_read_binding");
    std::vector<rz_instance_coverage> out(bytes / sizeof(rz_bvh_instance) + 1);
    if (ids) ids->assign((size_t)frame.width * (size_t)frame.height, -1);
    detail::selectionCheck(r, rz_coverage(r.context(), &frame, rect, out.data(), out.size() * sizeof(rz_instance_coverage),
                                          ids ? ids->data() : nullptr, ids ? ids->size() * sizeof(int32_t) : 0, RZ_COVERAGE_HOST),
                           "rz_coverage");
    return out;
}

inline std::vector<std::pair<int, uint32_t>> selectRect(Renderer& r, const rz_frame_params& frame, const rz_coverage_params& rect,
                                                        uint32_t minPixels = 1) {
    const std::vector<rz_instance_coverage> rec = coverage(r, frame, &rect);
    std::vector<std::pair<int, uint32_t>> out;
    for (size_t i = 0; i + 1 < rec.size(); ++i)
        if (rec[i].pixels >= std::max<uint32_t>(minPixels, 1)) out.emplace_back((int)i, rec[i].pixels);
    std::stable_sort(out.begin(), out.end(), [](const auto& a, const auto& b) { return a.second > b.second; });
    return out;
}

// selected: instance indices.  rgba8 (width * height * 4 bytes) and rgb32f (width * height * 3 floats): each optional, at least
// one; modified in place.
inline void outline(Renderer& r, int width, int height, const std::vector<int32_t>& ids, const std::vector<int>& selected,
                    std::vector<uint8_t>* rgba8, std::vector<float>* rgb32f, int radius = 2, float red = 1.0f, float green = 0.6f,
                    float blue = 0.0f, float alpha = 1.0f) {
    size_t n = 0;
    for (int i : selected) {
        if (i < 0) throw std::invalid_argument("outline: negative instance index");
        n = std::max(n, (size_t)i + 1);
    }
    std::vector<uint32_t> words((n + 31) / 32, 0u);
    for (int i : selected) words[(size_t)i >> 5] |= 1u << (i & 31);
    rz_outline_params p{};
    p.width = width; p.height = height; p.radius = radius;
    p.color[0] = red; p.color[1] = green; p.color[2] = blue;
    p.alpha = alpha;
    detail::selectionCheck(r, rz_outline(r.context(), &p, ids.data(), ids.size() * sizeof(int32_t), n ? words.data() : nullptr, n,
                                         rgba8 ? rgba8->data() : nullptr, rgba8 ? rgba8->size() : 0, rgb32f ? rgb32f->data() : nullptr,
                                         rgb32f ? rgb32f->size() * sizeof(float) : 0, RZ_OUTLINE_HOST),
                           "rz_outline");
}

}  // namespace rayzen

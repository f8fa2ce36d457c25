// CostMap.h -- where a frame is expensive: the per-pixel traversal cost map of include/rayzen_hip.h (rz_render_cost,
// rz_cost_view, rz_present_cost) for programs that use the front end of Renderer.h.  Header-only free functions over
// Renderer::context(); width and height are those of the last sendSceneDataToShader.
//
//   renderCost(r, w, h)            the map: w x h rz_pixel_cost, row 0 = bottom -- what the reference shader would touch for each
//                                  pixel's samples; optionally the frame's totals as rz_render_counted reports them
//   costView(r, w, h)              the map as a false colour (w x h x 3 floats): black, blue, green, yellow, red up to `scale`
//                                  (0: the frame's maximum), white above a caller's scale; optionally its statistics
//   presentCost(r, w, h, present)  rz_present with that colour in place of the resolve: wireframe, light markers and FPS digits
//                                  on top of the heat map
// Nothing here touches the accumulation or any other render state.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "Renderer.h"
#include "rayzen_hip.h"

namespace rayzen {

namespace detail {
inline void costCheck(Renderer& r, int rc, const char* what) {
    if (rc != RZ_OK) throw std::runtime_error(std::string(what) + ": " + rz_last_error(r.context()));
}
}  // namespace detail

// spp 0: the frame's own.  totals: optional, what rz_render_counted returns for the frame at sample_base 0.
inline std::vector<rz_pixel_cost> renderCost(Renderer& r, int width, int height, int spp = 0, rz_counters* totals = nullptr) {
    rz_cost_params p{};
    p.spp = spp;
    std::vector<rz_pixel_cost> out((size_t)width * (size_t)height);
    detail::costCheck(r, rz_render_cost(r.context(), &p, out.data(), out.size() * sizeof(rz_pixel_cost), totals, RZ_COST_HOST), "rz_render_cost");
    return out;
}

// cost null: the context's last map.  params null: bytes, linear, the frame's maximum at the top of the ramp.
inline std::vector<float> costView(Renderer& r, int width, int height, const rz_cost_view_params* params = nullptr,
                                   const std::vector<rz_pixel_cost>* cost = nullptr, rz_cost_stats* stats = nullptr) {
    std::vector<float> out((size_t)width * (size_t)height * 3);
    detail::costCheck(r, rz_cost_view(r.context(), params, cost ? cost->data() : nullptr, cost ? cost->size() * sizeof(rz_pixel_cost) : 0,
                                      out.data(), out.size() * sizeof(float), stats, RZ_COST_HOST), "rz_cost_view");
    return out;
}

// RGBA8 (width x height x 4, row 0 = bottom) of the context's last map with the overlays drawn on top.
inline std::vector<uint8_t> presentCost(Renderer& r, int width, int height, const rz_present_params& present,
                                        const rz_cost_view_params* params = nullptr) {
    std::vector<uint8_t> out((size_t)width * (size_t)height * 4);
    detail::costCheck(r, rz_present_cost(r.context(), &present, params, out.data(), out.size(), nullptr, 0), "rz_present_cost");
    return out;
}

}  // namespace rayzen

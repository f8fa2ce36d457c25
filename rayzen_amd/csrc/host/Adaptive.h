// Adaptive.h -- adaptive sampling: rz_render_adaptive and rz_adaptive_plan of include/rayzen_hip.h for programs that use the
// front end of Renderer.h.  Header-only free functions over Renderer::context(); width and height are those of the last
// sendSceneDataToShader, whose frame the call renders (its spp is ignored: the batches decide).
//
//   renderAdaptive(r, w, h, params)  the frame in batches of params.batch_spp samples, sampling on only the 8 x 8 tiles whose
//                                    estimated error is above params.threshold.  The result is the context's accumulation (a is
//                                    each pixel's own sample count), which every presenting call of Renderer.h divides by per
//                                    pixel; returned are rz_adaptive_info, the batches every tile received and its last error
//                                    (row-major tiles, row 0 = bottom).  Returns when the frame is complete
//   adaptiveParams()                 the defaults of rz_adaptive_params, spelled out
//   adaptivePlan(active, current)    the runs of tiles a batch renders, from one flag per tile; needs no GPU
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "Renderer.h"
#include "rayzen_hip.h"

namespace rayzen {

struct AdaptiveResult {
    rz_adaptive_info info{};
    std::vector<int32_t> tileBatches;   // ceil(w / 8) * ceil(h / 8)
    std::vector<float> tileError;
};

inline rz_adaptive_params adaptiveParams() {
    rz_adaptive_params p{};
    p.batch_spp = 8; p.min_batches = 4; p.max_batches = 8;
    p.threshold = 0.02f; p.luminance_floor = 0.01f;
    p.merge_gap = 8; p.max_runs = 1;
    return p;
}

inline AdaptiveResult renderAdaptive(Renderer& r, int width, int height, const rz_adaptive_params& params = adaptiveParams()) {
    AdaptiveResult out;
    const size_t tiles = (size_t)((width + 7) / 8) * (size_t)((height + 7) / 8);
    out.tileBatches.resize(tiles);
    out.tileError.resize(tiles);
    rz_adaptive_params p = params;
    p.flags |= RZ_ADAPTIVE_HOST;
    const int rc = rz_render_adaptive(r.context(), &p, &out.info, out.tileBatches.data(), tiles * sizeof(int32_t), out.tileError.data(),
                                      tiles * sizeof(float));
    if (rc != RZ_OK) throw std::runtime_error(std::string("rz_render_adaptive: ") + rz_last_error(r.context()));
    return out;
}

// merge_gap and max_runs are taken as given (0 merges nothing in the rule's second step)
inline std::vector<rz_tile_run> adaptivePlan(const std::vector<uint8_t>& active, const std::vector<uint8_t>& current, int mergeGap = 8,
                                             int maxRuns = 1) {
    if (active.size() != current.size()) throw std::runtime_error("adaptivePlan: active and current differ in length");
    std::vector<rz_tile_run> runs(active.size() / 2 + 1);
    size_t n = 0;
    if (rz_adaptive_plan(active.data(), current.data(), active.size(), mergeGap, maxRuns, runs.data(), runs.size(), &n) != RZ_OK)
        throw std::runtime_error(std::string("rz_adaptive_plan: ") + rz_last_error(nullptr));
    runs.resize(n);
    return runs;
}

}  // namespace rayzen

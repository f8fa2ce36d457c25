// AmbientOcclusion.h -- ray-traced ambient occlusion for previews: rz_ambient_occlusion and rz_ao_directions of
// include/rayzen_hip.h for programs that use the front end of Renderer.h.  Header-only free functions over Renderer::context().
//
//   ambientOcclusion(r, frame, params, rgbIn, want)   the occlusion of the pixel-centre hits of `frame` (its width, height,
//                                   inv_view, inv_proj and cam_pos are read; no rz_set_frame is needed), smoothed unless
//                                   params.smooth is 0.  rgbIn: a width x height x 3 image to darken (Renderer's editor image),
//                                   null: white.  want: which of the three outputs to fill -- ao (width * height floats),
//                                   rgb32f (x 3 floats), rgba8 (x 4 bytes); row 0 = bottom
//   aoParams()                      the defaults of rz_ao_params
//   aoDirections()                  the 256 unit directions the samples are drawn from; needs no GPU
// Nothing here touches the accumulation or any other render state.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "Renderer.h"
#include "rayzen_hip.h"

namespace rayzen {

struct AmbientOcclusionImages {
    std::vector<float> ao;          // width * height
    std::vector<float> rgb32f;      // width * height * 3
    std::vector<uint8_t> rgba8;     // width * height * 4
};
enum AmbientOcclusionWant : unsigned { AO_WANT_AO = 1u, AO_WANT_RGB32F = 2u, AO_WANT_RGBA8 = 4u };

inline rz_ao_params aoParams() {
    rz_ao_params p{};
    p.samples = 4; p.radius = 1.0f; p.smooth = 1; p.strength = 1.0f;
    p.normal_cos = 0.9f; p.plane_tol = 2.0f;
    return p;
}

inline AmbientOcclusionImages ambientOcclusion(Renderer& r, const rz_frame_params& frame, const rz_ao_params& params = aoParams(),
                                               const std::vector<float>* rgbIn = nullptr, unsigned want = AO_WANT_AO) {
    const size_t np = (size_t)frame.width * (size_t)frame.height;
    AmbientOcclusionImages out;
    if (want & AO_WANT_AO) out.ao.resize(np);
    if (want & AO_WANT_RGB32F) out.rgb32f.resize(np * 3);
    if (want & AO_WANT_RGBA8) out.rgba8.resize(np * 4);
    const int rc = rz_ambient_occlusion(r.context(), &frame, &params, rgbIn ? rgbIn->data() : nullptr,
                                        rgbIn ? rgbIn->size() * sizeof(float) : 0, out.ao.empty() ? nullptr : out.ao.data(),
                                        out.ao.size() * sizeof(float), out.rgb32f.empty() ? nullptr : out.rgb32f.data(),
                                        out.rgb32f.size() * sizeof(float), out.rgba8.empty() ? nullptr : out.rgba8.data(),
                                        out.rgba8.size(), RZ_AO_HOST);
    if (rc != RZ_OK) throw std::runtime_error(std::string("rz_ambient_occlusion: ") + rz_last_error(r.context()));
    return out;
}

inline std::vector<float> aoDirections() {
    std::vector<float> out(256 * 3);
    if (rz_ao_directions(out.data(), out.size() * sizeof(float)) != RZ_OK)
        throw std::runtime_error(std::string("rz_ao_directions: ") + rz_last_error(nullptr));
    return out;
}

}  // namespace rayzen

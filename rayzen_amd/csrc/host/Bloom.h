// Bloom.h -- HDR glare: rz_bloom and rz_present_bloomed of include/rayzen_hip.h for programs that use the front end of
// Renderer.h.  Header-only free functions over Renderer::context().
//
//   bloom(r, width, height, rgb, ...)        the frame with glare (width * height * 3 floats, linear, unclamped) of `rgb`, or of
//                                            the accumulation when rgb is null; `glare`, when given, receives the normalised glare
//                                            alone.  width and height are those of the frame last set
//   presentBloomed(r, width, height, ...)    Renderer::presentDisplay() with the glare between the source's colour and the display
//                                            stage: the RGBA8 frame, overlays on top.  bloom null: the library's defaults; a
//                                            bloom with intensity 0 gives presentDisplay()'s bytes
// Neither touches the accumulation or any other render state (source 2 advances the temporal history, as presentTemporal does).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "Renderer.h"
#include "rayzen_hip.h"

namespace rayzen {

inline std::vector<float> bloom(Renderer& r, int width, int height, const std::vector<float>* rgb = nullptr,
                                const rz_bloom_params* params = nullptr, std::vector<float>* glare = nullptr) {
    const size_t n = (size_t)width * (size_t)height * 3;
    if (rgb && rgb->size() < n) throw std::invalid_argument("bloom: rgb holds fewer than width * height * 3 floats");
    std::vector<float> out(n);
    if (glare) glare->resize(n);
    const int rc = rz_bloom(r.context(), params, rgb ? rgb->data() : nullptr, rgb ? rgb->size() * sizeof(float) : 0, out.data(),
                            out.size() * sizeof(float), glare ? glare->data() : nullptr, glare ? glare->size() * sizeof(float) : 0,
                            RZ_BLOOM_HOST);
    if (rc != RZ_OK) throw std::runtime_error(std::string("rz_bloom: ") + rz_last_error(r.context()));
    return out;
}

inline std::vector<uint8_t> presentBloomed(Renderer& r, int width, int height, const rz_present_params& present,
                                           const rz_display_params* display = nullptr, const rz_bloom_params* bloomParams = nullptr,
                                           int source = 0, const void* filterParams = nullptr, std::vector<float>* rgb32f = nullptr) {
    const size_t n = (size_t)width * (size_t)height;
    std::vector<uint8_t> px(n * 4);
    if (rgb32f) rgb32f->resize(n * 3);
    const int rc = rz_present_bloomed(r.context(), &present, display, bloomParams, source, filterParams, px.data(), px.size(),
                                      rgb32f ? rgb32f->data() : nullptr, rgb32f ? rgb32f->size() * sizeof(float) : 0);
    if (rc != RZ_OK) throw std::runtime_error(std::string("rz_present_bloomed: ") + rz_last_error(r.context()));
    return px;
}

}  // namespace rayzen

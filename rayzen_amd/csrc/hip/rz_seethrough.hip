// rz_seethrough.hip -- see-through guides for the guided upsampler (include/rayzen_hip.h: rz_upscale_seethrough /
// rz_present_upscaled_seethrough).  rz_upscale's guide is the first hit, so what is seen in a mirror or through glass is
// interpolated as colour on the mirror or the glass.  Both events are deterministic in the path loop (rz_path.h: scatter): a
// transparent surface always refracts (or reflects on total internal reflection) and a surface with reflectivity >= 1 always
// mirrors.  The guide can therefore follow the pixel-centre ray through them to the first surface that scatters diffusely and
// the colour is interpolated THERE.
//
//   rz_seethrough_guides   rz_denoise_guides' shape: a persistent grid of one-wave workgroups, 64 pixels of a row per step.  The
//                          chain is a wave-uniform loop that runs while a ballot says a lane is live -- at most max_depth + 1
//                          queries -- and a finished lane stays out of the query (the predicated body of rz_shadow_rays_kernel).
//                          Per pixel a 48-B record, three 16-B stores: (n, L | x, final hit word | T, cls), and the rz_hit of
//                          the final hit with t = L and the rz_chain when asked.
//   rz_seethrough_gather   rz_upscale_gather's body (rz_upscale_body.h, CHAIN = true) on those records: alpha = T * albedo and
//                          the class term.
//
// The chain of a pixel (the header states it; operands in scatter()'s order, binary32, no fused multiply-add):
//   o = cam_pos, d = rz_denoise's guide direction, ior = 1, T = (1, 1, 1), L = 0, k = 0; repeat: h = closest hit of (o, d); a
//   miss ends the chain (final = miss); L += t; M = materials[clamp(h.material)]; if k == max_depth the chain ends at h; else
//   if M.transparency > 0 the dielectric step of scatter(); else if M.reflectivity >= 1 d = reflect(d, n), T *= 0.95; else the
//   chain ends at h.  After a step o = hp + (hn * pushDir) * 0.003 and k += 1.  cls = 0 if k == 0, else m_first + 1.
// The pixel's ray, the chain loop and the (n, L | x, word) part of the record are rz_pixel_cast.h's, the step rz_chain_step.h's,
// the rz_hit rz_query.h's (store_hit), the gather rz_upscale_body.h's.
#include "rz_upscale_body.h"
#include "rz_pixel_cast.h"

namespace rz {

template <bool OVF>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_seethrough_guides(const KParams K, const SeethroughGuideLaunch G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    const int lane = threadIdx.x & 63;
    const v3 cam = mk3(K.camPos[0], K.camPos[1], K.camPos[2]);
    bool cut = false;
    for (long long u = blockIdx.x; u < G.units; u += gridDim.x) {
        const int py = (int)(u / G.unitsX), px = (int)(u - (long long)py * G.unitsX) * 64 + lane;
        const bool inside = px < K.width;
        v3 o = cam, d = mk3(0.0f, 0.0f, 0.0f);
        if (inside) d = pixel_centre_dir(K, px, py, K.width, K.height);
        const ChainEnd e = cast_chain<OVF>(K, G.maxDepth, o, d, inside, bstk, cut);
        if (!inside) continue;
        const size_t pix = (size_t)py * K.width + px;
        float4 g0, g1;
        guide_record(K, e.found, e.h, e.L, g0, g1);
        G.rec[3 * pix] = g0;
        G.rec[3 * pix + 1] = g1;
        G.rec[3 * pix + 2] = make_float4(e.T.x, e.T.y, e.T.z, __int_as_float(e.cls()));
        // rz_trace_rays_kernel's record of the final query, with t = L
        if (G.hits) store_hit(K, G.instTriOff, G.hits, pix, e.found, e.h, e.tri, e.L);
        if (G.chains) G.chains[pix] = make_float4(e.T.x, e.T.y, e.T.z, __int_as_float(e.k | ((e.first + 1) << 8)));
    }
    rays_backstop(G.errWord, cut);
}

__global__ __launch_bounds__(256) void rz_seethrough_gather(const UpscaleLaunch U) { upscale_gather_body<true>(U); }

void launch_seethrough_guides(const KParams& K, const SeethroughGuideLaunch& G, hipStream_t stream) {
    const dim3 g((unsigned)G.grid), b(64);
    const size_t lds = (size_t)K.blasStackCap * 64 * sizeof(uint2);
    if (K.blasOvfCap > 0) hipLaunchKernelGGL((rz_seethrough_guides<true>), g, b, lds, stream, K, G);
    else hipLaunchKernelGGL((rz_seethrough_guides<false>), g, b, lds, stream, K, G);
}

void launch_seethrough_gather(const UpscaleLaunch& U, hipStream_t stream) {
    const int W = U.w * U.s, H = U.h * U.s;
    const dim3 g((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), b(64, 4);
    hipLaunchKernelGGL(rz_seethrough_gather, g, b, 0, stream, U);
}

}  // namespace rz

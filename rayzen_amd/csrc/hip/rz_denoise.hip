// rz_denoise.hip -- an edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) for the low-sample frame
// (include/rayzen_hip.h: rz_denoise / rz_present_denoised).  The render path does not change: these kernels read the
// accumulation (or a caller buffer in the same sum-and-count form) and the device scene, and write buffers of their own.
//
//   rz_denoise_guides   one lane per pixel: the closest hit of the ray through the pixel centre (rz_path.h:
//                       camera_ray_centre, from cam_pos; rz_query.h: ray_query -- the very query rz_trace_rays runs, not clipped),
//                       as a 32-B guide record (normal, t | point, hit word) and, when asked, as the rz_hit record rz_trace_rays
//                       writes for that ray.  A wave covers 64 pixels of one row per step of a grid-stride loop over a persistent
//                       grid of one-wave workgroups (rz_editor.hip's structure); a walk stopped at its backstop sets
//                       RZ_BACKSTOP_RAYS.
//   rz_denoise_atrous   one pass per launch, 64 x 4 pixels per workgroup (a wave = 64 pixels of one row), ping-ponging between
//                       two context-owned float4 buffers.  Pass 0 reads the accumulation and resolves and demodulates every tap
//                       it reads (FIRST); pass K-1 re-modulates and writes the outputs (LAST).  The 25 taps are gathered from
//                       L1 / L2: no LDS staging (an LDS tile plus halo was not needed to meet the cost target --
//                       profiles/denoise/README.md).
//   rz_denoise_resolve  K = 0: c_p itself.
//
// The filter, per pixel p (row 0 = the bottom row), with guide G_p = (hit_p, x_p, n_p, t_p, m_p):
//   c_p = accum.rgb / n, n = accum.a > 0 ? accum.a : 1;  alpha_p = materials[m_p].albedo for a hit, (1, 1, 1) for a miss
//   d_p = c_p / max(alpha_p, 1e-3) (demodulate = 1), else c_p
//   pass i = 0..K-1, s = 2^i:  d'_p = sum_q w_pq d_q / sum_q w_pq over q = p + s (a, b), a, b in -2..2, q inside the image
//     w_pq = h_a h_b [hit_p == hit_q] W_geom exp(-|d_p - d_q|^2 2^i / sigma_c^2),  h = (1/16, 1/4, 3/8, 1/4, 1/16)
//     W_geom = max(0, n_p.n_q)^sigma_n exp(-|n_p.(x_q - x_p)| / (sigma_x t_p f s max(|a|, |b|)))  when both are hits,
//              1 when both are misses and for the centre tap;  f = 2 |inv_proj[5]| / height
//   out_p = d_p alpha_p after the last pass (demodulate = 1), else d_p;  K = 0: out_p = c_p exactly.
// A pixel whose c has a NaN or an infinite channel is bad: pass 0 drops it as a tap (as a tap outside the image), and as a centre
// it drops its own term, takes every remaining tap at colour weight 1 and becomes num / den, or (0, 0, 0) when no tap is left.  So
// pass 0's output is finite and the later passes need no test (include/rayzen_hip.h states the rule).
// Arithmetic is binary32 (tests/denoise_ref.py restates it in binary64; tests/test_denoise_gpu.py states the tolerance).
// rz_denoise_guides is made of shared pieces: the pixel's ray and the guide record are rz_pixel_cast.h's, the rz_hit record
// rz_query.h's (store_hit); the colour outputs go through store_colour (rz_internal.h).
#include "rz_internal.h"
#include "rz_pixel_cast.h"

namespace rz {

template <bool OVF>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_denoise_guides(const KParams K, const DenoiseGuideLaunch G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    const int lane = threadIdx.x & 63;
    const v3 cam = mk3(K.camPos[0], K.camPos[1], K.camPos[2]);
    bool cut = false;
    for (long long u = blockIdx.x; u < G.units; u += gridDim.x) {
        const int py = (int)(u / G.unitsX), px = (int)(u - (long long)py * G.unitsX) * 64 + lane;
        if (px >= K.width) continue;
        const v3 d = pixel_centre_dir(K, px, py, K.width, K.height);
        HitRec h;
        TraceExtra x;
        const bool found = ray_query<OVF, false>(K, cam, d, h, bstk, x);
        cut = cut || x.cut;
        const size_t pix = (size_t)py * K.width + px;
        float4 g0, g1;
        guide_record(K, found, h, h.t, g0, g1);
        G.guide[2 * pix] = g0;
        G.guide[2 * pix + 1] = g1;
        if (G.hits) store_hit(K, G.instTriOff, G.hits, pix, found, h, x.tri, h.t);      // rz_trace_rays_kernel's record, miss included
    }
    rays_backstop(G.errWord, cut);
}

// c_p = accum.rgb / n, as rz_present_kernel divides (without its clamp)
__device__ __forceinline__ v3 resolve_px(const float4 a) {
    const float n = a.w > 0.0f ? a.w : 1.0f;
    return mk3(a.x / n, a.y / n, a.z / n);
}
__device__ __forceinline__ v3 albedo_of(const DenoiseLaunch& D, int word) {
    if (word < 0) return mk3(1.0f, 1.0f, 1.0f);
    const DevMaterial& m = D.materials[word];
    return mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
}
// the colour d_q a pass filters: pass 0 resolves (and demodulates) the input and says whether c_q is bad; later passes read the
// previous pass's output, which is finite
template <bool FIRST>
__device__ __forceinline__ v3 pass_input(const DenoiseLaunch& D, size_t q, int word, bool& bad) {
    bad = false;
    if (!FIRST) {
        const float4 s = D.src[q];
        return mk3(s.x, s.y, s.z);
    }
    v3 c = resolve_px(D.accum[q]);
    bad = nonfinite_(c);
    if (D.demodulate && word >= 0) {
        const v3 al = albedo_of(D, word);
        c = mk3(c.x / fmax_(al.x, 1e-3f), c.y / fmax_(al.y, 1e-3f), c.z / fmax_(al.z, 1e-3f));
    }
    return c;
}

// h = (1/16, 1/4, 3/8, 1/4, 1/16), indexed by a in -2..2 (a compile-time constant once the tap loops are unrolled)
__device__ constexpr float atrous_h(int a) { return a == 0 ? 0.375f : (a == 1 || a == -1 ? 0.25f : 0.0625f); }

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void rz_denoise_atrous(const DenoiseLaunch D) {
    const int px = blockIdx.x * 64 + threadIdx.x, py = blockIdx.y * 4 + threadIdx.y;
    if (px >= D.width || py >= D.height) return;
    const size_t p = (size_t)py * D.width + px;
    const float4 g0 = D.guide[2 * p], g1 = D.guide[2 * p + 1];
    const int wordP = __float_as_int(g1.w);
    const bool hitP = wordP >= 0;
    const v3 np_ = mk3(g0.x, g0.y, g0.z), xp = mk3(g1.x, g1.y, g1.z);
    bool badP, badQ;
    const v3 dp = pass_input<FIRST>(D, p, wordP, badP);
    // 1 / (sigma_x t_p f s): the plane term's denominator without max(|a|, |b|)
    const float invPlane = hitP ? D.planeScale / g0.w : 0.0f;
    const float centre = atrous_h(0) * atrous_h(0);
    v3 num = dp * centre;
    float den = centre;
    if (FIRST && badP) {        // a bad centre leaves its own term out
        num = mk3(0.0f, 0.0f, 0.0f);
        den = 0.0f;
    }
#pragma unroll
    for (int b = -2; b <= 2; ++b) {
        const int qy = py + b * D.step;
        if (qy < 0 || qy >= D.height) continue;
#pragma unroll
        for (int a = -2; a <= 2; ++a) {
            if (a == 0 && b == 0) continue;
            const int qx = px + a * D.step;
            if (qx < 0 || qx >= D.width) continue;
            const size_t q = (size_t)qy * D.width + qx;
            const float4 h1 = D.guide[2 * q + 1];
            const int wordQ = __float_as_int(h1.w);
            if ((wordQ >= 0) != hitP) continue;                 // a hit and a miss never mix
            float w = atrous_h(a) * atrous_h(b);
            if (hitP) {
                const float4 h0 = D.guide[2 * q];
                const float nd = fmax_(dot(np_, mk3(h0.x, h0.y, h0.z)), 0.0f);
                const float wn = nd > 0.0f ? __builtin_exp2f(D.sigmaNormal * __builtin_log2f(nd)) : (D.sigmaNormal == 0.0f ? 1.0f : 0.0f);
                const float m = (a == 2 || a == -2 || b == 2 || b == -2) ? 0.5f : 1.0f;       // 1 / max(|a|, |b|)
                const float pl = __builtin_fabsf(dot(np_, mk3(h1.x, h1.y, h1.z) - xp)) * (invPlane * m);
                w *= wn * __builtin_expf(-pl);
            }
            const v3 dq = pass_input<FIRST>(D, q, wordQ, badQ);
            if (FIRST && badQ) continue;                        // a bad tap is dropped like one outside the image
            if (!(FIRST && badP)) {                             // (a bad centre has no colour to compare with: weight 1)
                const v3 e = dp - dq;
                w *= __builtin_expf(-dot(e, e) * D.invColor);
            }
            num = num + dq * w;
            den += w;
        }
    }
    v3 out = mk3(num.x / den, num.y / den, num.z / den);
    if (FIRST && badP && !(den > 0.0f)) out = mk3(0.0f, 0.0f, 0.0f);       // every tap dropped
    if (LAST && D.demodulate) {
        const v3 al = albedo_of(D, wordP);
        out = mk3(out.x * al.x, out.y * al.y, out.z * al.z);
    }
    store_colour(D.dst, LAST ? D.rgb : nullptr, p, out, LAST ? 1.0f : 0.0f);
}

__global__ __launch_bounds__(256) void rz_denoise_resolve(const DenoiseLaunch D) {
    const int px = blockIdx.x * 64 + threadIdx.x, py = blockIdx.y * 4 + threadIdx.y;
    if (px >= D.width || py >= D.height) return;
    const size_t p = (size_t)py * D.width + px;
    const v3 c = resolve_px(D.accum[p]);
    store_colour(D.dst, D.rgb, p, c, 1.0f);
}

void launch_denoise_guides(const KParams& K, const DenoiseGuideLaunch& G, hipStream_t stream) {
    const dim3 g((unsigned)G.grid), b(64);
    const size_t lds = (size_t)K.blasStackCap * 64 * sizeof(uint2);
    if (K.blasOvfCap > 0) hipLaunchKernelGGL((rz_denoise_guides<true>), g, b, lds, stream, K, G);
    else hipLaunchKernelGGL((rz_denoise_guides<false>), g, b, lds, stream, K, G);
}

void launch_denoise_pass(const DenoiseLaunch& D, bool first, bool last, hipStream_t stream) {
    const dim3 g((unsigned)((D.width + 63) / 64), (unsigned)((D.height + 3) / 4)), b(64, 4);
    if (first && last) hipLaunchKernelGGL((rz_denoise_atrous<true, true>), g, b, 0, stream, D);
    else if (first) hipLaunchKernelGGL((rz_denoise_atrous<true, false>), g, b, 0, stream, D);
    else if (last) hipLaunchKernelGGL((rz_denoise_atrous<false, true>), g, b, 0, stream, D);
    else hipLaunchKernelGGL((rz_denoise_atrous<false, false>), g, b, 0, stream, D);
}

void launch_denoise_resolve(const DenoiseLaunch& D, hipStream_t stream) {
    const dim3 g((unsigned)((D.width + 63) / 64), (unsigned)((D.height + 3) / 4)), b(64, 4);
    hipLaunchKernelGGL(rz_denoise_resolve, g, b, 0, stream, D);
}

}  // namespace rz

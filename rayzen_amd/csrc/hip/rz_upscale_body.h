// rz_upscale_body.h -- the gather of the guided upsampler, shared by its two kernels so that they cannot drift apart:
//   rz_upscale_gather     (rz_upscale.hip)     CHAIN = false: first-hit guides, 32-B records (n, t | x, material word)
//   rz_seethrough_gather  (rz_seethrough.hip)  CHAIN = true: see-through guides, 48-B records (n, L | x, material word | T, cls)
// The filter is the one stated at the head of rz_upscale.hip.  With CHAIN the guide is the final hit of the pixel's chain,
// alpha is T * albedo (T alone for a final miss: a miss is demodulated too), and a tap is admissible only if its class equals
// the pixel's.  Everything that differs sits behind `if constexpr (CHAIN)`: the first-hit instantiation is the code it was.
// rz_antialias_edges (rz_antialias.hip) evaluates the same reconstruction (upscale_pixel<false>) on guides it casts itself.
#pragma once
#include "rz_internal.h"
#include "rz_device_math.h"

namespace rz {

// c_q of the low frame: the packed colour as it is, or rgb / n of a sum and count (rz_present's divide without its clamp)
__device__ __forceinline__ v3 upscale_colour(const UpscaleLaunch& U, size_t q) {
    if (U.in4) {
        const float4 a = U.in4[q];
        const float n = a.w > 0.0f ? a.w : 1.0f;
        return mk3(a.x / n, a.y / n, a.z / n);
    }
    return mk3(U.in3[3 * q], U.in3[3 * q + 1], U.in3[3 * q + 2]);
}
__device__ __forceinline__ v3 upscale_albedo(const UpscaleLaunch& U, int word) {
    if (word < 0) return mk3(1.0f, 1.0f, 1.0f);
    const DevMaterial& m = U.materials[word];
    return mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
}
// alpha of a see-through record: T * albedo(final material), T for a final miss (albedo (1, 1, 1): T * 1 is T)
__device__ __forceinline__ v3 upscale_chain_alpha(const UpscaleLaunch& U, int word, const float4 h2) {
    return mk3(h2.x, h2.y, h2.z) * upscale_albedo(U, word);
}

// One tap inside the low image: adds w d_q to num and w to den when it is admissible, and says whether it was.
template <bool CHAIN>
__device__ __forceinline__ bool upscale_tap(const UpscaleLaunch& U, int qx, int qy, bool hitP, int clsP, const v3 nP, const v3 xP,
                                            float invPlane, float B, v3& num, float& den) {
    constexpr int REC = CHAIN ? 3 : 2;
    const size_t q = (size_t)qy * U.w + qx;
    const float4 h1 = U.guideLo[REC * q + 1];
    const int wordQ = __float_as_int(h1.w);
    if ((wordQ >= 0) != hitP) return false;                     // a hit and a miss never mix
    float4 h2 = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    if constexpr (CHAIN) {
        h2 = U.guideLo[REC * q + 2];
        if (__float_as_int(h2.w) != clsP) return false;         // nor do two classes
    }
    v3 c = upscale_colour(U, q);
    if (nonfinite_(c)) return false;                            // a bad low pixel is no tap
    float wg = 1.0f;
    if (hitP) {
        const float4 h0 = U.guideLo[REC * q];
        const float nd = fmax_(dot(nP, mk3(h0.x, h0.y, h0.z)), 0.0f);
        const float wn = nd > 0.0f ? __builtin_exp2f(U.sigmaNormal * __builtin_log2f(nd)) : (U.sigmaNormal == 0.0f ? 1.0f : 0.0f);
        const float pl = __builtin_fabsf(dot(nP, mk3(h1.x, h1.y, h1.z) - xP)) * invPlane;
        wg = wn * __builtin_expf(-pl);
    }
    if constexpr (CHAIN) {
        if (U.demodulate) {
            const v3 al = upscale_chain_alpha(U, wordQ, h2);
            c = mk3(c.x / fmax_(al.x, 1e-3f), c.y / fmax_(al.y, 1e-3f), c.z / fmax_(al.z, 1e-3f));
        }
    } else {
        if (U.demodulate && wordQ >= 0) {
            const v3 al = upscale_albedo(U, wordQ);
            c = mk3(c.x / fmax_(al.x, 1e-3f), c.y / fmax_(al.y, 1e-3f), c.z / fmax_(al.z, 1e-3f));
        }
    }
    const float w = B * fmax_(wg, 1e-4f);
    num = num + c * w;
    den += w;
    return true;
}

// The reconstruction of one HIGH pixel (X, Y) from its guide record held in registers (g2: CHAIN only): stages 1 to 3.  The
// gather kernels read the record from U.guideHi; rz_antialias_edges (rz_antialias.hip) has just cast it.
template <bool CHAIN>
__device__ __forceinline__ v3 upscale_pixel(const UpscaleLaunch& U, int X, int Y, const float4 g0, const float4 g1, const float4 g2) {
    const int wordP = __float_as_int(g1.w), clsP = __float_as_int(g2.w);
    const bool hitP = wordP >= 0;
    const v3 nP = mk3(g0.x, g0.y, g0.z), xP = mk3(g1.x, g1.y, g1.z);
    const float invPlane = hitP ? U.planeScale / g0.w : 0.0f;   // 1 / (sigma_x t_P f)
    // the footprint, in integers: r >= 1 - s > -2s, so the floor of r / 2s is -1 for a negative r
    const int s2 = 2 * U.s;
    const int rx = 2 * X + 1 - U.s, ry = 2 * Y + 1 - U.s;
    const int i0 = rx < 0 ? -1 : rx / s2, j0 = ry < 0 ? -1 : ry / s2;
    const float fx = (float)(rx - s2 * i0) / (float)s2, fy = (float)(ry - s2 * j0) / (float)s2;
    v3 num = mk3(0.0f, 0.0f, 0.0f);
    float den = 0.0f;
    bool any = false;
#pragma unroll
    for (int b = 0; b <= 1; ++b) {
        const int qy = j0 + b;
        if (qy < 0 || qy >= U.h) continue;
#pragma unroll
        for (int a = 0; a <= 1; ++a) {
            const int qx = i0 + a;
            if (qx < 0 || qx >= U.w) continue;
            const float B = (a ? fx : 1.0f - fx) * (b ? fy : 1.0f - fy);
            if (!(B > 0.0f)) continue;
            any = upscale_tap<CHAIN>(U, qx, qy, hitP, clsP, nP, xP, invPlane, B, num, den) || any;
        }
    }
    if (!any) {                 // stage 2: the ring around the footprint
        for (int b = -1; b <= 2; ++b) {
            const int qy = j0 + b;
            if (qy < 0 || qy >= U.h) continue;
            for (int a = -1; a <= 2; ++a) {
                const int qx = i0 + a;
                if ((a >= 0 && a <= 1 && b >= 0 && b <= 1) || qx < 0 || qx >= U.w) continue;
                any = upscale_tap<CHAIN>(U, qx, qy, hitP, clsP, nP, xP, invPlane, 1.0f, num, den) || any;
            }
        }
    }
    v3 out;
    if (any) {
        out = mk3(num.x / den, num.y / den, num.z / den);
        if (U.demodulate) {
            const v3 al = CHAIN ? upscale_chain_alpha(U, wordP, g2) : upscale_albedo(U, wordP);
            out = mk3(out.x * al.x, out.y * al.y, out.z * al.z);
        }
    } else {                    // stage 3: the nearest low pixel as it is
        out = upscale_colour(U, (size_t)(Y / U.s) * U.w + X / U.s);
        if (nonfinite_(out)) out = mk3(0.0f, 0.0f, 0.0f);
    }
    return out;
}

// The body of both gather kernels: one lane per HIGH pixel, launched as 64 x 4 pixels per workgroup.
template <bool CHAIN>
__device__ __forceinline__ void upscale_gather_body(const UpscaleLaunch& U) {
    constexpr int REC = CHAIN ? 3 : 2;
    const int W = U.w * U.s, H = U.h * U.s;
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
    if (X >= W || Y >= H) return;
    const size_t P = (size_t)Y * W + X;
    const float4 g0 = U.guideHi[REC * P], g1 = U.guideHi[REC * P + 1];
    float4 g2 = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    if constexpr (CHAIN) g2 = U.guideHi[REC * P + 2];
    const v3 out = upscale_pixel<CHAIN>(U, X, Y, g0, g1, g2);
    store_colour(U.dst, U.rgb, P, out, 1.0f);
}

}  // namespace rz

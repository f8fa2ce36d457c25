// rz_upscale.hip -- guided upsampling of a frame rendered below display size (include/rayzen_hip.h: rz_upscale /
// rz_present_upscaled).  The render path does not change: the frame is rendered at w x h, and this pass reconstructs it at
// W x H = s w x s h from a G-buffer cast at the HIGH size, so silhouettes and material boundaries are as sharp as in a native
// frame and only the demodulated, slowly varying colour is interpolated.
//
//   the guides          two launches of rz_denoise_guides (rz_denoise.hip, unchanged): one at W x H, one at w x h.
//   rz_upscale_gather   one lane per HIGH pixel, 64 x 4 pixels per workgroup (a wave = 64 pixels of one row, as in
//                       rz_denoise_atrous).  The lane reads its own guide record (32 B) and, per tap, a low guide record and a
//                       low colour; resolve, bad-pixel test and demodulation happen inside the tap read.  The low pixels a
//                       wave's row touches are 64 / s + 1 contiguous ones, each shared by s lanes and by s rows, so the taps
//                       are gathered from L1 / L2 without LDS staging (profiles/upscale/README.md).  Stage 2 (the twelve outer
//                       taps of the 4 x 4 window) and stage 3 (the nearest low pixel) are divergent tails that almost no lane
//                       takes.
//
// The filter, per high pixel P = (X, Y) (row 0 = the bottom row), with G_P = (hit_P, x_P, n_P, t_P, m_P) the high guide and
// g_q the low one; c_q the low colour (rgb / n of a sum-and-count input), alpha(m) = materials[m].albedo for a hit, (1, 1, 1)
// for a miss; d_q = c_q / max(alpha(m_q), 1e-3) (demodulate = 1), else c_q:
//   footprint  r_x = 2X + 1 - s, i0 = floor(r_x / 2s) in integers, fx = (float)(r_x - 2s i0) / (float)(2s); likewise j0, fy
//   a tap q is admissible iff it lies inside the low image, c_q has no NaN or infinite channel, and hit_q == hit_P
//   W_geom = max(0, n_P.n_q)^sigma_n exp(-|n_P.(x_q - x_P)| / (sigma_x t_P f)), f = 2 |inv_proj[5]| / h; 1 between misses
//   stage 1    q = (i0 + a, j0 + b), a, b in 0..1, B = (a ? fx : 1 - fx)(b ? fy : 1 - fy); taps with B == 0 are skipped;
//              w = B max(W_geom, 1e-4);  out = alpha(m_P) sum w d_q / sum w   (no alpha(m_P) with demodulate = 0)
//   stage 2    only if stage 1 admitted no tap: the twelve outer taps of i0-1..i0+2 x j0-1..j0+2, w = max(W_geom, 1e-4)
//   stage 3    only if stage 2 admitted none either: out = c_q of q = (X / s, Y / s), or (0, 0, 0) if that c_q is bad
// Which stage a pixel takes depends on integers, hit flags and bit patterns only.  Taps are summed row by row (b outer, a
// inner).  Arithmetic is binary32 (tests/upscale_ref.py restates it in binary64; tests/test_upscale_gpu.py states the tolerance).
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

// One tap inside the low image: adds w d_q to num and w to den when it is admissible, and says whether it was.
__device__ __forceinline__ bool upscale_tap(const UpscaleLaunch& U, int qx, int qy, bool hitP, const v3 nP, const v3 xP, float invPlane,
                                            float B, v3& num, float& den) {
    const size_t q = (size_t)qy * U.w + qx;
    const float4 h1 = U.guideLo[2 * q + 1];
    const int wordQ = __float_as_int(h1.w);
    if ((wordQ >= 0) != hitP) return false;                     // a hit and a miss never mix
    v3 c = upscale_colour(U, q);
    if (nonfinite_(c)) return false;                            // a bad low pixel is no tap
    float wg = 1.0f;
    if (hitP) {
        const float4 h0 = U.guideLo[2 * q];
        const float nd = fmax_(dot(nP, mk3(h0.x, h0.y, h0.z)), 0.0f);
        const float wn = nd > 0.0f ? __builtin_exp2f(U.sigmaNormal * __builtin_log2f(nd)) : (U.sigmaNormal == 0.0f ? 1.0f : 0.0f);
        const float pl = __builtin_fabsf(dot(nP, mk3(h1.x, h1.y, h1.z) - xP)) * invPlane;
        wg = wn * __builtin_expf(-pl);
    }
    if (U.demodulate && wordQ >= 0) {
        const v3 al = upscale_albedo(U, wordQ);
        c = mk3(c.x / fmax_(al.x, 1e-3f), c.y / fmax_(al.y, 1e-3f), c.z / fmax_(al.z, 1e-3f));
    }
    const float w = B * fmax_(wg, 1e-4f);
    num = num + c * w;
    den += w;
    return true;
}

__global__ __launch_bounds__(256) void rz_upscale_gather(const UpscaleLaunch U) {
    const int W = U.w * U.s, H = U.h * U.s;
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
    if (X >= W || Y >= H) return;
    const size_t P = (size_t)Y * W + X;
    const float4 g0 = U.guideHi[2 * P], g1 = U.guideHi[2 * P + 1];
    const int wordP = __float_as_int(g1.w);
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
            any = upscale_tap(U, qx, qy, hitP, nP, xP, invPlane, B, num, den) || any;
        }
    }
    if (!any) {                 // stage 2: the ring around the footprint
        for (int b = -1; b <= 2; ++b) {
            const int qy = j0 + b;
            if (qy < 0 || qy >= U.h) continue;
            for (int a = -1; a <= 2; ++a) {
                const int qx = i0 + a;
                if ((a >= 0 && a <= 1 && b >= 0 && b <= 1) || qx < 0 || qx >= U.w) continue;
                any = upscale_tap(U, qx, qy, hitP, nP, xP, invPlane, 1.0f, num, den) || any;
            }
        }
    }
    v3 out;
    if (any) {
        out = mk3(num.x / den, num.y / den, num.z / den);
        if (U.demodulate) {
            const v3 al = upscale_albedo(U, wordP);
            out = mk3(out.x * al.x, out.y * al.y, out.z * al.z);
        }
    } else {                    // stage 3: the nearest low pixel as it is
        out = upscale_colour(U, (size_t)(Y / U.s) * U.w + X / U.s);
        if (nonfinite_(out)) out = mk3(0.0f, 0.0f, 0.0f);
    }
    if (U.dst) U.dst[P] = make_float4(out.x, out.y, out.z, 1.0f);
    if (U.rgb) {
        U.rgb[3 * P] = out.x;
        U.rgb[3 * P + 1] = out.y;
        U.rgb[3 * P + 2] = out.z;
    }
}

void launch_upscale_gather(const UpscaleLaunch& U, hipStream_t stream) {
    const int W = U.w * U.s, H = U.h * U.s;
    const dim3 g((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), b(64, 4);
    hipLaunchKernelGGL(rz_upscale_gather, g, b, 0, stream, U);
}

}  // namespace rz

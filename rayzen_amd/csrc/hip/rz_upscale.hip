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
#include "rz_upscale_body.h"

namespace rz {

// (the body is upscale_gather_body of rz_upscale_body.h, which rz_seethrough_gather shares)
__global__ __launch_bounds__(256) void rz_upscale_gather(const UpscaleLaunch U) { upscale_gather_body<false>(U); }

void launch_upscale_gather(const UpscaleLaunch& U, hipStream_t stream) {
    const int W = U.w * U.s, H = U.h * U.s;
    const dim3 g((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), b(64, 4);
    hipLaunchKernelGGL(rz_upscale_gather, g, b, 0, stream, U);
}

}  // namespace rz

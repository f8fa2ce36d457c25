// rz_antialias.hip -- edge anti-aliasing from sub-pixel guides (include/rayzen_hip.h: rz_antialias / rz_present_antialiased).
// The path loop's camera jitter is rand * 2e-5 in uv, so a frame converges to its pixel-centre sample and its silhouettes stay
// stair-stepped at any sample count.  The render path does not change: this pass shades once per pixel, takes geometry at s x s
// sub-pixel positions on the pixels that have an edge, reconstructs each sub-pixel's colour from the neighbours on its own
// surface (rz_upscale's gather, rz_upscale_body.h: upscale_pixel) and averages.  A flat pixel keeps its colour bit for bit.
//
//   the frame-size guide   one launch of rz_denoise_guides (rz_denoise.hip, unchanged).
//   rz_antialias_edges     rz_denoise_guides' shape: a persistent grid of one-wave workgroups, the BLAS stack in LDS, a unit = 64
//                          pixels of a row.  Per unit every lane CLASSIFIES its pixel from the 3 x 3 guide records around it
//                          (gathered from L1 / L2 as the a-trous taps are), writes `edges`, and writes c_p if the pixel is flat.
//                          A ballot and a prefix count append the edge pixels' indices to a QUEUE of the wave in LDS, which lives
//                          across units.  Whenever the queue holds 64 / s^2 pixels (16, 7 or 4), and once more after the wave's
//                          last unit, the wave takes that many: lane g s^2 + k casts sub-sample k = b s + a of pixel g
//                          (ray_query, the high pixel's centre: bit for bit what rz_upscale casts at s w x s h), evaluates u with
//                          upscale_pixel, and the group's first lane sums the group in the stated order through __shfl and
//                          writes the pixel.  No global atomics, no second colour buffer; no result depends on the grouping.
//
// DIFFERENT (q from p), EDGE and the edge pixel's mean are stated in the header; the classification is binary32, one rounding per
// operation (tests/antialias_ref.py restates it bit for bit).  The steps themselves -- DIFFERENT, the append, a sub-pixel's ray,
// the group's mean -- are rz_antialias_body.h's (CHAIN = false), shared with rz_antialias_seethrough.hip; the sub-pixel's guide
// record is rz_pixel_cast.h's, as rz_denoise_guides writes it.  This file is the schedule and the 3 x 3 loop.
#include "rz_antialias_body.h"

namespace rz {

template <bool OVF>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_antialias_edges(const KParams K, const AntialiasLaunch A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    int* queue = reinterpret_cast<int*>(lds_raw + (size_t)K.blasStackCap * 64 * sizeof(uint2));     // RZ_AA_QUEUE entries
    const UpscaleLaunch& U = A.U;
    const int lane = threadIdx.x & 63;
    const v3 cam = mk3(K.camPos[0], K.camPos[1], K.camPos[2]);
    const int s = U.s, ss = s * s, take = 64 / ss;
    const int grp = lane / ss, sub = lane - grp * ss;       // the pixel of a batch this lane works on, and its sub-sample
    const int sb = sub / s, sa = sub - sb * s;
    int count = 0;              // pixels in the queue (wave-uniform)
    bool cut = false;
    long long u = blockIdx.x;
    for (;;) {
        const bool more = u < A.units;
        if (more) {             // classify one unit and queue its edge pixels
            const int py = (int)(u / A.unitsX), px = (int)(u - (long long)py * A.unitsX) * 64 + lane;
            bool edge = false;
            const size_t p = (size_t)py * U.w + (px < U.w ? px : 0);
            if (px < U.w) {
                const v3 c = upscale_colour(U, p);
                edge = nonfinite_(c);
                const float4 g0 = U.guideLo[2 * p], g1 = U.guideLo[2 * p + 1];
                const int wordP = __float_as_int(g1.w);
                const v3 nP = mk3(g0.x, g0.y, g0.z), xP = mk3(g1.x, g1.y, g1.z);
#pragma unroll
                for (int b = -1; b <= 1; ++b) {
#pragma unroll
                    for (int a = -1; a <= 1; ++a) {
                        if (a == 0 && b == 0) continue;
                        const int qx = px + a, qy = py + b;
                        const bool inside = qx >= 0 && qx < U.w && qy >= 0 && qy < U.h;
                        // (a neighbour outside the image does not count: its lane reads p's own record and drops the answer)
                        const size_t q = inside ? (size_t)qy * U.w + qx : p;
                        edge = edge | (inside & aa_different<false>(A, q, wordP >= 0, wordP, 0, nP, xP, g0.w));
                    }
                }
                if (A.edges) A.edges[p] = edge ? 1 : 0;
                if (!edge || s == 1) store_colour(U.dst, U.rgb, p, c, 1.0f);        // out = c_p exactly
            }
            u += gridDim.x;        // (strided, not consecutive units: measured, profiles/antialias/README.md)
            if (s == 1) continue;
            aa_append(queue, count, edge, p);       // (count <= take - 1 here, so the index stays below RZ_AA_QUEUE)
            __syncthreads();    // (one wave: orders the queue's writes before the reads below)
        }
        // cast and gather: full batches while there are any, and whatever is left after the last unit
        while (count >= take || (!more && count > 0)) {
            const int n = count < take ? count : take;
            const bool act = grp < n;
            v3 uo = mk3(0.0f, 0.0f, 0.0f);
            int pix = 0;
            if (act) {
                pix = queue[count - n + grp];
                int X, Y;
                const v3 d = aa_sub_pixel(K, U, pix, sa, sb, X, Y);
                HitRec h;
                TraceExtra tx;
                const bool found = ray_query<OVF, false>(K, cam, d, h, bstk, tx);
                cut = cut || tx.cut;
                float4 g0, g1;          // rz_denoise_guides' record of the high pixel
                guide_record(K, found, h, h.t, g0, g1);
                uo = upscale_pixel<false>(U, X, Y, g0, g1, make_float4(1.0f, 1.0f, 1.0f, 0.0f));
            }
            aa_store_mean(U, uo, lane, ss, act && sub == 0, pix);
            count -= n;
        }
        if (!more) break;
    }
    rays_backstop(A.errWord, cut);
}

void launch_antialias(const KParams& K, const AntialiasLaunch& A, hipStream_t stream) {
    const dim3 g((unsigned)A.grid), b(64);
    const size_t lds = (size_t)K.blasStackCap * 64 * sizeof(uint2) + RZ_AA_QUEUE * sizeof(int);
    if (K.blasOvfCap > 0) hipLaunchKernelGGL((rz_antialias_edges<true>), g, b, lds, stream, K, A);
    else hipLaunchKernelGGL((rz_antialias_edges<false>), g, b, lds, stream, K, A);
}

}  // namespace rz

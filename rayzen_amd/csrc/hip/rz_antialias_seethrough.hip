// rz_antialias_seethrough.hip -- edge anti-aliasing on see-through guides (include/rayzen_hip.h: rz_antialias_seethrough /
// rz_present_antialiased_seethrough).  rz_antialias classifies and reconstructs on first hits, so the silhouette of what stands
// behind a pane or in a mirror stays stair-stepped, and a pixel on the pane's own border mixes colour across the edge seen
// through it.  Here the record of a pixel is the final record of its chain (rz_seethrough.hip: the path loop's deterministic
// events, glass and perfect mirrors, followed to the first surface that scatters diffusely), the class is one more reason to be
// DIFFERENT, and a sub-pixel is what rz_upscale_seethrough reconstructs (rz_upscale_body.h: upscale_pixel<true>).
//
//   the frame-size records          one launch of rz_seethrough_guides (rz_seethrough.hip, unchanged): 48 B per pixel,
//                                   (n, L | x, final hit word | T, cls).
//   rz_antialias_seethrough_classify  a persistent grid of one-wave workgroups, a unit = 64 pixels of a row, classified as
//                                   rz_antialias_edges classifies (rz_antialias.hip), without a branch, from the 3 x 3 records
//                                   (three 16-B words each now; the third gives cls).  Writes `edges` and the flat pixels, and
//                                   appends the unit's edge pixels by ballot and prefix count to the wave's OWN segment of a
//                                   list in global memory; at the end the wave stores its count.  No atomics.
//   rz_antialias_seethrough_edges   the same grid, the BLAS stack in LDS.  Every wave sums the segments' counts to the same
//                                   prefix (64 lanes x grid / 64 counts, one shuffle scan), which numbers the edge pixels of
//                                   the frame 0 .. total - 1, and takes the batches of 64 / s^2 consecutive numbers b = wave,
//                                   wave + grid, ...: the edge pixels are handed out EVENLY, whichever wave found them.  Lane
//                                   g s^2 + k runs the CHAIN of sub-sample k of the batch's pixel g as the wave-uniform loop of
//                                   rz_seethrough_guides -- while a ballot says a lane is live, at most max_depth + 1 trips,
//                                   the step itself shared with that kernel (rz_chain_step.h) -- evaluates u on its final
//                                   record, and the group's first lane sums the group in the stated order through __shfl.
//                                   No global atomics, no second colour buffer; no result depends on the grouping.
//
// Why two launches where rz_antialias has one: with the chains run by the wave that found the pixels (a queue in LDS, as
// rz_antialias_edges keeps it) the pass was bound by its busiest wave -- half of a curved glass blob classifies as edge, a
// 64-pixel unit inside it was four batches of up to nine sequential queries while most of the grid idled -- and took longer
// than rz_upscale_seethrough at the same factor (profiles/antialias_seethrough/README.md).  Compaction of the live lanes inside
// a wave was built for that form and was slower still (same README, "Stage B").
//
// With max_depth = 0 every chain is its first query, L = 0 + t = t, T = (1, 1, 1) and cls = 0: rz_antialias' bytes exactly.
// That holds by construction: both files run the steps of rz_antialias_body.h (here CHAIN = true: rz_antialias' rule on the
// FINAL records, t_p = L_p, or another class), and the chain and its record are rz_pixel_cast.h's, which rz_seethrough_guides
// runs too.  This file is the schedule and the 3 x 3 loop.
#include "rz_antialias_body.h"

namespace rz {

__global__ __launch_bounds__(64) void rz_antialias_seethrough_classify(const AntialiasSeethroughLaunch A) {
    const UpscaleLaunch& U = A.U;
    const int lane = threadIdx.x & 63;
    const int s = U.s;
    int* seg = A.list + (size_t)blockIdx.x * A.segCap;      // this wave's segment: segCap = 64 x the units a wave can get
    int count = 0;              // edge pixels in it (wave-uniform)
    for (long long u = blockIdx.x; u < A.units; u += gridDim.x) {
        const int py = (int)(u / A.unitsX), px = (int)(u - (long long)py * A.unitsX) * 64 + lane;
        bool edge = false;
        const size_t p = (size_t)py * U.w + (px < U.w ? px : 0);
        if (px < U.w) {
            const v3 c = upscale_colour(U, p);
            edge = nonfinite_(c);
            const float4 g0 = U.guideLo[3 * p], g1 = U.guideLo[3 * p + 1];
            const int wordP = __float_as_int(g1.w), clsP = __float_as_int(U.guideLo[3 * p + 2].w);
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
                    edge = edge | (inside & aa_different<true>(A, q, wordP >= 0, wordP, clsP, nP, xP, g0.w));
                }
            }
            if (A.edges) A.edges[p] = edge ? 1 : 0;
            if (!edge || s == 1) store_colour(U.dst, U.rgb, p, c, 1.0f);        // out = c_p exactly
        }
        if (s == 1) continue;
        aa_append(seg, count, edge, p);         // (a unit adds at most 64, so the index stays below segCap)
    }
    if (lane == 0) A.counts[blockIdx.x] = count;
}

template <bool OVF>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_antialias_seethrough_edges(const KParams K, const AntialiasSeethroughLaunch A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    const UpscaleLaunch& U = A.U;
    const int lane = threadIdx.x & 63;
    const v3 cam = mk3(K.camPos[0], K.camPos[1], K.camPos[2]);
    const int s = U.s, ss = s * s, take = 64 / ss;
    const int grp = lane / ss, sub = lane - grp * ss;       // the pixel of a batch this lane works on, and its sub-sample
    const int sb = sub / s, sa = sub - sb * s;
    // the prefix of the segments' counts, the same in every wave: lane l holds the sum of segments l C .. l C + C - 1
    const int G = (int)gridDim.x, C = (G + 63) / 64;
    int mySum = 0;
    for (int i = 0; i < C; ++i) {
        const int idx = lane * C + i;
        if (idx < G) mySum += A.counts[idx];
    }
    int incl = mySum;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const int lanePrefix = incl - mySum;
    const int total = __shfl(incl, 63);
    const int batches = (total + take - 1) / take;
    bool cut = false;
    for (int b = blockIdx.x; b < batches; b += G) {
        const int n = min(take, total - b * take);
        const bool act = grp < n;
        // edge pixel number p of the frame: the segment that holds it, and where
        const int p = b * take + (act ? grp : 0);
        int blk = 0, base = 0;
        for (int l = 0; l < 64; ++l) {          // the last lane block that starts at or below p (empty blocks start where the next does)
            const int lp = __shfl(lanePrefix, l);
            if (p >= lp) { blk = l; base = lp; }
        }
        int segi = blk * C;
        bool found_seg = false;
        for (int i = 0; i < C; ++i) {
            const int idx = blk * C + i;
            const int c = idx < G ? A.counts[idx] : 0;
            if (!found_seg) {
                if (p >= base + c) { base += c; segi = idx + 1; }
                else found_seg = true;
            }
        }
        segi = min(segi, G - 1);                // (p < total, so the walk ends inside the grid; the clamp keeps a wrong count in bounds)
        const int at = min(max(p - base, 0), A.segCap - 1);
        int pix = 0, X = 0, Y = 0;
        v3 d = mk3(0.0f, 0.0f, 0.0f);
        if (act) {
            pix = A.list[(size_t)segi * A.segCap + at];
            d = aa_sub_pixel(K, U, pix, sa, sb, X, Y);
        }
        // the chain of the high pixel (X, Y): rz_seethrough_guides' loop, bit for bit what it casts at s w x s h
        const ChainEnd e = cast_chain<OVF>(K, A.maxDepth, cam, d, act, bstk, cut);
        v3 uo = mk3(0.0f, 0.0f, 0.0f);
        if (act) {          // rz_seethrough_guides' record of the high pixel
            float4 g0, g1;
            guide_record(K, e.found, e.h, e.L, g0, g1);
            uo = upscale_pixel<true>(U, X, Y, g0, g1, make_float4(e.T.x, e.T.y, e.T.z, __int_as_float(e.cls())));
        }
        aa_store_mean(U, uo, lane, ss, act && sub == 0, pix);
    }
    rays_backstop(A.errWord, cut);
}

void launch_antialias_seethrough(const KParams& K, const AntialiasSeethroughLaunch& A, hipStream_t stream) {
    const dim3 g((unsigned)A.grid), b(64);
    hipLaunchKernelGGL(rz_antialias_seethrough_classify, g, b, 0, stream, A);
    if (A.U.s == 1) return;                     // classify only
    const size_t lds = (size_t)K.blasStackCap * 64 * sizeof(uint2);
    if (K.blasOvfCap > 0) hipLaunchKernelGGL((rz_antialias_seethrough_edges<true>), g, b, lds, stream, K, A);
    else hipLaunchKernelGGL((rz_antialias_seethrough_edges<false>), g, b, lds, stream, K, A);
}

}  // namespace rz

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
#include "rz_upscale_body.h"
#include "rz_query.h"
#include "rz_path.h"
#include "rz_chain_step.h"

namespace rz {

// is the neighbour q DIFFERENT from p?  rz_antialias' rule (rz_antialias.hip: aa_different) on the FINAL records, t_p = L_p, or
// another class.  Branch-free for the same reason: the eight neighbours' loads are in flight together.
__device__ __forceinline__ bool aas_different(const AntialiasLaunch& A, size_t q, bool hitP, int wordP, int clsP, const v3 nP, const v3 xP,
                                              float tP) {
    const float4 h0 = A.U.guideLo[3 * q], h1 = A.U.guideLo[3 * q + 1];
    const int clsQ = __float_as_int(A.U.guideLo[3 * q + 2].w);
    const int wordQ = __float_as_int(h1.w);
    const bool hitQ = wordQ >= 0;
    const bool crease = dot(nP, mk3(h0.x, h0.y, h0.z)) < A.edgeNormal;
    const bool step = __builtin_fabsf(dot(nP, mk3(h1.x, h1.y, h1.z) - xP)) > A.edgePlane * tP;
    return (hitQ != hitP) | (clsQ != clsP) | (hitP & hitQ & ((wordQ != wordP) | crease | step));
}

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
                    edge = edge | (inside & aas_different(A, q, wordP >= 0, wordP, clsP, nP, xP, g0.w));
                }
            }
            if (A.edges) A.edges[p] = edge ? 1 : 0;
            if (!edge || s == 1) {          // out = c_p exactly
                if (U.dst) U.dst[p] = make_float4(c.x, c.y, c.z, 1.0f);
                if (U.rgb) {
                    U.rgb[3 * p] = c.x;
                    U.rgb[3 * p + 1] = c.y;
                    U.rgb[3 * p + 2] = c.z;
                }
            }
        }
        if (s == 1) continue;
        const unsigned long long m = rz_ballot(edge);
        // (the prefix count: the edge lanes below this one; a unit adds at most 64, so the index stays below segCap)
        const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (edge) seg[count + before] = (int)p;
        count += mask_count(m);
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
        v3 o = cam, d = mk3(0.0f, 0.0f, 0.0f);
        if (act) {
            pix = A.list[(size_t)segi * A.segCap + at];
            const int y = pix / U.w, x = pix - y * U.w;
            X = s * x + sa;
            Y = s * y + sb;
            v2 uv;
            uv.x = ((float)X + 0.5f) / (float)(U.w * s);
            uv.y = ((float)Y + 0.5f) / (float)(U.h * s);
            d = camera_ray_centre(K.invProj, K.invView, uv);
        }
        // the chain of the high pixel (X, Y): rz_seethrough_guides' loop, bit for bit what it casts at s w x s h
        float ior = 1.0f, L = 0.0f;
        v3 T = mk3(1.0f, 1.0f, 1.0f);
        int k = 0, first = -1;
        bool found = false;
        HitRec h = {};
        bool run = act;
        while (rz_ballot(run) != 0ull) {    // at most max_depth + 1 trips: a lane with k == max_depth ends at its hit
            if (run) {
                HitRec hq;
                TraceExtra tx;
                found = ray_query<OVF, false>(K, o, d, hq, bstk, tx);
                cut = cut || tx.cut;
                run = false;
                if (found) {
                    h = hq;
                    run = chain_step(K, A.maxDepth, hq, o, d, T, ior, L, k, first);     // rz_chain_step.h
                }
            }
        }
        v3 uo = mk3(0.0f, 0.0f, 0.0f);
        if (act) {          // rz_seethrough_guides' record of the high pixel
            const int word = found ? min(max(h.mat, 0), K.nMaterials - 1) : -1;
            const int cls = k == 0 ? 0 : first + 1;
            const float4 g0 = found ? make_float4(h.n.x, h.n.y, h.n.z, L) : make_float4(0.0f, 0.0f, 0.0f, 1e30f);
            const float4 g1 = found ? make_float4(h.p.x, h.p.y, h.p.z, __int_as_float(word))
                                    : make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            uo = upscale_pixel<true>(U, X, Y, g0, g1, make_float4(T.x, T.y, T.z, __int_as_float(cls)));
        }
        v3 sum = uo;        // (((u_0 + u_1) + ...) + u_{s^2 - 1}), b outer and a inner: the group's lanes in order
        for (int j = 1; j < ss; ++j) {
            sum.x = sum.x + __shfl(uo.x, lane + j);
            sum.y = sum.y + __shfl(uo.y, lane + j);
            sum.z = sum.z + __shfl(uo.z, lane + j);
        }
        if (act && sub == 0) {
            const float inv = (float)ss;
            const v3 out = mk3(sum.x / inv, sum.y / inv, sum.z / inv);
            if (U.dst) U.dst[pix] = make_float4(out.x, out.y, out.z, 1.0f);
            if (U.rgb) {
                U.rgb[3 * (size_t)pix] = out.x;
                U.rgb[3 * (size_t)pix + 1] = out.y;
                U.rgb[3 * (size_t)pix + 2] = out.z;
            }
        }
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

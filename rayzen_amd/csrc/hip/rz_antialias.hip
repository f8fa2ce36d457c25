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
// operation (tests/antialias_ref.py restates it bit for bit).
#include "rz_upscale_body.h"
#include "rz_query.h"
#include "rz_path.h"

namespace rz {

// is the neighbour q DIFFERENT from p?  (n_p, x_p, t_p, m_p: p's record; ke = (float)(edge_plane f))
// Written without a branch, both records fetched whatever they hold: the eight neighbours' sixteen loads are then in flight
// together, where a test after every load would make them eight round trips to L2 one after the other.
__device__ __forceinline__ bool aa_different(const AntialiasLaunch& A, size_t q, bool hitP, int wordP, const v3 nP, const v3 xP, float tP) {
    const float4 h0 = A.U.guideLo[2 * q], h1 = A.U.guideLo[2 * q + 1];
    const int wordQ = __float_as_int(h1.w);
    const bool hitQ = wordQ >= 0;
    const bool crease = dot(nP, mk3(h0.x, h0.y, h0.z)) < A.edgeNormal;
    const bool step = __builtin_fabsf(dot(nP, mk3(h1.x, h1.y, h1.z) - xP)) > A.edgePlane * tP;
    return (hitQ != hitP) | (hitP & hitQ & ((wordQ != wordP) | crease | step));
}

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
                        edge = edge | (inside & aa_different(A, q, wordP >= 0, wordP, nP, xP, g0.w));
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
            u += gridDim.x;         // (strided, not consecutive units: measured, profiles/antialias/README.md)
            if (s == 1) continue;
            const unsigned long long m = rz_ballot(edge);
            // (the prefix count: the edge lanes below this one; count <= take - 1 here, so the index stays below RZ_AA_QUEUE)
            const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (edge) queue[count + before] = (int)p;
            count += mask_count(m);
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
                const int y = pix / U.w, x = pix - y * U.w;
                const int X = s * x + sa, Y = s * y + sb;
                v2 uv;
                uv.x = ((float)X + 0.5f) / (float)(U.w * s);
                uv.y = ((float)Y + 0.5f) / (float)(U.h * s);
                const v3 d = camera_ray_centre(K.invProj, K.invView, uv);
                HitRec h;
                TraceExtra tx;
                const bool found = ray_query<OVF, false>(K, cam, d, h, bstk, tx);
                cut = cut || tx.cut;
                // rz_denoise_guides' record of the high pixel
                const int word = found ? min(max(h.mat, 0), K.nMaterials - 1) : -1;
                const float4 g0 = found ? make_float4(h.n.x, h.n.y, h.n.z, h.t) : make_float4(0.0f, 0.0f, 0.0f, 1e30f);
                const float4 g1 = found ? make_float4(h.p.x, h.p.y, h.p.z, __int_as_float(word))
                                        : make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
                uo = upscale_pixel<false>(U, X, Y, g0, g1, make_float4(1.0f, 1.0f, 1.0f, 0.0f));
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

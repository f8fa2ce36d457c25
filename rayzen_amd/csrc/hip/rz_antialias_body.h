// rz_antialias_body.h -- the steps of edge anti-aliasing, shared by its kernels so that they cannot drift apart:
//   rz_antialias_edges                (rz_antialias.hip)             CHAIN = false: first-hit records, 32 B (n, t | x, word)
//   rz_antialias_seethrough_classify  (rz_antialias_seethrough.hip)  CHAIN = true: chain records, 48 B (n, L | x, word | T, cls)
//   rz_antialias_seethrough_edges     (rz_antialias_seethrough.hip)  CHAIN = true
// The kernels keep the schedule: which wave classifies which unit (and the 3 x 3 loop itself), where the edge pixels wait (a queue
// in LDS, a segment in global memory) and which wave casts them.  DIFFERENT, EDGE and the edge pixel's mean are stated in
// include/rayzen_hip.h; binary32, one rounding per operation (tests/antialias_ref.py restates them bit for bit).  As in
// rz_upscale_body.h everything that differs sits behind `if constexpr (CHAIN)`: with CHAIN = false no third record word is
// loaded and no class is compared.
#pragma once
#include "rz_upscale_body.h"
#include "rz_pixel_cast.h"

namespace rz {

// is the neighbour q DIFFERENT from p?  (n_p, x_p, t_p, m_p, cls_p: p's record, t_p = L_p with CHAIN; ke = (float)(edge_plane f))
// Written without a branch, the records fetched whatever they hold: the eight neighbours' loads are then in flight together,
// where a test after every load would make them eight round trips to L2 one after the other.
template <bool CHAIN>
__device__ __forceinline__ bool aa_different(const AntialiasLaunch& A, size_t q, bool hitP, int wordP, int clsP, const v3 nP,
                                             const v3 xP, float tP) {
    constexpr int REC = CHAIN ? 3 : 2;
    const float4 h0 = A.U.guideLo[REC * q], h1 = A.U.guideLo[REC * q + 1];
    int clsQ = clsP;
    if constexpr (CHAIN) clsQ = __float_as_int(A.U.guideLo[REC * q + 2].w);
    const int wordQ = __float_as_int(h1.w);
    const bool hitQ = wordQ >= 0;
    const bool crease = dot(nP, mk3(h0.x, h0.y, h0.z)) < A.edgeNormal;
    const bool step = __builtin_fabsf(dot(nP, mk3(h1.x, h1.y, h1.z) - xP)) > A.edgePlane * tP;
    return (hitQ != hitP) | (clsQ != clsP) | (hitP & hitQ & ((wordQ != wordP) | crease | step));
}

// (The 3 x 3 loop around aa_different stays written out in rz_antialias_edges and rz_antialias_seethrough_classify: as a shared
// function it compiled to four batches of neighbour loads where the kernels have one, and both calls measured slower --
// profiles/offframe_shared/README.md.)

// Appends the unit's edge pixels to list[count ..] in lane order, by a ballot and a prefix count (the edge lanes below this
// one), and advances the wave-uniform count.  The caller keeps room for 64 more entries.
__device__ __forceinline__ void aa_append(int* list, int& count, bool edge, size_t p) {
    const unsigned long long m = rz_ballot(edge);
    const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (edge) list[count + before] = (int)p;
    count += mask_count(m);
}

// Sub-sample k = b s + a of pixel `pix`: the high pixel (X, Y) = (s x + a, s y + b) and the ray through its centre, bit for bit
// what rz_upscale casts at s w x s h.
__device__ __forceinline__ v3 aa_sub_pixel(const KParams& K, const UpscaleLaunch& U, int pix, int sa, int sb, int& X, int& Y) {
    const int y = pix / U.w, x = pix - y * U.w;
    X = U.s * x + sa;
    Y = U.s * y + sb;
    return pixel_centre_dir(K, X, Y, U.w * U.s, U.h * U.s);
}

// The mean of a group of ss consecutive lanes' uo, (((u_0 + u_1) + ...) + u_{ss - 1}) / ss -- b outer and a inner: the group's
// lanes in order -- summed through __shfl by every lane and written as pixel `pix` by the lanes with `first` (a group's first).
__device__ __forceinline__ void aa_store_mean(const UpscaleLaunch& U, const v3 uo, int lane, int ss, bool first, int pix) {
    v3 sum = uo;
    for (int j = 1; j < ss; ++j) {
        sum.x = sum.x + __shfl(uo.x, lane + j);
        sum.y = sum.y + __shfl(uo.y, lane + j);
        sum.z = sum.z + __shfl(uo.z, lane + j);
    }
    if (first) {
        const float inv = (float)ss;
        store_colour(U.dst, U.rgb, (size_t)pix, mk3(sum.x / inv, sum.y / inv, sum.z / inv), 1.0f);
    }
}

}  // namespace rz

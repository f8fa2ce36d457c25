// rz_query.h -- what the kernels that query the device scene outside a frame share (rz_rays.hip: rz_trace_rays /
// rz_shadow_rays; rz_editor.hip: rz_render_editor): their occupancy, the closest-hit query they run, their BLAS stack and
// the way a walk cut short at its backstop is reported.
#pragma once
#include "rz_trace.h"

namespace rz {

// One wave per workgroup; 4 waves per SIMD = 16 per CU, the occupancy the LDS budget of size_blas_stack is cut for.
#ifndef RZ_RAYS_MIN_WAVES
#define RZ_RAYS_MIN_WAVES 4
#endif

__device__ __forceinline__ void rays_backstop(unsigned* errWord, bool cut) {
    const unsigned long long m = rz_ballot(cut);
    if (m != 0ull && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicOr(errWord, RZ_BACKSTOP_RAYS);
}

template <bool OVF, bool SPREAD>
__device__ __forceinline__ bool ray_query(const KParams& K, v3 o, v3 d, HitRec& h, const BlasStackT<OVF>& bstk, TraceExtra& x) {
    Tally c = {};
    return SPREAD ? trace_spread<false, OVF, true>(K, o, d, h, bstk, c, &x) : trace_closest<false, OVF, true>(K, o, d, h, bstk, c, &x);
}

template <bool OVF>
__device__ __forceinline__ BlasStackT<OVF> rays_stack(const KParams& K, unsigned char* lds_raw) {
    const int lane = threadIdx.x & 63;
    return BlasStackT<OVF>{reinterpret_cast<uint2*>(lds_raw) + lane,
                           OVF ? K.blasOvf + ((size_t)blockIdx.x * K.blasOvfCap) * 64 + lane : nullptr, K.blasStackCap};
}

}  // namespace rz

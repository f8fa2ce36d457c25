// rz_query.h -- what the kernels that query the device scene outside a frame share (rz_rays.hip: rz_trace_rays /
// rz_shadow_rays; rz_editor.hip: rz_render_editor; the guide and antialias casts through rz_pixel_cast.h): their occupancy, the
// closest-hit query they run, their BLAS stack, the way a walk cut short at its backstop is reported and the rz_hit record.
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

// The transparency-aware visibility walk of FS:507-528 for the lanes with `run`, the whole wave in step (rz_shadow_rays_kernel,
// rz_ao_walks): up to 32 queries a ray.  A lane whose walk has ended stays out of the wave's further queries (the wave-uniform
// loop with a predicated body of the render's single trace call site).  Leaves (vis, lit) as rz_visibility states them; a lane
// without `run` keeps (1, false).  A query stopped at its backstop sets `cut`.
template <bool OVF, bool SPREAD>
__device__ __forceinline__ void shadow_walk(const KParams& K, v3 o, v3 d, float maxDist, bool run, const BlasStackT<OVF>& bstk,
                                            bool& cut, float& vis, bool& lit) {
    vis = 1.0f;
    lit = false;
    float traveled = 0.0f;
    int iter = 0;
    bool anyRun = rz_ballot(run) != 0ull;
    while (anyRun) {
        if (run) {
            HitRec h;
            TraceExtra x;
            const bool found = ray_query<OVF, SPREAD>(K, o, d, h, bstk, x);
            cut = cut || x.cut;
            bool done = false;
            if (!found) { done = true; lit = true; }                        // FS:514
            else if (h.t < 0.001f) { o = o + d * 0.001f; }                  // FS:515
            else {
                traveled += h.t;                                            // FS:516-517
                if (traveled >= maxDist) { done = true; lit = true; }
                else {
                    const float tr = K.materials[h.mat].transparency;       // FS:518-525
                    if (tr > 0.0f) { vis *= tr; o = h.p + d * 0.001f; }
                    else { vis = 0.0f; done = true; lit = false; }
                }
            }
            if (!done) {
                iter += 1;
                if (!(iter < 32 && vis > 0.05f)) { done = true; lit = vis > 0.05f; }    // FS:511, 527
            }
            run = !done;
        }
        anyRun = rz_ballot(run) != 0ull;
    }
}

// The rz_hit of a query, three 16-B stores at hits[3 i ..]: (t, point | normal, material | instance, triangle, prim, reserved).
// tri: the winner (TraceExtra::tri); t: the distance the record states -- h.t, or what the caller measured along its own ray
// (rz_editor_kernel past the near plane, the length of a see-through chain).  A miss: the shader's initial tHit (FS:459), ids
// -1, point and normal zero.
__device__ __forceinline__ void store_hit(const KParams& K, const int32_t* instTriOff, float4* hits, size_t i, bool found,
                                          const HitRec& h, int tri, float t) {
    float4 r0 = make_float4(1e30f, 0.0f, 0.0f, 0.0f);
    float4 r1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    float4 r2 = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), 0.0f);
    if (found) {
        const int prim = K.tris[tri].src;           // the winner's index in binding 0
        r0 = make_float4(t, h.p.x, h.p.y, h.p.z);
        r1 = make_float4(h.n.x, h.n.y, h.n.z, __int_as_float(h.mat));
        r2 = make_float4(__int_as_float(h.inst), __int_as_float(prim - instTriOff[h.inst]), __int_as_float(prim), 0.0f);
    }
    hits[3 * i] = r0;
    hits[3 * i + 1] = r1;
    hits[3 * i + 2] = r2;
}

template <bool OVF>
__device__ __forceinline__ BlasStackT<OVF> rays_stack(const KParams& K, unsigned char* lds_raw) {
    const int lane = threadIdx.x & 63;
    return BlasStackT<OVF>{reinterpret_cast<uint2*>(lds_raw) + lane,
                           OVF ? K.blasOvf + ((size_t)blockIdx.x * K.blasOvfCap) * 64 + lane : nullptr, K.blasStackCap};
}

}  // namespace rz

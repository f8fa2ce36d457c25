// rz_pixel_cast.h -- what the kernels that cast a pixel's own ray outside a frame share, so that a pixel, a guide record and a
// chain are the same bytes whichever pass asks (the tests compare them bit for bit):
//   pixel_centre_dir   rz_denoise_guides, rz_seethrough_guides, rz_editor_kernel, and the sub-pixels of rz_antialias_edges and
//                      rz_antialias_seethrough_edges (pixel (s x + a, s y + b) of the s w x s h image: what rz_upscale casts)
//   guide_record       the same kernels but the editor: (n, t | x, hit word)
//   cast_chain         rz_seethrough_guides and rz_antialias_seethrough_edges: the wave-uniform loop around ray_query
//                      (rz_query.h) and chain_step (rz_chain_step.h)
// The rz_hit record is store_hit of rz_query.h.  Binary32, one rounding per operation.
#pragma once
#include "rz_query.h"
#include "rz_path.h"
#include "rz_chain_step.h"

namespace rz {

// the ray through the centre of pixel (X, Y) of a W x H image (row 0 = the bottom row): gl_FragCoord.xy / resolution (FS:669)
__device__ __forceinline__ v3 pixel_centre_dir(const KParams& K, int X, int Y, int W, int H) {
    v2 uv;
    uv.x = ((float)X + 0.5f) / (float)W;
    uv.y = ((float)Y + 0.5f) / (float)H;
    return camera_ray_centre(K.invProj, K.invView, uv);
}

// the guide record of a query: (n, t) | (x, hit word = the clamped material index, -1 for a miss); t is h.t, or a chain's L
__device__ __forceinline__ void guide_record(const KParams& K, bool found, const HitRec& h, float t, float4& g0, float4& g1) {
    const int word = found ? min(max(h.mat, 0), K.nMaterials - 1) : -1;
    g0 = found ? make_float4(h.n.x, h.n.y, h.n.z, t) : make_float4(0.0f, 0.0f, 0.0f, 1e30f);
    g1 = found ? make_float4(h.p.x, h.p.y, h.p.z, __int_as_float(word)) : make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
}

// Where a see-through chain ended (include/rayzen_hip.h: "chain"): the final query's answer, its winning triangle, the
// transmittance, the length, the steps taken and the first material.
struct ChainEnd {
    bool found;
    HitRec h;
    int tri;
    v3 T;
    float L;
    int k, first;
    __device__ __forceinline__ int cls() const { return k == 0 ? 0 : first + 1; }
};

// The chain of (o, d) for the lanes with `run`, the whole wave in step: a wave-uniform loop that runs while a ballot says a lane
// is live -- at most maxDepth + 1 trips: a lane with k == maxDepth ends at its hit -- and a finished lane stays out of the query
// (the predicated body of rz_shadow_rays_kernel).  A walk stopped at its backstop sets `cut`.
template <bool OVF>
__device__ __forceinline__ ChainEnd cast_chain(const KParams& K, int maxDepth, v3 o, v3 d, bool run, const BlasStackT<OVF>& bstk,
                                               bool& cut) {
    float ior = 1.0f;
    ChainEnd e = {false, {}, 0, mk3(1.0f, 1.0f, 1.0f), 0.0f, 0, -1};
    while (rz_ballot(run) != 0ull) {
        if (run) {
            HitRec hq;
            TraceExtra x;
            e.found = ray_query<OVF, false>(K, o, d, hq, bstk, x);
            cut = cut || x.cut;
            run = false;
            if (e.found) {
                e.h = hq;
                e.tri = x.tri;
                run = chain_step(K, maxDepth, hq, o, d, e.T, ior, e.L, e.k, e.first);
            }
        }
    }
    return e;
}

}  // namespace rz

// rz_rays.hip -- batched ray queries on the device scene (include/rayzen_hip.h: rz_trace_rays, rz_shadow_rays).
//
// The render path is the only other user of the scene the context keeps on the device; these kernels ask it the two
// questions a caller outside the frame asks:
//   * rz_trace_rays_kernel: the closest hit of FS:457-503, one lane per ray, by the render's own query (rz_trace.h:
//     trace_closest, or trace_spread -- a scheduling choice, same bytes), plus the triangle that won (TraceExtra);
//   * rz_shadow_rays_kernel: the transparency-aware visibility walk of FS:507-528, one lane per ray, up to 32 queries a ray.
// Both run on a persistent grid of one-wave workgroups: each wave takes 64 consecutive rays per step of a grid-stride loop,
// reads a ray with two 16-B loads per lane and writes its result with three 16-B stores (a hit) or one 8-B store (a
// visibility).  The BLAS stack is an LDS window plus per-resident-wave overflow columns, sized by the render's rule
// (rz_context.hip: size_blas_stack).  Nothing of the render state -- accumulation, currentIor, pools, the claim counter -- is
// touched; a walk that stops at its backstop sets RZ_BACKSTOP_RAYS in the context's backstop word, as the render kernels do.
// The rz_hit record is store_hit of rz_query.h, which every pass that returns one calls.
#include <algorithm>

#include "rz_internal.h"
#include "rz_query.h"

namespace rz {

// rays: n x rz_ray (2 float4: origin, max_dist | dir, reserved); hits: n x rz_hit (3 float4: t, point | normal, material |
// instance, triangle, prim, reserved); instTriOff: globalTriOffset of every instance (rz_bvh_instance)
template <bool OVF, bool SPREAD>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_trace_rays_kernel(const KParams K, const float4* __restrict__ rays,
                                                                               float4* __restrict__ hits, const int n,
                                                                               const int32_t* __restrict__ instTriOff, unsigned* errWord) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    const int lane = threadIdx.x & 63;
    bool cut = false;
    for (long long base = (long long)blockIdx.x * 64; base < n; base += (long long)gridDim.x * 64) {
        const long long i = base + lane;
        if (i < n) {
            const float4 a = rays[2 * i], b = rays[2 * i + 1];
            HitRec h;
            TraceExtra x;
            const bool found = ray_query<OVF, SPREAD>(K, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), h, bstk, x);
            cut = cut || x.cut;
            store_hit(K, instTriOff, hits, (size_t)i, found, h, x.tri, h.t);
        }
    }
    rays_backstop(errWord, cut);
}

// FS:507-528 per ray: origin, max_dist | dir.  out: n x rz_visibility (visibility, lit).  The walk is shadow_walk (rz_query.h),
// which rz_ao_walks calls too.
template <bool OVF, bool SPREAD>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_shadow_rays_kernel(const KParams K, const float4* __restrict__ rays,
                                                                                float2* __restrict__ out, const int n, unsigned* errWord) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    const int lane = threadIdx.x & 63;
    bool cut = false;
    for (long long base = (long long)blockIdx.x * 64; base < n; base += (long long)gridDim.x * 64) {
        const long long i = base + lane;
        bool run = i < n;
        v3 o = mk3(0.0f, 0.0f, 0.0f), d = o;
        float maxDist = 0.0f;
        if (run) {
            const float4 a = rays[2 * i], b = rays[2 * i + 1];
            o = mk3(a.x, a.y, a.z);
            maxDist = a.w;
            d = mk3(b.x, b.y, b.z);
        }
        float vis;
        bool lit;
        shadow_walk<OVF, SPREAD>(K, o, d, maxDist, run, bstk, cut, vis, lit);
        if (i < n) out[i] = make_float2(vis, __int_as_float(lit ? 1 : 0));
    }
    rays_backstop(errWord, cut);
}

long long rays_grid(long long n) {
    static int nCU = 0;
    if (nCU == 0) {
        int dev = 0; hipDeviceProp_t prop;
        nCU = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                  ? prop.multiProcessorCount : 256;
    }
    return std::min<long long>((n + 63) / 64, (long long)nCU * RZ_RAYS_WAVES_PER_CU);
}

void launch_rays(const KParams& K, const RaysLaunch& R, hipStream_t stream) {
    const dim3 g((unsigned)R.grid), b(64);
    const size_t lds = (size_t)K.blasStackCap * 64 * sizeof(uint2);
    const bool ovf = K.blasOvfCap > 0;
    const float4* rays = static_cast<const float4*>(R.rays);
#define RZ_LAUNCH_RAYS(O, S)                                                                                                        \
    do {                                                                                                                            \
        if (R.shadow) hipLaunchKernelGGL((rz_shadow_rays_kernel<O, S>), g, b, lds, stream, K, rays, static_cast<float2*>(R.out),  \
                                         R.n, R.errWord);                                                                           \
        else hipLaunchKernelGGL((rz_trace_rays_kernel<O, S>), g, b, lds, stream, K, rays, static_cast<float4*>(R.out), R.n,        \
                                R.instTriOff, R.errWord);                                                                           \
    } while (0)
    if (ovf) { if (R.spread) RZ_LAUNCH_RAYS(true, true); else RZ_LAUNCH_RAYS(true, false); }
    else { if (R.spread) RZ_LAUNCH_RAYS(false, true); else RZ_LAUNCH_RAYS(false, false); }
#undef RZ_LAUNCH_RAYS
}

}  // namespace rz

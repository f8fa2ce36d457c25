// rz_cost.hip -- where a frame is expensive: the per-pixel traversal cost map (rz_render_cost, rz_cost_view, rz_present_cost).
// Compile with --offload-arch=gfx950 -ffp-contract=off.  Plain C++ HIP.
//
//   rz_cost_pixels          one lane per pixel, one wave per 8x8 tile: rz_render_pixels<true>'s launch shape, LDS stack and path
//                           loop (rz_path.h: begin_sample / advance, rz_trace.h: trace_closest, all counting) over samples
//                           0 .. spp-1 of every pixel from currentIor 1 and colour 0.  It reads and writes no accumulation or ior
//                           buffer and throws the colour away; what it keeps is the lane's Tally, which rz_render_pixels<true>
//                           dissolves into the frame's counters: its eight traversal-side counts go out as the pixel's
//                           rz_pixel_cost (two 16-B stores), and all of it is added to a DevCounters block, so the block holds
//                           what rz_render_counted reports for the frame at sample_base 0.  A TLAS walk cut at its backstop sets
//                           RZ_BACKSTOP_RAYS in the context's backstop word, as the ray-casting passes do.
//   rz_cost_reduce_partials the metric's maximum, the lowest pixel index that attains it and its sum over a strided share of
//                           the pixels, per workgroup;
//   rz_cost_reduce_final    ... over the partial records: the rz_cost_stats of the frame.  Integers throughout and an order on
//                           (value, index) that does not depend on who arrives first: the same bytes every time.
//   rz_cost_view            one lane per pixel, 64x4 workgroups as rz_denoise_resolve: the metric's value as a false colour
//                           (include/rayzen_hip.h states the ramp; tests/cost_ref.py restates it in np.float32).
#include <hip/hip_runtime.h>

#include "rayzen_hip.h"
#include "rz_path.h"
#include "rz_query.h"
#include "rz_internal.h"

namespace rz {

__global__ __launch_bounds__(WAVES_PER_BLOCK * 64, RZ_MIN_WAVES_PER_SIMD) void rz_cost_pixels(const KParams K, const CostLaunch C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const size_t perWave = (size_t)K.blasStackCap * 64 * sizeof(uint2) + (size_t)K.tlasStackCap * 64 * sizeof(int);
    unsigned char* base = lds_raw + perWave * wave;
    const BlasStackT<false> bstk{reinterpret_cast<uint2*>(base) + lane, nullptr, K.blasStackCap};

    const int localTile = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (localTile >= K.nLocalTiles) return;
    const int tile = localTile * K.tileNRanks + K.tileRank;
    const int tx = tile % K.tilesX, ty = tile / K.tilesX;
    const int px = tx * RZ_TILE_W + (lane & 7), py = ty * RZ_TILE_H + (lane >> 3);
    const bool inside = px < K.width && py < K.height;
    const size_t pix = (size_t)py * K.width + px;

    Tally c = {};
    Path P;
    P.mode = MODE_DONE;
    P.samp = 0;
    P.sampEnd = inside ? K.spp : 0;
    if (inside) {
        const float fragx = (float)px + 0.5f, fragy = (float)py + 0.5f;
        P.uv.x = fragx / (float)K.width;
        P.uv.y = fragy / (float)K.height;
        P.fragSum = fragx + fragy;
        P.color = mk3(0.0f, 0.0f, 0.0f);
        P.ior = 1.0f;
    }
    bool cut = false;
    while (P.samp < P.sampEnd) {
        if (P.mode == MODE_DONE) begin_sample<true>(K, P, c);
        HitRec h;
        TraceExtra x;
        const bool found = trace_closest<true, false, true>(K, P.o, P.d, h, bstk, c, &x);
        cut = cut || x.cut;
        advance<true>(K, P, found, h, c);
    }
    if (inside) {
        C.cost[2 * pix] = make_uint4(c.traversals, c.tlas_nodes, c.tlas_leaf_indices, c.instances);
        C.cost[2 * pix + 1] = make_uint4(c.blas_nodes, c.triangles, c.materials, c.light_fetches);
    }
    // the wave's tallies to the call's counters: DevCounters is an array of 64-bit words in this order, `pixels` is word 9
    const unsigned v[14] = {c.samples, c.traversals, c.tlas_nodes, c.tlas_leaf_indices, c.instances, c.blas_nodes,
                            c.triangles, c.materials, c.light_fetches, c.scatters, c.diffuse_scatters, c.hemi_draws, c.lit_lights, c.triangles_past_u};
    unsigned long long* g = reinterpret_cast<unsigned long long*>(K.counters);
    for (int k = 0; k < 14; ++k) {
        unsigned s = v[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0 && s) atomicAdd(&g[k < 9 ? k : k + 1], (unsigned long long)s);
    }
    const unsigned long long im = rz_ballot(inside);
    if (lane == 0 && im) atomicAdd(&g[9], (unsigned long long)__popcll(im));
    rays_backstop(C.errWord, cut);
}

// The value of a pixel under a metric (include/rayzen_hip.h): 0 the reference's bytes (SURVEY.md section 8d, 16 for the pixel
// itself), 1 node visits, 2 triangle tests, 3 traversals, 4 instances entered.
__device__ __forceinline__ unsigned long long cost_value(const uint4 a, const uint4 b, int metric) {
    switch (metric) {
        case 0:
            return 32ull * a.y + 4ull * a.z + 144ull * a.w + 32ull * b.x + 68ull * b.y + 32ull * b.z + 32ull * b.w + 16ull;
        case 1: return (unsigned long long)a.y + b.x;
        case 2: return b.y;
        case 3: return a.x;
        default: return a.w;
    }
}

// (value, index) pairs are ordered by value, then by the LOWER index: a total order, so any reduction tree gives one answer
__device__ __forceinline__ void cost_better(unsigned long long& m, unsigned long long& mi, unsigned long long v, unsigned long long i) {
    if (v > m || (v == m && i < mi)) { m = v; mi = i; }
}

// 256 lanes' (maximum, index, sum) -> lane 0's, through LDS
__device__ __forceinline__ void cost_block_reduce(unsigned long long& m, unsigned long long& mi, unsigned long long& s) {
    __shared__ unsigned long long sm[256], si[256], ss[256];
    const int t = threadIdx.x;
    sm[t] = m; si[t] = mi; ss[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            cost_better(m, mi, sm[t + o], si[t + o]);
            s += ss[t + o];
            sm[t] = m; si[t] = mi; ss[t] = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void rz_cost_reduce_partials(const CostReduceLaunch R) {
    unsigned long long m = 0ull, mi = ~0ull, s = 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < R.n; i += (long long)R.blocks * 256) {
        const unsigned long long v = cost_value(R.cost[2 * i], R.cost[2 * i + 1], R.metric);
        cost_better(m, mi, v, (unsigned long long)i);
        s += v;
    }
    cost_block_reduce(m, mi, s);
    if (threadIdx.x == 0) {
        unsigned long long* p = R.partials + 3 * (size_t)blockIdx.x;
        p[0] = m; p[1] = mi; p[2] = s;
    }
}

__global__ __launch_bounds__(256) void rz_cost_reduce_final(const CostReduceLaunch R) {
    unsigned long long m = 0ull, mi = ~0ull, s = 0ull;
    for (int b = threadIdx.x; b < R.blocks; b += 256) {
        const unsigned long long* p = R.partials + 3 * (size_t)b;
        cost_better(m, mi, p[0], p[1]);
        s += p[2];
    }
    cost_block_reduce(m, mi, s);
    if (threadIdx.x == 0) {
        rz_cost_stats o;
        o.max_value = m;
        o.sum_value = s;
        o.max_x = (int32_t)(mi % (unsigned long long)R.width);
        o.max_y = (int32_t)(mi / (unsigned long long)R.width);
        o.scale_used = R.scale > 0.0f ? R.scale : (m > 0ull ? (float)m : 1.0f);
        o.reserved = 0;
        *R.stats = o;
    }
}

__global__ __launch_bounds__(256) void rz_cost_view(const CostViewLaunch V) {
    const int px = blockIdx.x * 64 + threadIdx.x, py = blockIdx.y * 4 + threadIdx.y;
    if (px >= V.width || py >= V.height) return;
    const size_t p = (size_t)py * V.width + px;
    const float S = V.stats->scale_used;
    const float fv = (float)cost_value(V.cost[2 * p], V.cost[2 * p + 1], V.metric);
    v3 c = mk3(1.0f, 1.0f, 1.0f);               // above the top of the ramp: only a caller's scale can be
    if (!(fv > S)) {
        const float u = V.curve == 0 ? fminf(fv / S, 1.0f) : fminf(log2f(1.0f + fv) / log2f(1.0f + S), 1.0f);
        const float u4 = u * 4.0f;
        const int k = min((int)u4, 3);
        const float w = u4 - (float)k;
        // stops (0,0,0) (0,0,1) (0,1,0) (1,1,0) (1,0,0): a_k and a_{k+1} - a_k per channel
        const float ar = k == 3 ? 1.0f : 0.0f, dr = k == 2 ? 1.0f : 0.0f;
        const float ag = k >= 2 ? 1.0f : 0.0f, dg = k == 1 ? 1.0f : (k == 3 ? -1.0f : 0.0f);
        const float ab = k == 1 ? 1.0f : 0.0f, db = k == 0 ? 1.0f : (k == 1 ? -1.0f : 0.0f);
        c = mk3(ar + dr * w, ag + dg * w, ab + db * w);
    }
    store_colour(V.dst, V.rgb, p, c, 1.0f);
}

void launch_cost_pixels(const KParams& K, const CostLaunch& C, hipStream_t stream) {
    const int blocks = (K.nLocalTiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks <= 0) return;
    const size_t perWave = (size_t)K.blasStackCap * 64 * sizeof(uint2) + (size_t)K.tlasStackCap * 64 * sizeof(int);
    hipLaunchKernelGGL(rz_cost_pixels, dim3(blocks), dim3(WAVES_PER_BLOCK * 64), perWave * WAVES_PER_BLOCK, stream, K, C);
}

// four pixels per lane before a second workgroup is worth its partial record
int cost_reduce_blocks(long long n) {
    const long long b = (n + 1023) / 1024;
    return (int)(b < 1 ? 1 : (b > RZ_COST_REDUCE_BLOCKS ? RZ_COST_REDUCE_BLOCKS : b));
}

void launch_cost_reduce(const CostReduceLaunch& R, hipStream_t stream) {
    hipLaunchKernelGGL(rz_cost_reduce_partials, dim3(R.blocks), dim3(256), 0, stream, R);
    hipLaunchKernelGGL(rz_cost_reduce_final, dim3(1), dim3(256), 0, stream, R);
}

void launch_cost_view(const CostViewLaunch& V, hipStream_t stream) {
    const dim3 g((unsigned)((V.width + 63) / 64), (unsigned)((V.height + 3) / 4)), b(64, 4);
    hipLaunchKernelGGL(rz_cost_view, g, b, 0, stream, V);
}

}  // namespace rz

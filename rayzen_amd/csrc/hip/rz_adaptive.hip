// rz_adaptive.hip -- the metering pass of rz_render_adaptive (include/rayzen_hip.h states it operation by operation;
// tests/adaptive_ref.py restates it in np.float32).  Compile with --offload-arch=gfx950 -ffp-contract=off.  Plain C++ HIP.
//
//   rz_adaptive_meter   one lane per pixel, one wave per 8 x 8 tile (rz_cost_pixels' tile shape), over the tiles the batch just
//                       rendered (a list; batch 1: every tile).  A lane reads its pixel of the accumulation (16 B) and, after
//                       batch 1, its prev (16 B) and moments (8 B), updates both and gives the tile its e and |m|; two xor
//                       butterflies over the wave's lanes sum them, lane 0 writes the tile's E, its batch count and its flags.
//                       prev and the moments are the context's own, so they are kept tile by tile: lane l of tile t at t * 64
//                       + l, a wave's loads and stores are whole lines.  No LDS, no atomics: the same bytes on every run.
#include <hip/hip_runtime.h>

#include "rayzen_hip.h"
#include "rz_internal.h"

namespace rz {

__global__ __launch_bounds__(256) void rz_adaptive_meter(const AdaptiveMeterLaunch A) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= A.nSlots) return;
    const int tile = A.tiles ? A.tiles[slot] : slot;
    const int tx = tile % A.tilesX, ty = tile / A.tilesX;
    const int px = tx * RZ_TILE_W + (lane & 7), py = ty * RZ_TILE_H + (lane >> 3);
    const bool inside = px < A.width && py < A.height;
    const size_t own = (size_t)tile * 64 + lane;

    float e = 0.0f, am = 0.0f;
    if (inside) {
        const float4 I = A.accum[(size_t)py * A.width + px];
        float4 prev = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float2 S = make_float2(0.0f, 0.0f);
        if (A.batch > 1) {
            prev = A.prev[own];
            S = A.moments[own];
        }
        const float fs = (float)A.spp, fB = (float)A.batch;
        const float dr = (I.x - prev.x) / fs, dg = (I.y - prev.y) / fs, db = (I.z - prev.z) / fs;
        const float L = (0.2126f * dr + 0.7152f * dg) + 0.0722f * db;
        S.x = S.x + L;
        S.y = S.y + L * L;
        A.prev[own] = I;
        A.moments[own] = S;
        const float m = S.x / fB;
        if (A.batch >= 2) {
            const float x = (S.y - S.x * m) / (float)(A.batch - 1);
            const float v = x > 0.0f ? x : (x != x ? x : 0.0f);
            e = __builtin_sqrtf(v / fB);
        }
        am = __builtin_fabsf(m);
    }
    for (int o = 32; o > 0; o >>= 1) {
        e = e + __shfl_xor(e, o);
        am = am + __shfl_xor(am, o);
    }
    if (lane != 0) return;
    const int nx = min(RZ_TILE_W, A.width - tx * RZ_TILE_W), ny = min(RZ_TILE_H, A.height - ty * RZ_TILE_H);
    const float den = am + A.floor * (float)(nx * ny);
    const float E = e / den;
    const int received = (A.batch > 1 ? A.tileBatches[tile] : 0) + 1;
    const bool wasActive = A.batch > 1 ? (A.tileFlags[tile] & RZ_ADAPTIVE_ACTIVE) != 0 : true;
    const bool active = wasActive && !(A.batch >= A.minBatches && E <= A.threshold);
    A.tileError[tile] = E;
    A.tileBatches[tile] = received;
    A.tileFlags[tile] = (uint8_t)((active ? RZ_ADAPTIVE_ACTIVE : 0) | (received == A.batch ? RZ_ADAPTIVE_CURRENT : 0));
}

void launch_adaptive_meter(const AdaptiveMeterLaunch& A, hipStream_t stream) {
    if (A.nSlots <= 0) return;
    hipLaunchKernelGGL(rz_adaptive_meter, dim3((unsigned)((A.nSlots + 3) / 4)), dim3(256), 0, stream, A);
}

}  // namespace rz

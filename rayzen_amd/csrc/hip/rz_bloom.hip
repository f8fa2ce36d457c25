// rz_bloom.hip -- HDR glare in front of the display stage (rz_bloom / rz_present_bloomed; include/rayzen_hip.h, "Glare"):
//   rz_bloom_down<SRC>  a workgroup of 256 lanes makes 16 x 16 texels of the next pyramid level: the 34 x 34 source texels it
//                       needs are staged in LDS (indices clamped there), the row pass of the (1, 3, 3, 1) filter goes into a
//                       second LDS array and the column pass reads that.  SRC 0: the rgb frame, prefiltered at staging; SRC 1:
//                       the RGBA32F accumulation, resolved and prefiltered at staging; SRC 2: a pyramid level.
//   rz_bloom_up         one lane per texel of level k: four taps of U_{k+1} and its own D_k; writes U_k in place of D_k.
//   rz_bloom_combine    one lane per pixel: the last Up fused with the normalisation and the add; rgb32f / glare / (colour, 1).
// Pyramid texels are float4 (the fourth lane is 0 and never read).  The rgb frame is staged as the flat run of floats a tile row
// is -- lane i loads float i of the row, whatever the base's alignment -- so one form serves a 16-byte and a 4-byte aligned base.
// Numerics: binary32 as written (-ffp-contract=off), one rounding per operation.
#include <hip/hip_runtime.h>

#include "rayzen_hip.h"
#include "rz_device_math.h"
#include "rz_internal.h"

namespace rz {

namespace {

constexpr int kTile = 16;                   // outputs per workgroup and axis
constexpr int kSrc = 2 * kTile + 2;         // source texels per axis: 2X - 1 .. 2X + 2 for X = 0 .. 15
constexpr int kSrcRow = kSrc * 3;           // floats of a staged row
// pitches in floats.  The row pass reads a half-wave's texels 6 floats apart in two rows: an odd pitch puts the second row on
// the odd banks.  The column pass reads two output rows 2 * kRowPitch apart, 3 floats apart within one: 8 mod 16 interleaves them.
constexpr int kSrcPitch = kSrcRow + 1;
constexpr int kRowPitch = 56;
constexpr int kDownBlock = 256;

__device__ __forceinline__ v3 resolve4(const float4 a) {
    const float n = a.w > 0.0f ? a.w : 1.0f;
    return mk3(a.x / n, a.y / n, a.z / n);
}

// step 2 of the definition
__device__ __forceinline__ v3 prefilter(v3 c, float threshold, float knee, float limit) {
    if (nonfinite_(c)) return mk3(0.0f, 0.0f, 0.0f);
    const float r = c.x > 0.0f ? c.x : 0.0f, g = c.y > 0.0f ? c.y : 0.0f, bl = c.z > 0.0f ? c.z : 0.0f;
    const float b = fmax_(fmax_(r, g), bl);
    const float d = b - threshold;
    const float s = fmin_(fmax_(d + knee, 0.0f), 2.0f * knee);
    const float q = knee > 0.0f ? (s * s) / (4.0f * knee) : 0.0f;
    const float m = fmin_(fmax_(q, d), limit);
    const float f = m > 0.0f ? m / fmax_(b, 1e-4f) : 0.0f;
    return mk3(r * f, g * f, bl * f);
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ((t0 + 3 t1) + 3 t2) + t3
__device__ __forceinline__ float taps4(float t0, float t1, float t2, float t3) { return ((t0 + 3.0f * t1) + 3.0f * t2) + t3; }

template <int SRC>
__global__ __launch_bounds__(kDownBlock) void rz_bloom_down(const BloomDown K) {
    __shared__ float src[kSrc * kSrcPitch];
    __shared__ float rows[kSrc * kRowPitch];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * (2 * kTile) - 1, y0 = (int)blockIdx.y * (2 * kTile) - 1;
    if (SRC == 0) {
        for (int i = tid; i < kSrc * kSrcRow; i += kDownBlock) {
            const int row = i / kSrcRow, j = i - row * kSrcRow;
            const int px = j / 3, ch = j - px * 3;
            const int sx = clampi(x0 + px, K.sw - 1), sy = clampi(y0 + row, K.sh - 1);
            src[row * kSrcPitch + j] = K.rgb[((long long)sy * K.sw + sx) * 3 + ch];
        }
        __syncthreads();
        for (int t = tid; t < kSrc * kSrc; t += kDownBlock) {
            const int row = t / kSrc, px = t - row * kSrc;
            float* a = &src[row * kSrcPitch + px * 3];
            const v3 p = prefilter(mk3(a[0], a[1], a[2]), K.threshold, K.knee, K.limit);
            a[0] = p.x; a[1] = p.y; a[2] = p.z;
        }
    } else {
        for (int t = tid; t < kSrc * kSrc; t += kDownBlock) {
            const int row = t / kSrc, px = t - row * kSrc;
            const int sx = clampi(x0 + px, K.sw - 1), sy = clampi(y0 + row, K.sh - 1);
            const float4 v = K.src4[(long long)sy * K.sw + sx];
            const v3 p = SRC == 1 ? prefilter(resolve4(v), K.threshold, K.knee, K.limit) : mk3(v.x, v.y, v.z);
            float* a = &src[row * kSrcPitch + px * 3];
            a[0] = p.x; a[1] = p.y; a[2] = p.z;
        }
    }
    __syncthreads();
    // rows first: every staged row, the 16 outputs of the tile
    for (int i = tid; i < kSrc * kTile; i += kDownBlock) {
        const int row = i / kTile, ox = i - row * kTile;
        const float* a = &src[row * kSrcPitch + ox * 6];
        float* r = &rows[row * kRowPitch + ox * 3];
        r[0] = taps4(a[0], a[3], a[6], a[9]);
        r[1] = taps4(a[1], a[4], a[7], a[10]);
        r[2] = taps4(a[2], a[5], a[8], a[11]);
    }
    __syncthreads();
    const int ox = tid & (kTile - 1), oy = tid / kTile;
    const int X = (int)blockIdx.x * kTile + ox, Y = (int)blockIdx.y * kTile + oy;
    if (X >= K.dw || Y >= K.dh) return;
    const float* r = &rows[(2 * oy) * kRowPitch + ox * 3];
    K.dst[(long long)Y * K.dw + X] =
        make_float4(taps4(r[0], r[kRowPitch], r[2 * kRowPitch], r[3 * kRowPitch]) * 0.015625f,
                    taps4(r[1], r[kRowPitch + 1], r[2 * kRowPitch + 1], r[3 * kRowPitch + 1]) * 0.015625f,
                    taps4(r[2], r[kRowPitch + 2], r[2 * kRowPitch + 2], r[3 * kRowPitch + 2]) * 0.015625f, 0.0f);
}

// step 4 of the definition at texel (x, y) of the fine image: S is cw x ch
__device__ __forceinline__ v3 upsample(const float4* __restrict__ S, int cw, int ch, int x, int y) {
    const int nx = x >> 1, ny = y >> 1;
    const int fx = (x & 1) ? (nx + 1 < cw ? nx + 1 : cw - 1) : (nx > 0 ? nx - 1 : 0);
    const int fy = (y & 1) ? (ny + 1 < ch ? ny + 1 : ch - 1) : (ny > 0 ? ny - 1 : 0);
    const float4 nn = S[(long long)ny * cw + nx], nf = S[(long long)ny * cw + fx];
    const float4 fn = S[(long long)fy * cw + nx], ff = S[(long long)fy * cw + fx];
    const v3 rn = mk3(3.0f * nn.x + nf.x, 3.0f * nn.y + nf.y, 3.0f * nn.z + nf.z);
    const v3 rf = mk3(3.0f * fn.x + ff.x, 3.0f * fn.y + ff.y, 3.0f * fn.z + ff.z);
    return mk3((3.0f * rn.x + rf.x) * 0.0625f, (3.0f * rn.y + rf.y) * 0.0625f, (3.0f * rn.z + rf.z) * 0.0625f);
}

// (a wave is 64 texels of one row: its coarse taps are 33 neighbours of two rows)
__global__ __launch_bounds__(256) void rz_bloom_up(const BloomUp U) {
    const int x = (int)(blockIdx.x * 64 + threadIdx.x), y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (x >= U.w || y >= U.h) return;
    const v3 up = upsample(U.coarse, U.cw, U.ch, x, y);
    float4* t = &U.fine[(long long)y * U.w + x];
    const float4 d = *t;
    *t = make_float4(d.x + U.spread * up.x, d.y + U.spread * up.y, d.z + U.spread * up.z, 0.0f);
}

// (C.rgb may be C.in and C.out4 may be C.in4: a lane reads its pixel before it writes it, and no other lane touches it)
__global__ __launch_bounds__(256) void rz_bloom_combine(const BloomCombine C) {
    const int x = (int)(blockIdx.x * 64 + threadIdx.x), y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (x >= C.w || y >= C.h) return;
    const long long i = (long long)y * C.w + x;
    v3 c;
    if (C.in4) c = resolve4(C.in4[i]);
    else c = mk3(C.in[3 * i], C.in[3 * i + 1], C.in[3 * i + 2]);
    v3 g = mk3(0.0f, 0.0f, 0.0f);
    if (C.u0) {
        const v3 up = upsample(C.u0, C.cw, C.ch, x, y);
        g = mk3(up.x * C.n, up.y * C.n, up.z * C.n);
    }
    const v3 o = C.copy ? c : mk3(c.x + C.intensity * g.x, c.y + C.intensity * g.y, c.z + C.intensity * g.z);
    if (C.glare) { C.glare[3 * i] = g.x; C.glare[3 * i + 1] = g.y; C.glare[3 * i + 2] = g.z; }
    if (C.rgb) { C.rgb[3 * i] = o.x; C.rgb[3 * i + 1] = o.y; C.rgb[3 * i + 2] = o.z; }
    if (C.out4) C.out4[i] = make_float4(o.x, o.y, o.z, 1.0f);
}

}  // namespace

void launch_bloom_down(const BloomDown& K, hipStream_t s) {
    const dim3 grid((unsigned)((K.dw + kTile - 1) / kTile), (unsigned)((K.dh + kTile - 1) / kTile));
    if (K.rgb) hipLaunchKernelGGL(rz_bloom_down<0>, grid, dim3(kDownBlock), 0, s, K);
    else if (K.prefilter) hipLaunchKernelGGL(rz_bloom_down<1>, grid, dim3(kDownBlock), 0, s, K);
    else hipLaunchKernelGGL(rz_bloom_down<2>, grid, dim3(kDownBlock), 0, s, K);
}

void launch_bloom_up(const BloomUp& U, hipStream_t s) {
    hipLaunchKernelGGL(rz_bloom_up, dim3((unsigned)((U.w + 63) / 64), (unsigned)((U.h + 3) / 4)), dim3(64, 4), 0, s, U);
}

void launch_bloom_combine(const BloomCombine& C, hipStream_t s) {
    hipLaunchKernelGGL(rz_bloom_combine, dim3((unsigned)((C.w + 63) / 64), (unsigned)((C.h + 3) / 4)), dim3(64, 4), 0, s, C);
}

}  // namespace rz

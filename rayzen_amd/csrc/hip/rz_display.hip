// rz_display.hip -- the HDR display stage (rz_display / rz_present_display; include/rayzen_hip.h, "Display transform"):
//   rz_display_meter   the luminance histogram of the frame: 128 bins over [2^-16, 2^16) read off the float's bit pattern,
//                      plus `below` and `above`.  Integer counts, integer atomics: exact and independent of scheduling.
//   rz_display_expose  one wave: the trimmed log-average (binary64), the target exposure and the adaptation step; writes the
//                      exposure and the rz_display_info record into the context's device state, clears the working histogram.
//   rz_display_tone    one lane per pixel: exposure, tone curve, clamp, transfer; rgb32f / rgba8 / (colour, 1).
// The reference has no such stage (its shader clamps: FS:772-773); with exposure 1, curve 0 and transfer 0 the tone kernel
// computes clamp_(c * 1) and rz_present_kernel on its (colour, 1) output reproduces rz_present's bytes.
// Numerics: binary32 as written (-ffp-contract=off), binary64 where the header says so.
#include <hip/hip_runtime.h>

#include "rayzen_hip.h"
#include "rz_device_math.h"
#include "rz_internal.h"

namespace rz {

namespace {

constexpr int kBins = RZ_DISPLAY_BINS;              // + below at kBins, above at kBins + 1
constexpr int kCounters = RZ_DISPLAY_BINS + 2;
constexpr int kMeterBlock = 256;
constexpr int kAggregateRounds = 4;

__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// step 2 of the definition: the counter a luminance lands in
__device__ __forceinline__ int meter_bin(float l) {
    const unsigned u = __float_as_uint(l);
    const int b = (int)(u >> 21) - 444;
    if ((u >> 31) != 0u || b < 0) return kBins;
    return b > kBins - 1 ? kBins + 1 : b;
}

// One counter per lane (bin < 0: none) into the workgroup's LDS counters.  A frame is mostly a few bins (sky, a flat wall), so
// most lanes of a wave name the same address: the lanes that share the first active lane's bin are counted with one ballot and
// added by that lane, a few rounds of that, then plain LDS atomics for whoever is left.
__device__ __forceinline__ void count_wave(unsigned* counters, int bin) {
    const int lane = (int)(threadIdx.x & 63u);
    for (int round = 0; round < kAggregateRounds; ++round) {
        const unsigned long long active = __ballot(bin >= 0);
        if (active == 0ull) return;
        const int leader = __ffsll((long long)active) - 1;
        const int lb = __shfl(bin, leader);
        const unsigned long long same = __ballot(bin == lb);
        if (lane == leader) atomicAdd(&counters[lb], (unsigned)__popcll(same));
        if (bin == lb) bin = -1;
    }
    if (bin >= 0) atomicAdd(&counters[bin], 1u);
}

__device__ __forceinline__ float3 resolve4(const float4 a) {
    const float n = a.w > 0.0f ? a.w : 1.0f;
    return make_float3(a.x / n, a.y / n, a.z / n);
}

// FORM 0: rgb, 3 floats per pixel; base 16-byte aligned: four pixels per lane as three 16-byte loads.
// FORM 1: rgb, 3 floats per pixel, scalar loads (a base that is only 4-byte aligned).
// FORM 2: RGBA32F sum and count, one 16-byte load per pixel.
template <int FORM>
__global__ __launch_bounds__(kMeterBlock) void rz_display_meter(const float* __restrict__ in, long long n, unsigned* __restrict__ hist) {
    __shared__ unsigned counters[kCounters];
    for (int k = (int)threadIdx.x; k < kCounters; k += kMeterBlock) counters[k] = 0u;
    __syncthreads();
    const long long tid = (long long)blockIdx.x * kMeterBlock + threadIdx.x;
    const long long stride = (long long)gridDim.x * kMeterBlock;
    if (FORM == 0) {
        const long long groups = n >> 2;            // whole groups of four pixels = 12 floats = 3 float4
        const long long rounds = (groups + stride - 1) / stride;        // every lane of a wave runs the same number of rounds
        const float4* in4 = reinterpret_cast<const float4*>(in);
        for (long long r = 0; r < rounds; ++r) {
            const long long g = r * stride + tid;
            int b0 = -1, b1 = -1, b2 = -1, b3 = -1;
            if (g < groups) {
                const float4 p = in4[3 * g], q = in4[3 * g + 1], s = in4[3 * g + 2];
                b0 = meter_bin(luminance(p.x, p.y, p.z));
                b1 = meter_bin(luminance(p.w, q.x, q.y));
                b2 = meter_bin(luminance(q.z, q.w, s.x));
                b3 = meter_bin(luminance(s.y, s.z, s.w));
            }
            count_wave(counters, b0);
            count_wave(counters, b1);
            count_wave(counters, b2);
            count_wave(counters, b3);
        }
        // the last n % 4 pixels: the first lanes of workgroup 0
        const long long i = (groups << 2) + tid;
        if (blockIdx.x == 0 && threadIdx.x < 64u)
            count_wave(counters, i < n ? meter_bin(luminance(in[3 * i], in[3 * i + 1], in[3 * i + 2])) : -1);
    } else {
        const long long rounds = (n + stride - 1) / stride;
        for (long long r = 0; r < rounds; ++r) {
            const long long i = r * stride + tid;
            int b = -1;
            if (i < n) {
                if (FORM == 1) {
                    b = meter_bin(luminance(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
                } else {
                    const float3 c = resolve4(reinterpret_cast<const float4*>(in)[i]);
                    b = meter_bin(luminance(c.x, c.y, c.z));
                }
            }
            count_wave(counters, b);
        }
    }
    __syncthreads();
    for (int k = (int)threadIdx.x; k < kCounters; k += kMeterBlock) {
        const unsigned v = counters[k];
        if (v != 0u) atomicAdd(&hist[k], v);
    }
}

// log2 mid-points of the four bins of an octave: (log2(1 + m/4) + log2(1 + (m+1)/4)) / 2
__device__ const double kBinMid[4] = {0x1.49a784bcd1b8bp-3, 0x1.d053f6d260896p-2, 0x1.646eea247c5c2p-1, 0x1.ceaecfea8085ap-1};

// One wave.  mode 0: a manual call that commits `manual` as the exposure.  mode 1: an auto call (steps 3 and 4); writes this
// call's exposure to S->call and, unless keep, commits it with the rz_display_info record; clears the working histogram.
__global__ __launch_bounds__(64) void rz_display_expose(DisplayState* __restrict__ S, const DisplayExpose X) {
    __shared__ unsigned h[kCounters];
    const int lane = (int)threadIdx.x;
    if (X.mode == 0) {
        if (lane == 0) {
            S->exposure = X.manual;
            S->have = 1u;
            S->info.exposure = X.manual;
            S->info.target = X.manual;
            S->info.log2_mean = 0.0f;
        }
        return;
    }
    for (int k = lane; k < kCounters; k += 64) {
        h[k] = S->work[k];
        S->work[k] = 0u;
    }
    __syncthreads();
    if (!X.keep)
        for (int k = lane; k < kBins; k += 64) S->info.histogram[k] = h[k];
    if (lane != 0) return;
    long long N = 0;
    for (int b = 0; b < kBins; ++b) N += (long long)h[b];
    const float prev = S->have ? S->exposure : 1.0f;
    float E = prev, T = prev, mean = 0.0f;
    if (N > 0) {
        const long long lo = N * (long long)X.lowPermille / 1000, hi = N - N * (long long)X.highPermille / 1000;
        const long long K = hi - lo;
        long long C = 0, I = 0, M[4] = {0, 0, 0, 0};
        for (int b = 0; b < kBins; ++b) {
            const long long C1 = C + (long long)h[b];
            const long long top = C1 < hi ? C1 : hi, bottom = C > lo ? C : lo;
            const long long kept = top > bottom ? top - bottom : 0;
            I += kept * (long long)(b >> 2);
            M[b & 3] += kept;
            C = C1;
        }
        const double dK = (double)K;
        const double log2Mean = (double)I / dK - 16.0 +
                                ((((double)M[0] * kBinMid[0] + (double)M[1] * kBinMid[1]) + (double)M[2] * kBinMid[2]) + (double)M[3] * kBinMid[3]) / dK;
        const float t = (float)((double)X.key / exp2(log2Mean));
        T = t < X.minExposure ? X.minExposure : (t > X.maxExposure ? X.maxExposure : t);
        E = (!S->have || X.adapt == 1.0f) ? T : prev + X.adapt * (T - prev);
        mean = (float)log2Mean;
    }
    S->call = E;
    if (!X.keep) {
        if (N > 0) { S->exposure = E; S->have = 1u; }
        S->info.exposure = E;
        S->info.target = T;
        S->info.log2_mean = mean;
        S->info.counted = (unsigned)N;
        S->info.below = h[kBins];
        S->info.above = h[kBins + 1];
    }
}

__device__ __forceinline__ float tone_channel(float c, float E, int curve, float white2, int transfer) {
    float x = c * E, y = x;
    if (curve == 1) {
        x = fmax_(x, 0.0f);
        y = (x * (1.0f + x / white2)) / (1.0f + x);
    } else if (curve == 2) {
        x = fmax_(x, 0.0f);
        y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    }
    y = clamp_(y, 0.0f, 1.0f);
    if (transfer == 1) y = y <= 0.0031308f ? 12.92f * y : 1.055f * powf(y, 1.0f / 2.4f) - 0.055f;
    return y;
}

// (T.rgb may be T.in and T.out4 may be T.in4: a lane reads its pixel before it writes it, and no other lane touches it)
__global__ __launch_bounds__(256) void rz_display_tone(const DisplayTone T) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T.n) return;
    float3 c;
    if (T.in4) c = resolve4(T.in4[i]);
    else c = make_float3(T.in[3 * i], T.in[3 * i + 1], T.in[3 * i + 2]);
    const float E = T.state ? T.state->call : T.exposure;
    const float r = tone_channel(c.x, E, T.curve, T.white2, T.transfer), g = tone_channel(c.y, E, T.curve, T.white2, T.transfer),
                b = tone_channel(c.z, E, T.curve, T.white2, T.transfer);
    if (T.rgb) { T.rgb[3 * i] = r; T.rgb[3 * i + 1] = g; T.rgb[3 * i + 2] = b; }
    if (T.out4) T.out4[i] = make_float4(r, g, b, 1.0f);
    if (T.rgba8)
        T.rgba8[i] = make_uchar4((unsigned char)__builtin_rintf(clamp_(r, 0.0f, 1.0f) * 255.0f),
                                 (unsigned char)__builtin_rintf(clamp_(g, 0.0f, 1.0f) * 255.0f),
                                 (unsigned char)__builtin_rintf(clamp_(b, 0.0f, 1.0f) * 255.0f), 255);
}

}  // namespace

void launch_display_meter(const float* rgb, const float4* rgba, long long n, DisplayState* S, hipStream_t s) {
    unsigned* hist = S->work;       // (an address computed on the host, never read there)
    // four pixels per lane and workgroup round in the vector form, one in the others; enough workgroups to fill the device and
    // few enough that the flush stays a handful of atomics per bin
    const int form = rgba ? 2 : ((reinterpret_cast<uintptr_t>(rgb) & 15u) == 0 ? 0 : 1);
    const long long items = form == 0 ? (n >> 2) : n;
    long long grid = (items + kMeterBlock - 1) / kMeterBlock;
    grid = grid < 1 ? 1 : (grid > 1024 ? 1024 : grid);
    if (form == 0) hipLaunchKernelGGL(rz_display_meter<0>, dim3((unsigned)grid), dim3(kMeterBlock), 0, s, rgb, n, hist);
    else if (form == 1) hipLaunchKernelGGL(rz_display_meter<1>, dim3((unsigned)grid), dim3(kMeterBlock), 0, s, rgb, n, hist);
    else hipLaunchKernelGGL(rz_display_meter<2>, dim3((unsigned)grid), dim3(kMeterBlock), 0, s, reinterpret_cast<const float*>(rgba), n, hist);
}

void launch_display_expose(DisplayState* S, const DisplayExpose& X, hipStream_t s) {
    hipLaunchKernelGGL(rz_display_expose, dim3(1), dim3(64), 0, s, S, X);
}

void launch_display_tone(const DisplayTone& T, hipStream_t s) {
    hipLaunchKernelGGL(rz_display_tone, dim3((unsigned)((T.n + 255) / 256)), dim3(256), 0, s, T);
}

}  // namespace rz

// rz_temporal.hip -- temporal accumulation by reprojection and a variance-guided a-trous filter (SVGF: Schied et al., HPG 2017)
// for the one-sample frame of a moving camera and moving instances (include/rayzen_hip.h: rz_denoise_temporal /
// rz_present_temporal).  Like rz_denoise.hip it sits beside the render path: it reads the accumulation (or a caller buffer in
// the same form) and the device scene, and writes buffers of its own.  The guide is rz_denoise_guides' (launch_denoise_guides,
// unchanged): its rz_hit records are the history's guide, its 32-B records feed the filter.
//
//   rz_temporal_instances   one lane per instance: copies the instance's transform pair (the first 96 B of DevInstance) into the
//                           history being written and flags the instances whose transform equals the stored one bit for bit.
//   rz_temporal_accumulate  one lane per pixel, 64 x 4 pixels per workgroup: resolves and demodulates the pixel, reprojects it
//                           into the previous frame (through the instance's previous transform), gathers the (up to) four
//                           bilinear taps of the previous guide, colour and moments, and blends.  Writes the new colour | N and
//                           the new moments; K = 0: the outputs too.  A sample with a NaN or infinite channel is replaced by
//                           the reprojected history colour (black without one) before the blend: what is stored is finite.
//   rz_temporal_variance    one lane per pixel: the variance the filter is guided by -- the temporal one where N >= 4 (two loads,
//                           one store: the steady state), a 7 x 7 spatial estimate elsewhere (a fresh history only) -- as the .w
//                           of the filter's input (colour | variance), and the stats.
//   rz_temporal_atrous      rz_denoise_atrous with the colour weight replaced by the luminance weight under the 3 x 3-filtered
//                           variance; the variance rides in the colour's .w, so a tap moves the same 48 B.  LAST re-modulates and
//                           writes the outputs.  (No FIRST variant: the accumulate kernel has resolved and demodulated already.)
//
// The arithmetic, operation by operation, is stated in include/rayzen_hip.h; tests/temporal_ref.py restates it in binary64.
#include "rz_internal.h"
#include "rz_query.h"
#include "rz_path.h"

namespace rz {

__global__ __launch_bounds__(64) void rz_temporal_instances(const DevInstance* inst, const float* prev, float* next, int* same,
                                                            int n, int havePrev) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* cur = inst[i].inv;             // inv[12] then fwd[12]: 24 contiguous floats
    bool eq = havePrev != 0;
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        const float v = cur[k];
        next[24 * i + k] = v;
        if (havePrev && k >= 12) eq = eq && __float_as_uint(v) == __float_as_uint(prev[24 * i + k]);
    }
    same[i] = eq ? 1 : 0;
}

__device__ __forceinline__ float lum_of(v3 d) { return (0.2126f * d.x + 0.7152f * d.y) + 0.0722f * d.z; }
// m: a 3 x 4 matrix as DevInstance packs it (columns 0..3, rows 0..2)
__device__ __forceinline__ v3 affine_point(const float* m, v3 p) {
    return mk3(((m[0] * p.x + m[3] * p.y) + m[6] * p.z) + m[9], ((m[1] * p.x + m[4] * p.y) + m[7] * p.z) + m[10],
               ((m[2] * p.x + m[5] * p.y) + m[8] * p.z) + m[11]);
}
// mat3(transpose(m)) * v: the dot products with m's columns
__device__ __forceinline__ v3 transposed_dir(const float* m, v3 v) {
    return mk3(dot(mk3(m[0], m[1], m[2]), v), dot(mk3(m[3], m[4], m[5]), v), dot(mk3(m[6], m[7], m[8]), v));
}

__global__ __launch_bounds__(256) void rz_temporal_accumulate(const TemporalLaunch T) {
    const int px = blockIdx.x * 64 + threadIdx.x, py = blockIdx.y * 4 + threadIdx.y;
    if (px >= T.width || py >= T.height) return;
    const size_t p = (size_t)py * T.width + px;
    const float4 a4 = T.accum[p];
    const float cnt = a4.w > 0.0f ? a4.w : 1.0f;
    const v3 c = mk3(a4.x / cnt, a4.y / cnt, a4.z / cnt);
    const float4 h0 = T.hits[3 * p], h1 = T.hits[3 * p + 1], h2 = T.hits[3 * p + 2];
    const int inst = __float_as_int(h2.x);
    const bool hit = inst >= 0;
    v3 al = mk3(1.0f, 1.0f, 1.0f);
    if (hit) {
        const DevMaterial& m = T.materials[min(max(__float_as_int(h1.w), 0), T.nMaterials - 1)];
        al = mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
    }
    v3 d = c;
    if (T.demodulate && hit) d = mk3(c.x / fmax_(al.x, 1e-3f), c.y / fmax_(al.y, 1e-3f), c.z / fmax_(al.z, 1e-3f));
    float l = lum_of(d);

    // ---- the history: reprojection, the taps
    float S = 0.0f, nH = 0.0f, n0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    v3 dH = mk3(0.0f, 0.0f, 0.0f);
    if (T.havePrev) {
        v3 xq = mk3(h0.y, h0.z, h0.w), nq = mk3(h1.x, h1.y, h1.z);      // x', n'
        bool still = T.cameraSame != 0;
        float w4 = 0.0f;                    // x' as a homogeneous point: w = 1 for a hit, 0 for a miss's direction
        if (hit) {
            w4 = 1.0f;
            if (!T.instSame[inst]) {
                still = false;
                const DevInstance& I = T.instances[inst];
                const float* P = T.instPrev + 24 * (size_t)inst;        // inversePrev[12], transformPrev[12]
                const v3 o = affine_point(I.inv, xq);
                xq = affine_point(P + 12, o);
                const v3 b = transposed_dir(P, transposed_dir(I.fwd, nq));
                const float len = __builtin_sqrtf(dot(b, b));
                nq = mk3(b.x / len, b.y / len, b.z / len);
            }
        } else if (!still) {
            v2 uv;
            uv.x = ((float)px + 0.5f) / (float)T.width;
            uv.y = ((float)py + 0.5f) / (float)T.height;
            xq = camera_ray_centre(T.invProj, T.invView, uv);
        }
        float u = (float)px, v = (float)py;
        bool have = true;
        if (!still) {
            const float* V = T.viewPrev;
            const float* Pm = T.projPrev;
            float e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = ((V[k] * xq.x + V[4 + k] * xq.y) + V[8 + k] * xq.z) + V[12 + k] * w4;
            const float cx = ((Pm[0] * e[0] + Pm[4] * e[1]) + Pm[8] * e[2]) + Pm[12] * e[3];
            const float cy = ((Pm[1] * e[0] + Pm[5] * e[1]) + Pm[9] * e[2]) + Pm[13] * e[3];
            const float cw = ((Pm[3] * e[0] + Pm[7] * e[1]) + Pm[11] * e[2]) + Pm[15] * e[3];
            have = cw > 0.0f;
            u = (cx / cw * 0.5f + 0.5f) * (float)T.width - 0.5f;
            v = (cy / cw * 0.5f + 0.5f) * (float)T.height - 0.5f;
            have = have && u > -1.0f && u < (float)T.width && v > -1.0f && v < (float)T.height;    // (false for a NaN)
        }
        if (have) {
            const v3 cp = mk3(T.camPrev[0], T.camPrev[1], T.camPrev[2]);
            const v3 dc = xq - cp;
            const float planeMax = T.planeTol * __builtin_sqrtf(dot(dc, dc)) * T.fPrev;       // plane_tol t' f_prev
            const float fu = __builtin_floorf(u), fv = __builtin_floorf(v);
            const int x0 = (int)fu, y0 = (int)fv;
            const float fx = u - fu, fy = v - fv;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
                if (!(w > 0.0f) || qx < 0 || qx >= T.width || qy < 0 || qy >= T.height) continue;
                const size_t q = (size_t)qy * T.width + qx;
                const int instQ = __float_as_int(T.hitsPrev[3 * q + 2].x);
                if ((instQ >= 0) != hit) continue;
                if (hit) {
                    if (instQ != inst) continue;
                    const float4 q0 = T.hitsPrev[3 * q], q1 = T.hitsPrev[3 * q + 1];
                    if (!(dot(nq, mk3(q1.x, q1.y, q1.z)) >= T.normalCos)) continue;
                    if (!(__builtin_fabsf(dot(nq, mk3(q0.y, q0.z, q0.w) - xq)) <= planeMax)) continue;
                }
                const float4 cq = T.colPrev[q];
                const float2 mq = T.momPrev[q];
                if (S == 0.0f) n0 = cq.w;          // the first counted tap's N: taps of one length give that length exactly
                S += w;
                dH = dH + mk3(cq.x, cq.y, cq.z) * w;
                nH += w * (cq.w - n0);
                m1 += w * mq.x;
                m2 += w * mq.y;
            }
        }
    }
    const bool accepted = S >= 0.01f;
    if (accepted) dH = mk3(dH.x / S, dH.y / S, dH.z / S);
    if (nonfinite_(c)) {        // a bad sample (NaN or Inf in c_p): the history's colour stands in for it, black without one
        d = accepted ? dH : mk3(0.0f, 0.0f, 0.0f);
        l = lum_of(d);
    }
    float N = 1.0f, M1 = l, M2 = l * l;
    v3 D = d;
    if (accepted) {
        nH = n0 + nH / S; m1 = m1 / S; m2 = m2 / S;
        N = fmin_(nH + 1.0f, T.maxHistory);
        const float a = fmax_(T.alpha, 1.0f / N), am = fmax_(T.alphaMoments, 1.0f / N);
        D = mk3(dH.x + a * (d.x - dH.x), dH.y + a * (d.y - dH.y), dH.z + a * (d.z - dH.z));
        M1 = m1 + am * (l - m1);
        M2 = m2 + am * (l * l - m2);
    }
    T.colNext[p] = make_float4(D.x, D.y, D.z, N);
    T.momNext[p] = make_float2(M1, M2);
    if (T.dst || T.rgb) {       // K = 0: D alpha; a pixel without history returns c_p itself (rz_denoise's K = 0)
        v3 out = c;
        if (accepted) out = (T.demodulate && hit) ? mk3(D.x * al.x, D.y * al.y, D.z * al.z) : D;
        store_colour(T.dst, T.rgb, p, out, 1.0f);
    }
}

// W_geom of rz_denoise for the pair (p, q) at tap distance `dist` pixels (step 1): invPlane = 1 / (sigma_x t_p f)
__device__ __forceinline__ float geom_weight(v3 np_, v3 xp, float4 h0, float4 h1, float sigmaNormal, float invPlaneOverDist) {
    const float nd = fmax_(dot(np_, mk3(h0.x, h0.y, h0.z)), 0.0f);
    const float wn = nd > 0.0f ? __builtin_exp2f(sigmaNormal * __builtin_log2f(nd)) : (sigmaNormal == 0.0f ? 1.0f : 0.0f);
    const float pl = __builtin_fabsf(dot(np_, mk3(h1.x, h1.y, h1.z) - xp)) * invPlaneOverDist;
    return wn * __builtin_expf(-pl);
}

__global__ __launch_bounds__(256) void rz_temporal_variance(const TemporalVarLaunch V) {
    const int px = blockIdx.x * 64 + threadIdx.x, py = blockIdx.y * 4 + threadIdx.y;
    if (px >= V.width || py >= V.height) return;
    const size_t p = (size_t)py * V.width + px;
    const float4 cp = V.col[p];
    float var;
    if (cp.w >= 4.0f) {
        const float2 m = V.mom[p];
        var = fmax_(0.0f, m.y - m.x * m.x);
    } else {        // a young history: the weighted variance of D's luminance over 7 x 7, scaled by 4 / N
        const float4 g0 = V.guide[2 * p], g1 = V.guide[2 * p + 1];
        const bool hitP = __float_as_int(g1.w) >= 0;
        const v3 np_ = mk3(g0.x, g0.y, g0.z), xp = mk3(g1.x, g1.y, g1.z);
        const float invPlane = hitP ? V.planeScale / g0.w : 0.0f;
        const float lp = lum_of(mk3(cp.x, cp.y, cp.z));
        float sw = 1.0f, s1 = lp, s2 = lp * lp;
        for (int b = -3; b <= 3; ++b) {
            const int qy = py + b;
            if (qy < 0 || qy >= V.height) continue;
            for (int a = -3; a <= 3; ++a) {
                const int qx = px + a;
                if ((a == 0 && b == 0) || qx < 0 || qx >= V.width) continue;
                const size_t q = (size_t)qy * V.width + qx;
                const float4 h1 = V.guide[2 * q + 1];
                if ((__float_as_int(h1.w) >= 0) != hitP) continue;
                float w = 1.0f;
                if (hitP) {
                    const int dist = max(a < 0 ? -a : a, b < 0 ? -b : b);
                    w = geom_weight(np_, xp, V.guide[2 * q], h1, V.sigmaNormal, invPlane / (float)dist);
                }
                const float4 cq = V.col[q];
                const float lq = lum_of(mk3(cq.x, cq.y, cq.z));
                sw += w;
                s1 += w * lq;
                s2 += w * (lq * lq);
            }
        }
        const float mean = s1 / sw;
        var = fmax_(0.0f, s2 / sw - mean * mean) * (4.0f / cp.w);
    }
    if (V.dst) V.dst[p] = make_float4(cp.x, cp.y, cp.z, var);
    if (V.stats) {
        V.stats[2 * p] = cp.w;
        V.stats[2 * p + 1] = var;
    }
}

__device__ constexpr float tatrous_h(int a) { return a == 0 ? 0.375f : (a == 1 || a == -1 ? 0.25f : 0.0625f); }

template <bool LAST>
__global__ __launch_bounds__(256) void rz_temporal_atrous(const TemporalFilterLaunch F) {
    const int px = blockIdx.x * 64 + threadIdx.x, py = blockIdx.y * 4 + threadIdx.y;
    if (px >= F.width || py >= F.height) return;
    const size_t p = (size_t)py * F.width + px;
    const float4 g0 = F.guide[2 * p], g1 = F.guide[2 * p + 1];
    const int wordP = __float_as_int(g1.w);
    const bool hitP = wordP >= 0;
    const v3 np_ = mk3(g0.x, g0.y, g0.z), xp = mk3(g1.x, g1.y, g1.z);
    const float4 sp = F.src[p];
    const v3 dp = mk3(sp.x, sp.y, sp.z);
    const float lp = lum_of(dp);
    // g_p: the variance under the 3 x 3 Gaussian (1/4, 1/8, 1/16), renormalised over the taps inside the image
    float gs = 0.25f * sp.w, gw = 0.25f;
#pragma unroll
    for (int b = -1; b <= 1; ++b) {
        const int qy = py + b;
        if (qy < 0 || qy >= F.height) continue;
#pragma unroll
        for (int a = -1; a <= 1; ++a) {
            const int qx = px + a;
            if ((a == 0 && b == 0) || qx < 0 || qx >= F.width) continue;
            const float k = (a != 0 && b != 0) ? 0.0625f : 0.125f;
            gs += k * F.src[(size_t)qy * F.width + qx].w;
            gw += k;
        }
    }
    const float invLum = 1.0f / (F.sigmaL * __builtin_sqrtf(fmax_(gs / gw, 0.0f)) + 1e-8f);
    const float invPlane = hitP ? F.planeScale / g0.w : 0.0f;
    const float centre = tatrous_h(0) * tatrous_h(0);
    v3 num = dp * centre;
    float den = centre, vnum = (centre * centre) * sp.w;
#pragma unroll
    for (int b = -2; b <= 2; ++b) {
        const int qy = py + b * F.step;
        if (qy < 0 || qy >= F.height) continue;
#pragma unroll
        for (int a = -2; a <= 2; ++a) {
            if (a == 0 && b == 0) continue;
            const int qx = px + a * F.step;
            if (qx < 0 || qx >= F.width) continue;
            const size_t q = (size_t)qy * F.width + qx;
            const float4 h1 = F.guide[2 * q + 1];
            if ((__float_as_int(h1.w) >= 0) != hitP) continue;
            float w = tatrous_h(a) * tatrous_h(b);
            if (hitP) {
                const float m = (a == 2 || a == -2 || b == 2 || b == -2) ? 0.5f : 1.0f;       // 1 / max(|a|, |b|)
                w *= geom_weight(np_, xp, F.guide[2 * q], h1, F.sigmaNormal, invPlane * m);
            }
            const float4 sq = F.src[q];
            const v3 dq = mk3(sq.x, sq.y, sq.z);
            w *= __builtin_expf(-__builtin_fabsf(lp - lum_of(dq)) * invLum);
            num = num + dq * w;
            den += w;
            vnum += (w * w) * sq.w;
        }
    }
    v3 out = mk3(num.x / den, num.y / den, num.z / den);
    const float var = vnum / (den * den);
    if (LAST && F.demodulate && hitP) {
        const DevMaterial& m = F.materials[wordP];
        out = mk3(out.x * m.albedo[0], out.y * m.albedo[1], out.z * m.albedo[2]);
    }
    store_colour(F.dst, LAST ? F.rgb : nullptr, p, out, LAST ? 1.0f : var);
}

static dim3 pixel_grid(int w, int h) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)); }

void launch_temporal_instances(const DevInstance* inst, const float* prev, float* next, int* same, int n, bool havePrev, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(rz_temporal_instances, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, inst, prev, next, same, n, havePrev ? 1 : 0);
}
void launch_temporal_accumulate(const TemporalLaunch& T, hipStream_t stream) {
    hipLaunchKernelGGL(rz_temporal_accumulate, pixel_grid(T.width, T.height), dim3(64, 4), 0, stream, T);
}
void launch_temporal_variance(const TemporalVarLaunch& V, hipStream_t stream) {
    hipLaunchKernelGGL(rz_temporal_variance, pixel_grid(V.width, V.height), dim3(64, 4), 0, stream, V);
}
void launch_temporal_pass(const TemporalFilterLaunch& F, bool last, hipStream_t stream) {
    if (last) hipLaunchKernelGGL((rz_temporal_atrous<true>), pixel_grid(F.width, F.height), dim3(64, 4), 0, stream, F);
    else hipLaunchKernelGGL((rz_temporal_atrous<false>), pixel_grid(F.width, F.height), dim3(64, 4), 0, stream, F);
}

}  // namespace rz

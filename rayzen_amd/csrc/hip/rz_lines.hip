// rz_lines.hip -- depth-tested 3D lines blended over a presented image, in place (include/rayzen_hip.h: rz_draw_lines).  The
// kernels read the caller's lines, the instances' transforms and a hit image, and write the caller's images and a workspace of
// the context's; they touch no render state.
//
//   rz_lines_project    one lane per line: steps 1 to 4 of the header's definition.  It writes the projected record -- the screen
//                       end A_s with ab = B_s - A_s and L = |ab|^2 (what step 5 would compute per pixel, computed once with the
//                       same operations), ia and ib - ia, the colour -- and what the passes below cull with: the rectangle and
//                       the reach (LINE CULL below).  A dropped line gets the empty rectangle.
//   rz_lines_bin<FILL>  one workgroup per (cell of 128 x 128 pixels, segment of RZ_LINES_SEG lines).  It scans its segment in
//                       chunks of 256 and keeps the lines that can touch the cell, by a ballot and a prefix per wave: the count
//                       pass writes how many, rz_lines_scan takes the exclusive scan of the counts in (cell, segment) order, and
//                       the fill pass, the same scan of the same records, writes the indices behind its offset.  So a cell's
//                       list is contiguous, in ascending line index without a sort, has no fixed capacity and drops nothing.
//   rz_lines_draw       one workgroup of 32 x 8 lanes per 32 x 8 pixels.  A tile whose cell list is empty ends at once (two
//                       loads).  Otherwise it walks the list in chunks of 256, tests each line against the tile itself and stages
//                       the survivors' records in LDS, by ballot again so the order is kept; every lane then runs steps 5 to 7
//                       over the staged records with its pixel in registers: the pixel is loaded when the first line touches it,
//                       its hit record when the first line covers it, and it is written once, if touched.  Blending therefore
//                       runs in ascending line index per pixel, and the bytes are the same on every run.
//                       Without lists (LinesLaunch::list == nullptr: RZ_LINES_UNBINNED=1, the A/B form profiles/lines/ times)
//                       every tile walks all n records behind the rectangle test alone.
//
// LINE CULL.  With A_s, B_s the finite screen ends, per axis lo / hi their least / greatest coordinate and M = max(|lo|, |hi|):
//     g = (hw + 1) + M * 2^-21, plus 0.5 when smooth          (binary32, evaluated as written)
// and the rectangle is [lo - g, hi + g] per axis: project_box's guard (rz_present.hip, the comment above ProjBox, gives the
// derivation: the point c = A_s + t * ab a pixel is measured against lies within 3 M 2^-23 of the exact segment, the rest pays
// for the roundings around it) with the line's reach hw, or hw + 0.5, in the place of `thickness`.  A pixel outside it is not
// covered.  The rectangle of a long diagonal is most of the frame, so cells and tiles also measure the line itself: with
// (cx, cy) the middle of a cell's or tile's pixel centres, R a bound on the distance from there to any of them (90 for 128 x 128,
// 16 for 32 x 8) and d the distance step 5 computes for (cx, cy), the line is skipped iff d > R + reach,
//     reach = max(g_x, g_y) + max(M_x, M_y) * 2^-19.
// A covered pixel p has d_p < hw + 0.5, its point c_p lies within 3 M 2^-23 of the exact segment S, so dist(p, S) < hw + 0.5 +
// 3 M 2^-23 and dist((cx, cy), S) < R + that.  The d computed for (cx, cy) exceeds dist((cx, cy), S) by the error of its own t
// -- the quotient's numerator carries 2^-24 |pa| |ab| of rounding, which moves c by 2^-24 |pa| <= M 2^-22 (|pa| <= 2 M + R) --
// plus c's 3 M 2^-23 and the roundings of the distance: under M 2^-20 in all, where the reach allows M 2^-19 + M 2^-21 + 1.
// A NaN d fails the comparison and keeps the line.  tests/lines_ref.py restates both tests and tests/test_lines_abi.py holds
// them against 3 000 random lines whose ends lie up to 2^30 pixels off the frame.
#include "rz_internal.h"
#include "rz_device_math.h"

namespace rz {

constexpr int LN_TW = 32, LN_TH = 8;            // a tile of rz_lines_draw
constexpr int LN_CHUNK = 256;                   // records staged at a time = lanes of a workgroup
constexpr float LN_BIG = 3.0e38f;
constexpr float LN_CELL_R = 90.0f, LN_TILE_R = 16.0f;       // >= sqrt(2) * 63.5 and >= sqrt(15.5^2 + 3.5^2)
static_assert(sizeof(rz_line) == 32 && sizeof(rz_lines_params) == 32 && sizeof(rz_hit) == 48, "the records the kernels load as 16-byte words");
static_assert(RZ_LINES_CELL % LN_TW == 0 && RZ_LINES_CELL % LN_TH == 0, "a tile lies in one cell");

// Step 5's t and d for the point (fx, fy): g = (A_s.x, A_s.y, ab.x, ab.y), L = ab.x * ab.x + ab.y * ab.y.
__device__ __forceinline__ float ln_dist(float fx, float fy, const float4 g, float L, float& t) {
    const float pax = fx - g.x, pay = fy - g.y;
    t = L == 0.0f ? 0.0f : clamp_((pax * g.z + pay * g.w) / L, 0.0f, 1.0f);
    const float dx = fx - (g.x + t * g.z), dy = fy - (g.y + t * g.w);
    return __builtin_sqrtf(dx * dx + dy * dy);
}

// LINE CULL: can the line touch a pixel whose centre lies in [x0, x1] x [y0, y1]?  R: LN_CELL_R or LN_TILE_R; measure: the
// second test (off in the unbinned form).
__device__ __forceinline__ bool ln_meets(const float4 rect, const float4* geo, const float4* misc, const float* reach, int i,
                                         float x0, float y0, float x1, float y1, float R, bool measure) {
    if (rect.z < x0 || rect.x > x1 || rect.w < y0 || rect.y > y1) return false;
    if (!measure) return true;
    float t;
    const float d = ln_dist((x0 + x1) * 0.5f, (y0 + y1) * 0.5f, geo[i], misc[i].w, t);
    return !(d > R + reach[i]);
}

// the exclusive prefix of a kept lane among the kept lanes of its wave
__device__ __forceinline__ unsigned ln_prefix(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__global__ __launch_bounds__(256) void rz_lines_project(const LinesLaunch V) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= V.n) return;
    const uint4* line = static_cast<const uint4*>(V.lines) + 2 * (size_t)i;
    const uint4 la = line[0], lb = line[1];
    float ax = __uint_as_float(la.x), ay = __uint_as_float(la.y), az = __uint_as_float(la.z);
    float bx = __uint_as_float(lb.x), by = __uint_as_float(lb.y), bz = __uint_as_float(lb.z);
    const int inst = (int)lb.w;
    bool drop = false;
    if (inst >= 0) {                                            // step 1
        if (inst >= V.nInst) {
            drop = true;
        } else {
            const float* m = V.instances[inst].fwd;             // columns 0..3, rows 0..2; m4v's sums with w = 1
            const float x0 = ((m[0] * ax + m[3] * ay) + m[6] * az) + m[9] * 1.0f, y0 = ((m[1] * ax + m[4] * ay) + m[7] * az) + m[10] * 1.0f,
                        z0 = ((m[2] * ax + m[5] * ay) + m[8] * az) + m[11] * 1.0f;
            const float x1 = ((m[0] * bx + m[3] * by) + m[6] * bz) + m[9] * 1.0f, y1 = ((m[1] * bx + m[4] * by) + m[7] * bz) + m[10] * 1.0f,
                        z1 = ((m[2] * bx + m[5] * by) + m[8] * bz) + m[11] * 1.0f;
            ax = x0; ay = y0; az = z0; bx = x1; by = y1; bz = z1;
        }
    }
    const float* vp = V.viewProj;                               // step 2 (z is not used)
    float Ax = ((vp[0] * ax + vp[4] * ay) + vp[8] * az) + vp[12] * 1.0f, Ay = ((vp[1] * ax + vp[5] * ay) + vp[9] * az) + vp[13] * 1.0f,
          Aw = ((vp[3] * ax + vp[7] * ay) + vp[11] * az) + vp[15] * 1.0f;
    float Bx = ((vp[0] * bx + vp[4] * by) + vp[8] * bz) + vp[12] * 1.0f, By = ((vp[1] * bx + vp[5] * by) + vp[9] * bz) + vp[13] * 1.0f,
          Bw = ((vp[3] * bx + vp[7] * by) + vp[11] * bz) + vp[15] * 1.0f;
    const float nw = V.nearW;                                   // step 3
    const bool aok = Aw >= nw, bok = Bw >= nw;
    if (!aok && !bok) {
        drop = true;
    } else if (!aok) {
        const float k = (nw - Aw) / (Bw - Aw);
        Ax = Ax + k * (Bx - Ax); Ay = Ay + k * (By - Ay); Aw = nw;
    } else if (!bok) {
        const float k = (nw - Bw) / (Aw - Bw);
        Bx = Bx + k * (Ax - Bx); By = By + k * (Ay - By); Bw = nw;
    }
    const float resx = (float)V.width, resy = (float)V.height;  // step 4
    const float sax = (Ax / Aw * 0.5f + 0.5f) * resx, say = (Ay / Aw * 0.5f + 0.5f) * resy;
    const float sbx = (Bx / Bw * 0.5f + 0.5f) * resx, sby = (By / Bw * 0.5f + 0.5f) * resy;
    if (nonfinite_(sax) || nonfinite_(say) || nonfinite_(sbx) || nonfinite_(sby)) drop = true;
    if (drop) {
        V.rect[i] = make_float4(LN_BIG, LN_BIG, -LN_BIG, -LN_BIG);
        V.geo[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        V.misc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        V.reach[i] = 0.0f;
        return;
    }
    const float ia = 1.0f / Aw, ib = 1.0f / Bw;
    const float abx = sbx - sax, aby = sby - say;
    V.geo[i] = make_float4(sax, say, abx, aby);
    V.misc[i] = make_float4(ia, ib - ia, __uint_as_float(la.w), abx * abx + aby * aby);
    // LINE CULL
    const float lox = fmin_(sax, sbx), hix = fmax_(sax, sbx), loy = fmin_(say, sby), hiy = fmax_(say, sby);
    const float mx = fmax_(__builtin_fabsf(lox), __builtin_fabsf(hix)), my = fmax_(__builtin_fabsf(loy), __builtin_fabsf(hiy));
    float gx = (V.halfWidth + 1.0f) + mx * 0x1p-21f, gy = (V.halfWidth + 1.0f) + my * 0x1p-21f;
    if (V.smooth) { gx = gx + 0.5f; gy = gy + 0.5f; }
    V.rect[i] = make_float4(lox - gx, loy - gy, hix + gx, hiy + gy);
    V.reach[i] = fmax_(gx, gy) + fmax_(mx, my) * 0x1p-19f;
}

template <bool FILL>
__global__ __launch_bounds__(LN_CHUNK) void rz_lines_bin(const LinesLaunch V) {
    __shared__ unsigned wsum[LN_CHUNK / 64];
    const long long slot = blockIdx.x;                          // cell * nSeg + segment
    const int cell = (int)(slot / V.nSeg), seg = (int)(slot - (long long)cell * V.nSeg);
    const int cy = cell / V.cellsX, cx = cell - cy * V.cellsX;
    const float x0 = (float)(cx * RZ_LINES_CELL) + 0.5f, y0 = (float)(cy * RZ_LINES_CELL) + 0.5f;
    const float x1 = x0 + (float)(RZ_LINES_CELL - 1), y1 = y0 + (float)(RZ_LINES_CELL - 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int first = seg * RZ_LINES_SEG, last = min(V.n, first + RZ_LINES_SEG);
    int* out = FILL ? V.list + V.offsets[slot] : nullptr;
    unsigned base = 0;
    for (int c = first; c < last; c += LN_CHUNK) {
        const int i = c + (int)threadIdx.x;
        const bool keep = i < last && ln_meets(V.rect[i], V.geo, V.misc, V.reach, i, x0, y0, x1, y1, LN_CELL_R, true);
        const unsigned long long m = rz_ballot(keep);
        if (lane == 0) wsum[wave] = (unsigned)__builtin_popcountll(m);
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < LN_CHUNK / 64; ++w) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        if (FILL && keep) out[base + before + ln_prefix(m)] = i;
        base += total;
        __syncthreads();
    }
    if (!FILL && threadIdx.x == 0) V.counts[slot] = base;
}

// offsets[e] = counts[0] + ... + counts[e - 1] for e = 0 .. m: one workgroup, 256 counts at a time
__global__ __launch_bounds__(256) void rz_lines_scan(const unsigned* counts, unsigned long long* offsets, long long m) {
    __shared__ unsigned long long part[256];
    unsigned long long run = 0;
    for (long long c = 0; c < m; c += 256) {
        const long long e = c + threadIdx.x;
        const unsigned long long v = e < m ? counts[e] : 0ull;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned long long a = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0ull;
            __syncthreads();
            part[threadIdx.x] += a;
            __syncthreads();
        }
        if (e < m) offsets[e] = run + part[threadIdx.x] - v;
        run += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[m] = run;
}

__global__ __launch_bounds__(LN_TW * LN_TH) void rz_lines_draw(const LinesLaunch V) {
    __shared__ float4 sGeo[LN_CHUNK], sMisc[LN_CHUNK];
    __shared__ unsigned wsum[LN_CHUNK / 64];
    const int tileY = (int)(blockIdx.x / (unsigned)V.tilesX), tileX = (int)(blockIdx.x - (unsigned)tileY * (unsigned)V.tilesX);
    long long beg = 0, end = V.n;
    if (V.list) {
        const long long cell = (long long)(tileY / (RZ_LINES_CELL / LN_TH)) * V.cellsX + tileX / (RZ_LINES_CELL / LN_TW);
        beg = (long long)V.offsets[cell * V.nSeg];
        end = (long long)V.offsets[(cell + 1) * V.nSeg];
    }
    if (beg == end) return;
    const int tid = (int)(threadIdx.y * LN_TW + threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int px = tileX * LN_TW + (int)threadIdx.x, py = tileY * LN_TH + (int)threadIdx.y;
    const bool inside = px < V.width && py < V.height;
    const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
    const float tx0 = (float)(tileX * LN_TW) + 0.5f, ty0 = (float)(tileY * LN_TH) + 0.5f;
    const float tx1 = tx0 + (float)(LN_TW - 1), ty1 = ty0 + (float)(LN_TH - 1);
    const size_t p = (size_t)py * V.width + px;
    const float* vp = V.viewProj;
    bool touched = false, haveHit = false, isHit = false;
    float wh = 0.0f;
    float r = 0.0f, g = 0.0f, b = 0.0f, q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
    unsigned char qa = 0;
    for (long long c = beg; c < end; c += LN_CHUNK) {
        const long long e = c + tid;
        bool keep = false;
        int i = 0;
        if (e < end) {
            i = V.list ? V.list[e] : (int)e;
            keep = ln_meets(V.rect[i], V.geo, V.misc, V.reach, i, tx0, ty0, tx1, ty1, LN_TILE_R, V.list != nullptr);
        }
        const unsigned long long m = rz_ballot(keep);
        if (lane == 0) wsum[wave] = (unsigned)__builtin_popcountll(m);
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < LN_CHUNK / 64; ++w) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        if (keep) {
            const unsigned at = before + ln_prefix(m);
            sGeo[at] = V.geo[i];
            sMisc[at] = V.misc[i];
        }
        __syncthreads();
        if (inside) {
            for (unsigned k = 0; k < total; ++k) {
                const float4 ge = sGeo[k], mi = sMisc[k];
                float t;
                const float d = ln_dist(fx, fy, ge, mi.w, t);   // step 5
                float cov = 1.0f;
                if (V.smooth) {
                    cov = clamp_((V.halfWidth + 0.5f) - d, 0.0f, 1.0f);
                    if (!(cov > 0.0f)) continue;
                } else if (!(d < V.halfWidth)) {
                    continue;
                }
                const unsigned color = __float_as_uint(mi.z);   // step 6
                float alpha = (float)(color >> 24) / 255.0f;
                if (V.hits) {
                    if (!haveHit) {
                        const float4 h0 = V.hits[3 * p];
                        isHit = __float_as_int(V.hits[3 * p + 2].x) >= 0;
                        wh = ((vp[3] * h0.y + vp[7] * h0.z) + vp[11] * h0.w) + vp[15];
                        haveHit = true;
                    }
                    if (isHit) {
                        const float ws = 1.0f / (mi.x + t * mi.y);
                        if (ws * V.depthKeep > wh) alpha = alpha * V.hiddenAlpha;
                    }
                }
                alpha = alpha * cov;
                if (alpha == 0.0f) continue;
                if (!touched) {                                 // step 7
                    touched = true;
                    if (V.rgb) { r = V.rgb[3 * p]; g = V.rgb[3 * p + 1]; b = V.rgb[3 * p + 2]; }
                    if (V.rgba8) {
                        const uchar4 in = V.rgba8[p];
                        q0 = (float)in.x / 255.0f; q1 = (float)in.y / 255.0f; q2 = (float)in.z / 255.0f;
                        qa = in.w;
                    }
                }
                const float keepIn = 1.0f - alpha;
                const float cr = (float)(color & 255u) / 255.0f, cg = (float)((color >> 8) & 255u) / 255.0f,
                            cb = (float)((color >> 16) & 255u) / 255.0f;
                r = r * keepIn + cr * alpha; g = g * keepIn + cg * alpha; b = b * keepIn + cb * alpha;
                q0 = q0 * keepIn + cr * alpha; q1 = q1 * keepIn + cg * alpha; q2 = q2 * keepIn + cb * alpha;
            }
        }
        __syncthreads();
    }
    if (!touched) return;
    if (V.rgb) { V.rgb[3 * p] = r; V.rgb[3 * p + 1] = g; V.rgb[3 * p + 2] = b; }
    if (V.rgba8)
        V.rgba8[p] = make_uchar4((unsigned char)__builtin_rintf(clamp_(q0, 0.0f, 1.0f) * 255.0f),
                                 (unsigned char)__builtin_rintf(clamp_(q1, 0.0f, 1.0f) * 255.0f),
                                 (unsigned char)__builtin_rintf(clamp_(q2, 0.0f, 1.0f) * 255.0f), qa);
}

void launch_lines_project(const LinesLaunch& V, hipStream_t stream) {
    hipLaunchKernelGGL(rz_lines_project, dim3((unsigned)((V.n + 255) / 256)), dim3(256), 0, stream, V);
}

void launch_lines_count(const LinesLaunch& V, hipStream_t stream) {
    const long long slots = (long long)V.cells * V.nSeg;
    hipLaunchKernelGGL(rz_lines_bin<false>, dim3((unsigned)slots), dim3(LN_CHUNK), 0, stream, V);
    hipLaunchKernelGGL(rz_lines_scan, dim3(1), dim3(256), 0, stream, V.counts, V.offsets, slots);
}

void launch_lines_fill(const LinesLaunch& V, hipStream_t stream) {
    hipLaunchKernelGGL(rz_lines_bin<true>, dim3((unsigned)((long long)V.cells * V.nSeg)), dim3(LN_CHUNK), 0, stream, V);
}

void launch_lines_draw(LinesLaunch V, hipStream_t stream) {
    V.tilesX = (V.width + LN_TW - 1) / LN_TW;
    const dim3 grid((unsigned)V.tilesX * (unsigned)((V.height + LN_TH - 1) / LN_TH)), block(LN_TW, LN_TH);   // (one dimension: no 65535-row limit)
    hipLaunchKernelGGL(rz_lines_draw, grid, block, 0, stream, V);
}

}  // namespace rz

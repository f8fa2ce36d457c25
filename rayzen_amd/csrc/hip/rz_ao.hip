// rz_ao.hip -- distance-limited ambient occlusion for previews (include/rayzen_hip.h: rz_ambient_occlusion).  The render path
// does not change: these kernels read the device scene and a guide of the context's and write buffers of the caller's.
//
//   rz_denoise_guides   (rz_denoise.hip, as it stands) the pixel-centre cast: the 32-B guide record of every pixel, in a buffer of
//                       the context's.  The resolve kernel needs (n, x, t, hit) of a pixel's fifteen neighbours from memory
//                       anyway, so the records are written once and both kernels below read them.
//   rz_ao_walks         one wave per 8 x 8 tile, a persistent grid of one-wave workgroups.  The unit a wave takes is one trip of
//                       a tile (unit = tile * N + trip: a tile has at most N trips; a trip past the tile's last costs the guide
//                       read and ends), taken from one of 64 counters the call zeroes, each serving an interleaved share of
//                       the units and 1/64 of the waves; which wave walks which trip changes no byte.  The lanes of a tile are
//                       ordered by direction pattern (tile_x, tile_y).  A lane reads its pixel's guide, turns
//                       the normal against the ray (n_f) and lifts the hit point (o); a miss writes raw = 1 and is done.  The
//                       tile's H hit pixels are numbered by a ballot prefix and their records (o, n_f, the pixel's lane) go to
//                       LDS in that order, 32 B each.  The H N walks are then numbered pixel-major -- item k is sample k % N of
//                       hit pixel k / N -- and lane l of trip r takes item 64 r + l: every trip but the tile's last runs 64 live walks,
//                       however much sky the tile holds, and the N samples of a pixel sit in adjacent lanes of one trip because N
//                       divides 64.  The walk is shadow_walk (rz_query.h), the loop of rz_shadow_rays_kernel and the kernel's
//                       only ray_query call site.  tree(a) is then log2 N butterfly steps over lane distances 1, 2, 4, 8 -- lane
//                       2i adds lane 2i + 1 at every level, which is s[i] = s[2i] + s[2i + 1] -- and the pixel's first lane
//                       writes raw: no atomic touches a float, and no float lands in memory out of order.
//   rz_ao_resolve       32 x 8 pixels per workgroup.  SMOOTH: it stages raw and (n, x) of its tile and a halo of two pixels
//                       below / left and one above / right -- the 4 x 4 window that holds each of the 16 direction patterns
//                       once -- in LDS, raw = -1 standing for "outside the image or a miss" (raw itself is never negative),
//                       gathers the taps that pass the normal and plane tests, and divides.  Then it modulates and quantises.
//                       Without SMOOTH it reads raw_p alone.
// Binary32, one rounding per operation (the library is compiled without contraction); normalize is v / sqrt(dot(v, v)) with the
// correctly rounded quotient and root (rz_device_math.h).  The direction table is built on the host (ao_direction_table).
#include <cmath>

#include "rz_internal.h"
#include "rz_pixel_cast.h"

namespace rz {

// Marsaglia's sphere points from an R2 lattice (include/rayzen_hip.h: "direction table"): candidate k is accepted iff S < 1.
const float* ao_direction_table() {
    static const struct Table {
        float p[RZ_AO_DIRS * 3];
        Table() {
            int j = 0;
            for (uint32_t k = 1; j < RZ_AO_DIRS; ++k) {
                const uint32_t a = (k * 3242174889u) >> 8, b = (k * 2447445414u) >> 8;
                const float x1 = (float)a * 1.1920928955078125e-07f - 1.0f, x2 = (float)b * 1.1920928955078125e-07f - 1.0f;
                const float S = x1 * x1 + x2 * x2;
                if (!(S < 1.0f)) continue;
                const float q = std::sqrt(1.0f - S);
                p[3 * j] = (2.0f * x1) * q;
                p[3 * j + 1] = (2.0f * x2) * q;
                p[3 * j + 2] = 1.0f - 2.0f * S;
                ++j;
            }
        }
    } table;
    return table.p;
}

// Which pixel of its 8 x 8 tile a lane holds: the lanes are ordered by direction pattern, the four pixels of pattern l >> 2 --
// (x, y), (x + 4, y), (x, y + 4), (x + 4, y + 4) with x + 4 y = l >> 2 -- in adjacent lanes (a tile starts at multiples of 8, so
// the pattern of a pixel is that of its place in the tile).  A trip of 64 items then holds 16 / N patterns, at most 16 distinct
// directions shared by four lanes each -- what a run of 16 pixels of one row holds -- where row-major lanes held twice as many.
__device__ __forceinline__ int tile_x(int l) { return ((l >> 2) & 3) + 4 * (l & 1); }
__device__ __forceinline__ int tile_y(int l) { return (l >> 4) + 4 * ((l >> 1) & 1); }

template <bool OVF>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_ao_walks(const KParams K, const AoWalkLaunch A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    float4* rec = reinterpret_cast<float4*>(lds_raw + (size_t)K.blasStackCap * 64 * sizeof(uint2));     // 2 float4 per hit pixel
    const int lane = threadIdx.x & 63;
    const int mask = A.samples - 1;
    const float scale = 1.0f / (float)A.samples;
    bool cut = false;
    // Units are handed out in `counters` interleaved sequences (unit j C + k belongs to sequence k), sequence blockIdx.x % C to a
    // wave: from a counter per sequence the call zeroes (one integer atomic per unit and wave), or, counters == 0, one sequence
    // per wave and no atomic.  A unit is a tile, or with perTrip one trip of a tile (unit = tile * N + trip).  Why 64 counters
    // and trips (profiles/ao/README.md): a tile costs between nothing (sky) and N trips of some 50 us, so a wave with a fixed
    // share of eight tiles ends long after the others, and 4 096 waves at one counter queue there.
    const int perTile = A.perTrip ? A.samples : 1;
    const long long units = A.tiles * perTile;
    const long long C = A.counters > 0 ? A.counters : gridDim.x;
    const long long k = blockIdx.x % C;
    unsigned own = 0u;
    for (;;) {
        int next = (int)own++;
        if (A.counters > 0) {
            if (lane == 0) next = (int)atomicAdd(A.claim + k * 32, 1u);
            next = __builtin_amdgcn_readfirstlane(next);
        }
        const long long unit = (long long)(unsigned)next * C + k;
        if (unit >= units) break;
        const long long u = unit / perTile;
        const int trip = (int)(unit - u * perTile);
        const int ty = (int)(u / A.tilesX), tx = (int)(u - (long long)ty * A.tilesX);
        const int bx = tx * 8, by = ty * 8;
        const int px = bx + tile_x(lane), py = by + tile_y(lane);
        const bool inside = px < K.width && py < K.height;
        bool hit = false;
        v3 o = mk3(0.0f, 0.0f, 0.0f), nf = o;
        if (inside) {
            const size_t p = (size_t)py * K.width + px;
            const float4 g0 = A.guide[2 * p], g1 = A.guide[2 * p + 1];
            hit = __float_as_int(g1.w) >= 0;
            if (hit) {
                const v3 d = pixel_centre_dir(K, px, py, K.width, K.height);
                const v3 n = mk3(g0.x, g0.y, g0.z);
                nf = dot(n, d) > 0.0f ? -n : n;
                o = mk3(g1.x, g1.y, g1.z) + nf * 0.001f;
            } else if (trip == 0) {
                A.raw[p] = 1.0f;
            }
        }
        const unsigned long long hits = rz_ballot(hit);
        const int items = __builtin_popcountll(hits) << A.log2Samples;
        if (trip * 64 >= items) continue;
        if (hit) {
            const int slot = __builtin_popcountll(hits & ((1ull << lane) - 1ull));
            rec[2 * slot] = make_float4(o.x, o.y, o.z, nf.x);
            rec[2 * slot + 1] = make_float4(nf.y, nf.z, __int_as_float(lane), 0.0f);
        }
        __syncthreads();
        const int end = A.perTrip ? min(items, trip * 64 + 64) : items;
        for (int base = trip * 64; base < end; base += 64) {
            const int item = base + lane;
            bool run = item < items;
            int src = 0;
            v3 wo = mk3(0.0f, 0.0f, 0.0f), wd = wo;
            if (run) {
                const int slot = item >> A.log2Samples, i = item & mask;
                const float4 r0 = rec[2 * slot], r1 = rec[2 * slot + 1];
                src = __float_as_int(r1.z);
                const int c = ((bx + tile_x(src)) & 3) + 4 * ((by + tile_y(src)) & 3);
                const float* P = A.dirs + 3 * (16 * i + c);
                wo = mk3(r0.x, r0.y, r0.z);
                const v3 v = mk3(r0.w + P[0], r1.x + P[1], r1.y + P[2]);
                const float l2 = dot(v, v);
                if (l2 >= 1e-6f) wd = normalize(v);
                else run = false;               // a_i = 1, nothing walked (this also keeps NaN out of the walk)
            }
            const bool walked = run;
            float vis;
            bool lit;
            shadow_walk<OVF, false>(K, wo, wd, A.radius, run, bstk, cut, vis, lit);
            float a = walked ? (lit ? vis : 0.0f) : 1.0f;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1)
                if (off < A.samples) a = a + __shfl_xor(a, off, 64);
            if (item < items && (item & mask) == 0) A.raw[(size_t)(by + tile_y(src)) * K.width + bx + tile_x(src)] = a * scale;
        }
        __syncthreads();        // the records are read before the next tile's are written
    }
    rays_backstop(A.errWord, cut);
}

constexpr int AO_W = 32, AO_H = 8, AO_LO = 2, AO_HI = 1;        // the tile; taps a, b = -AO_LO .. AO_HI
constexpr int AO_SW = AO_W + AO_LO + AO_HI, AO_SH = AO_H + AO_LO + AO_HI;

template <bool SMOOTH>
__global__ __launch_bounds__(AO_W * AO_H) void rz_ao_resolve(const AoResolveLaunch R, const int tilesX) {
    __shared__ float sRaw[SMOOTH ? AO_SH : 1][SMOOTH ? AO_SW : 1];
    __shared__ float sG[SMOOTH ? 6 : 1][SMOOTH ? AO_SH : 1][SMOOTH ? AO_SW : 1];       // n.xyz, x.xyz
    const int tileY = (int)(blockIdx.x / (unsigned)tilesX), tileX = (int)(blockIdx.x - (unsigned)tileY * (unsigned)tilesX);
    const int bx = tileX * AO_W, by = tileY * AO_H;
    if (SMOOTH) {
        const int tid = threadIdx.y * AO_W + threadIdx.x;
        for (int e = tid; e < AO_SW * AO_SH; e += AO_W * AO_H) {
            const int sy = e / AO_SW, sx = e - sy * AO_SW;
            const int qx = bx + sx - AO_LO, qy = by + sy - AO_LO;
            float raw = -1.0f;
            float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0;
            if (qx >= 0 && qx < R.width && qy >= 0 && qy < R.height) {
                const size_t q = (size_t)qy * R.width + qx;
                g1 = R.guide[2 * q + 1];
                if (__float_as_int(g1.w) >= 0) {
                    g0 = R.guide[2 * q];
                    raw = R.raw[q];
                }
            }
            sRaw[sy][sx] = raw;
            sG[0][sy][sx] = g0.x; sG[1][sy][sx] = g0.y; sG[2][sy][sx] = g0.z;
            sG[3][sy][sx] = g1.x; sG[4][sy][sx] = g1.y; sG[5][sy][sx] = g1.z;
        }
        __syncthreads();
    }
    const int px = bx + threadIdx.x, py = by + threadIdx.y;
    if (px >= R.width || py >= R.height) return;
    const size_t p = (size_t)py * R.width + px;
    float ao;
    if (!SMOOTH) {
        ao = R.raw[p];
    } else {
        const int cx = threadIdx.x + AO_LO, cy = threadIdx.y + AO_LO;
        ao = 1.0f;
        if (sRaw[cy][cx] >= 0.0f) {
            const v3 np_ = mk3(sG[0][cy][cx], sG[1][cy][cx], sG[2][cy][cx]), xp = mk3(sG[3][cy][cx], sG[4][cy][cx], sG[5][cy][cx]);
            const float tol = (R.planeTol * R.guide[2 * p].w) * R.f;
            float sum = 0.0f;
            int count = 0;
#pragma unroll
            for (int b = -AO_LO; b <= AO_HI; ++b) {
#pragma unroll
                for (int a = -AO_LO; a <= AO_HI; ++a) {
                    const int qy = cy + b, qx = cx + a;
                    const float rq = sRaw[qy][qx];
                    if (!(rq >= 0.0f)) continue;
                    if (a != 0 || b != 0) {
                        const v3 nq = mk3(sG[0][qy][qx], sG[1][qy][qx], sG[2][qy][qx]), xq = mk3(sG[3][qy][qx], sG[4][qy][qx], sG[5][qy][qx]);
                        if (!(dot(np_, nq) >= R.normalCos)) continue;
                        const float m = (a == -2 || b == -2) ? 2.0f : 1.0f;        // max(|a|, |b|)
                        if (!(__builtin_fabsf(dot(np_, xq - xp)) <= tol * m)) continue;
                    }
                    sum += rq;
                    count += 1;
                }
            }
            ao = sum / (float)count;
        }
    }
    if (R.ao) R.ao[p] = ao;
    if (!R.rgb && !R.rgba8) return;
    const float m = 1.0f - R.strength * (1.0f - ao);
    v3 c = mk3(m, m, m);
    if (R.rgbIn) c = mk3(R.rgbIn[3 * p] * m, R.rgbIn[3 * p + 1] * m, R.rgbIn[3 * p + 2] * m);
    if (R.rgb) {
        R.rgb[3 * p] = c.x;
        R.rgb[3 * p + 1] = c.y;
        R.rgb[3 * p + 2] = c.z;
    }
    if (R.rgba8)
        R.rgba8[p] = make_uchar4((unsigned char)__builtin_rintf(clamp_(c.x, 0.0f, 1.0f) * 255.0f),
                                 (unsigned char)__builtin_rintf(clamp_(c.y, 0.0f, 1.0f) * 255.0f),
                                 (unsigned char)__builtin_rintf(clamp_(c.z, 0.0f, 1.0f) * 255.0f), 255);
}

void launch_ao_walks(const KParams& K, const AoWalkLaunch& A, hipStream_t stream) {
    const dim3 g((unsigned)A.grid), b(64);
    const size_t lds = (size_t)K.blasStackCap * 64 * sizeof(uint2) + RZ_AO_WALK_LDS;
    if (K.blasOvfCap > 0) hipLaunchKernelGGL((rz_ao_walks<true>), g, b, lds, stream, K, A);
    else hipLaunchKernelGGL((rz_ao_walks<false>), g, b, lds, stream, K, A);
}

void launch_ao_resolve(const AoResolveLaunch& R, bool smooth, hipStream_t stream) {
    const int tilesX = (R.width + AO_W - 1) / AO_W;
    const dim3 g((unsigned)tilesX * (unsigned)((R.height + AO_H - 1) / AO_H)), b(AO_W, AO_H);      // (one dimension: no 65535-row limit)
    if (smooth) hipLaunchKernelGGL((rz_ao_resolve<true>), g, b, 0, stream, R, tilesX);
    else hipLaunchKernelGGL((rz_ao_resolve<false>), g, b, 0, stream, R, tilesX);
}

}  // namespace rz

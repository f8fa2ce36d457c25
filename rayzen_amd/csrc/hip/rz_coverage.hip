// rz_coverage.hip -- which instances a rectangle of the screen shows, where and how near (include/rayzen_hip.h: rz_coverage).
// The render path does not change: these kernels read the device scene and write buffers of the caller's.
//
//   rz_coverage_init    one lane per record of every private set: the empty record (a memset cannot write INT32_MAX or 1e30f).
//                       Runs when the scratch is new or its layout changes: rz_coverage_merge leaves the sets empty again.
//   rz_coverage_runs    one wave per run of 64 pixels of a row of the clipped rectangle, a persistent grid of one-wave workgroups
//                       (rz_denoise_guides' structure).  A lane inside the rectangle casts the ray through its pixel centre
//                       (rz_pixel_cast.h: pixel_centre_dir, from cam_pos; rz_query.h: ray_query -- the query of
//                       rz_denoise_guides and rz_trace_rays, not clipped), writes its id and holds a key: the instance, or n for
//                       a miss.  The wave then groups its lanes by key: while lanes remain it takes the first remaining lane's
//                       key, ballots the lanes that hold it, and reduces them.  The count and the box come from the ballot alone
//                       (the run is one row, and the columns are the positions of the mask's first and last bit); the t range is
//                       a butterfly over the bit patterns, which are ordered as the floats are because the t of a hit is positive
//                       and finite.  The group goes into the wave's own table, which lives in registers: lane j holds entry j, a
//                       key and its record so far.  A ballot finds the lane that holds the key, or the next free lane takes it;
//                       every lane has the group's values (they come from ballots and the butterfly), so the merge is one
//                       predicated update and touches no memory.  When the wave has done its last run, every lane with an entry
//                       sends it to its workgroup's private set of records with integer atomics.  (A 65th key in one wave's runs
//                       finds the table full -- tableCap entries: 64, or fewer as a test aid -- and that group goes to the
//                       private set at once.)
//   rz_coverage_merge   one wave per record: the lanes stride over the sets, empty each copy they have read, reduce by a butterfly
//                       and lane 0 writes the caller's record.
// Why this shape (the measurements are in profiles/coverage/README.md).  A run of 64 pixels per wave, because an 8 x 8 tile per
// wave cast slower with 4 B per pixel written than rz_denoise_guides' runs do with 80 B (as rz_editor.hip found for this walk).
// A table per wave and private sets, because a frame has a floor or a background in most of its units: the 65 000 groups of a
// 1080p frame sending their atomics to the same two or three records took 2 ms, twelve times the cast, and sent to 256 private
// sets instead they still cost half the cast.  So a wave keeps its groups to itself until it ends, and what it sends then goes to
// one of `copies` private sets of records in a scratch of the context's, chosen by workgroup (blockIdx.x % copies) -- the partial
// records of the usual two-kernel reduction, at most RZ_COVERAGE_SETS of them and no more than RZ_COVERAGE_SCRATCH bytes: a scene
// of many instances gets fewer, and its keys spread the atomics by themselves.
// Every step uses integer operations that commute -- add for pixels, signed min / max for the box, unsigned min / max for t -- so
// the records are the same bytes on every run, whichever workgroup met which run.
#include "rz_internal.h"
#include "rz_pixel_cast.h"

namespace rz {

__global__ __launch_bounds__(256) void rz_coverage_init(uint4* sets, int copies, int strideWords, int count) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)copies * count) return;
    const int c = (int)(e / count), i = (int)(e - (long long)c * count);
    uint4* rec = sets + (size_t)c * (strideWords / 4);
    rec[2 * i] = make_uint4(0u, 0x7fffffffu, 0x7fffffffu, 0xffffffffu);                 // pixels, x_min, y_min, x_max = -1
    rec[2 * i + 1] = make_uint4(0xffffffffu, __float_as_uint(1e30f), 0u, 0u);           // y_max = -1, t_min, t_max, reserved
}

// A record in the making: a group of one run, or an entry of a wave's table.  t as bit patterns; a miss keeps the empty range.
struct CovPart {
    unsigned pixels;
    int xmin, ymin, xmax, ymax;
    unsigned tmin, tmax;
};
__device__ __forceinline__ void cov_add(CovPart& e, const CovPart& g) {
    e.pixels += g.pixels;
    e.xmin = min(e.xmin, g.xmin); e.ymin = min(e.ymin, g.ymin);
    e.xmax = max(e.xmax, g.xmax); e.ymax = max(e.ymax, g.ymax);
    e.tmin = min(e.tmin, g.tmin); e.tmax = max(e.tmax, g.tmax);
}
// into record k of a private set (8 words per rz_instance_coverage); a miss (k == nInst) has no t
__device__ __forceinline__ void cov_send(unsigned* set, int k, int nInst, const CovPart& e) {
    unsigned* w = set + 8 * (size_t)k;
    int* wi = reinterpret_cast<int*>(w);
    atomicAdd(w, e.pixels);
    atomicMin(wi + 1, e.xmin); atomicMin(wi + 2, e.ymin);
    atomicMax(wi + 3, e.xmax); atomicMax(wi + 4, e.ymax);
    if (k != nInst) {
        atomicMin(w + 5, e.tmin);
        atomicMax(w + 6, e.tmax);
    }
}

template <bool OVF>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_coverage_runs(const KParams K, const CoverageLaunch V) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    const int lane = threadIdx.x & 63;
    const v3 cam = mk3(K.camPos[0], K.camPos[1], K.camPos[2]);
    unsigned* set = V.records ? V.records + (size_t)(blockIdx.x % (unsigned)V.copies) * V.strideWords : nullptr;
    int ekey = -1, used = 0;            // this lane's entry of the wave's table (-1: free); entries taken
    CovPart e = {0u, 0x7fffffff, 0x7fffffff, -1, -1, 0xffffffffu, 0u};
    bool cut = false;
    for (long long u = blockIdx.x; u < V.units; u += gridDim.x) {
        const int uy = (int)(u / V.unitsX), ux = (int)(u - (long long)uy * V.unitsX);
        const int rx = V.x0 + ux * 64, py = V.y0 + uy, px = rx + lane;
        const bool inside = px < V.x1;
        int key = V.nInst;              // a miss
        unsigned tbits = 0u;
        if (inside) {
            const v3 d = pixel_centre_dir(K, px, py, K.width, K.height);
            HitRec h;
            TraceExtra x;
            const bool found = ray_query<OVF, false>(K, cam, d, h, bstk, x);
            cut = cut || x.cut;
            if (found) {
                key = h.inst;
                tbits = __float_as_uint(h.t);
            }
            if (V.ids) V.ids[(size_t)py * K.width + px] = found ? h.inst : -1;
        }
        if (!set) continue;
        unsigned long long rem = rz_ballot(inside);
        while (rem != 0ull) {
            const int first = __builtin_ctzll(rem);
            const int k = __builtin_amdgcn_readlane(key, first);
            const bool mine = inside && key == k;
            const unsigned long long m = rz_ballot(mine);
            rem &= ~m;
            CovPart g = {(unsigned)__builtin_popcountll(m), rx + (int)__builtin_ctzll(m), py, rx + 63 - (int)__builtin_clzll(m), py,
                         mine ? tbits : 0xffffffffu, mine ? tbits : 0u};
            if (k != V.nInst) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    g.tmin = min(g.tmin, (unsigned)__shfl_xor((int)g.tmin, off, 64));
                    g.tmax = max(g.tmax, (unsigned)__shfl_xor((int)g.tmax, off, 64));
                }
            } else {
                g.tmin = 0xffffffffu;
                g.tmax = 0u;
            }
            // A guard against corrupt bindings only: a TLAS index outside 0 .. n - 1 names no record, and writing one would be
            // out of bounds.  (With valid bindings every hit's instance is in range and `pixels` sums to the rectangle's area.)
            if ((unsigned)k > (unsigned)V.nInst) continue;
            const bool known = rz_ballot(ekey == k) != 0ull;
            if (!known && used == V.tableCap) {                             // the table is full: this group goes out by itself
                if (lane == first) cov_send(set, k, V.nInst, g);
                continue;
            }
            if (known ? ekey == k : lane == used) {
                ekey = k;
                cov_add(e, g);
            }
            if (!known) used += 1;
        }
    }
    if (ekey >= 0) cov_send(set, ekey, V.nInst, e);
    rays_backstop(V.errWord, cut);
}

// One wave per record: copy c of record blockIdx.x for c = lane, lane + 64, ..., each left empty for the next call; the butterfly
// leaves every lane with the result.
__global__ __launch_bounds__(64) void rz_coverage_merge(unsigned* sets, int copies, int strideWords, uint4* out) {
    const int lane = threadIdx.x;
    unsigned pixels = 0u, tmin = __float_as_uint(1e30f), tmax = 0u;
    int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    for (int c = lane; c < copies; c += 64) {
        uint4* r = reinterpret_cast<uint4*>(sets + (size_t)c * strideWords) + 2 * (size_t)blockIdx.x;
        const uint4 a = r[0], b = r[1];
        if (a.x == 0u) continue;            // an empty copy: nothing to add, nothing to clean
        r[0] = make_uint4(0u, 0x7fffffffu, 0x7fffffffu, 0xffffffffu);
        r[1] = make_uint4(0xffffffffu, __float_as_uint(1e30f), 0u, 0u);
        pixels += a.x;
        xmin = min(xmin, (int)a.y); ymin = min(ymin, (int)a.z); xmax = max(xmax, (int)a.w); ymax = max(ymax, (int)b.x);
        tmin = min(tmin, b.y); tmax = max(tmax, b.z);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        pixels += (unsigned)__shfl_xor((int)pixels, off, 64);
        xmin = min(xmin, __shfl_xor(xmin, off, 64)); ymin = min(ymin, __shfl_xor(ymin, off, 64));
        xmax = max(xmax, __shfl_xor(xmax, off, 64)); ymax = max(ymax, __shfl_xor(ymax, off, 64));
        tmin = min(tmin, (unsigned)__shfl_xor((int)tmin, off, 64)); tmax = max(tmax, (unsigned)__shfl_xor((int)tmax, off, 64));
    }
    if (lane == 0) {
        out[2 * (size_t)blockIdx.x] = make_uint4(pixels, (unsigned)xmin, (unsigned)ymin, (unsigned)xmax);
        out[2 * (size_t)blockIdx.x + 1] = make_uint4((unsigned)ymax, tmin, tmax, 0u);
    }
}

void launch_coverage_init(unsigned* sets, int copies, int strideWords, int count, hipStream_t stream) {
    const long long n = (long long)copies * count;
    hipLaunchKernelGGL(rz_coverage_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<uint4*>(sets), copies, strideWords, count);
}

void launch_coverage_merge(unsigned* sets, int copies, int strideWords, unsigned* out, int count, hipStream_t stream) {
    hipLaunchKernelGGL(rz_coverage_merge, dim3((unsigned)count), dim3(64), 0, stream, sets, copies, strideWords, reinterpret_cast<uint4*>(out));
}

void launch_coverage(const KParams& K, const CoverageLaunch& V, hipStream_t stream) {
    const dim3 g((unsigned)V.grid), b(64);
    const size_t lds = (size_t)K.blasStackCap * 64 * sizeof(uint2);
    if (K.blasOvfCap > 0) hipLaunchKernelGGL((rz_coverage_runs<true>), g, b, lds, stream, K, V);
    else hipLaunchKernelGGL((rz_coverage_runs<false>), g, b, lds, stream, K, V);
}

}  // namespace rz

// rz_quality.hip -- rz_geometry_quality's kernels: the SAH cost of every laid-out BLAS from the raw node array on the
// device (include/rayzen_hip.h states the cost; BVH::sahCost / rzh_blas_sah_cost state the same on the host).
//
// Two launches however many meshes there are, and no floating-point atomics, so two calls on an unchanged context
// return identical bytes:
//   * rz_quality_partials: the internal nodes of ALL views in one grid.  A view owns a run of whole workgroups
//     (QualityView::blockBase; a workgroup never straddles two views), a lane owns one internal node by its breadth-first
//     rank (the rankToNode lists of rz_refit_geometry: refit_topology).  The lane loads its node (32 B) and the two
//     adjacent children (64 B), all as 16-byte loads, and contributes the node's own area plus area x count of each
//     child that is a leaf -- every reachable node is counted exactly once, the root as an internal node.  wave64
//     shuffle reduction, the four waves' sums through LDS, one binary64 partial per workgroup, stored;
//   * rz_quality_finish, one wave per view: lane l adds the view's partials l, l + 64, ... in index order, the same
//     shuffle tree, and lane 0 divides by the root's area.  A root that is a leaf (a mesh of at most four triangles, or
//     the count == 0 root of an empty one) is handled here on its own.
// Every index was range-checked when the topology was derived, and the topology has not changed since.
#include <hip/hip_runtime.h>

#include "rayzen_hip.h"
#include "rz_internal.h"

namespace rz {

namespace {

// 2 (dx dy + dy dz + dz dx) of the binary32 bounds in binary64; 0 for an inverted or NaN box
__device__ inline double box_area(const float4 lo, const float4 hi) {
    const double dx = (double)hi.x - (double)lo.x, dy = (double)hi.y - (double)lo.y, dz = (double)hi.z - (double)lo.z;
    if (!(dx >= 0.0) || !(dy >= 0.0) || !(dz >= 0.0)) return 0.0;
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

__device__ inline double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;           // lane 0 holds the sum
}

}  // namespace

__global__ __launch_bounds__(256) void rz_quality_partials(const rz_bvh_node* __restrict__ nodes, const int32_t* __restrict__ rank,
                                                           const QualityView* __restrict__ views, int nViews, double* __restrict__ partials) {
    __shared__ double waveSums[4];
    // the view this workgroup belongs to: the last one whose blockBase is <= blockIdx.x (views[nViews] is the sentinel)
    int lo = 0, hi = nViews;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (views[mid].blockBase <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    const QualityView V = views[lo];
    const int k = ((int)blockIdx.x - V.blockBase) * 256 + (int)threadIdx.x;
    double mine = 0.0;
    if (k < V.nPairs) {
        const rz_bvh_node* base = nodes + V.nodeOff;
        const int n = rank[V.rankBase + k];
        const float4* p = reinterpret_cast<const float4*>(base + n);
        const float4 nlo = p[0], nhi = p[1];
        mine = box_area(nlo, nhi);
        const float4* q = reinterpret_cast<const float4*>(base + __float_as_int(nlo.w));
        const float4 llo = q[0], lhi = q[1], rlo = q[2], rhi = q[3];
        const int lc = __float_as_int(lhi.w), rc = __float_as_int(rhi.w);
        if (lc >= 0) mine += box_area(llo, lhi) * (double)lc;
        if (rc >= 0) mine += box_area(rlo, rhi) * (double)rc;
    }
    const double w = wave_sum(mine);
    if ((threadIdx.x & 63u) == 0u) waveSums[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((waveSums[0] + waveSums[1]) + waveSums[2]) + waveSums[3];
}

__global__ __launch_bounds__(64) void rz_quality_finish(const rz_bvh_node* __restrict__ nodes, const QualityView* __restrict__ views,
                                                        int nViews, const double* __restrict__ partials, double* __restrict__ cost) {
    const int v = (int)blockIdx.x;
    if (v >= nViews) return;
    const QualityView V = views[v];
    const int b0 = V.blockBase, b1 = views[v + 1].blockBase;
    double s = 0.0;
    for (int b = b0 + (int)threadIdx.x; b < b1; b += 64) s += partials[b];
    s = wave_sum(s);
    if (threadIdx.x != 0) return;
    const float4* p = reinterpret_cast<const float4*>(nodes + V.nodeOff);
    const float4 rlo = p[0], rhi = p[1];
    const double area = box_area(rlo, rhi);
    const int count = __float_as_int(rhi.w);
    if (V.nPairs == 0) s = count > 0 ? area * (double)count : 0.0;     // the root is a leaf
    cost[v] = (area == 0.0) ? 0.0 : s / area;
}

int quality_device(const rz_bvh_node* nodes, const int32_t* rank, const QualityView* views, int nViews, int nBlocks, double* partials,
                   double* cost, hipStream_t s) {
    if (nViews <= 0) return 0;
    if (nBlocks > 0)
        hipLaunchKernelGGL(rz_quality_partials, dim3((unsigned)nBlocks), dim3(256), 0, s, nodes, rank, views, nViews, partials);
    hipLaunchKernelGGL(rz_quality_finish, dim3((unsigned)nViews), dim3(64), 0, s, nodes, views, nViews, partials, cost);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}

}  // namespace rz

// rz_refit.hip -- rz_refit_geometry's kernels: the boxes of an existing BLAS recomputed from moved triangles, bottom-up,
// and everything the traversal derived from that BLAS patched in place (include/rayzen_hip.h states the result).
//
// What it replaces for a deformed mesh: rz_build_geometry (three sorts + level kernels) plus the whole re-layout of
// rz_relayout.hip.  A refit keeps the topology, so nothing is sorted, scanned or re-numbered:
//   * the pair index of an internal node is its rank in the breadth-first order of the internal nodes (rz_relayout.hip),
//     so the ranks of one tree level are one contiguous range, and `rankToNode` (derived once per layout on the host,
//     rz_context.hip: refit_topology) is all a level's launch needs: lane k owns internal node rankToNode[k] and
//     DevPair k, whose two halves are that node's two children;
//   * rz_refit_tris, one lane per leaf slot: the slot's triangle from the (already patched) raw array -> DevTri with the
//     one-rounding edge subtractions of rl_gather, DevTriN with rl_tri_normals' expression, material index checked, the
//     view's "transparent" bit or-ed;
//   * rz_refit_level, deepest level first, one launch per level (a kernel boundary is the only hand-off between levels:
//     no data crosses workgroups inside a launch): a leaf child's box from its triangles (computeBounds), an internal
//     child's box as the previous launch left it in the node array; both go into the DevPair, their glm::min / glm::max
//     into the node's own 32-byte record (a bound equal to the one held keeps its bits), the "irregular child box" bit is or-ed as rl_write does;
//   * rz_refit_roots: every instance's root box (and its "may hold glass" flag) from its view, and the views' root
//     nodes gathered for the host; rz_tlas_refit (rz_tlas_device.hip) then rebuilds world boxes and TLAS as it is.
// Every index these kernels use was range-checked when the view was laid out, and the topology has not changed since.
#include <hip/hip_runtime.h>

#include "rayzen_hip.h"
#include "rz_device_math.h"
#include "rz_internal.h"

namespace rz {

namespace {

__device__ inline float gmin(float a, float b) { return (b < a) ? b : a; }   // glm::min
__device__ inline float gmax(float a, float b) { return (a < b) ? b : a; }   // glm::max
// An internal node's refitted bound: the union's, unless it compares equal to the bound the node holds -- then the node's own
// bits stay.  Only the sign of a zero can differ.  BVH::buildBLAS folds a node's box over its triangles in the order they had
// BEFORE the node's range was sorted for its children (BVH.cpp:112, 131-133), an order a refit cannot know; the union of the
// children keeps the first zero of the FINAL order.  With this rule a refit of unmoved vertices is the identity.
__device__ inline float keep_equal(float held, float fresh) { return (fresh == held) ? held : fresh; }

struct Box { float mn[3], mx[3]; };

// computeBounds (RayZen/src/BVH.cpp:11-19) over the slots [first, first + count) of a view
__device__ inline Box leaf_bounds(const rz_triangle* __restrict__ tris, long long nTris, const int32_t* __restrict__ idx, int gTriOff,
                                  int first, int count) {
    const float FMAX = 3.402823466e+38f;
    Box b;
    for (int a = 0; a < 3; ++a) { b.mn[a] = FMAX; b.mx[a] = -FMAX; }
    for (int s = 0; s < count; ++s) {
        const long long src = (long long)gTriOff + idx[first + s];
        if (src < 0 || src >= nTris) continue;          // (cannot happen: checked by the re-layout)
        const float4* t = reinterpret_cast<const float4*>(tris + src);
        const float4 v0 = t[0], v1 = t[1], v2 = t[2];
        b.mn[0] = gmin(b.mn[0], gmin(v0.x, gmin(v1.x, v2.x))); b.mx[0] = gmax(b.mx[0], gmax(v0.x, gmax(v1.x, v2.x)));
        b.mn[1] = gmin(b.mn[1], gmin(v0.y, gmin(v1.y, v2.y))); b.mx[1] = gmax(b.mx[1], gmax(v0.y, gmax(v1.y, v2.y)));
        b.mn[2] = gmin(b.mn[2], gmin(v0.z, gmin(v1.z, v2.z))); b.mx[2] = gmax(b.mx[2], gmax(v0.z, gmax(v1.z, v2.z)));
    }
    return b;
}

__device__ inline void store_node(rz_bvh_node* n, const Box& b, int leftFirst, int count) {
    float4* p = reinterpret_cast<float4*>(n);
    p[0] = make_float4(b.mn[0], b.mn[1], b.mn[2], __int_as_float(leftFirst));
    p[1] = make_float4(b.mx[0], b.mx[1], b.mx[2], __int_as_float(count));
}

// one bit into a view's flag word, one atomic per wave that has it
__device__ inline void or_flag(unsigned* word, bool mine, unsigned bit) {
    const unsigned long long m = __ballot(mine);
    if (m != 0ull && (unsigned)__lane_id() == (unsigned)(__ffsll((long long)m) - 1)) atomicOr(word, bit);
}

}  // namespace

// vflags[0]: bit 0 a transparent material is in use, bit 1 an irregular child box, bit 2 a material index out of range
// (vflags[1] = the caller's index of one such triangle)
__global__ __launch_bounds__(256) void rz_refit_tris(const rz_triangle* __restrict__ raw, long long nTris, const int32_t* __restrict__ idx,
                                                     int gTriOff, int nSlots, DevTri* __restrict__ out, DevTriN* __restrict__ outN,
                                                     const rz_material* __restrict__ mats, int nMat, unsigned* vflags) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    bool glass = false, bad = false;
    long long src = 0;
    if (s < nSlots) {
        src = (long long)gTriOff + idx[s];
        if (src >= 0 && src < nTris) {                  // (always: checked by the re-layout)
            const float4* p = reinterpret_cast<const float4*>(raw + src);
            const float4 v0 = p[0], v1 = p[1], v2 = p[2];
            const int mat = __float_as_int(p[3].x);
            DevTri d;
            d.v0[0] = v0.x; d.v0[1] = v0.y; d.v0[2] = v0.z;
            d.e1x = v1.x - v0.x; d.e1y = v1.y - v0.y; d.e1z = v1.z - v0.z;   // FS:392
            d.e2x = v2.x - v0.x; d.e2y = v2.y - v0.y; d.e2z = v2.z - v0.z;   // FS:393
            d.mat = mat;
            d.src = (int32_t)src;
            d.pad = 0;
            out[s] = d;
            const v3 ln = normalize(cross(mk3(d.e1x, d.e1y, d.e1z), mk3(d.e2x, d.e2y, d.e2z)));    // rl_tri_normals
            DevTriN o;
            o.n[0] = ln.x; o.n[1] = ln.y; o.n[2] = ln.z; o.mat = mat;
            outN[s] = o;
            if (mat < 0 || mat >= nMat) bad = true;
            else { const float tr = mats[mat].transparency; glass = tr > 0.0f || !(tr == tr); }
        }
    }
    or_flag(vflags, glass, 1u);
    if (bad && atomicOr(vflags, 4u) == 0u) vflags[1] = (unsigned)src;     // (any one of them; the next upload words the error)
}

// Internal nodes of one tree level: ranks [k0, k1) of the view.  nodes / idx / rankToNode / pairs are the VIEW's.
__global__ __launch_bounds__(256) void rz_refit_level(rz_bvh_node* __restrict__ nodes, const int32_t* __restrict__ idx,
                                                      const rz_triangle* __restrict__ raw, long long nTris, int gTriOff,
                                                      const int32_t* __restrict__ rankToNode, int k0, int k1, DevPair* __restrict__ pairs,
                                                      unsigned* vflags) {
    const int k = k0 + blockIdx.x * blockDim.x + threadIdx.x;
    bool irregular = false;
    if (k < k1) {
        const int n = rankToNode[k];
        const int L = nodes[n].leftFirst, own = nodes[n].count;
        Box b[2];
        for (int c = 0; c < 2; ++c) {
            const float4* p = reinterpret_cast<const float4*>(nodes + L + c);
            const float4 lo = p[0], hi = p[1];
            const int lf = __float_as_int(lo.w), cnt = __float_as_int(hi.w);
            if (cnt > 0) {
                b[c] = leaf_bounds(raw, nTris, idx, gTriOff, lf, cnt);
                store_node(nodes + L + c, b[c], lf, cnt);
            } else {        // an internal child: the deeper level's launch wrote it (count == 0: left as it is)
                b[c].mn[0] = lo.x; b[c].mn[1] = lo.y; b[c].mn[2] = lo.z;
                b[c].mx[0] = hi.x; b[c].mx[1] = hi.y; b[c].mx[2] = hi.z;
            }
        }
        float4* P = reinterpret_cast<float4*>(pairs + k);           // lx ly | lz rx | ry rz | (the references stay)
        P[0] = make_float4(b[0].mn[0], b[0].mx[0], b[0].mn[1], b[0].mx[1]);
        P[1] = make_float4(b[0].mn[2], b[0].mx[2], b[1].mn[0], b[1].mx[0]);
        P[2] = make_float4(b[1].mn[1], b[1].mx[1], b[1].mn[2], b[1].mx[2]);
        irregular = !(b[0].mn[0] <= b[0].mx[0] && b[0].mn[1] <= b[0].mx[1] && b[0].mn[2] <= b[0].mx[2] &&
                      b[1].mn[0] <= b[1].mx[0] && b[1].mn[1] <= b[1].mx[1] && b[1].mn[2] <= b[1].mx[2]);
        // a bound that compares equal to the one the node holds keeps the node's bits (the sign of a zero: keep_equal)
        const float4* Pn = reinterpret_cast<const float4*>(nodes + n);
        const float4 olo = Pn[0], ohi = Pn[1];
        const float omn[3] = {olo.x, olo.y, olo.z}, omx[3] = {ohi.x, ohi.y, ohi.z};
        Box u;
        for (int a = 0; a < 3; ++a) {
            u.mn[a] = keep_equal(omn[a], gmin(b[0].mn[a], b[1].mn[a]));
            u.mx[a] = keep_equal(omx[a], gmax(b[0].mx[a], b[1].mx[a]));
        }
        store_node(nodes + n, u, L, own);
    }
    or_flag(vflags, irregular, 2u);
}

// a view whose root is a leaf with triangles (a mesh of at most four)
__global__ void rz_refit_leaf_root(rz_bvh_node* __restrict__ nodes, const int32_t* __restrict__ idx, const rz_triangle* __restrict__ raw,
                                   long long nTris, int gTriOff) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int lf = nodes[0].leftFirst, cnt = nodes[0].count;
    if (cnt <= 0) return;
    const Box b = leaf_bounds(raw, nTris, idx, gTriOff, lf, cnt);
    store_node(nodes, b, lf, cnt);
}

// lanes [0, nInst): the instance's root box and flag bit 1 from its view; lanes [nInst, nInst + nViews): the views' root nodes
__global__ __launch_bounds__(256) void rz_refit_roots(DevInstance* __restrict__ inst, int nInst, const int32_t* __restrict__ instView,
                                                      const int32_t* __restrict__ viewNodeOff, int nViews, const rz_bvh_node* __restrict__ nodes,
                                                      const unsigned* __restrict__ vflags, rz_bvh_node* __restrict__ rootsOut) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nInst) {
        const int v = instView[i];
        if (v < 0 || v >= nViews) return;
        const rz_bvh_node r = nodes[viewNodeOff[v]];
        DevInstance& D = inst[i];
        D.rootMin[0] = r.boundsMin[0]; D.rootMin[1] = r.boundsMin[1]; D.rootMin[2] = r.boundsMin[2];
        D.rootMax[0] = r.boundsMax[0]; D.rootMax[1] = r.boundsMax[1]; D.rootMax[2] = r.boundsMax[2];
        D.flags = (D.flags & 1) | ((vflags[4 * v] & 1u) ? 2 : 0);
    } else if (i < nInst + nViews) {
        const int v = i - nInst;
        rootsOut[v] = nodes[viewNodeOff[v]];
    }
}

int refit_view_device(const RefitViewWork& W, hipStream_t s) {
    if (W.nSlots > 0)
        hipLaunchKernelGGL(rz_refit_tris, dim3((unsigned)((W.nSlots + 255) / 256)), dim3(256), 0, s, W.rawTris, W.nTris, W.idx, W.gTriOff,
                           W.nSlots, W.tris, W.triN, W.mats, W.nMat, W.vflags);
    if (W.nLevels == 0)
        hipLaunchKernelGGL(rz_refit_leaf_root, dim3(1), dim3(64), 0, s, W.nodes, W.idx, W.rawTris, W.nTris, W.gTriOff);
    for (int d = W.nLevels - 1; d >= 0; --d) {
        const int k0 = W.levelStart[d], k1 = W.levelStart[d + 1];
        if (k1 <= k0) continue;
        hipLaunchKernelGGL(rz_refit_level, dim3((unsigned)((k1 - k0 + 255) / 256)), dim3(256), 0, s, W.nodes, W.idx, W.rawTris, W.nTris,
                           W.gTriOff, W.rankToNode, k0, k1, W.pairs, W.vflags);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}

int refit_roots_device(DevInstance* inst, int nInst, const int32_t* instView, const int32_t* viewNodeOff, int nViews,
                       const rz_bvh_node* nodes, const unsigned* vflags, rz_bvh_node* rootsOut, hipStream_t s) {
    const int n = nInst + nViews;
    if (n > 0)
        hipLaunchKernelGGL(rz_refit_roots, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, inst, nInst, instView, viewNodeOff, nViews,
                           nodes, vflags, rootsOut);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}

}  // namespace rz

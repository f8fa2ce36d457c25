// rz_skin.hip -- rz_skin_pose's kernel: a mesh posed on the device from the rest pose its rig keeps there, into the triangle
// buffer rz_refit_geometry's path then takes (include/rayzen_hip.h, "Skinned meshes", states every bit of the result;
// rzh_skin_triangles of librayzen_host.so is the byte partner).
//
// One lane per triangle, everything streamed as whole 16-byte vectors (as rz_refit_tris reads and writes): 4 of the rest
// triangle, 4 of its rz_skin_triangle, 3 per morph target, 4 written.  The kernel is templated on the two halves of a rig, so a
// morph-only rig never touches a bone and a skin-only rig has no target loop.  A bone is read as its four columns (the fourth
// row is never used); the table is at most 16 KB and every lane gathers from it up to twelve times, so each workgroup stages
// it in LDS first: measured against gathering through L1, 9 % faster on a two-bone bend and 30-36 % on rigs with four
// influences per corner at 1 M triangles, a tie within the noise at 69 k (profiles/skin/README.md).  A bone index
// was range-checked when the rig was made (rz_skin_create), and an influence of weight 0 does not read its bone at all, so
// nothing is checked here.
// No multiply is contracted with an add: the file is compiled with -ffp-contract=off like every other.
#include <hip/hip_runtime.h>

#include "rayzen_hip.h"
#include "rz_internal.h"

namespace rz {

namespace {

struct P3 { float x, y, z; };

extern __shared__ float4 skin_lds_bones[];      // the workgroup's copy of the bone table: 4 columns per bone

// one corner: the influences in order, weight == 0 skipped (its bone is not read), the first kept one starts the sum
__device__ inline P3 skin_corner(unsigned idx, const float4 w4, const P3 p) {
    const float w[4] = {w4.x, w4.y, w4.z, w4.w};
    P3 o = p;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (w[j] == 0.0f) continue;
        const unsigned m = 4u * ((idx >> (8 * j)) & 255u);
        const float4 c0 = skin_lds_bones[m], c1 = skin_lds_bones[m + 1], c2 = skin_lds_bones[m + 2], c3 = skin_lds_bones[m + 3];
        const float qx = ((c0.x * p.x + c1.x * p.y) + c2.x * p.z) + c3.x;
        const float qy = ((c0.y * p.x + c1.y * p.y) + c2.y * p.z) + c3.y;
        const float qz = ((c0.z * p.x + c1.z * p.y) + c2.z * p.z) + c3.z;
        if (!any) { o.x = w[j] * qx; o.y = w[j] * qy; o.z = w[j] * qz; any = true; }
        else { o.x = o.x + w[j] * qx; o.y = o.y + w[j] * qy; o.z = o.z + w[j] * qz; }
    }
    return o;
}

}  // namespace

template <bool kBones, bool kMorphs>
__global__ __launch_bounds__(256) void rz_skin_tris(const rz_triangle* __restrict__ rest, const rz_skin_triangle* __restrict__ skin,
                                                    const float4* __restrict__ bones, const rz_morph_triangle* __restrict__ morphs,
                                                    const float* __restrict__ morphWeights, int nMorphs, int nBones, long long n,
                                                    rz_triangle* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (kBones) {                                       // (every lane of the workgroup, the tail's idle ones included)
        for (int k = threadIdx.x; k < 4 * nBones; k += blockDim.x) skin_lds_bones[k] = bones[k];
        __syncthreads();
    }
    if (i >= n) return;
    const float4* r = reinterpret_cast<const float4*>(rest + i);
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    P3 p[3] = {{r0.x, r0.y, r0.z}, {r1.x, r1.y, r1.z}, {r2.x, r2.y, r2.z}};
    if (kMorphs) {
        for (int k = 0; k < nMorphs; ++k) {             // every target, a zero weight included
            const float w = morphWeights[k];
            const float4* d = reinterpret_cast<const float4*>(morphs + ((long long)k * n + i));
            const float4 d0 = d[0], d1 = d[1], d2 = d[2];
            p[0].x = p[0].x + w * d0.x; p[0].y = p[0].y + w * d0.y; p[0].z = p[0].z + w * d0.z;
            p[1].x = p[1].x + w * d1.x; p[1].y = p[1].y + w * d1.y; p[1].z = p[1].z + w * d1.z;
            p[2].x = p[2].x + w * d2.x; p[2].y = p[2].y + w * d2.y; p[2].z = p[2].z + w * d2.z;
        }
    }
    if (kBones) {
        const float4* s = reinterpret_cast<const float4*>(skin + i);
        const float4 b = s[0], w0 = s[1], w1 = s[2], w2 = s[3];
        p[0] = skin_corner(__float_as_uint(b.x), w0, p[0]);
        p[1] = skin_corner(__float_as_uint(b.y), w1, p[1]);
        p[2] = skin_corner(__float_as_uint(b.z), w2, p[2]);
    }
    float4* o = reinterpret_cast<float4*>(out + i);     // pads and materialIndex are the rest triangle's
    o[0] = make_float4(p[0].x, p[0].y, p[0].z, r0.w);
    o[1] = make_float4(p[1].x, p[1].y, p[1].z, r1.w);
    o[2] = make_float4(p[2].x, p[2].y, p[2].z, r2.w);
    o[3] = r3;
}

int skin_device(const SkinWork& W, hipStream_t s) {
    if (W.n <= 0) return 0;
    const dim3 grid((unsigned)((W.n + 255) / 256)), block(256);
    const float4* bones = reinterpret_cast<const float4*>(W.bones);
    const bool hasBones = W.skin != nullptr, hasMorphs = W.nMorphs > 0;
    const size_t lds = hasBones ? (size_t)W.nBones * 64 : 0;
    if (hasBones && hasMorphs)
        hipLaunchKernelGGL((rz_skin_tris<true, true>), grid, block, lds, s, W.rest, W.skin, bones, W.morphs, W.morphWeights, W.nMorphs, W.nBones, W.n, W.out);
    else if (hasBones)
        hipLaunchKernelGGL((rz_skin_tris<true, false>), grid, block, lds, s, W.rest, W.skin, bones, W.morphs, W.morphWeights, W.nMorphs, W.nBones, W.n, W.out);
    else
        hipLaunchKernelGGL((rz_skin_tris<false, true>), grid, block, lds, s, W.rest, W.skin, bones, W.morphs, W.morphWeights, W.nMorphs, W.nBones, W.n, W.out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}

}  // namespace rz

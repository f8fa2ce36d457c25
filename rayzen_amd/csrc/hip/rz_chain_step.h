// rz_chain_step.h -- one step of the see-through chain (include/rayzen_hip.h: "chain"), shared by the kernels that follow it so
// that they execute the same statement and cannot drift apart:
//   rz_seethrough_guides            (rz_seethrough.hip)            one chain per pixel of a frame
//   rz_antialias_seethrough_edges   (rz_antialias_seethrough.hip)  one chain per sub-sample of an edge pixel
// Binary32, one rounding per operation, no fused multiply-add, operands in scatter()'s order (rz_path.h).
#pragma once
#include "rz_internal.h"
#include "rz_device_math.h"
#include "rz_path.h"

namespace rz {

// The chain has just found hq along (o, d).  Adds its length to L, notes the first material, and -- unless the chain ends on
// this surface: k == maxDepth, or a surface that scatters diffusely -- takes the dielectric or the mirror step of scatter():
// (o, d) becomes the next segment, T and ior follow, k += 1.  Returns whether the chain goes on.
__device__ __forceinline__ bool chain_step(const KParams& K, int maxDepth, const HitRec& hq, v3& o, v3& d, v3& T, float& ior,
                                           float& L, int& k, int& first) {
    bool run = false;
    L = L + hq.t;
    const int m = min(max(hq.mat, 0), K.nMaterials - 1);
    if (k == 0) first = m;
    const DevMaterial M = K.materials[m];
    const v3 hitNormal = hq.n;
    v3 dir = d;
    if (k == maxDepth) {
        // the chain is exhausted on this surface, specular or not
    } else if (M.transparency > 0.0f) {     // scatter(): FS:723-746
        const bool entering = dot(-dir, hitNormal) > 0.0f;
        const v3 N = entering ? hitNormal : -hitNormal;
        const float extIor = ior;
        const float nextIor = entering ? M.ior : 1.0f;
        const float eta = extIor / nextIor;
        const float cosi = clamp_(dot(-dir, N), 0.0f, 1.0f);
        const float F0 = pow2_((extIor - nextIor) / (extIor + nextIor));
        const float fresnel = F0 + (1.0f - F0) * pow5_(1.0f - cosi);
        v3 refr;
        if (!refract_dir(dir, N, eta, refr)) {
            dir = reflect_ray(dir, N);
            T = T * 0.98f;
        } else {
            dir = refr;
            ior = nextIor;
            const float tr = M.transparency;
            const v3 tint = mk3(mix_(1.0f, M.albedo[0], tr), mix_(1.0f, M.albedo[1], tr), mix_(1.0f, M.albedo[2], tr));
            const v3 tw = (tint * tr) * (1.0f - fresnel);
            T = T * mk3(clamp_(tw.x, 0.0f, 1.0f), clamp_(tw.y, 0.0f, 1.0f), clamp_(tw.z, 0.0f, 1.0f));
        }
        run = true;
    } else if (M.reflectivity >= 1.0f) {    // scatter(): randVal < reflectivity holds for every randVal in [0, 1)
        dir = reflect_ray(dir, hitNormal);
        T = T * 0.95f;
        run = true;
    }
    if (run) {
        const float pushDir = dot(dir, hitNormal) > 0.0f ? 1.0f : -1.0f;
        o = hq.p + (hitNormal * pushDir) * 0.003f;
        d = dir;
        k += 1;
    }
    return run;
}

}  // namespace rz

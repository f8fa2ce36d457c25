// Skin.cpp -- Mesh::skin: linear-blend skinning and morph targets on the host, the byte partner of rz_skin_pose's kernel
// (rz_skin.hip).  The definition of every bit is rz_skin_pose's in include/rayzen_hip.h ("THE POSED TRIANGLE"); this file is
// compiled with -ffp-contract=off, so every product and every sum below is rounded on its own.  No counterpart in the reference.
#include "RayZenScene.h"

#include <cstring>

namespace rayzen {

namespace {

// one corner: p morphed by every target in order, then blended over the kept influences in order
void poseCorner(float p[3], size_t t, size_t n, int corner, const rz_skin_triangle* skin, const float* bones,
                const rz_morph_triangle* morphs, const float* morphWeights, int nMorphs) {
    for (int k = 0; k < nMorphs; ++k) {
        const float w = morphWeights[k];
        const float* d = morphs[(size_t)k * n + t].d[corner];
        p[0] = p[0] + w * d[0];
        p[1] = p[1] + w * d[1];
        p[2] = p[2] + w * d[2];
    }
    if (!skin) return;
    const uint32_t idx = skin[t].bones[corner];
    const float* weights = skin[t].weights[corner];
    float o[3] = {p[0], p[1], p[2]};
    bool any = false;
    for (int j = 0; j < 4; ++j) {
        const float w = weights[j];
        if (w == 0.0f) continue;            // (its bone is not read)
        const float* m = bones + 16 * (size_t)((idx >> (8 * j)) & 255u);
        const float qx = ((m[0] * p[0] + m[4] * p[1]) + m[8] * p[2]) + m[12];
        const float qy = ((m[1] * p[0] + m[5] * p[1]) + m[9] * p[2]) + m[13];
        const float qz = ((m[2] * p[0] + m[6] * p[1]) + m[10] * p[2]) + m[14];
        if (!any) { o[0] = w * qx; o[1] = w * qy; o[2] = w * qz; any = true; }
        else { o[0] = o[0] + w * qx; o[1] = o[1] + w * qy; o[2] = o[2] + w * qz; }
    }
    p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
}

}  // namespace

void Mesh::skin(const Triangle* rest, size_t n, const rz_skin_triangle* skin, const float* bones, const rz_morph_triangle* morphs,
                const float* morphWeights, int nMorphs, Triangle* out) {
    for (size_t t = 0; t < n; ++t) {
        rz_triangle tri;                    // every byte of the rest triangle, then the three corners
        std::memcpy(&tri, &rest[t], sizeof tri);
        poseCorner(tri.v0, t, n, 0, skin, bones, morphs, morphWeights, nMorphs);
        poseCorner(tri.v1, t, n, 1, skin, bones, morphs, morphWeights, nMorphs);
        poseCorner(tri.v2, t, n, 2, skin, bones, morphs, morphWeights, nMorphs);
        std::memcpy(static_cast<void*>(&out[t]), &tri, sizeof tri);
    }
}

void Mesh::pose(const Mesh& restPose, const std::vector<rz_skin_triangle>& skinData, const std::vector<mat4>& bones,
                const std::vector<rz_morph_triangle>& morphs, const std::vector<float>& morphWeights) {
    const size_t n = restPose.triangles.size();
    triangles.resize(n);
    static_assert(sizeof(mat4) == 64, "a bone is 16 column-major floats");
    skin(restPose.triangles.data(), n, skinData.empty() ? nullptr : skinData.data(),
         bones.empty() ? nullptr : bones[0].m, morphs.data(), morphWeights.data(), (int)morphWeights.size(), triangles.data());
}

}  // namespace rayzen

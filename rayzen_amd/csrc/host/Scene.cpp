// Scene.cpp -- Scene -> the six geometry arrays of RayZen's SSBOs.
//   SceneBuffers::build          <- RayZen/src/main.cpp:941-1035 (initializeSSBOs, no disk cache)
//   SceneBuffers::updateDynamic  <- RayZen/src/main.cpp:1138-1194 (updateDynamicBVHAndSSBOs)
//   worldRootNode                <- RayZen/src/main.cpp:974-993
//   Camera::rotate               <- RayZen/include/Camera.h:72-90
#include "RayZenScene.h"

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

namespace rayzen {

void Camera::rotate(float offsetX, float offsetY) {
    yaw += offsetX * sensitivity;
    pitch += offsetY * sensitivity;
    if (pitch > 89.0f) pitch = 89.0f;
    if (pitch < -89.0f) pitch = -89.0f;
    vec3 direction;
    direction.x = std::cos(radians(yaw)) * std::cos(radians(pitch));
    direction.y = std::sin(radians(pitch));
    direction.z = std::sin(radians(yaw)) * std::cos(radians(pitch));
    target = normalize(direction);
    vec3 right = normalize(cross(target, vec3(0.0f, 1.0f, 0.0f)));
    up = normalize(cross(right, target));
    updateViewMatrix();
}

BVHNode worldRootNode(const BVHNode& meshRoot, const mat4& transform) {
    const vec3& lo = meshRoot.boundsMin;
    const vec3& hi = meshRoot.boundsMax;
    vec3 bmin(1e30f), bmax(-1e30f);
    for (int c = 0; c < 8; ++c) {
        vec4 corner{(c & 4) ? hi.x : lo.x, (c & 2) ? hi.y : lo.y, (c & 1) ? hi.z : lo.z, 1.0f};
        vec4 t = transform * corner;
        vec3 tc(t.x, t.y, t.z);
        bmin = vmin(bmin, tc);
        bmax = vmax(bmax, tc);
    }
    BVHNode r = meshRoot;
    r.boundsMin = bmin;
    r.boundsMax = bmax;
    return r;
}

bool SceneBuffers::build(const Scene& scene, bool shareMeshes) {
    allTriangles.clear(); allBLASNodes.clear(); allBLASTriIndices.clear();
    meshInstances.clear(); tlasNodes.clear(); tlasTriIndices.clear(); blasRoots.clear();
    maxBLASDepth = 1;

    struct Placed { int nodeOffset, triOffset, triBase; BVHNode root; };
    std::map<const Mesh*, BVH> built;          // a BLAS depends only on the mesh: build each once
    std::map<const Mesh*, Placed> placed;      // shareMeshes: where the single copy lives
    std::vector<BVHNode> worldRootNodes;
    worldRootNodes.reserve(scene.gameObjects.size());

    for (size_t i = 0; i < scene.gameObjects.size(); ++i) {
        const GameObject& obj = scene.gameObjects[i];
        const Mesh* mesh = obj.mesh.get();
        static const Mesh kEmpty;
        if (!mesh) mesh = &kEmpty;
        auto it = built.find(mesh);
        if (it == built.end()) {
            it = built.emplace(mesh, BVH{}).first;
            if (blasBuilder) { if (!blasBuilder(*mesh, it->second)) return false; }
            else it->second.buildBLAS(mesh->triangles);
            maxBLASDepth = std::max(maxBLASDepth, it->second.depth());
        }
        const BVH& blas = it->second;
        Placed where;
        auto pit = placed.find(mesh);
        if (shareMeshes && pit != placed.end()) {
            where = pit->second;
        } else {
            where.nodeOffset = (int)allBLASNodes.size();
            where.triOffset = (int)allBLASTriIndices.size();
            where.triBase = (int)allTriangles.size();
            where.root = blas.nodes[0];
            allTriangles.insert(allTriangles.end(), mesh->triangles.begin(), mesh->triangles.end());
            allBLASNodes.insert(allBLASNodes.end(), blas.nodes.begin(), blas.nodes.end());
            allBLASTriIndices.insert(allBLASTriIndices.end(), blas.triIndices.begin(), blas.triIndices.end());
            placed[mesh] = where;
        }
        worldRootNodes.push_back(worldRootNode(where.root, obj.transform));
        blasRoots.push_back(where.root);
        BVHInstance inst;
        inst.blasNodeOffset = where.nodeOffset;
        inst.blasTriOffset = where.triOffset;
        inst.globalTriOffset = where.triBase;
        inst.meshIndex = (int)i;
        inst.transform = obj.transform;
        inst.inverseTransform = inverse(obj.transform);
        meshInstances.push_back(inst);
    }
    BVH tlas;
    tlas.buildTLAS(meshInstances, worldRootNodes);
    tlasNodes = tlas.nodes;
    tlasTriIndices = tlas.triIndices;
    tlasDepth = tlas.depth();
    return true;
}

bool SceneBuffers::refitMesh(const Scene& scene, const Mesh* mesh) {
    const size_t nObj = std::min(meshInstances.size(), scene.gameObjects.size());
    const int nTris = (int)mesh->triangles.size();
    // where the copies of this mesh live: node offset -> (index offset, triangle base, node count)
    struct Copy { int triOffset, triBase, nNodes; };
    std::map<int, Copy> copies;
    std::vector<int> starts;
    for (const BVHInstance& inst : meshInstances) starts.push_back(inst.blasNodeOffset);
    starts.push_back((int)allBLASNodes.size());
    std::sort(starts.begin(), starts.end());
    for (size_t i = 0; i < nObj; ++i) {
        if (scene.gameObjects[i].mesh.get() != mesh) continue;
        const BVHInstance& inst = meshInstances[i];
        const int end = *std::upper_bound(starts.begin(), starts.end(), inst.blasNodeOffset);
        if (inst.blasTriOffset < 0 || (size_t)inst.blasTriOffset + (size_t)nTris > allBLASTriIndices.size() || inst.globalTriOffset < 0 ||
            (size_t)inst.globalTriOffset + (size_t)nTris > allTriangles.size())
            return false;
        copies[inst.blasNodeOffset] = {inst.blasTriOffset, inst.globalTriOffset, end - inst.blasNodeOffset};
    }
    if (copies.empty()) return false;
    for (const auto& kv : copies) {
        const Copy& c = kv.second;
        std::copy(mesh->triangles.begin(), mesh->triangles.end(), allTriangles.begin() + c.triBase);
        BVH::refit(allTriangles.data() + c.triBase, allBLASNodes.data() + kv.first, c.nNodes, allBLASTriIndices.data() + c.triOffset);
    }
    for (size_t i = 0; i < meshInstances.size(); ++i)
        if (copies.count(meshInstances[i].blasNodeOffset)) blasRoots[i] = allBLASNodes[(size_t)meshInstances[i].blasNodeOffset];
    std::vector<BVHNode> worldRootNodes(meshInstances.size());
    for (size_t i = 0; i < meshInstances.size(); ++i) worldRootNodes[i] = worldRootNode(blasRoots[i], meshInstances[i].transform);
    BVH tlas;
    tlas.buildTLAS(meshInstances, worldRootNodes);
    tlasNodes = tlas.nodes;
    tlasTriIndices = tlas.triIndices;
    tlasDepth = tlas.depth();
    return true;
}

bool SceneBuffers::rebuildMesh(const Scene& scene, const Mesh* mesh) {
    const size_t nObj = std::min(meshInstances.size(), scene.gameObjects.size());
    const int nTris = (int)mesh->triangles.size();
    // the node extents of every stored BLAS, ascending: [start, the next larger distinct start or the end of the array)
    std::vector<int> starts;
    for (const BVHInstance& inst : meshInstances) starts.push_back(inst.blasNodeOffset);
    std::sort(starts.begin(), starts.end());
    starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
    if (starts.empty() || starts.front() < 0 || (size_t)starts.back() >= allBLASNodes.size()) return false;
    starts.push_back((int)allBLASNodes.size());
    struct Copy { int triOffset, triBase; };
    std::map<int, Copy> copies;             // the copies of this mesh, by node offset
    for (size_t i = 0; i < nObj; ++i) {
        if (scene.gameObjects[i].mesh.get() != mesh) continue;
        const BVHInstance& inst = meshInstances[i];
        if (inst.blasTriOffset < 0 || (size_t)inst.blasTriOffset + (size_t)nTris > allBLASTriIndices.size() || inst.globalTriOffset < 0 ||
            (size_t)inst.globalTriOffset + (size_t)nTris > allTriangles.size())
            return false;
        copies[inst.blasNodeOffset] = {inst.blasTriOffset, inst.globalTriOffset};
    }
    if (copies.empty()) return false;
    std::vector<BVHNode> nodes(allBLASNodes.begin(), allBLASNodes.begin() + starts.front());   // (nodes no instance names stay)
    std::map<int, int> moved;               // node offset before -> after
    for (size_t k = 0; k + 1 < starts.size(); ++k) {
        const int at = starts[k], end = starts[k + 1];
        moved[at] = (int)nodes.size();
        const auto it = copies.find(at);
        if (it == copies.end()) {
            nodes.insert(nodes.end(), allBLASNodes.begin() + at, allBLASNodes.begin() + end);
            continue;
        }
        BVH blas;
        if (blasBuilder) {
            Mesh current;
            current.triangles.assign(allTriangles.begin() + it->second.triBase, allTriangles.begin() + it->second.triBase + nTris);
            if (!blasBuilder(current, blas)) return false;
        } else {
            blas.buildBLAS(allTriangles.data() + it->second.triBase, nTris);
        }
        nodes.insert(nodes.end(), blas.nodes.begin(), blas.nodes.end());
        std::copy(blas.triIndices.begin(), blas.triIndices.end(), allBLASTriIndices.begin() + it->second.triOffset);
    }
    allBLASNodes.swap(nodes);
    // the deepest BLAS now stored, as build() would find it on these triangles (the rebuilt tree may be shallower than the old one)
    maxBLASDepth = 1;
    for (const auto& kv : moved) {
        std::vector<std::pair<int, int>> st{{kv.second, 1}};
        while (!st.empty()) {
            const auto [n, d] = st.back();
            st.pop_back();
            maxBLASDepth = std::max(maxBLASDepth, d);
            const BVHNode& N = allBLASNodes[(size_t)n];
            if (N.count < 0) { st.push_back({kv.second + N.leftFirst, d + 1}); st.push_back({kv.second + N.leftFirst + 1, d + 1}); }
        }
    }
    for (size_t i = 0; i < meshInstances.size(); ++i) {
        meshInstances[i].blasNodeOffset = moved.at(meshInstances[i].blasNodeOffset);
        blasRoots[i] = allBLASNodes[(size_t)meshInstances[i].blasNodeOffset];
    }
    std::vector<BVHNode> worldRootNodes(meshInstances.size());
    for (size_t i = 0; i < meshInstances.size(); ++i) worldRootNodes[i] = worldRootNode(blasRoots[i], meshInstances[i].transform);
    BVH tlas;
    tlas.buildTLAS(meshInstances, worldRootNodes);
    tlasNodes = tlas.nodes;
    tlasTriIndices = tlas.triIndices;
    tlasDepth = tlas.depth();
    return true;
}

void SceneBuffers::updateDynamic(const Scene& scene) {
    size_t n = std::min(meshInstances.size(), scene.gameObjects.size());
    std::vector<BVHNode> worldRootNodes(meshInstances.size());
    for (size_t i = 0; i < meshInstances.size(); ++i) {
        if (i < n) {
            meshInstances[i].transform = scene.gameObjects[i].transform;
            meshInstances[i].inverseTransform = inverse(scene.gameObjects[i].transform);
        }
        worldRootNodes[i] = worldRootNode(blasRoots[i], meshInstances[i].transform);
    }
    BVH tlas;
    tlas.buildTLAS(meshInstances, worldRootNodes);
    tlasNodes = tlas.nodes;
    tlasTriIndices = tlas.triIndices;
    tlasDepth = tlas.depth();
}

}  // namespace rayzen

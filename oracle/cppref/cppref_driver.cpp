// cppref_driver.cpp -- C entry points around RayZen's own BVH / Mesh classes.  TEST INFRASTRUCTURE ONLY.
//
// Compiled together with the reference's src/BVH.cpp and src/Mesh.cpp, which are read from the reference checkout at build
// time and never copied (oracle/cppref/cppref.py).  <glm/glm.hpp> resolves to the stand-in next to this file.  Nothing here
// restates the reference: the driver moves plain arrays in and out of BVH::buildBLAS, BVH::buildTLAS, Mesh::loadFromOBJ and
// BVH::saveToFile / loadFromFile.
#include "BVH.h"
#include "Mesh.h"

#include <cstddef>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rayzen_hip.h"

// the element types the product uploads are the reference's, byte for byte
static_assert(sizeof(Triangle) == 64 && sizeof(Triangle) == sizeof(rz_triangle), "Triangle");
static_assert(sizeof(BVHNode) == 32 && sizeof(BVHNode) == sizeof(rz_bvh_node), "BVHNode");
static_assert(sizeof(BVHInstance) == 144 && sizeof(BVHInstance) == sizeof(rz_bvh_instance), "BVHInstance");
static_assert(offsetof(Triangle, v0) == offsetof(rz_triangle, v0) && offsetof(Triangle, v1) == offsetof(rz_triangle, v1) &&
              offsetof(Triangle, v2) == offsetof(rz_triangle, v2) &&
              offsetof(Triangle, materialIndex) == offsetof(rz_triangle, materialIndex), "Triangle fields");
static_assert(offsetof(BVHNode, boundsMin) == offsetof(rz_bvh_node, boundsMin) &&
              offsetof(BVHNode, leftFirst) == offsetof(rz_bvh_node, leftFirst) &&
              offsetof(BVHNode, boundsMax) == offsetof(rz_bvh_node, boundsMax) &&
              offsetof(BVHNode, count) == offsetof(rz_bvh_node, count), "BVHNode fields");

namespace {

// rz_triangle[n] -> std::vector<Triangle>, field by field (the reference's Triangle has 12 bytes of tail padding)
std::vector<Triangle> to_triangles(const rz_triangle* in, int n) {
    std::vector<Triangle> tris((size_t)n);
    for (int i = 0; i < n; ++i) {
        Triangle& t = tris[(size_t)i];
        t.v0 = glm::vec3(in[i].v0[0], in[i].v0[1], in[i].v0[2]);
        t.v1 = glm::vec3(in[i].v1[0], in[i].v1[1], in[i].v1[2]);
        t.v2 = glm::vec3(in[i].v2[0], in[i].v2[1], in[i].v2[2]);
        t.pad0 = in[i].pad0; t.pad1 = in[i].pad1; t.pad2 = in[i].pad2;
        t.materialIndex = in[i].materialIndex;
    }
    return tris;
}

}  // namespace

extern "C" {

// BVH::buildBLAS over tris[n].  method: 0 = BVHSplitMethod::Midpoint, 1 = BVHSplitMethod::SAH (the class's default, and the
// only one RayZen's main.cpp ever uses).  Returns a handle for the cppref_bvh_* calls, or NULL.
void* cppref_build_blas(const rz_triangle* tris, int n, int method) {
    if (n < 0 || (n > 0 && !tris) || (method != 0 && method != 1)) return nullptr;
    try {
        BVH* b = new BVH();
        b->splitMethod = method ? BVHSplitMethod::SAH : BVHSplitMethod::Midpoint;
        b->buildBLAS(to_triangles(tris, n));
        return b;
    } catch (...) {
        return nullptr;
    }
}

// BVH::buildTLAS over roots[n] (only boundsMin / boundsMax of a root are read) and n default instances (never read).
// n == 0 is refused: the reference's loop never terminates there (count == 0 is never a leaf).
void* cppref_build_tlas(const rz_bvh_node* roots, int n) {
    if (n <= 0 || !roots) return nullptr;
    try {
        std::vector<BVHNode> r((size_t)n);
        std::memcpy(static_cast<void*>(r.data()), roots, (size_t)n * sizeof(BVHNode));
        std::vector<BVHInstance> inst((size_t)n);
        BVH* b = new BVH();
        b->buildTLAS(inst, r);
        return b;
    } catch (...) {
        return nullptr;
    }
}

size_t cppref_bvh_node_count(const void* h) { return static_cast<const BVH*>(h)->nodes.size(); }
size_t cppref_bvh_index_count(const void* h) { return static_cast<const BVH*>(h)->triIndices.size(); }

void cppref_bvh_copy(const void* h, rz_bvh_node* nodes, int32_t* indices) {
    const BVH* b = static_cast<const BVH*>(h);
    if (nodes && !b->nodes.empty()) std::memcpy(nodes, b->nodes.data(), b->nodes.size() * sizeof(BVHNode));
    if (indices && !b->triIndices.empty()) std::memcpy(indices, b->triIndices.data(), b->triIndices.size() * sizeof(int));
}

// BVH::saveToFile / BVH::loadFromFile (the reference's BLAS cache format)
int cppref_bvh_save(const void* h, const char* path) {
    try { return static_cast<const BVH*>(h)->saveToFile(path) ? 0 : -1; } catch (...) { return -2; }
}

void* cppref_bvh_load(const char* path) {
    try {
        BVH* b = new BVH();
        if (!b->loadFromFile(path)) { delete b; return nullptr; }
        return b;
    } catch (...) {
        return nullptr;
    }
}

void cppref_bvh_free(void* h) { delete static_cast<BVH*>(h); }

// How often, since the library was loaded, the reference indexed a vec3 outside 0..2 (the stand-in's operator[] counts them):
// BVH.cpp:140-144 with axis == -1.  The difference across a build tells whether that build went there.
unsigned long long cppref_out_of_range_reads(void) { return glm::vec3::standin_out_of_range_reads(); }

// Mesh::loadFromOBJ.  Returns the triangle count, -1 if the file cannot be opened, -2 if the reference threw (std::stoi on a
// face token that is not a number).  out (cap records, may be NULL) receives v0 / v1 / v2 / pad0-2 / materialIndex field by
// field in records that are otherwise zero: the reference leaves its Triangle's tail padding uninitialised.
int cppref_load_obj(const char* path, int materialIndex, rz_triangle* out, int cap) {
    try {
        Mesh m;
        if (!m.loadFromOBJ(path, materialIndex)) return -1;
        int n = (int)m.triangles.size();
        for (int i = 0; out && i < n && i < cap; ++i) {
            const Triangle& t = m.triangles[(size_t)i];
            rz_triangle r;
            std::memset(&r, 0, sizeof r);
            r.v0[0] = t.v0.x; r.v0[1] = t.v0.y; r.v0[2] = t.v0.z; r.pad0 = t.pad0;
            r.v1[0] = t.v1.x; r.v1[1] = t.v1.y; r.v1[2] = t.v1.z; r.pad1 = t.pad1;
            r.v2[0] = t.v2.x; r.v2[1] = t.v2.y; r.v2[2] = t.v2.z; r.pad2 = t.pad2;
            r.materialIndex = t.materialIndex;
            out[i] = r;
        }
        return n;
    } catch (...) {
        return -2;
    }
}

}  // extern "C"

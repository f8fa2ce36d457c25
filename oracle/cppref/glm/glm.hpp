// glm/glm.hpp -- a STAND-IN for GLM, written for oracle/cppref and nothing else.  TEST INFRASTRUCTURE ONLY.
//
// RayZen's src/BVH.cpp and src/Mesh.cpp (and BVH.h / Mesh.h / Logger.h) include <glm/glm.hpp> and nothing else that
// this project's build machine lacks.  GLM is not installed and not vendored, so this header supplies the dozen
// operations those two files use -- and only those.  No line of GLM is copied: every definition below is our own text,
// written to compute what GLM 0.9.9.8 (the version tests/test_linalg_glm.py cites) publishes for that operation, with
// the published definition quoted in words next to it.  What this header computes is therefore part of what
// oracle/cppref's results rest on (oracle/cppref/README.md says which results lean on which line).
//
// Used by the reference and provided here:
//   vec3: vec3(), vec3(scalar), vec3(x, y, z); .x .y .z; operator[]; vec + vec, vec - vec, vec * float, vec / float
//   glm::min(vec3, vec3), glm::max(vec3, vec3)
//   mat4: only ever a struct member (BVHInstance) -- 16 floats
#pragma once

#include <cassert>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <limits>

namespace glm {

struct vec3 {
    float x, y, z;

    // GLM 0.9.9.8, type_vec3.hpp: `vec() = default` -- the components are UNINITIALISED unless GLM_FORCE_CTOR_INIT is
    // defined (RayZen does not define it).  Zero is one of the values an uninitialised float may hold; taking it makes
    // the harness deterministic.  The only place the reference reads a default-constructed vec3 before writing it is
    // Mesh.cpp:19-21 (`glm::vec3 v; iss >> v.x >> v.y >> v.z;` when an extraction fails): the components AFTER the
    // failing one are whatever was on RayZen's stack, and no test may assert them.
    vec3() : x(0.0f), y(0.0f), z(0.0f) {}
    // type_vec3.inl: vec(T scalar): x(scalar), y(scalar), z(scalar).  BVH.cpp passes a float (FLT_MAX) and an int (0).
    explicit vec3(float s) : x(s), y(s), z(s) {}
    // type_vec3.inl: vec(T _x, T _y, T _z): x(_x), y(_y), z(_z)
    vec3(float _x, float _y, float _z) : x(_x), y(_y), z(_z) {}

    // type_vec3.inl, operator[](length_type i): `assert(i >= 0 && i < this->length());` and then a switch over i whose
    // `default:` label shares its statement with `case 0:` (-> x), `case 1:` -> y, `case 2:` -> z.  With NDEBUG the
    // assert is gone and ANY index outside 1..2 yields x.  BVH.cpp:140-144 indexes with axis == -1 when findSAHSplit
    // found no split and x is the widest extent: a release build of RayZen reads x there (a debug build aborts).  An
    // indexing written as (&x)[i] would read the stack instead.
    // The harness counts the reads that took the `default:` road with an index other than 0 (standin_out_of_range_reads,
    // below): that is how the fixtures flag the inputs that reach axis == -1, instead of guessing from the data.
    float& operator[](int i) {
        switch (i) {
        case 0: return x;
        case 1: return y;
        case 2: return z;
        default: ++standin_out_of_range_reads(); return x;
        }
    }
    const float& operator[](int i) const {
        switch (i) {
        case 0: return x;
        case 1: return y;
        case 2: return z;
        default: ++standin_out_of_range_reads(); return x;
        }
    }
    static unsigned long long& standin_out_of_range_reads() {      // not GLM: the harness's own tally (single-threaded use)
        static unsigned long long n = 0;
        return n;
    }
};

// type_vec3.inl, binary operators: each builds vec(v1.x OP v2.x, v1.y OP v2.y, v1.z OP v2.z), resp. (v.x OP scalar, ...).
// `/` is a true division per component (no reciprocal is formed), `*` one multiplication per component.
inline vec3 operator+(const vec3& a, const vec3& b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3& a, const vec3& b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(const vec3& v, float s) { return vec3(v.x * s, v.y * s, v.z * s); }
inline vec3 operator/(const vec3& v, float s) { return vec3(v.x / s, v.y / s, v.z / s); }

// func_common.inl: min(x, y) returns `(y < x) ? y : x`, max(x, y) returns `(x < y) ? y : x`; the vector forms apply the
// scalar one per component (detail::functor2).  With equal operands -- +0 against -0 included -- both return the FIRST
// argument, which is what decides the sign of a zero bound in computeBounds (BVH.cpp:16-17).
inline float min(float x, float y) { return (y < x) ? y : x; }
inline float max(float x, float y) { return (x < y) ? y : x; }
inline vec3 min(const vec3& a, const vec3& b) { return vec3(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
inline vec3 max(const vec3& a, const vec3& b) { return vec3(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }

// type_mat4x4.hpp: four column vec4s = 16 floats, 64 bytes.  The reference never computes with it in BVH.cpp / Mesh.cpp.
struct mat4 {
    float m[16];
    mat4() : m{} {}
};

}  // namespace glm

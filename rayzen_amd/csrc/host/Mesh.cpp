// Mesh.cpp -- OBJ reader with the exact quirks of RayZen/src/Mesh.cpp:6-50:
// only "v " and "f " lines; a face token is cut at its first '/'; indices are
// 1-based and never negative; polygons are fan-triangulated around their
// first vertex; everything else (vn, vt, o, g, s, usemtl ...) is ignored.
// Coordinates are read the way `std::istringstream >> float` reads them there (Mesh.cpp:18-20), not the way strtof does:
// pinned against the reference's own reader by tests/test_cppref.py (tests/golden/cppref_obj.npz).
#include "RayZenScene.h"

#include <cctype>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace rayzen {

// One `stream >> float` of libstdc++ in the "C" locale, on the text at p.  The stream skips white space, then gathers the
// longest run of the form [+-] digits [. digits] [e|E [+-] digits] -- an exponent letter only after a digit -- and nothing
// else: no `nan`, no `inf`, no hexadecimal.  The run goes through strtof; unless strtof takes all of it ("1e", "-", ".")
// the result is 0 and the stream fails.  Overflow stores +-FLT_MAX and fails the stream; underflow stores the denormal
// or the zero strtof returns and does not.  At the end of the line the stream fails and stores nothing.
// Returns false when the stream has failed: the reference's later extractions on that line then do nothing.
static bool extractFloat(const char*& p, float& value) {
    while (std::isspace((unsigned char)*p)) ++p;
    if (!*p) return false;
    std::string run;
    if (*p == '+' || *p == '-') run += *p++;
    bool mantissa = false, point = false, exponent = false;
    while (*p == '0') {                                   // leading zeros: one is kept
        if (!mantissa) { run += '0'; mantissa = true; }
        ++p;
    }
    for (;;) {
        if (*p >= '0' && *p <= '9') { run += *p++; mantissa = true; }
        else if (*p == '.' && !point && !exponent) { run += *p++; point = true; }
        else if ((*p == 'e' || *p == 'E') && !exponent && mantissa) {
            run += 'e'; ++p; exponent = true;
            if (*p == '+' || *p == '-') run += *p++;
        } else break;
    }
    char* end = nullptr;
    float f = std::strtof(run.c_str(), &end);
    if (end == run.c_str() || *end != 0) { value = 0.0f; return false; }
    if (f == HUGE_VALF) { value = FLT_MAX; return false; }
    if (f == -HUGE_VALF) { value = -FLT_MAX; return false; }
    value = f;
    return true;
}

bool Mesh::loadFromOBJ(const std::string& filename, int materialIndex) {
    FILE* f = std::fopen(filename.c_str(), "r");
    if (!f) {
        std::fprintf(stderr, "[ERROR] Failed to open OBJ file: %s\n", filename.c_str());
        return false;
    }
    std::vector<vec3> vertices;
    std::vector<unsigned> face;
    char* line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, f) >= 0) {
        if (line[0] == 'v' && line[1] == ' ') {
            vec3 v;                      // zero where the reference's `glm::vec3 v;` is left unwritten after a failure
            const char* p = line + 2;
            if (extractFloat(p, v.x) && extractFloat(p, v.y)) extractFloat(p, v.z);
            vertices.push_back(v);
        } else if (line[0] == 'f' && line[1] == ' ') {
            face.clear();
            char* save = nullptr;
            for (char* tok = strtok_r(line + 2, " \t\r\n\v\f", &save); tok; tok = strtok_r(nullptr, " \t\r\n\v\f", &save)) {
                if (char* slash = std::strchr(tok, '/')) *slash = 0;
                face.push_back((unsigned)std::atoi(tok));
            }
            if (face.size() >= 3) {
                for (size_t i = 1; i + 1 < face.size(); ++i) {
                    unsigned a = face[0] - 1, b = face[i] - 1, c = face[i + 1] - 1;
                    if (a >= vertices.size() || b >= vertices.size() || c >= vertices.size()) continue;  // reference: UB
                    Triangle tri;
                    std::memset(static_cast<void*>(&tri), 0, sizeof tri);   // tail padding travels to the GPU: keep it defined
                    tri.v0 = vertices[a];
                    tri.v1 = vertices[b];
                    tri.v2 = vertices[c];
                    tri.materialIndex = materialIndex;
                    triangles.push_back(tri);
                }
            }
        }
    }
    std::free(line);
    std::fclose(f);
    return true;
}

}  // namespace rayzen

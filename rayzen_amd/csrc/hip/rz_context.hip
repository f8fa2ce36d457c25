// rz_context.hip -- the C-ABI of include/rayzen_hip.h: context, uploads, the
// one-time re-layout of RayZen's SSBO arrays into the device structures of
// rz_scene_dev.h, launches and read-back.  Host code, compiled by hipcc.
// struct rz_ctx and what this file shares are declared in rz_ctx.h; the render calls (rz_render, rz_render_counted,
// rz_render_adaptive and the timing ring) are in rz_ctx_render.hip.
//
// Replaces, call for call, what RayZen/src/main.cpp does with OpenGL:
//   rz_upload     <- glGenBuffers+glBufferData+glBindBufferBase (main.cpp:1072-1119)
//   rz_update     <- glBufferSubData                            (main.cpp:1196-1207)
//   rz_set_frame  <- glUniform* in sendSceneDataToShader        (main.cpp:1356-1379)
//   rz_render     <- glDrawArrays(GL_TRIANGLE_FAN,0,4)          (main.cpp:637)
//   rz_sync       <- glFinish                                   (main.cpp:1347)
#include "rz_ctx.h"
#include "rz_device_math.h"      // RZ_MATH_FLAVOUR (rz_math_flavour())

using namespace rz;

namespace {

thread_local std::string g_last_error = "";

size_t elem_size(int b) {
    switch (b) {
        case RZ_BIND_TRIANGLES: return sizeof(rz_triangle);
        case RZ_BIND_MATERIALS: return sizeof(rz_material);
        case RZ_BIND_LIGHTS: return sizeof(rz_light);
        case RZ_BIND_TLAS_NODES: return sizeof(rz_bvh_node);
        case RZ_BIND_TLAS_INDICES: return sizeof(int32_t);
        case RZ_BIND_BLAS_NODES: return sizeof(rz_bvh_node);
        case RZ_BIND_BLAS_INDICES: return sizeof(int32_t);
        case RZ_BIND_INSTANCES: return sizeof(rz_bvh_instance);
        default: return 0;
    }
}
// (materials and lights have a host copy only: finalize uploads it whenever it has changed)
int group_of(int b) {
    switch (b) {
        case RZ_BIND_TRIANGLES: return kTris;
        case RZ_BIND_BLAS_NODES: case RZ_BIND_BLAS_INDICES: return kBlas;
        case RZ_BIND_INSTANCES: case RZ_BIND_TLAS_NODES: case RZ_BIND_TLAS_INDICES: return kTlas;
        default: return kNoGroup;
    }
}

}  // namespace

// ---- declared in rz_ctx.h: rz_ctx_render.hip calls these too ----
namespace rz {

int fail(rz_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try {
        if (c) c->err = buf;
        g_last_error = buf;
    } catch (...) { }     // the code still tells the caller what happened
    return code;
}

void alloc_point(rz_ctx* c) {
    if (c->failAllocCountdown > 0 && --c->failAllocCountdown == 0) throw std::bad_alloc();
}

int ensure(rz_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap && b.p) return RZ_OK;
    b.release();
    size_t want = std::max<size_t>(bytes, 256);
    RZ_HIP(c, hipMalloc(&b.p, want));
    b.cap = want;
    return RZ_OK;
}

// Scratch a launch can do without (the cross-claim pools: without them a claim works its parked paths off by itself, as in
// round 2): taken only if it leaves at least half of the device's free memory to the caller, and a refusal is not an error.
bool ensure_optional(DevBuf& b, size_t bytes) {
    if (bytes <= b.cap && b.p) return true;
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (bytes > (freeB + b.cap) / 2) return false;
    b.release();
    if (hipMalloc(&b.p, std::max<size_t>(bytes, 256)) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; b.cap = 0; return false; }
    b.cap = std::max<size_t>(bytes, 256);
    return true;
}

}  // namespace rz

namespace {

int upload_vec(rz_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    int rc = ensure(c, b, bytes);
    if (rc != RZ_OK) return rc;
    if (bytes) RZ_HIP(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return RZ_OK;
}

template <class T> const T* hostArr(const rz_ctx* c, int b) { return reinterpret_cast<const T*>(c->host[b].data()); }
template <class T> size_t hostCount(const rz_ctx* c, int b) { return c->host[b].size() / sizeof(T); }
size_t blasNodeCount(const rz_ctx* c) { return c->where[kBlas].host ? hostCount<rz_bvh_node>(c, RZ_BIND_BLAS_NODES) : c->devNodes; }
size_t blasIdxCount(const rz_ctx* c) { return c->where[kBlas].host ? hostCount<int32_t>(c, RZ_BIND_BLAS_INDICES) : c->devIdx; }

// ---- the four operations on a group's Residency (nothing else writes one) and the fetch they share ----------------------
// The device copy of a group brought to its host copy: one stream synchronisation, then the copies.  `skip`: a binding the
// caller is about to replace whole (rz_upload), which is not fetched; the others of its group must survive on the host.
int fetch_host(rz_ctx* c, int g, int skip) {
    struct Part { int binding; const DevBuf* src; size_t bytes; } parts[3];
    int n = 0;
    if (g == kTris) {
        parts[n++] = {RZ_BIND_TRIANGLES, &c->dRawTris, c->host[RZ_BIND_TRIANGLES].size()};
    } else if (g == kBlas) {
        parts[n++] = {RZ_BIND_BLAS_NODES, &c->dRawNodes, c->devNodes * sizeof(rz_bvh_node)};
        parts[n++] = {RZ_BIND_BLAS_INDICES, &c->dRawIdx, c->devIdx * sizeof(int32_t)};
        alloc_point(c);
    } else {        // (3.4 KB at 16 instances)
        parts[n++] = {RZ_BIND_INSTANCES, &c->dInstRef, c->host[RZ_BIND_INSTANCES].size()};
        parts[n++] = {RZ_BIND_TLAS_NODES, &c->dTlasNodes, (size_t)c->tlasHostCounts[0] * sizeof(rz_bvh_node)};
        parts[n++] = {RZ_BIND_TLAS_INDICES, &c->dTlasIdx, (size_t)c->tlasHostCounts[1] * sizeof(int32_t)};
    }
    if (n == 1 && parts[0].binding == skip) return RZ_OK;
    for (int k = 0; k < n; ++k)
        if (parts[k].binding != skip) c->host[parts[k].binding].resize(parts[k].bytes);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < n; ++k)
        if (parts[k].binding != skip && parts[k].bytes)
            RZ_HIP(c, hipMemcpy(c->host[parts[k].binding].data(), parts[k].src->p, parts[k].bytes, hipMemcpyDeviceToHost));
    return RZ_OK;
}

// Need host: whoever reads the host copy asks first.  A look: the device side stays as it was.
int need_host(rz_ctx* c, int g, int skip = -1) {
    if (c->where[g].host) return RZ_OK;
    const int rc = fetch_host(c, g, skip);
    if (rc == RZ_OK) c->where[g].host = true;
    return rc;
}

// Host changed: whoever writes the host copy, or lays the device scene out from it, takes the group to the host.
int host_changed(rz_ctx* c, int g, int skip = -1) {
    const int rc = need_host(c, g, skip);
    if (rc != RZ_OK) return rc;
    c->where[g].dev = false;
    if (g == kBlas) c->devRoots.clear();        // (they described the device copy)
    return RZ_OK;
}

// Device changed: a kernel or a device-to-device copy wrote the device copy.  Device mirrors host: the host copy was uploaded as it stands.
void device_changed(rz_ctx* c, int g) { c->where[g].host = false; c->where[g].dev = true; }
void device_mirrors_host(rz_ctx* c, int g) { c->where[g].host = c->where[g].dev = true; }

void drop_layout(rz_ctx* c) { c->views.clear(); c->hPairs.clear(); c->hTris.clear(); c->triNValid = -1; }
void drop_built_costs(rz_ctx* c) { c->costBuilt.clear(); c->costGen = ~0ull; }    // new trees: their "built" costs are measured again

// Lay out one BLAS: breadth-first walk from its root, one DevPair per internal
// node (so the hot top levels are contiguous), triangles gathered to leaf order.
int build_view(rz_ctx* c, int nodeOff, int triOff, int gTriOff, BlasView& V) {
    for (int g : {kBlas, kTris}) { const int rc = need_host(c, g); if (rc != RZ_OK) return rc; }
    const rz_bvh_node* nodes = hostArr<rz_bvh_node>(c, RZ_BIND_BLAS_NODES);
    const int32_t* idx = hostArr<int32_t>(c, RZ_BIND_BLAS_INDICES);
    const rz_triangle* tris = hostArr<rz_triangle>(c, RZ_BIND_TRIANGLES);
    const long long nNodes = (long long)hostCount<rz_bvh_node>(c, RZ_BIND_BLAS_NODES);
    const long long nIdx = (long long)hostCount<int32_t>(c, RZ_BIND_BLAS_INDICES);
    const long long nTris = (long long)hostCount<rz_triangle>(c, RZ_BIND_TRIANGLES);
    if (nodeOff < 0 || nodeOff >= nNodes) return fail(c, RZ_ERR_BAD_SCENE, "instance blasNodeOffset %d outside the BLAS node array (%lld)", nodeOff, nNodes);
    V.pairBase = (int)c->hPairs.size();
    V.triBase = (int)c->hTris.size();
    const rz_bvh_node& root = nodes[nodeOff];
    std::memcpy(V.rootMin, root.boundsMin, 12);
    std::memcpy(V.rootMax, root.boundsMax, 12);

    // slot s of this view's leaf-ordered triangle range <-> blasTriIndices[triOff + s]
    auto leafEnc = [&](const rz_bvh_node& n, int& enc) -> int {
        if (n.count > 15) return fail(c, RZ_ERR_BAD_SCENE, "BLAS leaf with %d triangles (max 15)", n.count);
        if (n.leftFirst < 0 || (long long)triOff + n.leftFirst + n.count > nIdx || triOff < 0)
            return fail(c, RZ_ERR_BAD_SCENE, "BLAS leaf range [%d,+%d) outside the index array", n.leftFirst, n.count);
        enc = ~((n.leftFirst << 4) | n.count);
        return RZ_OK;
    };
    int maxSlot = 0;
    V.depth = 1;
    if (root.count >= 0) {      // the root is a leaf (count 0: empty mesh, BVH.cpp:115-118)
        V.empty = (root.count == 0);
        int rc = leafEnc(root, V.rootEnc);
        if (rc != RZ_OK) return rc;
        maxSlot = root.leftFirst + root.count;
    } else {
        struct Item { int node; int depth; };
        std::vector<Item> queue;
        queue.push_back({0, 1});
        V.rootEnc = 0;          // the root's pair is pair 0 of the view
        size_t head = 0;
        // pair index of an internal node = its rank among internal nodes in BFS order
        while (head < queue.size()) {
            Item it = queue[head++];
            const rz_bvh_node& n = nodes[nodeOff + it.node];
            const int L = n.leftFirst, R = n.leftFirst + 1;
            if (L < 1 || (long long)nodeOff + R >= nNodes)
                return fail(c, RZ_ERR_BAD_SCENE, "BLAS node %d has children %d,%d outside the node array", it.node, L, R);
            if (queue.size() > (size_t)nNodes) return fail(c, RZ_ERR_BAD_SCENE, "BLAS at node offset %d is not a tree", nodeOff);
            DevPair P{};
            const rz_bvh_node& ln = nodes[nodeOff + L];
            const rz_bvh_node& rn = nodes[nodeOff + R];
            P.lx[0] = ln.boundsMin[0]; P.lx[1] = ln.boundsMax[0]; P.ly[0] = ln.boundsMin[1]; P.ly[1] = ln.boundsMax[1];
            P.lz[0] = ln.boundsMin[2]; P.lz[1] = ln.boundsMax[2];
            P.rx[0] = rn.boundsMin[0]; P.rx[1] = rn.boundsMax[0]; P.ry[0] = rn.boundsMin[1]; P.ry[1] = rn.boundsMax[1];
            P.rz[0] = rn.boundsMin[2]; P.rz[1] = rn.boundsMax[2];
            // (an inverted or NaN child box: the octant-specialised slab test is only the shader's test for regular boxes)
            if (!(ln.boundsMin[0] <= ln.boundsMax[0] && ln.boundsMin[1] <= ln.boundsMax[1] && ln.boundsMin[2] <= ln.boundsMax[2] &&
                  rn.boundsMin[0] <= rn.boundsMax[0] && rn.boundsMin[1] <= rn.boundsMax[1] && rn.boundsMin[2] <= rn.boundsMax[2]))
                c->irregularBoxes = true;
            V.depth = std::max(V.depth, it.depth + 1);
            const rz_bvh_node* ch[2] = {&ln, &rn};
            int32_t* encs[2] = {&P.lenc, &P.renc};
            const int chIdx[2] = {L, R};
            for (int k = 0; k < 2; ++k) {
                if (ch[k]->count >= 0) {
                    int e; int rc = leafEnc(*ch[k], e);
                    if (rc != RZ_OK) return rc;
                    *encs[k] = e;
                    maxSlot = std::max(maxSlot, ch[k]->leftFirst + ch[k]->count);
                } else {
                    *encs[k] = (int)queue.size();      // BFS rank of this internal child == its pair index
                    queue.push_back({chIdx[k], it.depth + 1});
                }
            }
            alloc_point(c);
            c->hPairs.push_back(P);
        }
        // queue[i] is the i-th internal node in BFS order and its pair was pushed i-th: enc == i holds by construction
    }
    // gather triangles into leaf order
    bool viewGlass = false;
    for (int s = 0; s < maxSlot; ++s) {
        const long long src = (long long)gTriOff + idx[triOff + s];
        if (src < 0 || src >= nTris) return fail(c, RZ_ERR_BAD_SCENE, "BLAS index %d -> triangle %lld outside the triangle array (%lld)", s, src, nTris);
        const rz_triangle& t = tris[src];
        DevTri d{};
        d.v0[0] = t.v0[0]; d.v0[1] = t.v0[1]; d.v0[2] = t.v0[2];
        d.e1x = t.v1[0] - t.v0[0]; d.e1y = t.v1[1] - t.v0[1]; d.e1z = t.v1[2] - t.v0[2];   // FS:392
        d.e2x = t.v2[0] - t.v0[0]; d.e2y = t.v2[1] - t.v0[1]; d.e2z = t.v2[2] - t.v0[2];   // FS:393
        d.mat = t.materialIndex;
        {   // (hint only: an index the material check will reject later counts as "may be transparent")
            const int nMat_ = (int)hostCount<rz_material>(c, RZ_BIND_MATERIALS);
            const rz_material* mats_ = hostArr<rz_material>(c, RZ_BIND_MATERIALS);
            if (t.materialIndex < 0 || t.materialIndex >= nMat_ || !(mats_[t.materialIndex].transparency <= 0.0f)) viewGlass = true;
        }
        d.src = (int32_t)src;
        if ((s & 1023) == 0) alloc_point(c);
        c->hTris.push_back(d);
    }
    V.mayGlass = viewGlass;
    V.nSlots = maxSlot;
    V.nPairs = (int)c->hPairs.size() - V.pairBase;
    return RZ_OK;
}

// The TLAS as the list of its nodes in the order FS:464-501 pops them (right child first), with the position that follows
// each subtree (TlasDfs, rz_scene_dev.h).  `below` is the number of stack entries under a node when it is popped: the
// shader's stack[64] holds no more, and the oracle drops a push that would not fit -- such a node never expands (count 0).
// Call after tlas_depth() has accepted the array (children in range, no more pops than nodes).
void tlas_pop_order(const rz_bvh_node* n, size_t count, const int32_t* idx, std::vector<TlasDfs>& out) {
    out.clear();
    if (count == 0) return;
    struct Item { int node, below, parentPos; };
    std::vector<Item> st;
    std::vector<int> parent;
    st.push_back({0, 0, -1});
    while (!st.empty()) {
        const Item it = st.back();
        st.pop_back();
        const rz_bvh_node& N = n[it.node];
        TlasDfs R{};
        std::memcpy(R.bmin, N.boundsMin, 12);
        std::memcpy(R.bmax, N.boundsMax, 12);
        R.first = N.leftFirst;
        R.count = N.count > 0 ? N.count : (N.count < 0 && it.below + 2 <= 64 ? -1 : 0);
        R.inst0 = N.count > 0 ? idx[N.leftFirst] : 0;
        const int pos = (int)out.size();
        out.push_back(R);
        parent.push_back(it.parentPos);
        if (N.count < 0) {                                          // (also under a node that never expands: the list is complete, like the device builder's)
            st.push_back({N.leftFirst, it.below, pos});             // popped after the right subtree, with the same entries below it
            st.push_back({N.leftFirst + 1, it.below + 1, pos});     // popped next, the left child below it
        }
    }
    std::vector<int> size(out.size(), 1);
    for (size_t p = out.size(); p-- > 1;) size[parent[p]] += size[p];
    for (size_t p = 0; p < out.size(); ++p) out[p].skip = (int)p + size[p];
}

int tlas_depth(const rz_bvh_node* n, size_t count) {
    if (count == 0) return 0;
    int best = 1;
    std::vector<std::pair<int, int>> st;
    st.push_back({0, 1});
    size_t visited = 0;
    while (!st.empty()) {
        auto [i, d] = st.back();
        st.pop_back();
        if (++visited > count) return -1;
        best = std::max(best, d);
        if (n[i].count <= 0) {   // the shader treats count <= 0 as internal (FS:470)
            if (n[i].count == 0) continue;     // empty root written by the host builder
            int L = n[i].leftFirst;
            if (L < 1 || (size_t)L + 1 >= count) return -1;
            st.push_back({L, d + 1});
            st.push_back({L + 1, d + 1});
        }
    }
    return best;
}

// Device re-layout of one view (rz_relayout.hip).  RZ_OK: V filled; 1: the arrays are inconsistent or something did
// not fit -- run the host re-layout, which words the error; other negatives: a HIP failure.
bool host_relayout_forced(const rz_ctx* c) {
    if (c->flags & RZ_FLAG_HOST_RELAYOUT) return true;
    const char* e = std::getenv("RZ_HOST_RELAYOUT");
    return e && *e && *e != '0';
}

int prepare_device_relayout(rz_ctx* c) {       // raw arrays + materials on the device, output buffers sized, scratch
    const size_t nNodes = blasNodeCount(c), nIdx = blasIdxCount(c);
    int rc;
    // a group goes up exactly when its device copy is not current (rz_build_geometry, a device refit, rz_rebuild_geometry left theirs there)
    if (!c->where[kBlas].dev) {
        rc = upload_vec(c, c->dRawNodes, c->host[RZ_BIND_BLAS_NODES].data(), c->host[RZ_BIND_BLAS_NODES].size());
        if (rc != RZ_OK) return rc;
        rc = upload_vec(c, c->dRawIdx, c->host[RZ_BIND_BLAS_INDICES].data(), c->host[RZ_BIND_BLAS_INDICES].size());
        if (rc != RZ_OK) return rc;
        device_mirrors_host(c, kBlas);
    }
    if (!c->where[kTris].dev) {
        rc = upload_vec(c, c->dRawTris, c->host[RZ_BIND_TRIANGLES].data(), c->host[RZ_BIND_TRIANGLES].size());
        if (rc != RZ_OK) return rc;
        device_mirrors_host(c, kTris);
    }
    rc = ensure(c, c->dPairs, std::max<size_t>(nNodes, 1) * sizeof(DevPair));
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dTris, std::max<size_t>(nIdx, 1) * sizeof(DevTri));
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dRelayoutWs, relayout_workspace_bytes(nNodes));
    if (rc != RZ_OK) return rc;
    if (!c->relayoutPinned) RZ_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->relayoutPinned), 64, hipHostMallocDefault));
    return RZ_OK;
}

int device_view(rz_ctx* c, int nodeOff, int triOff, int gTriOff, BlasView& V) {
    const long long nNodes = (long long)blasNodeCount(c);
    const long long nIdx = (long long)blasIdxCount(c);
    const long long nTris = (long long)hostCount<rz_triangle>(c, RZ_BIND_TRIANGLES);
    if (nodeOff < 0 || nodeOff >= nNodes) return 1;
    rz_bvh_node root;
    if (!c->where[kBlas].host) {
        auto it = c->devRoots.find(nodeOff);
        if (it == c->devRoots.end()) return 1;      // an instance that does not start at a mesh's root: let the host path look at it
        root = it->second;
    } else {
        root = hostArr<rz_bvh_node>(c, RZ_BIND_BLAS_NODES)[nodeOff];
    }
    RelayoutView R{};
    unsigned viewFlags = 0;         // bit 0: a triangle of this view uses a transparent material, bit 1: an irregular child box
    R.nodeOff = nodeOff; R.triOff = triOff; R.gTriOff = gTriOff;
    R.pairBase = (int)c->devPairsUsed; R.triBase = (int)c->devTrisUsed;
    const int rc = relayout_view_device(static_cast<const rz_bvh_node*>(c->dRawNodes.p), nNodes, static_cast<const int32_t*>(c->dRawIdx.p), nIdx,
                                        static_cast<const rz_triangle*>(c->dRawTris.p), nTris, static_cast<const rz_material*>(c->dMat.p),
                                        (int)hostCount<rz_material>(c, RZ_BIND_MATERIALS), root, R,
                                        static_cast<DevPair*>(c->dPairs.p), (long long)(c->dPairs.cap / sizeof(DevPair)),
                                        static_cast<DevTri*>(c->dTris.p), (long long)(c->dTris.cap / sizeof(DevTri)), c->dRelayoutWs.p,
                                        c->dRelayoutWs.cap, c->relayoutPinned, &viewFlags, c->stream);
    if (rc < 0) return fail(c, RZ_ERR_HIP, "device re-layout: %s", hipGetErrorString((hipError_t)(-rc)));
    if (rc > 0) return 1;
    c->devTransparent |= viewFlags;
    V.mayGlass = (viewFlags & 1u) != 0;
    V.irregular = (viewFlags & 2u) != 0;
    V.nPairs = R.nPairs; V.nSlots = R.nSlots;
    V.pairBase = R.pairBase; V.triBase = R.triBase; V.rootEnc = R.rootEnc; V.depth = R.depth; V.empty = R.empty != 0;
    std::memcpy(V.rootMin, R.rootMin, 12); std::memcpy(V.rootMax, R.rootMax, 12);
    c->devPairsUsed += R.nPairs; c->devTrisUsed += R.nSlots;
    return RZ_OK;
}

int finalize_body(rz_ctx* c) {
    if (!(c->geomDirty || c->instDirty || c->tlasDirty || c->matDirty || c->lightDirty)) return RZ_OK;
    for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS, RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES,
                  RZ_BIND_BLAS_NODES, RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES})
        if (!c->present[b]) return fail(c, RZ_ERR_NOT_READY, "binding %d has not been uploaded", b);

    // (the per-view "may hold transparent triangles" hints were taken from the materials of the moment the views were laid out)
    if (c->geomDirty) c->matChangedSinceLayout = false;
    else if (c->matDirty && !c->matChangedSinceLayout) { c->matChangedSinceLayout = true; c->instDirty = true; }
    // materials first: the device re-layout checks triangle material indices against them
    if (c->matDirty) {
        int rc = upload_vec(c, c->dMat, c->host[RZ_BIND_MATERIALS].data(), c->host[RZ_BIND_MATERIALS].size());
        if (rc != RZ_OK) return rc;
    }
    if (c->geomDirty) {
        // the traversal addresses a BLAS's pairs with a 32-bit byte offset (rz_trace.h: sload16_off): < 2^26 pairs per BLAS
        const size_t nodesNow = blasNodeCount(c);
        if (nodesNow >= ((size_t)1 << 27))
            return fail(c, RZ_ERR_BAD_SCENE, "BLAS node array holds %zu nodes; the limit is %zu", nodesNow, ((size_t)1 << 27) - 1);
        drop_layout(c);
        c->instDirty = true;
        c->devPairsUsed = c->devTrisUsed = 0; c->devTransparent = 0; c->irregularBoxes = false;
        c->layoutOnDevice = !host_relayout_forced(c);
        if (c->layoutOnDevice) { int rc = prepare_device_relayout(c); if (rc != RZ_OK) return rc; }
    }
    // instances and TLAS are laid out from their host copies: what rz_update_transforms left on the device is no longer in force
    if (c->instDirty || c->tlasDirty) { int rc = host_changed(c, kTlas); if (rc != RZ_OK) return rc; }
    if (c->instDirty) {
        const rz_bvh_instance* inst = hostArr<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
        const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
        alloc_point(c);
        std::vector<DevInstance> dev(nInst);
        ++c->layoutGen;             // (what rz_refit_geometry derived from the last layout is void)
        // Pass 1: lay out every BLAS view the instances name that is not laid out yet -- on the device
        // (rz_relayout.hip), or, if that finds the arrays inconsistent (or is switched off), on the host, which
        // also words the error.
        for (int attempt = 0; attempt < 2; ++attempt) {
            bool redo = false, grew = false;
            for (size_t i = 0; i < nInst && !redo; ++i) {
                auto key = std::make_tuple(inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset);
                if (c->views.find(key) != c->views.end()) continue;
                BlasView V;
                int rc;
                if (c->layoutOnDevice) {
                    rc = device_view(c, inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset, V);
                    if (rc == 1) {          // start over on the host (build_view asks for the host copies it reads)
                        c->layoutOnDevice = false;
                        drop_layout(c);
                        redo = true;
                        break;
                    }
                } else {
                    rc = build_view(c, inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset, V);
                }
                if (rc != RZ_OK) { drop_layout(c); c->geomDirty = true; return rc; }
                c->views.emplace(key, V);
                grew = true;
            }
            if (redo) continue;
            if (!c->layoutOnDevice && (grew || c->geomDirty)) {
                int rc = upload_vec(c, c->dPairs, c->hPairs.data(), c->hPairs.size() * sizeof(DevPair));
                if (rc != RZ_OK) return rc;
                rc = upload_vec(c, c->dTris, c->hTris.data(), c->hTris.size() * sizeof(DevTri));
                if (rc != RZ_OK) return rc;
            }
            break;
        }
        {   // per-triangle geometric normals of everything laid out (rz_relayout.hip: rl_tri_normals)
            const long long nLaid = c->layoutOnDevice ? (long long)c->devTrisUsed : (long long)c->hTris.size();
            if (nLaid != c->triNValid) {        // (views are only ever appended between two geometry uploads)
                int rc = ensure(c, c->dTriN, (size_t)std::max<long long>(nLaid, 1) * sizeof(DevTriN));
                if (rc != RZ_OK) return rc;
                const int nrc = tri_normals_device(static_cast<const DevTri*>(c->dTris.p), nLaid, static_cast<DevTriN*>(c->dTriN.p), c->stream);
                if (nrc != 0) return fail(c, RZ_ERR_HIP, "triangle normals: %s", hipGetErrorString((hipError_t)(-nrc)));
                c->triNValid = nLaid;
            }
        }
        c->maxBlasDepth = 1;
        c->rayInstOffStale = true;
        for (size_t i = 0; i < nInst; ++i) {
            const BlasView& V = c->views.at(std::make_tuple(inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset));
            DevInstance& D = dev[i];
            std::memset(&D, 0, sizeof D);
            for (int col = 0; col < 4; ++col)
                for (int row = 0; row < 3; ++row) {
                    D.inv[col * 3 + row] = inst[i].inverseTransform[col * 4 + row];
                    D.fwd[col * 3 + row] = inst[i].transform[col * 4 + row];
                }
            std::memcpy(D.rootMin, V.rootMin, 12);
            std::memcpy(D.rootMax, V.rootMax, 12);
            D.rootEnc = V.rootEnc;
            D.pairBase = V.pairBase;
            D.triBase = V.triBase;
            // bit 0: never hit (empty BLAS).  bit 1: the view may hold transparent triangles -- a hint for the compacting claims
            // (which rays not to park: rz_kernels.hip); when only the materials have changed since the views were laid out
            // nobody knows any more, and every instance says "may"
            D.flags = (V.empty ? 1 : 0) | ((V.mayGlass || c->matChangedSinceLayout) ? 2 : 0);
        }
        for (auto& kv : c->views) c->maxBlasDepth = std::max(c->maxBlasDepth, kv.second.depth);
        int rc = upload_vec(c, c->dInst, dev.data(), dev.size() * sizeof(DevInstance));
        if (rc != RZ_OK) return rc;
        // the staging vector dies at scope exit: the copy must have left it
        RZ_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (c->tlasDirty || c->instDirty) {
        const rz_bvh_node* tn = hostArr<rz_bvh_node>(c, RZ_BIND_TLAS_NODES);
        const size_t nTn = hostCount<rz_bvh_node>(c, RZ_BIND_TLAS_NODES);
        const int32_t* ti = hostArr<int32_t>(c, RZ_BIND_TLAS_INDICES);
        const size_t nTi = hostCount<int32_t>(c, RZ_BIND_TLAS_INDICES);
        const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
        int d = tlas_depth(tn, nTn);
        if (d < 0) return fail(c, RZ_ERR_BAD_SCENE, "TLAS node array is not a tree");
        for (size_t i = 0; i < nTn; ++i)
            if (tn[i].count > 0) {
                if (tn[i].leftFirst < 0 || (size_t)tn[i].leftFirst + (size_t)tn[i].count > nTi)
                    return fail(c, RZ_ERR_BAD_SCENE, "TLAS leaf %zu range outside the TLAS index array", i);
                for (int k = 0; k < tn[i].count; ++k) {
                    int ii = ti[tn[i].leftFirst + k];
                    if (ii < 0 || (size_t)ii >= nInst)
                        return fail(c, RZ_ERR_BAD_SCENE, "TLAS index %d names instance %d of %zu", tn[i].leftFirst + k, ii, nInst);
                }
            }
        c->tlasDepth = std::max(d, 1);
        int rc = upload_vec(c, c->dTlasNodes, tn, nTn * sizeof(rz_bvh_node));
        if (rc != RZ_OK) return rc;
        rc = upload_vec(c, c->dTlasIdx, ti, nTi * sizeof(int32_t));
        if (rc != RZ_OK) return rc;
        std::vector<TlasDfs> dfs;
        tlas_pop_order(tn, nTn, ti, dfs);
        c->nTlasDfs = (int)dfs.size();
        c->tlasEntry = tlas_entry_verdict(dfs.data(), c->nTlasDfs);
        rc = upload_vec(c, c->dTlasDfs, dfs.data(), dfs.size() * sizeof(TlasDfs));
        if (rc != RZ_OK) return rc;
        RZ_HIP(c, hipStreamSynchronize(c->stream));     // the staging vector dies at scope exit
    }
    if (c->lightDirty) {
        int rc = upload_vec(c, c->dLight, c->host[RZ_BIND_LIGHTS].data(), c->host[RZ_BIND_LIGHTS].size());
        if (rc != RZ_OK) return rc;
    }
    // material indices are data the kernels index with: check them once
    if (c->geomDirty || c->matDirty || c->instDirty) {
        const int nMat = (int)hostCount<rz_material>(c, RZ_BIND_MATERIALS);
        const rz_material* mats = hostArr<rz_material>(c, RZ_BIND_MATERIALS);
        bool transparent = false;
        if (c->layoutOnDevice) {
            // the gather of rz_relayout.hip checked the triangles it laid out against the materials uploaded above; when
            // only the materials changed, every laid-out triangle is checked again on the device
            if (c->matDirty && !c->geomDirty) {
                unsigned tr = 0; int detail = 0;
                const int rc = relayout_check_materials_device(static_cast<const DevTri*>(c->dTris.p), c->devTrisUsed, static_cast<const rz_material*>(c->dMat.p),
                                                               nMat, c->dRelayoutWs.p, c->relayoutPinned, &tr, &detail, c->stream);
                if (rc < 0) return fail(c, RZ_ERR_HIP, "material check: %s", hipGetErrorString((hipError_t)(-rc)));
                if (rc > 0) return fail(c, RZ_ERR_BAD_SCENE, "triangle %d has a materialIndex outside the %d materials uploaded", detail, nMat);
                c->devTransparent = (c->devTransparent & 2u) | (tr & 1u);
            }
            transparent = (c->devTransparent & 1u) != 0;
            c->irregularBoxes = (c->devTransparent & 2u) != 0;
        } else {
            for (const DevTri& t : c->hTris) {
                if (t.mat < 0 || t.mat >= nMat)
                    return fail(c, RZ_ERR_BAD_SCENE, "triangle %d has materialIndex %d, %d materials uploaded", t.src, t.mat, nMat);
                transparent = transparent || (mats[t.mat].transparency > 0.0f) || !(mats[t.mat].transparency == mats[t.mat].transparency);
            }
        }
        c->sceneHasTransparency = transparent;
    }
    // uploads read the caller-visible host copies: let them land before rz_update may patch those
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    c->geomDirty = c->instDirty = c->tlasDirty = c->matDirty = c->lightDirty = false;
    return RZ_OK;
}

long long tlas_index_count(const rz_ctx* c) {
    return c->where[kTlas].host ? (long long)hostCount<int32_t>(c, RZ_BIND_TLAS_INDICES) : (long long)c->tlasHostCounts[1];
}

unsigned* backstop_word(const rz_ctx* c) { return static_cast<unsigned*>(c->dGroupCtr.p) + RZ_ERRWORD; }

// Did a kernel run into one of its "cannot happen" bounds?  (rz_kernels.hip: rz_backstop)  Reads the word on the idle device
// (the caller has just synchronised) and clears it when set.  No counter yet: nothing that can set it has run, no bits.
int take_backstop(rz_ctx* c, unsigned& bits) {
    bits = 0;
    if (!c->dGroupCtr.p) return RZ_OK;
    unsigned* w = backstop_word(c);
    RZ_HIP(c, hipMemcpy(&bits, w, sizeof bits, hipMemcpyDeviceToHost));
    if (bits != 0u) RZ_HIP(c, hipMemset(w, 0, sizeof bits));
    return RZ_OK;
}

// a host-path call reads (and clears) the backstop word its launches may have set
int report_backstop(rz_ctx* c, const char* what, const char* consequence) {
    unsigned bits = 0;
    const int rc = take_backstop(c, bits);
    if (rc != RZ_OK) return rc;
    if (bits != 0u) return fail(c, RZ_ERR_INTERNAL, "%s: a kernel reached a backstop (bits 0x%x): %s", what, bits, consequence);
    return RZ_OK;
}

// What every kernel that walks the scene reads of it (render_samples / render_pixels, rz_rays.hip).
void scene_kparams(const rz_ctx* c, KParams& K) {
    K.pairs = static_cast<const DevPair*>(c->dPairs.p);
    K.tris = static_cast<const DevTri*>(c->dTris.p);
    K.triN = static_cast<const DevTriN*>(c->dTriN.p);
    K.instances = static_cast<const DevInstance*>(c->dInst.p);
    K.tlasDfs = static_cast<const TlasDfs*>(c->dTlasDfs.p);
    K.tlasIndices = static_cast<const int32_t*>(c->dTlasIdx.p);
    K.materials = static_cast<const DevMaterial*>(c->dMat.p);
    K.lights = static_cast<const DevLight*>(c->dLight.p);
    K.nTlasDfs = c->nTlasDfs;
    K.nMaterials = (int)hostCount<rz_material>(c, RZ_BIND_MATERIALS);
    K.blasStackCap = std::max(1, c->maxBlasDepth - 1);
    // a pop followed by two pushes never holds more entries than the tree has levels (FS:460: stack[64])
    K.tlasStackCap = 0;         // the TLAS walk keeps no stack (rz_trace.h: trace_closest)
    K.traceRoundCap = (int)std::min<long long>(0x7fffffff, tlas_index_count(c) + (long long)c->nTlasDfs + 64);
    K.regularBoxes = c->irregularBoxes ? 0 : 1;
#if RZ_TLAS_ENTRY
    K.tlasEntry = c->tlasEntry;
#endif
}

// ... and of the camera, for the kernels that cast one ray per pixel outside the frame loop: the scene as finalize left it,
// seen through this camera at this size.
void camera_kparams(const rz_ctx* c, KParams& K, int width, int height, const float* inv_view, const float* inv_proj, const float* cam_pos) {
    scene_kparams(c, K);
    K.width = width; K.height = height;
    std::memcpy(K.invView, inv_view, 64);
    std::memcpy(K.invProj, inv_proj, 64);
    std::memcpy(K.camPos, cam_pos, 12);
}

// What the guide casts share: the frame's camera at width x height, a wave per 64-pixel run of a row, the offsets and the word
// cast_ready made, and the BLAS stack of the launch (fixedLds: what the kernel keeps in LDS per wave beside the stack).
template <class Launch>
int cast_wiring(rz_ctx* c, int width, int height, KParams& K, Launch& G, size_t fixedLds = 0) {
    const rz_frame_params& f = c->frame;
    camera_kparams(c, K, width, height, f.inv_view, f.inv_proj, f.cam_pos);
    G.unitsX = (width + 63) / 64;
    G.units = (long long)G.unitsX * height;
    G.grid = rays_grid(G.units * 64);
    G.instTriOff = static_cast<const int32_t*>(c->dRayInstOff.p);
    G.errWord = backstop_word(c);
    return size_blas_stack(c, K, fixedLds, RZ_RAYS_WAVES_PER_CU, G.grid, c->dRayOvf);
}

// Where a pass reads its input and writes its outputs.  On the device path the caller's pointers are device pointers: nothing
// is staged and dev() hands them back.  Host buffers are staged through the ray-query buffers of the context: the input in
// dRayIn; in dRayOut the outputs that were asked for (a null pointer: not asked), in the order they were added, each starting
// on a 16-byte boundary.
struct HostStage {
    rz_ctx* c;
    bool host;
    struct { void* ptr; size_t bytes, off; } out[4] = {};
    int n = 0;
    size_t total = 0;
    HostStage(rz_ctx* ctx, bool hostPath) : c(ctx), host(hostPath) {}
    int add(void* ptr, size_t bytes) {          // returns the output's slot
        out[n] = {ptr, bytes, (total + 15) & ~size_t(15)};
        if (ptr) total = out[n].off + bytes;
        return n++;
    }
    // copies a host input (if given) to dRayIn on the stream and points `dev` at it
    template <class T>
    int input(const T* src, size_t bytes, const T*& dev) {
        if (!host || !src) return RZ_OK;
        const int rc = ensure(c, c->dRayIn, bytes);
        if (rc != RZ_OK) return rc;
        RZ_HIP(c, hipMemcpyAsync(c->dRayIn.p, src, bytes, hipMemcpyHostToDevice, c->stream));
        dev = static_cast<const T*>(c->dRayIn.p);
        return RZ_OK;
    }
    int place() { return host && total ? ensure(c, c->dRayOut, total) : RZ_OK; }
    // where the kernels write an output, after place(); null when it was not asked for
    template <class T>
    T* dev(int slot) const {
        if (!host || !out[slot].ptr) return static_cast<T*>(out[slot].ptr);
        return reinterpret_cast<T*>(static_cast<char*>(c->dRayOut.p) + out[slot].off);
    }
    // host path: copies the outputs back in the order they were added and waits for the stream
    int fetch() {
        const char* base = static_cast<const char*>(c->dRayOut.p);
        for (int k = 0; k < n; ++k)
            if (out[k].ptr) RZ_HIP(c, hipMemcpyAsync(out[k].ptr, base + out[k].off, out[k].bytes, hipMemcpyDeviceToHost, c->stream));
        RZ_HIP(c, hipStreamSynchronize(c->stream));
        return RZ_OK;
    }
};

}  // namespace

// ---- declared in rz_ctx.h, as above ----
namespace rz {

// A failure half-way through the re-layout (an exception from a growing vector) must not leave a half-built scene
// behind: drop the derived state, keep the caller's arrays, and let the next call redo it.
int finalize(rz_ctx* c) {
    try {
        return finalize_body(c);
    } catch (...) {
        drop_layout(c);
        c->geomDirty = true;
        throw;
    }
}

// The claim counter (word 0, zeroed per launch) and the backstop word (word RZ_ERRWORD, zeroed when made and when reported).
int ensure_group_counter(rz_ctx* c) {
    if (c->dGroupCtr.p) return RZ_OK;
    // (+ a row of 64 zeros at byte 512, read by every wave's ordered sums in place of a dark unit's light rows: rz_kernels.hip, zero_row)
    int rc = ensure(c, c->dGroupCtr, 1024);
    if (rc != RZ_OK) return rc;
    RZ_HIP(c, hipMemsetAsync(c->dGroupCtr.p, 0, 1024, c->stream));
    return RZ_OK;
}

// The BLAS stack of a launch of one-wave workgroups (K.blasStackCap entries per lane needed).  LDS budget: the stack's LDS
// window is cut to what keeps `wavesPerCu` waves on a CU beside `fixedLds` bytes of other LDS per wave; deeper entries go to
// global overflow columns in `ovf`, which are indexed by resident workgroup and therefore only exist for persistent launches
// (`residentWaves` > 0: the grid).  Sets K.blasStackCap (the window, when one is cut), K.blasOvfCap and K.blasOvf.
int size_blas_stack(rz_ctx* c, KParams& K, size_t fixedLds, int wavesPerCu, long long residentWaves, DevBuf& ovf) {
    const int need = K.blasStackCap;
    const size_t budget = (size_t)160 * 1024 / wavesPerCu;
    int window = budget > fixedLds ? (int)((budget - fixedLds) / 512) : 0;
    if (const char* e = std::getenv("RZ_BLAS_STACK_WINDOW")) window = std::atoi(e);        // test aid: force a small window
    window = std::max(window, 2);
    K.blasOvfCap = 0; K.blasOvf = nullptr;
    if (residentWaves > 0 && need > window) {
        K.blasStackCap = window;
        K.blasOvfCap = need - window;
        const int rc = ensure(c, ovf, (size_t)residentWaves * K.blasOvfCap * 64 * sizeof(uint2));
        if (rc != RZ_OK) return rc;
        K.blasOvf = static_cast<uint2*>(ovf.p);
    }
    return RZ_OK;
}

#ifndef RZ_SPREAD_MIN_INSTANCES
#define RZ_SPREAD_MIN_INSTANCES 3
#endif

// What a render launch reads of the scene and of the frame of rz_set_frame -- its tiles, camera, lights and bounce budget --
// for `spp` samples per pixel from sample `sampleBase` (do_render: the frame's own; rz_render_cost: its own spp from sample 0),
// and the check that the one-lane-per-pixel kernel's LDS stack fits.
int frame_kparams(rz_ctx* c, KParams& K, int spp, int sampleBase) {
    const rz_frame_params& f = c->frame;
    scene_kparams(c, K);
    K.nLights = std::max(0, std::min<int>(f.num_lights, (int)hostCount<rz_light>(c, RZ_BIND_LIGHTS)));
    K.width = f.width; K.height = f.height;
    K.tilesX = (f.width + RZ_TILE_W - 1) / RZ_TILE_W;
    K.tilesY = (f.height + RZ_TILE_H - 1) / RZ_TILE_H;
    const int nTiles = K.tilesX * K.tilesY;
    K.tileRank = f.tile_rank; K.tileNRanks = f.tile_nranks;
    K.nLocalTiles = (nTiles - f.tile_rank + f.tile_nranks - 1) / f.tile_nranks;
    K.maxBounces = f.bounce_budget > 0 ? f.bounce_budget : 5;      // FS:673
    K.spp = spp; K.sampleBase = sampleBase;
    std::memcpy(K.invView, f.inv_view, 64);
    std::memcpy(K.invProj, f.inv_proj, 64);
    std::memcpy(K.camPos, f.cam_pos, 12);
    std::memcpy(K.hemi0, c->hemi0, 12);
    {
        const long long nIdx = tlas_index_count(c);
        // Spread rays are traced lane by lane when they have several instances to spread over: with two (C2: floor + mesh) the
        // wave-cursor walk's scalar fetches and octant tests are worth more than walking both instances at once.
        // RZ_SPREAD_MIN_INSTANCES overrides the threshold (0 = never; A/B aid).
        long long minInst = RZ_SPREAD_MIN_INSTANCES;
        if (const char* e = std::getenv("RZ_SPREAD_MIN_INSTANCES")) minInst = std::atoll(e);
        K.spreadTrace = (minInst > 0 && nIdx >= minInst) ? 1 : 0;
    }
    const size_t perWave = (size_t)K.blasStackCap * 512 + (size_t)K.tlasStackCap * 256 + 4864;
    if (perWave * 4 > 160 * 1024)   // sized for the largest (4-wave) workgroup
        return fail(c, RZ_ERR_BAD_SCENE, "BLAS depth %d needs %zu B of LDS stack per wave; the limit is %d", c->maxBlasDepth, perWave, 40 * 1024);
    return RZ_OK;
}

}  // namespace rz

extern "C" {

// The hash of the sources and flags this library was built from (rayzen_amd/build.py: source_hash, passed as
// -DRZ_SOURCE_HASH): lets a benchmark or a test tie the LOADED library to the tree and to a committed counter file.
#ifndef RZ_SOURCE_HASH
#define RZ_SOURCE_HASH "unstamped"
#endif
static const char rz_stamp[] = "RZSRCHASH:" RZ_SOURCE_HASH;
const char* rz_source_hash(void) { return rz_stamp + 10; }
const char* rz_version(void) { return "rayzen_hip 0.5 (gfx950)"; }
int rz_abi_version(void) { return RZ_ABI_VERSION; }
int rz_math_flavour(void) { return RZ_MATH_FLAVOUR; }

int rz_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}

size_t rz_sizeof(int which) {
    switch (which) {
        case 0: return sizeof(rz_triangle);
        case 1: return sizeof(rz_bvh_node);
        case 2: return sizeof(rz_bvh_instance);
        case 3: return sizeof(rz_material);
        case 4: return sizeof(rz_light);
        case 5: return sizeof(rz_frame_params);
        case 6: return sizeof(rz_counters);
        case 7: return sizeof(rz_ray);
        case 8: return sizeof(rz_hit);
        case 9: return sizeof(rz_visibility);
        case 10: return sizeof(rz_editor_params);
        case 11: return sizeof(rz_denoise_params);
        case 12: return sizeof(rz_temporal_params);
        case 14: return sizeof(rz_display_params);       // (13 stays unassigned: callers probe it as the first unknown index)
        case 15: return sizeof(rz_display_info);
        case 17: return sizeof(rz_skin_triangle);        // (16 stays unassigned too: probed as an unknown index)
        case 18: return sizeof(rz_morph_triangle);
        case 20: return sizeof(rz_mesh_quality);         // (19 stays unassigned: probed as an unknown index)
        case 21: return sizeof(rz_upscale_params);
        case 23: return sizeof(rz_seethrough_params);    // (22 stays unassigned: probed as an unknown index)
        case 24: return sizeof(rz_chain);
        case 26: return sizeof(rz_antialias_params);     // (25 stays unassigned: probed as an unknown index)
        case 28: return sizeof(rz_pixel_cost);           // (27 stays unassigned too)
        case 29: return sizeof(rz_cost_params);
        case 30: return sizeof(rz_cost_view_params);
        case 31: return sizeof(rz_cost_stats);
        case 33: return sizeof(rz_coverage_params);      // (32 stays unassigned: probed as an unknown index)
        case 34: return sizeof(rz_instance_coverage);
        case 35: return sizeof(rz_outline_params);
        case 37: return sizeof(rz_ao_params);            // (36 stays unassigned: probed as an unknown index)
        case 38: return sizeof(rz_adaptive_params);
        case 39: return sizeof(rz_adaptive_info);
        case 40: return sizeof(rz_tile_run);
        case 42: return sizeof(rz_line);                 // (41 stays unassigned: probed as an unknown index)
        case 43: return sizeof(rz_lines_params);
        case 45: return sizeof(rz_bloom_params);         // (44 stays unassigned: probed as an unknown index)
        default: return 0;
    }
}

const char* rz_last_error(const rz_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

rz_ctx* rz_create(int device, unsigned flags) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { fail(nullptr, RZ_ERR_NO_DEVICE, "no HIP device (%s)", hipGetErrorString(e)); return nullptr; }
    if (device < 0 || device >= n) { fail(nullptr, RZ_ERR_INVALID_ARG, "device %d of %d", device, n); return nullptr; }
    rz_ctx* c = new (std::nothrow) rz_ctx();
    if (!c) { fail(nullptr, RZ_ERR_HIP, "out of host memory"); return nullptr; }
    c->device = device;
    c->flags = flags;
    bool ok = hipSetDevice(device) == hipSuccess &&
              hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < rz_ctx::kRing; ++i)
        ok = hipEventCreate(&c->evStart[i]) == hipSuccess && hipEventCreate(&c->evStop[i]) == hipSuccess;
    if (!ok) {
        fail(nullptr, RZ_ERR_HIP, "cannot create stream/events on device %d", device);
        rz_destroy(c);
        return nullptr;
    }
    c->stream = c->ownStream;
    const int hrc = compute_hemi0(c->hemi0, c->stream);
    if (hrc != 0) {
        fail(nullptr, RZ_ERR_HIP, "cannot run the set-up kernel on device %d: %s", device, hipGetErrorString((hipError_t)(-hrc)));
        rz_destroy(c);
        return nullptr;
    }
    return c;
}

void rz_destroy(rz_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    const hipStream_t own = c->ownStream;
    delete c;                                   // events, pinned blocks, then every device buffer
    if (own) (void)hipStreamDestroy(own);       // the stream goes last
}

// On the context's device, its stream idle (rz_destroy).  The events and the pinned blocks are few and go by hand; every
// device buffer -- the members once this body has run, the rigs' with their map -- is freed by its DevBuf.
rz_ctx::~rz_ctx() {
    for (hipEvent_t e : evSkin) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : evAdaptive) if (e) (void)hipEventDestroy(e);
    if (adPinned) (void)hipHostFree(adPinned);
    if (refitPinned) (void)hipHostFree(refitPinned);
    if (tlasHostCounts) (void)hipHostFree(tlasHostCounts);
    if (relayoutPinned) (void)hipHostFree(relayoutPinned);
    for (int i = 0; i < kRing; ++i) {
        if (evStart[i]) (void)hipEventDestroy(evStart[i]);
        if (evStop[i]) (void)hipEventDestroy(evStop[i]);
    }
}

// What rz_upload, rz_update and rz_read_binding share.  Before the call touches a binding's host copy: its group's, current
// (`replacing`: all of the group but the binding itself, which the call overwrites whole).  After the call has changed it:
// the device copy is not current any more, and finalize has the matching part of the device scene to redo.
static int host_copy_for(rz_ctx* c, int binding, bool replacing = false) {
    const int g = group_of(binding);
    return g == kNoGroup ? RZ_OK : need_host(c, g, replacing ? binding : -1);
}
static void mark_dirty(rz_ctx* c, int binding) {
    switch (binding) {
        case RZ_BIND_MATERIALS: c->matDirty = true; break;
        case RZ_BIND_LIGHTS: c->lightDirty = true; break;
        case RZ_BIND_TLAS_NODES: case RZ_BIND_TLAS_INDICES: c->tlasDirty = true; break;
        case RZ_BIND_INSTANCES: c->instDirty = true; break;
        default: c->geomDirty = true; break;
    }
}
static int host_copy_changed(rz_ctx* c, int binding) {
    const int g = group_of(binding);
    if (g != kNoGroup) { const int rc = host_changed(c, g); if (rc != RZ_OK) return rc; }
    if (g == kBlas) drop_built_costs(c);        // trees handed over
    mark_dirty(c, binding);
    return RZ_OK;
}

static int upload_impl(rz_ctx* c, rz_binding binding, const void* data, size_t bytes) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    const size_t es = elem_size((int)binding);
    if (es == 0) return fail(c, RZ_ERR_INVALID_ARG, "unknown binding %d", (int)binding);
    if (bytes % es) return fail(c, RZ_ERR_INVALID_ARG, "binding %d: %zu bytes is not a multiple of the %zu-byte element", (int)binding, bytes, es);
    if (bytes && !data) return fail(c, RZ_ERR_INVALID_ARG, "null data");
    alloc_point(c);
    c->host[binding].reserve(bytes);        // (the allocation that can fail, before the group is touched: assign() below cannot throw)
    { const int rc = host_copy_for(c, binding, true); if (rc != RZ_OK) return rc; }
    c->host[binding].assign(static_cast<const unsigned char*>(data), static_cast<const unsigned char*>(data) + bytes);
    if (binding == RZ_BIND_TRIANGLES || binding == RZ_BIND_BLAS_NODES || binding == RZ_BIND_BLAS_INDICES || binding == RZ_BIND_INSTANCES)
        c->tmpValid = false;                // new geometry or instances: rz_denoise_temporal's history describes another scene
    c->present[binding] = true;
    return host_copy_changed(c, binding);
}

static int update_impl(rz_ctx* c, rz_binding binding, size_t offset, const void* data, size_t bytes) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (elem_size((int)binding) == 0) return fail(c, RZ_ERR_INVALID_ARG, "unknown binding %d", (int)binding);
    if (!c->present[binding]) return fail(c, RZ_ERR_NOT_READY, "binding %d has not been uploaded", (int)binding);
    if (bytes && !data) return fail(c, RZ_ERR_INVALID_ARG, "null data");
    { const int rc = host_copy_for(c, binding); if (rc != RZ_OK) return rc; }
    if (offset > c->host[binding].size() || bytes > c->host[binding].size() - offset)
        return fail(c, RZ_ERR_OUT_OF_RANGE, "binding %d: update [%zu,+%zu) past its %zu bytes", (int)binding, offset, bytes, c->host[binding].size());
    if (bytes == 0) return RZ_OK;
    if (std::memcmp(c->host[binding].data() + offset, data, bytes) == 0) return RZ_OK;   // unchanged: nothing to redo
    std::memcpy(c->host[binding].data() + offset, data, bytes);
    return host_copy_changed(c, binding);
}

static int tlas_rebuild(rz_ctx* c, const float* transforms, size_t n);

static int update_transforms_impl(rz_ctx* c, const float* transforms, size_t n) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (!transforms && n) return fail(c, RZ_ERR_INVALID_ARG, "null transforms");
    RZ_HIP(c, hipSetDevice(c->device));
    int rc = finalize(c);           // the device scene must exist (BLAS root boxes live in DevInstance)
    if (rc != RZ_OK) return rc;
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    if (n != nInst) return fail(c, RZ_ERR_INVALID_ARG, "%zu transforms for %zu instances", n, nInst);
    return tlas_rebuild(c, transforms, n);
}

// World boxes, TLAS and TlasDfs from the root boxes in DevInstance and n transforms (rz_tlas_refit), then one
// synchronisation.  transforms == nullptr: the ones dXforms holds already (those of the last rz_update_transforms).
static int tlas_rebuild(rz_ctx* c, const float* transforms, size_t n) {
    int rc;
    if (n == 0) return RZ_OK;
    if (n > (size_t)1 << 20) return fail(c, RZ_ERR_INVALID_ARG, "too many instances for the device TLAS builder");
    if (!c->tlasHostCounts) RZ_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->tlasHostCounts), 64, hipHostMallocDefault));
    rc = ensure(c, c->dXforms, n * 64);
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dInstRef, n * sizeof(rz_bvh_instance));
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dTlasNodes, (2 * n) * sizeof(rz_bvh_node));
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dTlasIdx, n * sizeof(int32_t));
    if (rc != RZ_OK) return rc;
    // scratch: worldMin, worldMax (3n floats each), order + depth (2n+8 ints... the depth stack shares order's tail), stack 3*(2n+8), counts 16
    const size_t stackInts = 3 * (2 * n + 8), orderInts = n + (2 * n + 8);
    rc = ensure(c, c->dTlasDfs, (2 * n) * sizeof(TlasDfs));
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dTlasScratch, (6 * n) * 4 + orderInts * 4 + stackInts * 4 + 64 + (4 * n + 12 * (n + 1)) * 4);
    if (rc != RZ_OK) return rc;
    // the reference-layout records keep their offsets: seed them from the host copy once per host-side change
    RZ_HIP(c, hipMemcpyAsync(c->dInstRef.p, c->host[RZ_BIND_INSTANCES].data(), n * sizeof(rz_bvh_instance), hipMemcpyHostToDevice, c->stream));
    if (transforms) RZ_HIP(c, hipMemcpyAsync(c->dXforms.p, transforms, n * 64, hipMemcpyHostToDevice, c->stream));
    TlasWork W{};
    char* sc = static_cast<char*>(c->dTlasScratch.p);
    W.transforms = static_cast<const float*>(c->dXforms.p);
    W.instances = static_cast<DevInstance*>(c->dInst.p);
    W.refInstances = static_cast<rz_bvh_instance*>(c->dInstRef.p);
    W.nodes = static_cast<TlasNode*>(c->dTlasNodes.p);
    W.indices = static_cast<int32_t*>(c->dTlasIdx.p);
    W.dfs = static_cast<TlasDfs*>(c->dTlasDfs.p);
    W.worldMin = reinterpret_cast<float*>(sc);
    W.worldMax = W.worldMin + 3 * n;
    W.order = reinterpret_cast<int32_t*>(W.worldMax + 3 * n);
    W.stack = W.order + orderInts;
    W.outCounts = W.stack + stackInts;
    W.scratch = W.outCounts + 16;
    W.n = (int)n;
    launch_tlas_refit(W, c->stream);
    RZ_HIP(c, hipGetLastError());
    RZ_HIP(c, hipMemcpyAsync(c->tlasHostCounts, W.outCounts, 16, hipMemcpyDeviceToHost, c->stream));
    // the caller's transform array may die after this call returns, and the TLAS depth sizes the LDS stack
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    c->devTlasNodes = c->tlasHostCounts[0];
    c->nTlasDfs = c->tlasHostCounts[0];
    c->tlasEntry = c->tlasHostCounts[3];        // (the builder's own verdict on the list it wrote)
    c->tlasDepth = std::max(1, c->tlasHostCounts[2]);
    device_changed(c, kTlas);
    return RZ_OK;
}

// ---- rz_refit_geometry --------------------------------------------------------------------------------------------

// The views of the current layout, breadth first: rank of every internal node (== its pair index, rz_relayout.hip) and
// where each tree level starts; which view every instance uses.  Derived on the host from the node array (fetched once
// if it lives on the device), uploaded, and kept until the views are laid out again.
static int refit_topology(rz_ctx* c) {
    if (c->refitGen == c->layoutGen) return RZ_OK;
    int rc;
    for (int g : {kBlas, kTlas}) if ((rc = need_host(c, g)) != RZ_OK) return rc;
    const rz_bvh_node* nodes = hostArr<rz_bvh_node>(c, RZ_BIND_BLAS_NODES);
    const long long nNodes = (long long)hostCount<rz_bvh_node>(c, RZ_BIND_BLAS_NODES);
    alloc_point(c);
    std::vector<RefitView> rv;
    std::vector<int32_t> rank, viewOff;
    std::map<std::tuple<int, int, int>, int> viewIndex;
    for (const auto& kv : c->views) {
        const int nodeOff = std::get<0>(kv.first);
        RefitView R;
        R.key = kv.first;
        R.rankBase = (int)rank.size();
        if (nodeOff < 0 || nodeOff >= nNodes) return fail(c, RZ_ERR_INTERNAL, "rz_refit_geometry: a laid-out view starts outside the node array");
        if (nodes[nodeOff].count < 0) {
            // the host re-layout's queue (build_view): queue[i] is the i-th internal node, and its pair is pair i
            size_t head = rank.size(), levelEnd = head + 1;
            rank.push_back(0);
            R.levelStart.push_back(0);
            while (head < rank.size()) {
                if (head == levelEnd) { R.levelStart.push_back((int)(head - (size_t)R.rankBase)); levelEnd = rank.size(); }
                const int L = nodes[nodeOff + rank[head++]].leftFirst;
                if (L < 1 || (long long)nodeOff + L + 1 >= nNodes || rank.size() - (size_t)R.rankBase > (size_t)nNodes)
                    return fail(c, RZ_ERR_INTERNAL, "rz_refit_geometry: a laid-out view is not a tree");
                R.maxNode = std::max(R.maxNode, L + 1);
                for (int k = 0; k < 2; ++k)
                    if (nodes[nodeOff + L + k].count < 0) { if ((rank.size() & 4095) == 0) alloc_point(c); rank.push_back(L + k); }
            }
            R.levelStart.push_back((int)(rank.size() - (size_t)R.rankBase));
            if ((int)(rank.size() - (size_t)R.rankBase) != kv.second.nPairs)
                return fail(c, RZ_ERR_INTERNAL, "rz_refit_geometry: a view has %d pairs, its tree %zu internal nodes", kv.second.nPairs, rank.size() - (size_t)R.rankBase);
        }
        viewIndex[kv.first] = (int)rv.size();
        viewOff.push_back(nodeOff);
        rv.push_back(std::move(R));
    }
    const rz_bvh_instance* inst = hostArr<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    std::vector<int32_t> instView(nInst, -1);
    for (size_t i = 0; i < nInst; ++i) {
        auto it = viewIndex.find(std::make_tuple(inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset));
        if (it != viewIndex.end()) instView[i] = it->second;
    }
    // the views' flag words start from what the layout found (a view this call does not refit keeps its own)
    std::vector<unsigned> flags(4 * rv.size(), 0u);
    {
        size_t v = 0;
        for (const auto& kv : c->views) { flags[4 * v] = (kv.second.mayGlass ? 1u : 0u) | (kv.second.irregular ? 2u : 0u); ++v; }
    }
    if ((rc = upload_vec(c, c->dRefitRank, rank.data(), rank.size() * sizeof(int32_t))) != RZ_OK) return rc;
    if ((rc = upload_vec(c, c->dRefitInstView, instView.data(), instView.size() * sizeof(int32_t))) != RZ_OK) return rc;
    if ((rc = upload_vec(c, c->dRefitViewOff, viewOff.data(), viewOff.size() * sizeof(int32_t))) != RZ_OK) return rc;
    if ((rc = upload_vec(c, c->dRefitFlags, flags.data(), flags.size() * sizeof(unsigned))) != RZ_OK) return rc;
    if ((rc = ensure(c, c->dRefitRoots, std::max<size_t>(rv.size(), 1) * sizeof(rz_bvh_node))) != RZ_OK) return rc;
    // rz_geometry_quality's view of the same lists (rz_quality.hip): every view owns a run of whole workgroups
    std::vector<QualityView> qv(rv.size() + 1);
    long long blocks = 0;
    for (size_t v = 0; v < rv.size(); ++v) {
        const int nPairs = rv[v].levelStart.empty() ? 0 : rv[v].levelStart.back();
        qv[v] = QualityView{viewOff[v], rv[v].rankBase, nPairs, (int32_t)blocks};
        blocks += (nPairs + 255) / 256;
    }
    qv[rv.size()] = QualityView{0, 0, 0, (int32_t)blocks};
    if ((rc = upload_vec(c, c->dQualViews, qv.data(), qv.size() * sizeof(QualityView))) != RZ_OK) return rc;
    if ((rc = ensure(c, c->dQualPartials, (size_t)std::max<long long>(blocks, 1) * sizeof(double))) != RZ_OK) return rc;
    if ((rc = ensure(c, c->dQualCost, std::max<size_t>(rv.size(), 1) * sizeof(double))) != RZ_OK) return rc;
    c->qualBlocks = (int)blocks;
    const size_t pinnedNeed = rv.size() * (16 + sizeof(rz_bvh_node) + sizeof(double)) + 64;      // flag words, root nodes, costs
    if (pinnedNeed > c->refitPinnedCap) {
        if (c->refitPinned) (void)hipHostFree(c->refitPinned);
        c->refitPinned = nullptr; c->refitPinnedCap = 0;
        RZ_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->refitPinned), pinnedNeed, hipHostMallocDefault));
        c->refitPinnedCap = pinnedNeed;
    }
    RZ_HIP(c, hipStreamSynchronize(c->stream));     // the staging vectors die at scope exit
    c->refitViews.swap(rv);
    c->refitGen = c->layoutGen;
    return RZ_OK;
}

// The definition of include/rayzen_hip.h on the host copies of one mesh (the partner of BVH::refit, for node arrays whose
// children need not be numbered after their parents): breadth first from the root, then the visited nodes in reverse.
// *nSlots: the slots its leaves name.  false: the arrays are inconsistent (nothing written; the re-layout words the error).
static bool host_refit_mesh(rz_ctx* c, rz_bvh_node* nodes, long long nNodes, const int32_t* idx, long long nIdx, const rz_triangle* tris,
                            long long nTris, int nodeOff, int triOff, int gTriOff, bool write, long long* nSlots) {
    if (nodeOff < 0 || nodeOff >= nNodes || triOff < 0 || triOff > nIdx) return false;
    alloc_point(c);
    std::vector<int> order;
    order.push_back(0);
    long long maxSlot = 0;
    for (size_t head = 0; head < order.size(); ++head) {
        const rz_bvh_node& N = nodes[nodeOff + order[head]];
        if (N.count >= 0) {
            if (N.leftFirst < 0 || (long long)triOff + N.leftFirst + N.count > nIdx) return false;
            for (int s = 0; s < N.count; ++s) {
                const long long src = (long long)gTriOff + idx[triOff + N.leftFirst + s];
                if (src < 0 || src >= nTris) return false;
            }
            maxSlot = std::max(maxSlot, (long long)N.leftFirst + N.count);
            continue;
        }
        const int L = N.leftFirst;
        if (L < 1 || (long long)nodeOff + L + 1 >= nNodes || order.size() > (size_t)nNodes) return false;
        if ((order.size() & 4095) == 0) alloc_point(c);
        order.push_back(L);
        order.push_back(L + 1);
    }
    if (nSlots) *nSlots = maxSlot;
    if (!write) return true;
    const float fmax = std::numeric_limits<float>::max();
    auto gmin = [](float a, float b) { return (b < a) ? b : a; };      // glm::min
    auto gmax = [](float a, float b) { return (a < b) ? b : a; };      // glm::max
    for (size_t k = order.size(); k-- > 0;) {
        rz_bvh_node& N = nodes[nodeOff + order[k]];
        if (N.count > 0) {
            float mn[3] = {fmax, fmax, fmax}, mx[3] = {-fmax, -fmax, -fmax};
            for (int s = 0; s < N.count; ++s) {
                const rz_triangle& t = tris[(long long)gTriOff + idx[triOff + N.leftFirst + s]];
                for (int a = 0; a < 3; ++a) {
                    mn[a] = gmin(mn[a], gmin(t.v0[a], gmin(t.v1[a], t.v2[a])));
                    mx[a] = gmax(mx[a], gmax(t.v0[a], gmax(t.v1[a], t.v2[a])));
                }
            }
            std::memcpy(N.boundsMin, mn, 12); std::memcpy(N.boundsMax, mx, 12);
        } else if (N.count < 0) {
            const rz_bvh_node& A = nodes[nodeOff + N.leftFirst];
            const rz_bvh_node& B = nodes[nodeOff + N.leftFirst + 1];
            for (int a = 0; a < 3; ++a) {       // a bound equal to the one held keeps its bits (rz_refit.hip: keep_equal)
                const float mn = gmin(A.boundsMin[a], B.boundsMin[a]), mx = gmax(A.boundsMax[a], B.boundsMax[a]);
                if (!(mn == N.boundsMin[a])) N.boundsMin[a] = mn;
                if (!(mx == N.boundsMax[a])) N.boundsMax[a] = mx;
            }
        }
    }
    return true;
}

// The transforms in force, for the TLAS step: dXforms if rz_update_transforms wrote the current ones, else the instances'.
static int refit_tlas_step(rz_ctx* c) {
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    if (nInst == 0) return RZ_OK;
    if (c->where[kTlas].dev) return tlas_rebuild(c, nullptr, nInst);
    const rz_bvh_instance* inst = hostArr<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    alloc_point(c);
    std::vector<float> xf(nInst * 16);
    for (size_t i = 0; i < nInst; ++i) std::memcpy(&xf[i * 16], inst[i].transform, 64);
    return tlas_rebuild(c, xf.data(), nInst);      // (synchronises before xf dies)
}

// ---- the SAH cost of the laid-out trees (rz_geometry_quality) -------------------------------------------------------

// The cost of include/rayzen_hip.h on the host copy of one mesh (the partner of BVH::sahCost for node arrays whose children
// need not be numbered after their parents): breadth first from the root.  false: the nodes do not form a tree inside the array.
static bool host_sah_cost(rz_ctx* c, const rz_bvh_node* nodes, long long nNodes, int nodeOff, double* cost) {
    if (nodeOff < 0 || nodeOff >= nNodes) return false;
    auto area = [](const rz_bvh_node& N) {
        const double dx = (double)N.boundsMax[0] - (double)N.boundsMin[0], dy = (double)N.boundsMax[1] - (double)N.boundsMin[1],
                     dz = (double)N.boundsMax[2] - (double)N.boundsMin[2];
        if (!(dx >= 0.0) || !(dy >= 0.0) || !(dz >= 0.0)) return 0.0;
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    };
    alloc_point(c);
    std::vector<int> order;
    order.push_back(0);
    double sum = 0.0;
    for (size_t head = 0; head < order.size(); ++head) {
        const rz_bvh_node& N = nodes[nodeOff + order[head]];
        if (N.count >= 0) { sum += area(N) * (double)N.count; continue; }
        const int L = N.leftFirst;
        if (L < 1 || (long long)nodeOff + L + 1 >= nNodes || order.size() > (size_t)nNodes) return false;
        sum += area(N);
        if ((order.size() & 4095) == 0) alloc_point(c);
        order.push_back(L);
        order.push_back(L + 1);
    }
    const double rootArea = area(nodes[nodeOff]);
    *cost = rootArea == 0.0 ? 0.0 : sum / rootArea;
    return true;
}

// The cost of every laid-out view, in the order of `views`, measured now: on the device where the layout lives there (two
// launches on the context's stream, rz_quality.hip), else on the host copies.  Synchronises; `costs` gets views.size()
// doubles.  The layout must be current (finalize).
static int measure_costs(rz_ctx* c, std::vector<double>& costs) {
    int rc;
    const size_t nViews = c->views.size();
    alloc_point(c);
    costs.assign(nViews, 0.0);
    if (c->layoutOnDevice) {
        if ((rc = refit_topology(c)) != RZ_OK) return rc;
        double* h = reinterpret_cast<double*>(c->refitPinned + nViews * (16 + sizeof(rz_bvh_node)));
        if (nViews) {
            const int e = quality_device(static_cast<const rz_bvh_node*>(c->dRawNodes.p), static_cast<const int32_t*>(c->dRefitRank.p),
                                         static_cast<const QualityView*>(c->dQualViews.p), (int)nViews, c->qualBlocks,
                                         static_cast<double*>(c->dQualPartials.p), static_cast<double*>(c->dQualCost.p), c->stream);
            if (e != 0) return fail(c, RZ_ERR_HIP, "rz_geometry_quality: %s", hipGetErrorString((hipError_t)(-e)));
            RZ_HIP(c, hipMemcpyAsync(h, c->dQualCost.p, nViews * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        RZ_HIP(c, hipStreamSynchronize(c->stream));
        if (nViews) std::memcpy(costs.data(), h, nViews * sizeof(double));
        return RZ_OK;
    }
    if ((rc = need_host(c, kBlas)) != RZ_OK) return rc;
    size_t v = 0;
    for (const auto& kv : c->views) {
        if (!host_sah_cost(c, hostArr<rz_bvh_node>(c, RZ_BIND_BLAS_NODES), (long long)hostCount<rz_bvh_node>(c, RZ_BIND_BLAS_NODES),
                           std::get<0>(kv.first), &costs[v]))
            return fail(c, RZ_ERR_INTERNAL, "rz_geometry_quality: a laid-out view is not a tree");
        ++v;
    }
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return RZ_OK;
}

// The first look at every tree that was handed over or built since the last one: its cost becomes rz_mesh_quality::sah_cost_built.
// rz_refit_geometry and rz_skin_pose call this before they move a box; `costs` (measure_costs) may be passed by a caller
// that has measured already.  Trees that are no longer laid out lose their entry.
static int note_built_costs(rz_ctx* c, const std::vector<double>* measured) {
    if (c->costGen == c->layoutGen) return RZ_OK;
    bool missing = false;
    for (const auto& kv : c->views) missing = missing || !c->costBuilt.count(kv.first);
    std::vector<double> own;
    if (missing && !measured) { const int rc = measure_costs(c, own); if (rc != RZ_OK) return rc; measured = &own; }
    alloc_point(c);
    std::map<std::tuple<int, int, int>, double> kept;
    size_t v = 0;
    for (const auto& kv : c->views) {
        const auto it = c->costBuilt.find(kv.first);
        kept[kv.first] = it != c->costBuilt.end() ? it->second : (*measured)[v];
        ++v;
    }
    c->costBuilt.swap(kept);
    c->costGen = c->layoutGen;
    return RZ_OK;
}

// n triangles from a host or a device pointer into the host copy of binding 0, from triangle `first` on
static int patch_host_triangles(rz_ctx* c, const rz_triangle* triangles, size_t first, size_t n, bool hostPtr) {
    unsigned char* dst = c->host[RZ_BIND_TRIANGLES].data() + first * sizeof(rz_triangle);
    if (hostPtr) std::memcpy(dst, triangles, n * sizeof(rz_triangle));
    else {
        RZ_HIP(c, hipStreamSynchronize(c->stream));
        RZ_HIP(c, hipMemcpy(dst, triangles, n * sizeof(rz_triangle), hipMemcpyDeviceToHost));
    }
    return RZ_OK;
}

// The host route: patch the host copies, refit there, and let the re-layout run (RZ_FLAG_HOST_RELAYOUT; a layout that
// fell back to the host; materials changed since the views were laid out).  Same bytes as the device route.
static int refit_on_host(rz_ctx* c, const rz_triangle* triangles, size_t first, size_t n, bool hostPtr) {
    int rc;
    for (int g : {kTlas, kTris, kBlas}) if ((rc = need_host(c, g)) != RZ_OK) return rc;
    if ((rc = note_built_costs(c, nullptr)) != RZ_OK) return rc;       // (before a box moves: rz_geometry_quality's sah_cost_built)
    for (int g : {kTlas, kTris, kBlas}) if ((rc = host_changed(c, g)) != RZ_OK) return rc;     // the host copies are the truth again
    if (n && (rc = patch_host_triangles(c, triangles, first, n, hostPtr)) != RZ_OK) return rc;
    rz_bvh_node* nodes = reinterpret_cast<rz_bvh_node*>(c->host[RZ_BIND_BLAS_NODES].data());
    const long long nNodes = (long long)hostCount<rz_bvh_node>(c, RZ_BIND_BLAS_NODES), nIdx = (long long)hostCount<int32_t>(c, RZ_BIND_BLAS_INDICES);
    const long long nTris = (long long)hostCount<rz_triangle>(c, RZ_BIND_TRIANGLES);
    const rz_bvh_instance* inst = hostArr<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    std::map<std::tuple<int, int, int>, bool> seen;
    for (size_t i = 0; i < nInst; ++i) {
        const auto key = std::make_tuple(inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset);
        if (seen.count(key)) continue;
        seen[key] = true;
        long long slots = 0;
        if (!host_refit_mesh(c, nodes, nNodes, hostArr<int32_t>(c, RZ_BIND_BLAS_INDICES), nIdx, hostArr<rz_triangle>(c, RZ_BIND_TRIANGLES), nTris,
                             inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset, false, &slots))
            continue;
        const long long lo = inst[i].globalTriOffset, hi = lo + slots;
        if (n && !((long long)first < hi && lo < (long long)(first + n))) continue;
        (void)host_refit_mesh(c, nodes, nNodes, hostArr<int32_t>(c, RZ_BIND_BLAS_INDICES), nIdx, hostArr<rz_triangle>(c, RZ_BIND_TRIANGLES), nTris,
                              inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset, true, nullptr);
    }
    c->geomDirty = true;
    if ((rc = finalize(c)) != RZ_OK) return rc;
    return refit_tlas_step(c);
}

// the first binding a refit needs that has not been uploaded, or -1 (rz_skin_pose asks before it launches anything)
static int refit_missing_binding(const rz_ctx* c) {
    for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_BLAS_NODES, RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS,
                  RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES})
        if (!c->present[b]) return b;
    return -1;
}

static int refit_geometry_impl(rz_ctx* c, const rz_triangle* triangles, size_t first, size_t n, unsigned flags) {
    const char* what = "rz_refit_geometry";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~RZ_REFIT_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (n && !triangles) return fail(c, RZ_ERR_INVALID_ARG, "%s: null triangles", what);
    const bool hostPtr = (flags & RZ_REFIT_HOST) != 0;
    if (n && !hostPtr && (reinterpret_cast<uintptr_t>(triangles) & 15u)) return fail(c, RZ_ERR_INVALID_ARG, "%s: the device pointer must be 16-byte aligned", what);
    { const int b = refit_missing_binding(c); if (b >= 0) return fail(c, RZ_ERR_NOT_READY, "%s: no scene (binding %d has not been uploaded)", what, b); }
    const size_t nTris = hostCount<rz_triangle>(c, RZ_BIND_TRIANGLES);
    if (first > nTris || n > nTris - first)
        return fail(c, RZ_ERR_OUT_OF_RANGE, "%s: triangles [%zu,+%zu) past the %zu of binding 0", what, first, n, nTris);
    RZ_HIP(c, hipSetDevice(c->device));
    int rc;
    bool copied = false;                // binding 0 holds the new triangles already
    if (c->geomDirty && n) {
        // a re-layout is pending anyway (the geometry was uploaded or patched since the last launch -- or an earlier refit left a
        // bad materialIndex behind): the new triangles go into the host copy first, so that it is their layout that is checked
        if ((rc = host_changed(c, kTris)) != RZ_OK) return rc;
        if ((rc = patch_host_triangles(c, triangles, first, n, hostPtr)) != RZ_OK) return rc;
        copied = true;                  // (the re-layout below uploads them with the rest)
    }
    rc = finalize(c);                   // the device scene must exist: the refit patches it
    if (rc != RZ_OK) return rc;
    if (!c->layoutOnDevice || c->matChangedSinceLayout) return refit_on_host(c, triangles, first, n, hostPtr);
    if ((rc = refit_topology(c)) != RZ_OK) return rc;
    if ((rc = note_built_costs(c, nullptr)) != RZ_OK) return rc;       // (before a box moves: rz_geometry_quality's sah_cost_built)
    // (every host allocation of the call happens before anything is enqueued: a failure leaves the context as it was)
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    alloc_point(c);
    std::vector<float> xf;              // the transforms in force, unless dXforms holds them (rz_update_transforms wrote the current ones)
    const bool devXforms = c->where[kTlas].dev;
    if (!devXforms) {
        const rz_bvh_instance* inst = hostArr<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
        xf.resize(nInst * 16);
        for (size_t i = 0; i < nInst; ++i) std::memcpy(&xf[i * 16], inst[i].transform, 64);
    }
    std::vector<char> touched(c->refitViews.size(), 0);

    // binding 0 first (every triangle of the interval, whether a mesh names it or not) ...
    if (n && !copied) {
        void* dst = static_cast<rz_triangle*>(c->dRawTris.p) + first;
        if (hostPtr) {      // both copies get the interval: each stays as current as it was (the device's is: the layout lives there)
            RZ_HIP(c, hipMemcpyAsync(dst, triangles, n * sizeof(rz_triangle), hipMemcpyHostToDevice, c->stream));
            std::memcpy(c->host[RZ_BIND_TRIANGLES].data() + first * sizeof(rz_triangle), triangles, n * sizeof(rz_triangle));
        } else {
            RZ_HIP(c, hipMemcpyAsync(dst, triangles, n * sizeof(rz_triangle), hipMemcpyDeviceToDevice, c->stream));
            device_changed(c, kTris);
        }
    }
    // ... then every view whose triangle range meets the interval
    const int nViews = (int)c->refitViews.size();
    const int nMat = (int)hostCount<rz_material>(c, RZ_BIND_MATERIALS);
    unsigned* dFlags = static_cast<unsigned*>(c->dRefitFlags.p);
    int nTouched = 0;
    for (int v = 0; v < nViews; ++v) {
        const RefitView& R = c->refitViews[(size_t)v];
        const BlasView& V = c->views.at(R.key);
        const long long lo = std::get<2>(R.key), hi = lo + V.nSlots;
        if (n && !((long long)first < hi && lo < (long long)(first + n))) continue;
        if (V.empty) continue;          // (a count == 0 root is left as it is)
        touched[(size_t)v] = 1; ++nTouched;
        RZ_HIP(c, hipMemsetAsync(dFlags + 4 * v, 0, 16, c->stream));
        RefitViewWork W{};
        W.nodes = static_cast<rz_bvh_node*>(c->dRawNodes.p) + std::get<0>(R.key);
        W.idx = static_cast<const int32_t*>(c->dRawIdx.p) + std::get<1>(R.key);
        W.rawTris = static_cast<const rz_triangle*>(c->dRawTris.p);
        W.nTris = (long long)nTris;
        W.gTriOff = std::get<2>(R.key);
        W.nSlots = V.nSlots;
        W.tris = static_cast<DevTri*>(c->dTris.p) + V.triBase;
        W.triN = static_cast<DevTriN*>(c->dTriN.p) + V.triBase;
        W.pairs = static_cast<DevPair*>(c->dPairs.p) + V.pairBase;
        W.rankToNode = static_cast<const int32_t*>(c->dRefitRank.p) + R.rankBase;
        W.levelStart = R.levelStart.data();
        W.nLevels = R.levelStart.empty() ? 0 : (int)R.levelStart.size() - 1;
        W.mats = static_cast<const rz_material*>(c->dMat.p);
        W.nMat = nMat;
        W.vflags = dFlags + 4 * v;
        const int e = refit_view_device(W, c->stream);
        if (e != 0) return fail(c, RZ_ERR_HIP, "%s: %s", what, hipGetErrorString((hipError_t)(-e)));
    }
    unsigned* hFlags = reinterpret_cast<unsigned*>(c->refitPinned);
    rz_bvh_node* hRoots = reinterpret_cast<rz_bvh_node*>(c->refitPinned + (size_t)nViews * 16);
    if (nTouched) {
        const int e = refit_roots_device(static_cast<DevInstance*>(c->dInst.p), (int)nInst, static_cast<const int32_t*>(c->dRefitInstView.p),
                                         static_cast<const int32_t*>(c->dRefitViewOff.p), nViews, static_cast<const rz_bvh_node*>(c->dRawNodes.p),
                                         dFlags, static_cast<rz_bvh_node*>(c->dRefitRoots.p), c->stream);
        if (e != 0) return fail(c, RZ_ERR_HIP, "%s: %s", what, hipGetErrorString((hipError_t)(-e)));
        RZ_HIP(c, hipMemcpyAsync(hFlags, dFlags, (size_t)nViews * 16, hipMemcpyDeviceToHost, c->stream));
        RZ_HIP(c, hipMemcpyAsync(hRoots, c->dRefitRoots.p, (size_t)nViews * sizeof(rz_bvh_node), hipMemcpyDeviceToHost, c->stream));
        // the node array on the device is the truth from here on, as after rz_build_geometry: seed what describes it from the host
        // copy, if that is current (devRoots: emptied when the host copy last changed; the roots of the views follow below)
        if (c->where[kBlas].host) {
            c->devNodes = hostCount<rz_bvh_node>(c, RZ_BIND_BLAS_NODES);
            c->devIdx = hostCount<int32_t>(c, RZ_BIND_BLAS_INDICES);
        }
        device_changed(c, kBlas);
    }
    // world boxes and the TLAS with the transforms in force; its synchronisation is this call's (host-pointer copies have left `triangles`)
    rc = tlas_rebuild(c, devXforms ? nullptr : xf.data(), nInst);
    if (rc != RZ_OK) return rc;
    if (nInst == 0) RZ_HIP(c, hipStreamSynchronize(c->stream));
    if (!nTouched) return RZ_OK;
    unsigned all = 0;
    int badTri = -1;
    {
        int v = 0;
        for (auto& kv : c->views) {
            BlasView& V = kv.second;
            if (touched[(size_t)v]) {
                V.mayGlass = (hFlags[4 * v] & 1u) != 0;
                V.irregular = (hFlags[4 * v] & 2u) != 0;
                if ((hFlags[4 * v] & 4u) && badTri < 0) badTri = (int)hFlags[4 * v + 1];
                std::memcpy(V.rootMin, hRoots[v].boundsMin, 12);
                std::memcpy(V.rootMax, hRoots[v].boundsMax, 12);
            }
            all |= (V.mayGlass ? 1u : 0u) | (V.irregular ? 2u : 0u);
            c->devRoots[std::get<0>(kv.first)] = hRoots[v];
            ++v;
        }
    }
    c->devTransparent = all;
    c->sceneHasTransparency = (all & 1u) != 0;
    c->irregularBoxes = (all & 2u) != 0;
    if (badTri >= 0) {
        c->geomDirty = true;            // what a fresh upload of these triangles says, now and at every later call
        return fail(c, RZ_ERR_BAD_SCENE, "%s: triangle %d has a materialIndex outside the %d materials uploaded", what, badTri, nMat);
    }
    return RZ_OK;
}

// ---- rz_skin_create / rz_skin_pose / rz_skin_destroy ---------------------------------------------------------------
static int skin_create_impl(rz_ctx* c, size_t first, size_t n, const rz_triangle* rest, const rz_skin_triangle* skin, int nBones,
                            const rz_morph_triangle* morphs, int nMorphs, int* rigOut) {
    const char* what = "rz_skin_create";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!rigOut) return fail(c, RZ_ERR_INVALID_ARG, "%s: null rig_out", what);
    if (n == 0) return fail(c, RZ_ERR_INVALID_ARG, "%s: no triangles", what);
    if (skin ? (nBones < 1 || nBones > 256) : nBones != 0)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: n_bones = %d (1..256 with skin, 0 without)", what, nBones);
    if (nMorphs < 0 || (nMorphs > 0 && !morphs)) return fail(c, RZ_ERR_INVALID_ARG, "%s: n_morphs = %d, morphs %s", what, nMorphs, morphs ? "given" : "NULL");
    if (!skin && nMorphs == 0) return fail(c, RZ_ERR_INVALID_ARG, "%s: neither skin nor morph targets", what);
    if (!c->present[RZ_BIND_TRIANGLES]) return fail(c, RZ_ERR_NOT_READY, "%s: binding 0 has not been uploaded", what);
    const size_t nTris = hostCount<rz_triangle>(c, RZ_BIND_TRIANGLES);
    if (first > nTris || n > nTris - first)
        return fail(c, RZ_ERR_OUT_OF_RANGE, "%s: triangles [%zu,+%zu) past the %zu of binding 0", what, first, n, nTris);
    if ((size_t)nMorphs > (std::numeric_limits<size_t>::max() / sizeof(rz_morph_triangle)) / n)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: %d morph targets of %zu triangles", what, nMorphs, n);
    if (skin) {
        for (size_t t = 0; t < n; ++t)
            for (int k = 0; k < 3; ++k)
                for (int j = 0; j < 4; ++j) {
                    const int b = (int)((skin[t].bones[k] >> (8 * j)) & 255u);
                    if (!(skin[t].weights[k][j] == 0.0f) && b >= nBones)
                        return fail(c, RZ_ERR_OUT_OF_RANGE, "%s: triangle %zu, corner %d, influence %d names bone %d of %d", what, t, k, j, b, nBones);
                }
    }
    if (!rest) {        // binding 0 as it stands (after a device-pointer refit only the device holds it: fetched first)
        const int rc = need_host(c, kTris);
        if (rc != RZ_OK) return rc;
        rest = hostArr<rz_triangle>(c, RZ_BIND_TRIANGLES) + first;
    }
    RZ_HIP(c, hipSetDevice(c->device));
    alloc_point(c);
    SkinRig R;
    R.first = first; R.n = n; R.nBones = nBones; R.nMorphs = nMorphs;
    struct Part { DevBuf* buf; const void* src; size_t bytes; };
    const Part parts[3] = {{&R.dRest, rest, n * sizeof(rz_triangle)},
                           {&R.dSkin, skin, skin ? n * sizeof(rz_skin_triangle) : 0},
                           {&R.dMorphs, morphs, (size_t)nMorphs * n * sizeof(rz_morph_triangle)}};
    for (const Part& P : parts) {      // (exact sizes and synchronous copies, not ensure(): R frees what it holds on every return)
        if (!P.bytes) continue;
        hipError_t e = hipMalloc(&P.buf->p, P.bytes);
        if (e == hipSuccess) { P.buf->cap = P.bytes; e = hipMemcpy(P.buf->p, P.src, P.bytes, hipMemcpyHostToDevice); }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, RZ_ERR_HIP, "%s: %zu bytes of device memory: %s", what, P.bytes, hipGetErrorString(e));
        }
    }
    const int id = c->nextRig;
    c->rigs.emplace(id, std::move(R));
    ++c->nextRig;
    *rigOut = id;
    return RZ_OK;
}

static int skin_pose_impl(rz_ctx* c, int rig, const float* bones, const float* morphWeights, unsigned flags) {
    const char* what = "rz_skin_pose";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~RZ_SKIN_DEVICE_ARGS) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const auto it = c->rigs.find(rig);
    if (it == c->rigs.end()) return fail(c, RZ_ERR_INVALID_ARG, "%s: no rig %d", what, rig);
    const SkinRig& R = it->second;
    if (R.nBones && !bones) return fail(c, RZ_ERR_INVALID_ARG, "%s: null bones for a rig with %d bones", what, R.nBones);
    if (R.nMorphs && !morphWeights) return fail(c, RZ_ERR_INVALID_ARG, "%s: null morph_weights for a rig with %d targets", what, R.nMorphs);
    const bool devArgs = (flags & RZ_SKIN_DEVICE_ARGS) != 0;
    if (devArgs && ((R.nBones && (reinterpret_cast<uintptr_t>(bones) & 15u)) || (R.nMorphs && (reinterpret_cast<uintptr_t>(morphWeights) & 3u))))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device bones must be 16-byte aligned, device morph_weights 4-byte aligned", what);
    { const int b = refit_missing_binding(c); if (b >= 0) return fail(c, RZ_ERR_NOT_READY, "%s: no scene (binding %d has not been uploaded)", what, b); }
    const size_t nTris = hostCount<rz_triangle>(c, RZ_BIND_TRIANGLES);
    if (R.first > nTris || R.n > nTris - R.first)
        return fail(c, RZ_ERR_OUT_OF_RANGE, "%s: rig %d poses triangles [%zu,+%zu), binding 0 has %zu now", what, rig, R.first, R.n, nTris);
    RZ_HIP(c, hipSetDevice(c->device));
    alloc_point(c);
    int rc;
    if ((rc = ensure(c, c->dSkinOut, R.n * sizeof(rz_triangle))) != RZ_OK) return rc;
    for (hipEvent_t& e : c->evSkin)
        if (!e) RZ_HIP(c, hipEventCreate(&e));
    bool staged = false;            // a host argument is on its way to the device: the caller's memory must outlive the copy
    if (!devArgs) {
        if (R.nBones) {
            if ((rc = ensure(c, c->dSkinBones, (size_t)R.nBones * 64)) != RZ_OK) return rc;
        }
        if (R.nMorphs) {
            if ((rc = ensure(c, c->dSkinWeights, (size_t)R.nMorphs * 4)) != RZ_OK) return rc;
        }
        if (R.nBones) RZ_HIP(c, hipMemcpyAsync(c->dSkinBones.p, bones, (size_t)R.nBones * 64, hipMemcpyHostToDevice, c->stream));
        if (R.nMorphs) {
            const hipError_t e = hipMemcpyAsync(c->dSkinWeights.p, morphWeights, (size_t)R.nMorphs * 4, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, RZ_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }
        }
        staged = true;
    }
    SkinWork W{};
    W.rest = static_cast<const rz_triangle*>(R.dRest.p);
    W.skin = R.nBones ? static_cast<const rz_skin_triangle*>(R.dSkin.p) : nullptr;
    W.bones = devArgs ? bones : static_cast<const float*>(c->dSkinBones.p);
    W.nBones = R.nBones;
    W.morphs = static_cast<const rz_morph_triangle*>(R.dMorphs.p);
    W.morphWeights = devArgs ? morphWeights : static_cast<const float*>(c->dSkinWeights.p);
    W.nMorphs = R.nMorphs;
    W.n = (long long)R.n;
    W.out = static_cast<rz_triangle*>(c->dSkinOut.p);
    c->skinTimed = false;
    hipError_t e = hipEventRecord(c->evSkin[0], c->stream);
    const int ke = e == hipSuccess ? skin_device(W, c->stream) : 0;
    if (e == hipSuccess && ke == 0) e = hipEventRecord(c->evSkin[1], c->stream);
    if (e != hipSuccess || ke != 0) {
        if (staged) (void)hipStreamSynchronize(c->stream);
        return fail(c, RZ_ERR_HIP, "%s: %s", what, hipGetErrorString(e != hipSuccess ? e : (hipError_t)(-ke)));
    }
    c->skinTimed = true;
    // ... and from here on the call IS rz_refit_geometry on a device pointer (its TLAS step synchronises the stream)
    rc = refit_geometry_impl(c, W.out, R.first, R.n, 0);
    if (rc != RZ_OK && staged) (void)hipStreamSynchronize(c->stream);
    return rc;
}

static int skin_destroy_impl(rz_ctx* c, int rig) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "rz_skin_destroy: null context");
    const auto it = c->rigs.find(rig);
    if (it == c->rigs.end()) return fail(c, RZ_ERR_INVALID_ARG, "rz_skin_destroy: no rig %d", rig);
    RZ_HIP(c, hipSetDevice(c->device));
    RZ_HIP(c, hipStreamSynchronize(c->stream));     // (a pose in flight reads the rig's buffers)
    c->rigs.erase(it);
    return RZ_OK;
}

static int skin_last_kernel_ms_impl(rz_ctx* c, float* ms) {
    if (!c || !ms) return fail(c, RZ_ERR_INVALID_ARG, "rz_skin_last_kernel_ms: null argument");
    if (!c->skinTimed) return fail(c, RZ_ERR_NOT_READY, "rz_skin_last_kernel_ms: no rz_skin_pose has run yet");
    RZ_HIP(c, hipEventSynchronize(c->evSkin[1]));
    RZ_HIP(c, hipEventElapsedTime(ms, c->evSkin[0], c->evSkin[1]));
    return RZ_OK;
}

// ---- rz_geometry_quality / rz_rebuild_geometry ------------------------------------------------------------------------

// One mesh of the scene -- a distinct triple among the uploaded instances -- with the cost of its tree as measured now
struct QualityMesh {
    std::tuple<int, int, int> key;
    int nSlots = 0, nPairs = 0, depth = 1;
    double cost = 0.0;
};

typedef std::map<std::tuple<int, int, int>, bool> NamedMeshes;

// the distinct triples among the uploaded instances
static void named_meshes(rz_ctx* c, NamedMeshes& named) {
    const rz_bvh_instance* inst = hostArr<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    alloc_point(c);
    named.clear();
    for (size_t i = 0; i < nInst; ++i) named[std::make_tuple(inst[i].blasNodeOffset, inst[i].blasTriOffset, inst[i].globalTriOffset)] = true;
}

// The meshes in ascending order of their triple, measured on the context's stream (synchronises); every tree that has not been
// looked at since it was handed over gets its sah_cost_built here.  Views the instances no longer name are not reported.
static int measure_meshes(rz_ctx* c, const NamedMeshes& named, std::vector<QualityMesh>& out) {
    std::vector<double> costs;
    int rc;
    if ((rc = measure_costs(c, costs)) != RZ_OK) return rc;
    if ((rc = note_built_costs(c, &costs)) != RZ_OK) return rc;
    out.clear();
    out.reserve(named.size());
    size_t v = 0;
    for (const auto& kv : c->views) {
        if (named.count(kv.first)) {
            QualityMesh m;
            m.key = kv.first;
            m.nSlots = kv.second.nSlots; m.nPairs = kv.second.nPairs; m.depth = kv.second.depth;
            m.cost = costs[v];
            out.push_back(m);
        }
        ++v;
    }
    return RZ_OK;
}

static rz_mesh_quality quality_record(const rz_ctx* c, const QualityMesh& m) {
    rz_mesh_quality q{};
    q.node_offset = q.node_offset_before = std::get<0>(m.key);
    q.index_offset = std::get<1>(m.key);
    q.tri_offset = std::get<2>(m.key);
    q.n_triangles = m.nSlots;
    q.n_nodes = 2 * m.nPairs + 1;
    q.depth = m.depth;
    q.flags = 0;
    q.sah_cost = q.sah_cost_before = m.cost;
    q.sah_cost_built = c->costBuilt.at(m.key);
    q.reserved = 0.0;
    return q;
}

static int geometry_quality_impl(rz_ctx* c, rz_mesh_quality* out, size_t cap, size_t* nMeshes) {
    const char* what = "rz_geometry_quality";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!out && !nMeshes) return fail(c, RZ_ERR_INVALID_ARG, "%s: neither out nor n_meshes", what);
    { const int b = refit_missing_binding(c); if (b >= 0) return fail(c, RZ_ERR_NOT_READY, "%s: no scene (binding %d has not been uploaded)", what, b); }
    RZ_HIP(c, hipSetDevice(c->device));
    int rc = finalize(c);               // a pending layout is brought up to date, as the refit does
    if (rc != RZ_OK) return rc;
    NamedMeshes named;
    named_meshes(c, named);
    const size_t n = named.size();
    if (nMeshes) *nMeshes = n;
    if (!out) return RZ_OK;
    if (cap < n) return fail(c, RZ_ERR_INVALID_ARG, "%s: out holds %zu records, the scene has %zu meshes", what, cap, n);
    std::vector<QualityMesh> M;
    if ((rc = measure_meshes(c, named, M)) != RZ_OK) return rc;
    for (size_t k = 0; k < M.size(); ++k) out[k] = quality_record(c, M[k]);
    return RZ_OK;
}

// What the rebuild replaces, kept until the new state has been laid out: a failure after the swap puts everything back
struct RebuildSaved {
    DevBuf nodes, idx;              // the fresh buffers before the swap, the context's old ones after it
    std::vector<unsigned char> host7, host8, host9;
    std::map<int, rz_bvh_node> devRoots;
    std::map<std::tuple<int, int, int>, double> costBuilt;
    Residency blas, tlas;           // of the arrays above (instances and TLAS: on the host, on either side of the swap)
    bool tmpValid = false;
    size_t devNodes = 0, devIdx = 0;
};

static void rebuild_swap(rz_ctx* c, RebuildSaved& S) {
    std::swap(c->dRawNodes, S.nodes);
    std::swap(c->dRawIdx, S.idx);
    c->host[RZ_BIND_BLAS_NODES].swap(S.host7);
    c->host[RZ_BIND_BLAS_INDICES].swap(S.host8);
    c->host[RZ_BIND_INSTANCES].swap(S.host9);
    c->devRoots.swap(S.devRoots);
    c->costBuilt.swap(S.costBuilt);
    std::swap(c->where[kBlas], S.blas);
    std::swap(c->where[kTlas], S.tlas);
    std::swap(c->tmpValid, S.tmpValid);
    std::swap(c->devNodes, S.devNodes);
    std::swap(c->devIdx, S.devIdx);
    c->costGen = ~0ull;
    c->geomDirty = true;            // the views are laid out again from whichever arrays are in place now
}

static int rebuild_geometry_impl(rz_ctx* c, double maxRatio, rz_mesh_quality* out, size_t cap, size_t* nMeshes, unsigned flags) {
    const char* what = "rz_rebuild_geometry";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (!(maxRatio >= 0.0)) return fail(c, RZ_ERR_INVALID_ARG, "%s: max_ratio must be >= 0", what);
    if (!out && !nMeshes) return fail(c, RZ_ERR_INVALID_ARG, "%s: neither out nor n_meshes", what);
    { const int b = refit_missing_binding(c); if (b >= 0) return fail(c, RZ_ERR_NOT_READY, "%s: no scene (binding %d has not been uploaded)", what, b); }
    RZ_HIP(c, hipSetDevice(c->device));
    int rc = finalize(c);
    if (rc != RZ_OK) return rc;
    NamedMeshes named;
    named_meshes(c, named);
    const size_t nM = named.size();
    if (nMeshes) *nMeshes = nM;
    if (!out) return RZ_OK;
    if (cap < nM) return fail(c, RZ_ERR_INVALID_ARG, "%s: out holds %zu records, the scene has %zu meshes", what, cap, nM);
    // 1. measure; 2. select
    std::vector<QualityMesh> M;
    if ((rc = measure_meshes(c, named, M)) != RZ_OK) return rc;
    alloc_point(c);
    std::vector<char> sel(M.size(), 0);
    bool any = false;
    for (size_t k = 0; k < M.size(); ++k) {
        sel[k] = !(M[k].cost <= maxRatio * c->costBuilt.at(M[k].key));
        any = any || sel[k];
    }
    if (!any) {                         // 3. the context is untouched
        for (size_t k = 0; k < M.size(); ++k) out[k] = quality_record(c, M[k]);
        return RZ_OK;
    }
    // Is the scene rebuildable this way?  Meshes in ascending blasNodeOffset; a mesh's node extent is [its offset, the next
    // larger distinct offset or the end of binding 7); its index extent is [blasTriOffset, + its slots).
    if ((rc = refit_topology(c)) != RZ_OK) return rc;
    const long long nNodes = (long long)blasNodeCount(c), nIdx = (long long)blasIdxCount(c);
    const long long nTris = (long long)hostCount<rz_triangle>(c, RZ_BIND_TRIANGLES);
    std::map<std::tuple<int, int, int>, int> maxNode;
    for (const RefitView& R : c->refitViews) maxNode[R.key] = R.maxNode;
    std::vector<std::pair<long long, long long>> idxExtents;
    for (size_t k = 0; k < M.size(); ++k) {
        const long long off = std::get<0>(M[k].key), end = k + 1 < M.size() ? std::get<0>(M[k + 1].key) : nNodes;
        if (end == off) return fail(c, RZ_ERR_INVALID_ARG, "%s: two meshes share the node extent at %lld", what, off);
        if (maxNode.at(M[k].key) >= end - off)
            return fail(c, RZ_ERR_INVALID_ARG, "%s: the mesh at node %lld reaches node %d, outside its extent of %lld", what, off, maxNode.at(M[k].key), end - off);
        const long long t0 = std::get<1>(M[k].key), g0 = std::get<2>(M[k].key);
        if (t0 < 0 || t0 + M[k].nSlots > nIdx || g0 < 0 || g0 + M[k].nSlots > nTris)
            return fail(c, RZ_ERR_INVALID_ARG, "%s: the mesh at node %lld names indices or triangles outside their arrays", what, off);
        if (M[k].nSlots > 0) idxExtents.push_back({t0, t0 + M[k].nSlots});
    }
    std::sort(idxExtents.begin(), idxExtents.end());
    for (size_t k = 1; k < idxExtents.size(); ++k)
        if (idxExtents[k].first < idxExtents[k - 1].second)
            return fail(c, RZ_ERR_INVALID_ARG, "%s: two meshes share the index extent at %lld", what, idxExtents[k].first);
    // 4. new bindings 7 and 8 in fresh buffers (as rz_build_geometry: the context's arrays are never written to)
    if ((rc = host_changed(c, kTlas)) != RZ_OK) return rc;      // the instances with the transforms in force: their node offsets are patched below
    const bool devGeom = c->where[kBlas].dev, devTris = c->where[kTris].dev;    // read where they are current (a device layout keeps a copy)
    const rz_bvh_node* srcNodes = devGeom ? static_cast<const rz_bvh_node*>(c->dRawNodes.p) : hostArr<rz_bvh_node>(c, RZ_BIND_BLAS_NODES);
    const int32_t* srcIdx = devGeom ? static_cast<const int32_t*>(c->dRawIdx.p) : hostArr<int32_t>(c, RZ_BIND_BLAS_INDICES);
    const rz_triangle* srcTris = devTris ? static_cast<const rz_triangle*>(c->dRawTris.p) : hostArr<rz_triangle>(c, RZ_BIND_TRIANGLES);
    const long long lead = M.empty() ? nNodes : std::get<0>(M[0].key);  // (nodes in front of the first mesh stay)
    size_t capNodes = (size_t)lead, maxN = 0;
    for (size_t k = 0; k < M.size(); ++k) {
        const long long off = std::get<0>(M[k].key), end = k + 1 < M.size() ? std::get<0>(M[k + 1].key) : nNodes;
        capNodes += sel[k] ? (M[k].nSlots ? 2 * (size_t)M[k].nSlots - 1 : 1) : (size_t)(end - off);
        if (sel[k]) maxN = std::max(maxN, (size_t)M[k].nSlots);
    }
    if (capNodes >= ((size_t)1 << 27)) return fail(c, RZ_ERR_INVALID_ARG, "%s: too many nodes", what);
    RebuildSaved S;
    if ((rc = ensure(c, S.nodes, std::max<size_t>(capNodes, 1) * sizeof(rz_bvh_node))) != RZ_OK) return rc;
    if ((rc = ensure(c, S.idx, std::max<size_t>((size_t)nIdx, 1) * sizeof(int32_t))) != RZ_OK) return rc;
    if (maxN) { rc = ensure(c, c->dBuildWs, blas_build_workspace_bytes(maxN)); if (rc != RZ_OK) return rc; }
    rz_bvh_node* dNodes = static_cast<rz_bvh_node*>(S.nodes.p);
    int32_t* dIdx = static_cast<int32_t*>(S.idx.p);
    if (nIdx) RZ_HIP(c, hipMemcpyAsync(dIdx, srcIdx, (size_t)nIdx * sizeof(int32_t), hipMemcpyDefault, c->stream));
    if (lead) RZ_HIP(c, hipMemcpyAsync(dNodes, srcNodes, (size_t)lead * sizeof(rz_bvh_node), hipMemcpyDefault, c->stream));
    std::vector<int> newOff(M.size(), 0);
    rz_bvh_node emptyRoot{};            // BVH.cpp:101-118 on an empty mesh: one root with an inverted box and no triangles
    for (int a = 0; a < 3; ++a) { emptyRoot.boundsMin[a] = std::numeric_limits<float>::max(); emptyRoot.boundsMax[a] = -std::numeric_limits<float>::max(); }
    size_t at = (size_t)lead;
    for (size_t k = 0; k < M.size(); ++k) {
        const long long off = std::get<0>(M[k].key), end = k + 1 < M.size() ? std::get<0>(M[k + 1].key) : nNodes;
        newOff[k] = (int)at;
        if (!sel[k]) {                  // its extent verbatim (leftFirst is mesh-relative), shifted
            RZ_HIP(c, hipMemcpyAsync(dNodes + at, srcNodes + off, (size_t)(end - off) * sizeof(rz_bvh_node), hipMemcpyDefault, c->stream));
            at += (size_t)(end - off);
        } else if (M[k].nSlots == 0) {  // (its cost is 0: only max_ratio = +inf selects it, inf * 0 being NaN)
            RZ_HIP(c, hipMemcpyAsync(dNodes + at, &emptyRoot, sizeof emptyRoot, hipMemcpyHostToDevice, c->stream));   // (left by the synchronisation below)
            at += 1;
        } else {                        // BVH::buildBLAS of its triangles of binding 0 as it stands, by the device builder
            int nn = 0, depth = 0;
            const int e = blas_build_device(srcTris + std::get<2>(M[k].key), (size_t)M[k].nSlots, c->dBuildWs.p, c->dBuildWs.cap, dNodes + at,
                                            dIdx + std::get<1>(M[k].key), &nn, &depth, nullptr, c->stream);
            if (e > 0) return fail(c, RZ_ERR_HIP, "%s: device BLAS build of the mesh at node %lld: %s", what, off, hipGetErrorString((hipError_t)e));
            if (e < 0) return fail(c, RZ_ERR_HIP, "%s: device BLAS build of the mesh at node %lld: internal limit", what, off);
            at += (size_t)nn;
        }
    }
    RZ_HIP(c, hipStreamSynchronize(c->stream));        // the copies have left the host arrays; nothing in flight reads the old ones
    // the new instances, root nodes and built costs: every allocation that can fail, before anything of the context changes
    alloc_point(c);
    S.host9 = c->host[RZ_BIND_INSTANCES];
    {
        rz_bvh_instance* inst = reinterpret_cast<rz_bvh_instance*>(S.host9.data());
        const size_t nInst = S.host9.size() / sizeof(rz_bvh_instance);
        std::map<int, int> moved;
        for (size_t k = 0; k < M.size(); ++k) moved[std::get<0>(M[k].key)] = newOff[k];
        for (size_t i = 0; i < nInst; ++i) inst[i].blasNodeOffset = moved.at(inst[i].blasNodeOffset);
    }
    for (size_t k = 0; k < M.size(); ++k) {
        rz_bvh_node root;
        RZ_HIP(c, hipMemcpy(&root, dNodes + newOff[k], sizeof root, hipMemcpyDeviceToHost));
        S.devRoots[newOff[k]] = root;
        if (!sel[k]) S.costBuilt[std::make_tuple(newOff[k], std::get<1>(M[k].key), std::get<2>(M[k].key))] = c->costBuilt.at(M[k].key);
    }
    S.blas.host = false; S.blas.dev = true; S.tmpValid = false;
    S.devNodes = at; S.devIdx = (size_t)nIdx;
    // the swap, then the re-layout and world boxes + TLAS with the transforms in force, exactly as rz_refit_geometry's host route
    rebuild_swap(c, S);
    std::vector<QualityMesh> After;
    try {
        rc = finalize(c);               // (binding 0 is laid out from where it is current: posed triangles stay on the device)
        if (rc == RZ_OK) rc = refit_tlas_step(c);
        if (rc == RZ_OK) { named_meshes(c, named); rc = measure_meshes(c, named, After); }
        if (rc == RZ_OK && After.size() != M.size()) rc = fail(c, RZ_ERR_INTERNAL, "%s: the rebuilt scene has %zu meshes, not %zu", what, After.size(), M.size());
    } catch (...) {
        rebuild_swap(c, S);
        throw;
    }
    if (rc != RZ_OK) { rebuild_swap(c, S); return rc; }
    for (size_t k = 0; k < M.size(); ++k) {
        rz_mesh_quality q = quality_record(c, After[k]);
        q.node_offset_before = std::get<0>(M[k].key);
        q.sah_cost_before = M[k].cost;
        q.flags = sel[k] ? RZ_QUALITY_REBUILT : 0u;
        out[k] = q;
    }
    return RZ_OK;
}

static int build_geometry_impl(rz_ctx* c, const rz_triangle* triangles, size_t nTris, rz_mesh_build* meshes, size_t nMeshes) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if ((nTris && !triangles) || (nMeshes && !meshes)) return fail(c, RZ_ERR_INVALID_ARG, "null argument");
    if (nTris > ((size_t)1 << 30)) return fail(c, RZ_ERR_INVALID_ARG, "too many triangles");
    size_t capNodes = 0, capIdx = 0, maxN = 0;
    for (size_t i = 0; i < nMeshes; ++i) {
        const rz_mesh_build& m = meshes[i];
        if (m.first_triangle > nTris || m.n_triangles > nTris - m.first_triangle)
            return fail(c, RZ_ERR_INVALID_ARG, "mesh %zu: triangles [%zu,+%zu) outside the %zu given", i, m.first_triangle, m.n_triangles, nTris);
        capNodes += m.n_triangles ? 2 * m.n_triangles - 1 : 1;
        capIdx += m.n_triangles;
        maxN = std::max(maxN, m.n_triangles);
    }
    if (capNodes > ((size_t)1 << 30)) return fail(c, RZ_ERR_INVALID_ARG, "too many nodes");
    RZ_HIP(c, hipSetDevice(c->device));
    // The build goes into FRESH buffers that replace the context's node / index arrays only when every mesh has been built:
    // a call that fails half-way (HIP error, internal limit, out of host memory) leaves the context exactly as it was -- the
    // arrays of an earlier rz_build_geometry, which devRoots / devNodes / the BLAS group's record still describe, are never written to.
    struct Fresh { DevBuf nodes, idx; } fresh;
    int rc = ensure(c, fresh.nodes, std::max<size_t>(capNodes, 1) * sizeof(rz_bvh_node));
    if (rc != RZ_OK) return rc;
    rc = ensure(c, fresh.idx, std::max<size_t>(capIdx, 1) * sizeof(int32_t));
    if (rc != RZ_OK) return rc;
    if (maxN) { rc = ensure(c, c->dBuildWs, blas_build_workspace_bytes(maxN)); if (rc != RZ_OK) return rc; }
    std::map<int, rz_bvh_node> roots;
    size_t nodeOff = 0, idxOff = 0;
    rz_bvh_node* dNodes = static_cast<rz_bvh_node*>(fresh.nodes.p);
    int32_t* dIdx = static_cast<int32_t*>(fresh.idx.p);
    for (size_t i = 0; i < nMeshes; ++i) {
        rz_mesh_build& m = meshes[i];
        int nn = 1, depth = 1;
        rz_bvh_node root{};
        if (m.n_triangles == 0) {       // BVH.cpp:101-118 on an empty mesh: one root with an inverted box and no triangles
            const float fmax = std::numeric_limits<float>::max();
            for (int k = 0; k < 3; ++k) { root.boundsMin[k] = fmax; root.boundsMax[k] = -fmax; }
            root.leftFirst = 0; root.count = 0;
            RZ_HIP(c, hipMemcpyAsync(dNodes + nodeOff, &root, sizeof root, hipMemcpyHostToDevice, c->stream));
            RZ_HIP(c, hipStreamSynchronize(c->stream));
        } else {
            const int e = blas_build_device(triangles + m.first_triangle, m.n_triangles, c->dBuildWs.p, c->dBuildWs.cap, dNodes + nodeOff,
                                            dIdx + idxOff, &nn, &depth, nullptr, c->stream);
            if (e > 0) return fail(c, RZ_ERR_HIP, "device BLAS build of mesh %zu: %s", i, hipGetErrorString((hipError_t)e));
            if (e < 0) return fail(c, RZ_ERR_HIP, "device BLAS build of mesh %zu: internal limit", i);
            RZ_HIP(c, hipMemcpy(&root, dNodes + nodeOff, sizeof root, hipMemcpyDeviceToHost));
        }
        m.node_offset = (int32_t)nodeOff; m.index_offset = (int32_t)idxOff; m.n_nodes = nn; m.depth = depth; m.root = root;
        alloc_point(c);
        roots[(int)nodeOff] = root;
        nodeOff += (size_t)nn; idxOff += m.n_triangles;
    }
    // the three geometry bindings now are: the caller's triangles (host copy, uploaded by the re-layout as usual) and the
    // device-resident node / index arrays
    alloc_point(c);
    {   // (the last allocation that can fail: a copy first, then nothing below throws)
        std::vector<unsigned char> tcopy(reinterpret_cast<const unsigned char*>(triangles), reinterpret_cast<const unsigned char*>(triangles) + nTris * sizeof(rz_triangle));
        c->host[RZ_BIND_TRIANGLES].swap(tcopy);
    }
    if ((rc = host_changed(c, kTris, RZ_BIND_TRIANGLES)) != RZ_OK) return rc;     // (replaced whole, as by rz_upload: nothing is fetched)
    RZ_HIP(c, hipStreamSynchronize(c->stream));        // nothing in flight reads the old arrays
    std::swap(c->dRawNodes, fresh.nodes);               // (the old ones are released with `fresh`)
    std::swap(c->dRawIdx, fresh.idx);
    c->host[RZ_BIND_BLAS_NODES].clear();
    c->host[RZ_BIND_BLAS_INDICES].clear();
    c->present[RZ_BIND_TRIANGLES] = c->present[RZ_BIND_BLAS_NODES] = c->present[RZ_BIND_BLAS_INDICES] = true;
    device_changed(c, kBlas);
    c->tmpValid = false;                    // (rz_denoise_temporal's history)
    c->devNodes = nodeOff; c->devIdx = idxOff;
    c->devRoots.swap(roots);
    drop_built_costs(c);
    c->geomDirty = true;
    return RZ_OK;
}

static int build_blas_impl(rz_ctx* c, const rz_triangle* tris, size_t n, rz_bvh_node* nodes_out, size_t nodes_cap, int32_t* indices_out,
                  size_t* n_nodes, int* depth, float* device_ms) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (n && !tris) return fail(c, RZ_ERR_INVALID_ARG, "null triangles");
    if (!nodes_out || (n && !indices_out)) return fail(c, RZ_ERR_INVALID_ARG, "null output");
    if (n > (size_t)1 << 30) return fail(c, RZ_ERR_INVALID_ARG, "too many triangles");
    if (nodes_cap < (n ? 2 * n - 1 : 1)) return fail(c, RZ_ERR_BUFFER_SIZE, "nodes_out holds %zu nodes, up to %zu are needed", nodes_cap, n ? 2 * n - 1 : (size_t)1);
    if (device_ms) *device_ms = 0.0f;
    if (n == 0) {        // BVH.cpp:101-118 on an empty mesh: one root with an inverted box and no triangles
        const float fmax = std::numeric_limits<float>::max();
        rz_bvh_node r{};
        for (int k = 0; k < 3; ++k) { r.boundsMin[k] = fmax; r.boundsMax[k] = -fmax; }
        r.leftFirst = 0; r.count = 0;
        nodes_out[0] = r;
        if (n_nodes) *n_nodes = 1;
        if (depth) *depth = 1;
        return RZ_OK;
    }
    RZ_HIP(c, hipSetDevice(c->device));
    const size_t ws = blas_build_workspace_bytes(n);
    int rc = ensure(c, c->dBuildWs, ws);
    if (rc != RZ_OK) return rc;
    std::vector<rz_bvh_node> tmp;
    alloc_point(c);
    tmp.resize(2 * n + 2);
    int nn = 0, dp = 0;
    const int e = blas_build_device(tris, n, c->dBuildWs.p, c->dBuildWs.cap, tmp.data(), indices_out, &nn, &dp, device_ms, c->stream);
    if (e > 0) return fail(c, RZ_ERR_HIP, "device BLAS build: %s", hipGetErrorString((hipError_t)e));
    if (e < 0) return fail(c, RZ_ERR_HIP, "device BLAS build: internal limit");
    if ((size_t)nn > nodes_cap) return fail(c, RZ_ERR_BUFFER_SIZE, "nodes_out holds %zu nodes, %d were built", nodes_cap, nn);
    std::memcpy(nodes_out, tmp.data(), (size_t)nn * sizeof(rz_bvh_node));
    if (n_nodes) *n_nodes = (size_t)nn;
    if (depth) *depth = dp;
    return RZ_OK;
}

static int read_binding_impl(rz_ctx* c, rz_binding binding, void* out, size_t bytes, size_t* needed) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (elem_size((int)binding) == 0) return fail(c, RZ_ERR_INVALID_ARG, "unknown binding %d", (int)binding);
    if (!c->present[binding]) return fail(c, RZ_ERR_NOT_READY, "binding %d has not been uploaded", (int)binding);
    { const int rc = host_copy_for(c, binding); if (rc != RZ_OK) return rc; }
    const size_t have = c->host[binding].size();
    if (needed) *needed = have;
    if (!out) return RZ_OK;
    if (bytes < have) return fail(c, RZ_ERR_BUFFER_SIZE, "binding %d holds %zu bytes, buffer has %zu", (int)binding, have, bytes);
    if (have) std::memcpy(out, c->host[binding].data(), have);
    return RZ_OK;
}

static int set_frame_impl(rz_ctx* c, const rz_frame_params* p) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (!p) return fail(c, RZ_ERR_INVALID_ARG, "null params");
    if (p->width <= 0 || p->height <= 0 || (long long)p->width * p->height > (1ll << 28))
        return fail(c, RZ_ERR_INVALID_ARG, "resolution %dx%d", p->width, p->height);
    if (p->spp <= 0) return fail(c, RZ_ERR_INVALID_ARG, "spp %d", p->spp);
    if (p->sample_base < 0) return fail(c, RZ_ERR_INVALID_ARG, "sample_base %d", p->sample_base);
    if (p->tile_nranks < 1 || p->tile_rank < 0 || p->tile_rank >= p->tile_nranks)
        return fail(c, RZ_ERR_INVALID_ARG, "tile_rank %d of %d", p->tile_rank, p->tile_nranks);
    RZ_HIP(c, hipSetDevice(c->device));
    const size_t nPix = (size_t)p->width * p->height;
    const bool resized = !c->haveFrame || c->frame.width != p->width || c->frame.height != p->height;
    if (resized) {
        int rc = ensure(c, c->dIor, nPix * sizeof(float));
        if (rc != RZ_OK) return rc;
        if (!c->extAccum) {
            rc = ensure(c, c->ownAccum, nPix * 16);
            if (rc != RZ_OK) return rc;
            RZ_HIP(c, hipMemsetAsync(c->ownAccum.p, 0, nPix * 16, c->stream));
        }
    }
    // a different tile assignment: pixels this context owned before and no longer owns must read as zero again
    // (the group's reduce sums every member's whole buffer)
    if (!resized && c->haveFrame && (c->frame.tile_rank != p->tile_rank || c->frame.tile_nranks != p->tile_nranks)) {
        void* acc = c->extAccum ? c->extAccum : c->ownAccum.p;
        if (acc && (!c->extAccum || c->extAccumBytes >= nPix * 16)) RZ_HIP(c, hipMemsetAsync(acc, 0, nPix * 16, c->stream));
    }
    c->frame = *p;
    c->haveFrame = true;
    return RZ_OK;
}

int rz_set_stream(rz_ctx* c, void* hip_stream) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    return guarded(c, "rz_set_stream", [&]() -> int {
        (void)hipStreamSynchronize(c->stream);
        c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->ownStream;
        return RZ_OK;
    });
}

static int bind_accum_impl(rz_ctx* c, void* device_rgba, size_t bytes) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    c->extAccum = device_rgba;
    c->extAccumBytes = device_rgba ? bytes : 0;
    if (!device_rgba && c->haveFrame) {
        const size_t nPix = (size_t)c->frame.width * c->frame.height;
        RZ_HIP(c, hipSetDevice(c->device));
        int rc = ensure(c, c->ownAccum, nPix * 16);
        if (rc != RZ_OK) return rc;
        RZ_HIP(c, hipMemsetAsync(c->ownAccum.p, 0, nPix * 16, c->stream));
    }
    return RZ_OK;
}

int rz_sync(rz_ctx* c) {
#ifdef RZ_GSTATS
    if (c) { (void)hipStreamSynchronize(c->stream); dump_gstats(); }
#endif
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    return guarded(c, "rz_sync", [&]() -> int {
        RZ_HIP(c, hipStreamSynchronize(c->stream));
        unsigned bits = 0;
        const int rc = take_backstop(c, bits);
        if (rc != RZ_OK) return rc;
        if (bits != 0u)
            return fail(c, RZ_ERR_INTERNAL, "a render kernel reached a backstop (bits 0x%x:%s%s%s%s): pixels of the last frame(s) may be missing",
                        bits, (bits & 1u) ? " claim without wait slots" : "", (bits & 2u) ? " pool did not drain" : "", (bits & 4u) ? " currentIor chains did not resolve" : "",
                        (bits & RZ_BACKSTOP_RAYS) ? " a ray query's walk was cut short" : "");
        return RZ_OK;
    });
}

int rz_debug_poke_backstop(rz_ctx* c, unsigned bits) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    return guarded(c, "rz_debug_poke_backstop", [&]() -> int {
        int rc = ensure_group_counter(c);
        if (rc != RZ_OK) return rc;
        RZ_HIP(c, hipStreamSynchronize(c->stream));
        RZ_HIP(c, hipMemcpy(static_cast<unsigned*>(c->dGroupCtr.p) + RZ_ERRWORD, &bits, sizeof bits, hipMemcpyHostToDevice));
        return RZ_OK;
    });
}

void* rz_stream_handle(rz_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

void* rz_accum_device_ptr(rz_ctx* c) {
    if (!c) return nullptr;
    return c->extAccum ? c->extAccum : c->ownAccum.p;
}

static int clear_accum_impl(rz_ctx* c) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "rz_set_frame has not been called");
    void* p = rz_accum_device_ptr(c);
    RZ_HIP(c, hipMemsetAsync(p, 0, (size_t)c->frame.width * c->frame.height * 16, c->stream));
    return RZ_OK;
}

static int read_accum_impl(rz_ctx* c, float* rgba, size_t bytes) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "rz_set_frame has not been called");
    const size_t need = (size_t)c->frame.width * c->frame.height * 16;
    if (!rgba || bytes < need) return fail(c, RZ_ERR_BUFFER_SIZE, "rz_read_accum needs %zu bytes, got %zu", need, bytes);
    RZ_HIP(c, hipMemcpyAsync(rgba, rz_accum_device_ptr(c), need, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return RZ_OK;
}

static int resolve_rgba8_impl(rz_ctx* c, uint8_t* rgba8, size_t bytes) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "rz_set_frame has not been called");
    const size_t nPix = (size_t)c->frame.width * c->frame.height;
    if (!rgba8 || bytes < nPix * 4) return fail(c, RZ_ERR_BUFFER_SIZE, "rz_resolve_rgba8 needs %zu bytes, got %zu", nPix * 4, bytes);
    int rc = ensure(c, c->dResolve, nPix * 4);
    if (rc != RZ_OK) return rc;
    launch_resolve(static_cast<const float4*>(rz_accum_device_ptr(c)), static_cast<uchar4*>(c->dResolve.p), (int)nPix, c->stream);
    RZ_HIP(c, hipGetLastError());
    RZ_HIP(c, hipMemcpyAsync(rgba8, c->dResolve.p, nPix * 4, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return RZ_OK;
}

// (accum: what to resolve -- the context's accumulation when null; rz_present_denoised passes the denoised (colour, 1).
//  width, height: the size of `accum` and of the outputs -- the frame's when 0; rz_present_upscaled passes the high size)
static int present_impl(rz_ctx* c, const rz_present_params* pp, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes,
                        const float4* accum = nullptr, int width = 0, int height = 0) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (!pp) return fail(c, RZ_ERR_INVALID_ARG, "null params");
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "rz_set_frame has not been called");
    int rc = finalize(c);
    if (rc != RZ_OK) return rc;
    if (width <= 0 || height <= 0) { width = c->frame.width; height = c->frame.height; }
    const size_t nPix = (size_t)width * height;
    if (rgba8 && rgba8_bytes < nPix * 4) return fail(c, RZ_ERR_BUFFER_SIZE, "rgba8 buffer needs %zu bytes", nPix * 4);
    if (rgb32f && rgb32f_bytes < nPix * 12) return fail(c, RZ_ERR_BUFFER_SIZE, "rgb32f buffer needs %zu bytes", nPix * 12);
    rc = ensure(c, c->dResolve, nPix * 4 + nPix * 12);
    if (rc != RZ_OK) return rc;
    PresentParams P{};
    P.accum = accum ? accum : static_cast<const float4*>(rz_accum_device_ptr(c));
    P.rgba8 = static_cast<uchar4*>(c->dResolve.p);
    P.rgb = reinterpret_cast<float*>(static_cast<char*>(c->dResolve.p) + nPix * 4);
    P.tlasNodes = static_cast<const TlasNode*>(c->dTlasNodes.p);
    P.tlasIndices = static_cast<const int32_t*>(c->dTlasIdx.p);
    P.instances = static_cast<const DevInstance*>(c->dInst.p);
    P.lights = static_cast<const DevLight*>(c->dLight.p);
    P.width = width; P.height = height;
    P.nTlasNodes = c->where[kTlas].host ? (int)hostCount<rz_bvh_node>(c, RZ_BIND_TLAS_NODES) : c->devTlasNodes;
    P.nInstances = (int)hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    P.nLights = std::max(0, std::min<int>(c->frame.num_lights, (int)hostCount<rz_light>(c, RZ_BIND_LIGHTS)));
    // camera.projectionMatrix * camera.viewMatrix, terms summed left to right (glsl:321)
    const float* A = c->frame.proj; const float* B = c->frame.view;
    for (int col = 0; col < 4; ++col)
        for (int row = 0; row < 4; ++row)
            P.viewProj[col * 4 + row] = ((A[0 * 4 + row] * B[col * 4 + 0] + A[1 * 4 + row] * B[col * 4 + 1]) +
                                         A[2 * 4 + row] * B[col * 4 + 2]) + A[3 * 4 + row] * B[col * 4 + 3];
    // rz_present_params.fps: a value whose conversion to int is undefined (non-finite, |fps| >= 2^31) draws 000.0
    P.fps = (std::isfinite(pp->fps) && std::fabs(pp->fps) < 2147483648.0f) ? pp->fps : 0.0f;
    P.showFps = pp->show_fps; P.showLights = pp->show_lights; P.showBvh = pp->show_bvh; P.bvhMode = pp->bvh_mode;
    P.pathLen = 0;
    if (pp->show_bvh && pp->bvh_mode == 1 && pp->selected_blas >= 0 && pp->selected_blas < P.nInstances) {
        // findBVHBranchIterative (glsl:257-307) does not depend on the pixel: walk it once here
        for (int g : {kTlas, kBlas}) if ((rc = need_host(c, g)) != RZ_OK) return rc;
        const rz_bvh_instance* inst = hostArr<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
        const rz_bvh_node* nodes = hostArr<rz_bvh_node>(c, RZ_BIND_BLAS_NODES);
        const int32_t* idx = hostArr<int32_t>(c, RZ_BIND_BLAS_INDICES);
        const long long nNodes = (long long)hostCount<rz_bvh_node>(c, RZ_BIND_BLAS_NODES), nIdx = (long long)hostCount<int32_t>(c, RZ_BIND_BLAS_INDICES);
        const rz_bvh_instance& S = inst[pp->selected_blas];
        const int nodeOffset = S.blasNodeOffset, triOffset = S.blasTriOffset;
        const int nodeCount = (pp->selected_blas + 1 < P.nInstances) ? inst[pp->selected_blas + 1].blasNodeOffset - nodeOffset : (int)nNodes - nodeOffset;
        auto leafHas = [&](const rz_bvh_node& n) {
            for (int k = 0; k < n.count; ++k) { long long j = (long long)triOffset + n.leftFirst + k; if (j >= 0 && j < nIdx && idx[j] == pp->selected_tri) return true; }
            return false;
        };
        int path[32], len = 0, cur = 0;
        for (int depth = 0; depth < 32; ++depth) {
            path[len++] = cur;
            if ((long long)nodeOffset + cur < 0 || (long long)nodeOffset + cur >= nNodes) { len = 0; break; }
            const rz_bvh_node& node = nodes[nodeOffset + cur];
            if (node.count > 0) { if (!leafHas(node)) len = 0; break; }
            bool inLeft = false;
            int stack[32], sp = 0;
            stack[sp++] = node.leftFirst;
            while (sp > 0) {
                const int nidx = stack[--sp];
                if (nidx < 0 || nidx >= nodeCount || (long long)nodeOffset + nidx >= nNodes) continue;
                const rz_bvh_node& n = nodes[nodeOffset + nidx];
                if (n.count > 0) inLeft = leafHas(n);
                else if (sp + 2 <= 32) { stack[sp++] = n.leftFirst; stack[sp++] = n.leftFirst + 1; }
                if (inLeft) break;
            }
            cur = inLeft ? node.leftFirst : node.leftFirst + 1;
        }
        P.pathLen = len;
        for (int k = 0; k < len; ++k) {
            std::memcpy(P.pathMin[k], nodes[nodeOffset + path[k]].boundsMin, 12);
            std::memcpy(P.pathMax[k], nodes[nodeOffset + path[k]].boundsMax, 12);
        }
        std::memcpy(P.selTransform, S.transform, 64);
    }
    {   // projected-corner cache: one 112-B record per box a pixel may draw
        const size_t nBoxes = (size_t)P.nTlasNodes + (size_t)P.nInstances + 32;
        rc = ensure(c, c->dProjBoxes, nBoxes * 112);
        if (rc != RZ_OK) return rc;
        P.boxes = static_cast<ProjBox*>(c->dProjBoxes.p);
    }
    launch_present(P, c->stream);
    RZ_HIP(c, hipGetLastError());
    if (rgba8) RZ_HIP(c, hipMemcpyAsync(rgba8, P.rgba8, nPix * 4, hipMemcpyDeviceToHost, c->stream));
    if (rgb32f) RZ_HIP(c, hipMemcpyAsync(rgb32f, P.rgb, nPix * 12, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return RZ_OK;
}

// The globalTriOffset of every instance on the device (RaysLaunch / EditorLaunch::instTriOff), re-uploaded after the
// instances change.
static int ensure_ray_inst_off(rz_ctx* c) {
    if (!c->rayInstOffStale) return RZ_OK;
    const rz_bvh_instance* inst = hostArr<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    alloc_point(c);
    std::vector<int32_t> off(nInst);
    for (size_t i = 0; i < nInst; ++i) off[i] = inst[i].globalTriOffset;     // (rz_update_transforms keeps the offsets)
    const int rc = upload_vec(c, c->dRayInstOff, off.data(), nInst * sizeof(int32_t));
    if (rc != RZ_OK) return rc;
    RZ_HIP(c, hipStreamSynchronize(c->stream));     // the staging vector dies at scope exit
    c->rayInstOffStale = false;
    return RZ_OK;
}

// The steps the off-frame passes below share (HostStage, cast_wiring, camera_kparams and report_backstop sit beside
// scene_kparams).  A new pass calls them in this order: its argument checks, in the order its header documents, with scene_ready,
// accum_fits and present_sizes among them; the early return when no output is asked for; HostStage (add every output, input,
// place); then finalize, cast_ready, its own ensure()s, guide_cast or a cast of its own wired by cast_wiring, and its kernels;
// on the host path HostStage::fetch, and report_backstop if a ray was cast.

// The scene a cast walks: all eight bindings uploaded and, for a pass that shades, at least one material.
static int scene_ready(rz_ctx* c, const char* what, bool materials) {
    for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS, RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES,
                  RZ_BIND_BLAS_NODES, RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES})
        if (!c->present[b]) return fail(c, RZ_ERR_NOT_READY, "%s: no scene (binding %d has not been uploaded)", what, b);
    if (materials && hostCount<rz_material>(c, RZ_BIND_MATERIALS) == 0) return fail(c, RZ_ERR_NOT_READY, "%s: no materials", what);
    return RZ_OK;
}

// A bound accumulation buffer (rz_bind_accum) must hold the frame a pass is about to read from it.
static int accum_fits(rz_ctx* c, const char* what) {
    const size_t need = (size_t)c->frame.width * c->frame.height * 16;
    if (c->extAccum && c->extAccumBytes < need)
        return fail(c, RZ_ERR_BUFFER_SIZE, "%s: bound accumulation buffer holds %zu bytes, frame needs %zu", what, c->extAccumBytes, need);
    return RZ_OK;
}

// The buffer checks of the rz_present_* family: the accumulation at the frame's size, the outputs at `pixels` (the frame's, or
// rz_present_upscaled's high size).
static int present_sizes(rz_ctx* c, const char* what, size_t pixels, const uint8_t* rgba8, size_t rgba8_bytes, const float* rgb32f,
                         size_t rgb32f_bytes) {
    const int rc = accum_fits(c, what);
    if (rc != RZ_OK) return rc;
    if (rgba8 && rgba8_bytes < pixels * 4) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba8 buffer needs %zu bytes", what, pixels * 4);
    if (rgb32f && rgb32f_bytes < pixels * 12) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f buffer needs %zu bytes", what, pixels * 12);
    return RZ_OK;
}

// What every cast needs on the device besides the scene: the backstop word and the instances' triangle offsets.
static int cast_ready(rz_ctx* c) {
    const int rc = ensure_group_counter(c);         // (only its backstop word: the claim counter is the render's)
    return rc != RZ_OK ? rc : ensure_ray_inst_off(c);
}

// One launch of rz_denoise's guide kernel at width x height with the frame's camera: the guide records, and the rz_hit records
// when asked.
static int guide_cast(rz_ctx* c, int width, int height, float4* guide, float4* hits) {
    KParams K{};
    DenoiseGuideLaunch G{};
    const int rc = cast_wiring(c, width, height, K, G);
    if (rc != RZ_OK) return rc;
    G.guide = guide;
    G.hits = hits;
    launch_denoise_guides(K, G, c->stream);
    RZ_HIP(c, hipGetLastError());
    return RZ_OK;
}

// rz_trace_rays / rz_shadow_rays (rz_rays.hip).  The queries read the device scene as the last upload / update / transform
// update left it (finalize), and nothing of the frame: no rz_set_frame needed, no render state touched.
static int rays_impl(rz_ctx* c, const rz_ray* rays, void* out, size_t n, unsigned flags, bool shadow) {
    const char* what = shadow ? "rz_shadow_rays" : "rz_trace_rays";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~(RZ_RAYS_HOST | RZ_RAYS_INCOHERENT)) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (n > (size_t)std::numeric_limits<int32_t>::max()) return fail(c, RZ_ERR_INVALID_ARG, "%s: %zu rays, at most %d per call", what, n, std::numeric_limits<int32_t>::max());
    if (n && (!rays || !out)) return fail(c, RZ_ERR_INVALID_ARG, "%s: null %s", what, rays ? "output" : "rays");
    const bool host = (flags & RZ_RAYS_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(out)) & 15u))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte aligned", what);
    int rc = scene_ready(c, what, false);
    if (rc != RZ_OK) return rc;
    if (n == 0) return RZ_OK;
    rc = finalize(c);
    if (rc != RZ_OK) return rc;
    KParams K{};
    scene_kparams(c, K);
    rc = ensure_group_counter(c);           // (only its backstop word: the claim counter is the render's)
    if (rc != RZ_OK) return rc;
    if (!shadow) {
        rc = ensure_ray_inst_off(c);
        if (rc != RZ_OK) return rc;
    }
    RaysLaunch R{};
    R.n = (int)n;
    R.grid = rays_grid((long long)n);
    R.shadow = shadow;
    R.spread = (flags & RZ_RAYS_INCOHERENT) != 0;
    R.instTriOff = static_cast<const int32_t*>(c->dRayInstOff.p);
    R.errWord = backstop_word(c);
    rc = size_blas_stack(c, K, 0, RZ_RAYS_WAVES_PER_CU, R.grid, c->dRayOvf);
    if (rc != RZ_OK) return rc;
    const size_t inBytes = n * sizeof(rz_ray), outBytes = n * (shadow ? sizeof(rz_visibility) : sizeof(rz_hit));
    R.rays = rays;
    R.out = out;
    if (host) {
        rc = ensure(c, c->dRayIn, inBytes);
        if (rc != RZ_OK) return rc;
        rc = ensure(c, c->dRayOut, outBytes);
        if (rc != RZ_OK) return rc;
        RZ_HIP(c, hipMemcpyAsync(c->dRayIn.p, rays, inBytes, hipMemcpyHostToDevice, c->stream));
        R.rays = c->dRayIn.p;
        R.out = c->dRayOut.p;
    }
    launch_rays(K, R, c->stream);
    RZ_HIP(c, hipGetLastError());
    if (!host) return RZ_OK;
    RZ_HIP(c, hipMemcpyAsync(out, c->dRayOut.p, outBytes, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return report_backstop(c, what, "results may be wrong");
}

// rz_render_editor (rz_editor.hip).  Like the ray queries it reads the device scene as finalize left it and touches no render
// state; of the frame it reads only what the call is given (width, height, the four matrices, cam_pos, num_lights).
static int editor_impl(rz_ctx* c, const rz_frame_params* f, const rz_editor_params* ep, uint8_t* rgba8, size_t rgba8_bytes,
                       float* rgb32f, size_t rgb32f_bytes, rz_hit* hits, size_t hits_bytes, unsigned flags) {
    const char* what = "rz_render_editor";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!f) return fail(c, RZ_ERR_INVALID_ARG, "%s: null frame", what);
    if (flags & ~(RZ_EDITOR_HOST | RZ_EDITOR_INCOHERENT)) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (f->width <= 0 || f->height <= 0) return fail(c, RZ_ERR_INVALID_ARG, "%s: bad size %dx%d", what, f->width, f->height);
    const size_t np = (size_t)f->width * (size_t)f->height;
    if (np > (size_t)std::numeric_limits<int32_t>::max())
        return fail(c, RZ_ERR_INVALID_ARG, "%s: %zu pixels, at most %d per frame", what, np, std::numeric_limits<int32_t>::max());
    const bool host = (flags & RZ_EDITOR_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(hits) & 15u) || ((reinterpret_cast<uintptr_t>(rgba8) | reinterpret_cast<uintptr_t>(rgb32f)) & 3u)))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte (hits) or 4-byte (rgba8, rgb32f) aligned", what);
    const size_t bRgba = np * 4, bRgb = np * 3 * sizeof(float), bHits = np * sizeof(rz_hit);
    if (rgba8 && rgba8_bytes < bRgba) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba8 needs %zu bytes, got %zu", what, bRgba, rgba8_bytes);
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (hits && hits_bytes < bHits) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: hits needs %zu bytes, got %zu", what, bHits, hits_bytes);
    int rc = scene_ready(c, what, true);
    if (rc != RZ_OK) return rc;
    rc = finalize(c);
    if (rc != RZ_OK) return rc;
    KParams K{};
    camera_kparams(c, K, f->width, f->height, f->inv_view, f->inv_proj, f->cam_pos);
    K.nLights = std::max(0, std::min<int>(f->num_lights, (int)hostCount<rz_light>(c, RZ_BIND_LIGHTS)));
    rc = cast_ready(c);
    if (rc != RZ_OK) return rc;
    EditorLaunch E{};
    std::memcpy(E.view, f->view, 64);
    std::memcpy(E.proj, f->proj, 64);
    static const rz_editor_params defaults = {{0.03f, 0.03f, 0.03f}, 0.0f, {0.05f, 0.05f, 0.07f, 1.0f}};   // main.cpp:1269, 260
    const rz_editor_params& P = ep ? *ep : defaults;
    std::memcpy(E.ambient, P.ambient, sizeof E.ambient);
    std::memcpy(E.clear, P.clear, sizeof E.clear);
    // A wave covers 64 pixels of one row: measured faster than an 8 x 8 tile on C2 (0.175 vs 0.222 ms), C4 (0.357 vs 0.503) and
    // C5 at 4K (0.620 vs 0.744), slower on c2close (0.479 vs 0.418) and RayZen's own scene (0.061 vs 0.059; profiles/editor/).
    // RZ_EDITOR_TILES=1 selects the tiles (A/B aid: same bytes).
    const char* tilesEnv = std::getenv("RZ_EDITOR_TILES");
    E.rows = (tilesEnv && std::atoi(tilesEnv) != 0) ? 0 : 1;
    const int unitW = E.rows ? 64 : RZ_TILE_W, unitH = E.rows ? 1 : RZ_TILE_H;
    E.unitsX = (f->width + unitW - 1) / unitW;
    E.units = (long long)E.unitsX * ((f->height + unitH - 1) / unitH);
    E.grid = rays_grid(E.units * 64);
    E.spread = (flags & RZ_EDITOR_INCOHERENT) != 0;
    E.instTriOff = static_cast<const int32_t*>(c->dRayInstOff.p);
    E.errWord = backstop_word(c);
    rc = size_blas_stack(c, K, 0, RZ_RAYS_WAVES_PER_CU, E.grid, c->dRayOvf);
    if (rc != RZ_OK) return rc;
    // host outputs are staged through one buffer of the context: hits, then rgb32f, then rgba8 (each 16-byte aligned)
    HostStage stage(c, host);
    const int sHits = stage.add(hits, bHits), sRgb = stage.add(rgb32f, bRgb), sRgba = stage.add(rgba8, bRgba);
    rc = stage.place();
    if (rc != RZ_OK) return rc;
    E.hits = stage.dev<float4>(sHits);
    E.rgb32f = stage.dev<float>(sRgb);
    E.rgba8 = stage.dev<uchar4>(sRgba);
    launch_editor(K, E, c->stream);
    RZ_HIP(c, hipGetLastError());
    if (!host) return RZ_OK;
    rc = stage.fetch();
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "pixels may be wrong");
}

// rz_denoise / rz_present_denoised (rz_denoise.hip).  Like the ray queries they read the device scene as finalize left it;
// of the frame they read what rz_set_frame set (size and camera), and they touch no render state.
static const rz_denoise_params kDenoiseDefaults = {5, 0.5f, 128.0f, 1.0f, 1, {0, 0, 0}};

static int denoise_check(rz_ctx* c, const char* what, const rz_denoise_params& P) {
    if (P.iterations < 0 || P.iterations > 10) return fail(c, RZ_ERR_INVALID_ARG, "%s: iterations %d outside 0..10", what, P.iterations);
    if (!(P.sigma_color > 0.0f && P.sigma_color < INFINITY) || !(P.sigma_plane > 0.0f && P.sigma_plane < INFINITY) ||
        !(P.sigma_normal >= 0.0f && P.sigma_normal < INFINITY))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: sigma_color %g, sigma_normal %g, sigma_plane %g (finite; > 0, >= 0, > 0)", what,
                    (double)P.sigma_color, (double)P.sigma_normal, (double)P.sigma_plane);
    if (P.demodulate != 0 && P.demodulate != 1) return fail(c, RZ_ERR_INVALID_ARG, "%s: demodulate %d (0 or 1)", what, P.demodulate);
    if (P.reserved[0] || P.reserved[1] || P.reserved[2]) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "%s: rz_set_frame has not been called", what);
    const int rc = scene_ready(c, what, true);
    if (rc != RZ_OK) return rc;
    if (c->frame.tile_nranks > 1)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: the frame is tile %d of %d; the filter needs the whole frame", what, c->frame.tile_rank, c->frame.tile_nranks);
    return RZ_OK;
}

// Casts the guide and runs the K passes on the stream.  in: RGBA32F sum and count (device); outputs (device, each optional):
// rgb (3 floats per pixel), out4 ((colour, 1) per pixel), hits (rz_hit per pixel).
static int denoise_run(rz_ctx* c, const rz_denoise_params& P, const float4* in, float* rgb, float4* out4, float4* hits) {
    if (!rgb && !out4 && !hits) return RZ_OK;
    const rz_frame_params& f = c->frame;
    const size_t np = (size_t)f.width * f.height;
    int rc = finalize(c);
    if (rc != RZ_OK) return rc;
    DenoiseLaunch D{};
    D.accum = in;
    D.materials = static_cast<const DevMaterial*>(c->dMat.p);
    D.width = f.width; D.height = f.height;
    D.demodulate = P.demodulate;
    if ((rgb || out4) && P.iterations == 0) {           // c_p itself: no guide needed
        D.dst = out4;
        D.rgb = rgb;
        launch_denoise_resolve(D, c->stream);
        RZ_HIP(c, hipGetLastError());
        if (!hits) return RZ_OK;
    }
    rc = cast_ready(c);
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dDnGuide, np * 32);
    if (rc != RZ_OK) return rc;
    float4* guide = static_cast<float4*>(c->dDnGuide.p);
    rc = guide_cast(c, f.width, f.height, guide, hits);
    if (rc != RZ_OK) return rc;
    if ((!rgb && !out4) || P.iterations == 0) return RZ_OK;
    if (P.iterations > 1) {
        rc = ensure(c, c->dDnPing, np * 16);
        if (rc != RZ_OK) return rc;
    }
    if (P.iterations > 2) {
        rc = ensure(c, c->dDnPong, np * 16);
        if (rc != RZ_OK) return rc;
    }
    D.guide = guide;
    const double fpx = 2.0 * std::fabs((double)f.inv_proj[5]) / (double)f.height;     // world size of a pixel at unit distance
    float4* ping = static_cast<float4*>(c->dDnPing.p);
    float4* pong = static_cast<float4*>(c->dDnPong.p);
    for (int i = 0; i < P.iterations; ++i) {
        const bool last = i == P.iterations - 1;
        const double s = (double)(1 << i);
        D.step = 1 << i;
        D.invColor = (float)(s / ((double)P.sigma_color * (double)P.sigma_color));
        D.sigmaNormal = P.sigma_normal;
        D.planeScale = (float)(1.0 / ((double)P.sigma_plane * fpx * s));
        D.src = (i % 2 == 1) ? ping : pong;         // pass i reads what pass i - 1 wrote (pass 0 reads D.accum)
        D.dst = last ? out4 : ((i % 2 == 0) ? ping : pong);
        D.rgb = last ? rgb : nullptr;
        launch_denoise_pass(D, i == 0, last, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    return RZ_OK;
}

static int denoise_impl(rz_ctx* c, const rz_denoise_params* pp, const float* rgba_in, size_t rgba_in_bytes, float* rgb32f,
                        size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, unsigned flags) {
    const char* what = "rz_denoise";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~RZ_DENOISE_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const rz_denoise_params& P = pp ? *pp : kDenoiseDefaults;
    int rc = denoise_check(c, what, P);
    if (rc != RZ_OK) return rc;
    const bool host = (flags & RZ_DENOISE_HOST) != 0;
    if (!host && (((reinterpret_cast<uintptr_t>(rgba_in) | reinterpret_cast<uintptr_t>(guides)) & 15u) || (reinterpret_cast<uintptr_t>(rgb32f) & 3u)))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte (rgba_in, guides) or 4-byte (rgb32f) aligned", what);
    const size_t np = (size_t)c->frame.width * c->frame.height;
    const size_t bIn = np * 16, bRgb = np * 3 * sizeof(float), bHits = np * sizeof(rz_hit);
    if (rgba_in && rgba_in_bytes < bIn) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba_in needs %zu bytes, got %zu", what, bIn, rgba_in_bytes);
    if (!rgba_in) {
        rc = accum_fits(c, what);
        if (rc != RZ_OK) return rc;
    }
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (guides && guides_bytes < bHits) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: guides needs %zu bytes, got %zu", what, bHits, guides_bytes);
    if (!rgb32f && !guides) return RZ_OK;
    const float4* in = rgba_in ? reinterpret_cast<const float4*>(rgba_in) : static_cast<const float4*>(rz_accum_device_ptr(c));
    // host buffers are staged through the ray-query buffers of the context: the input in dRayIn; hits, then rgb32f in dRayOut
    HostStage stage(c, host);
    const int sHits = stage.add(guides, bHits), sRgb = stage.add(rgb32f, bRgb);
    rc = stage.input(reinterpret_cast<const float4*>(rgba_in), bIn, in);
    if (rc == RZ_OK) rc = stage.place();
    if (rc != RZ_OK) return rc;
    rc = denoise_run(c, P, in, stage.dev<float>(sRgb), nullptr, stage.dev<float4>(sHits));
    if (rc != RZ_OK) return rc;
    if (!host) return RZ_OK;
    rc = stage.fetch();
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the guide may be wrong");
}

static int present_denoised_impl(rz_ctx* c, const rz_present_params* pp, const rz_denoise_params* dp, uint8_t* rgba8,
                                 size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    const char* what = "rz_present_denoised";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!pp) return fail(c, RZ_ERR_INVALID_ARG, "%s: null present params", what);
    const rz_denoise_params& P = dp ? *dp : kDenoiseDefaults;
    int rc = denoise_check(c, what, P);
    if (rc != RZ_OK) return rc;
    const size_t np = (size_t)c->frame.width * c->frame.height;
    rc = present_sizes(c, what, np, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dDnOut, np * 16);
    if (rc != RZ_OK) return rc;
    float4* out4 = static_cast<float4*>(c->dDnOut.p);
    rc = denoise_run(c, P, static_cast<const float4*>(rz_accum_device_ptr(c)), nullptr, out4, nullptr);
    if (rc != RZ_OK) return rc;
    rc = present_impl(c, pp, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, out4);
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the guide may be wrong");
}

// rz_render_cost / rz_cost_view / rz_present_cost (rz_cost.hip).  rz_render_cost runs the one-lane-per-pixel path loop over the
// frame of rz_set_frame with buffers of its own: no accumulation, no currentIor, no claim scratch, no event of the ring, and
// nothing of lastPlan / lastKernel is touched.  The other two read the frame's size only.
static const rz_cost_params kCostDefaults = {0, {0, 0, 0, 0, 0, 0, 0}};
static const rz_cost_view_params kCostViewDefaults = {0, 0, 0.0f, {0, 0, 0, 0, 0}};

static int cost_frame_check(rz_ctx* c, const char* what) {
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "%s: rz_set_frame has not been called", what);
    if (c->frame.tile_nranks > 1)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: the frame is tile %d of %d; the cost map covers the whole frame", what, c->frame.tile_rank, c->frame.tile_nranks);
    return RZ_OK;
}

static int cost_view_check(rz_ctx* c, const char* what, const rz_cost_view_params& V) {
    if (V.metric < 0 || V.metric > 4) return fail(c, RZ_ERR_INVALID_ARG, "%s: metric %d outside 0..4", what, V.metric);
    if (V.curve != 0 && V.curve != 1) return fail(c, RZ_ERR_INVALID_ARG, "%s: curve %d (0 linear, 1 logarithmic)", what, V.curve);
    if (!(V.scale >= 0.0f && V.scale < INFINITY)) return fail(c, RZ_ERR_INVALID_ARG, "%s: scale %g (finite, >= 0)", what, (double)V.scale);
    for (int r : V.reserved) if (r) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    return cost_frame_check(c, what);
}

// the context's last cost buffer, if it was measured at the frame's size
static int cost_kept(rz_ctx* c, const char* what) {
    if (!c->costValid) return fail(c, RZ_ERR_NOT_READY, "%s: rz_render_cost has not been called", what);
    if (c->costW != c->frame.width || c->costH != c->frame.height)
        return fail(c, RZ_ERR_NOT_READY, "%s: the cost buffer was measured at %dx%d, the frame is %dx%d", what, c->costW, c->costH, c->frame.width, c->frame.height);
    return RZ_OK;
}

static int render_cost_impl(rz_ctx* c, const rz_cost_params* pp, rz_pixel_cost* cost, size_t cost_bytes, rz_counters* totals, unsigned flags) {
    const char* what = "rz_render_cost";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~RZ_COST_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const rz_cost_params& P = pp ? *pp : kCostDefaults;
    if (P.spp < 0 || P.spp > 1024) return fail(c, RZ_ERR_INVALID_ARG, "%s: spp %d outside 0..1024", what, P.spp);
    for (int r : P.reserved) if (r) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    int rc = cost_frame_check(c, what);
    if (rc == RZ_OK) rc = scene_ready(c, what, true);
    if (rc != RZ_OK) return rc;
    const bool host = (flags & RZ_COST_HOST) != 0;
    if (!host && (reinterpret_cast<uintptr_t>(cost) & 15u)) return fail(c, RZ_ERR_INVALID_ARG, "%s: a device cost pointer must be 16-byte aligned", what);
    const rz_frame_params& f = c->frame;
    const size_t np = (size_t)f.width * f.height, bCost = np * sizeof(rz_pixel_cost);
    if (cost && cost_bytes < bCost) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: cost needs %zu bytes, got %zu", what, bCost, cost_bytes);
    rc = finalize(c);
    if (rc == RZ_OK) rc = ensure_group_counter(c);          // (only its backstop word)
    if (rc == RZ_OK) rc = ensure(c, c->dCost, bCost);
    if (rc == RZ_OK) rc = ensure(c, c->dCostCounters, sizeof(DevCounters));
    if (rc != RZ_OK) return rc;
    KParams K{};
    const int spp = P.spp > 0 ? P.spp : f.spp;
    rc = frame_kparams(c, K, spp, 0);
    if (rc != RZ_OK) return rc;
    K.counters = static_cast<DevCounters*>(c->dCostCounters.p);
    CostLaunch C{static_cast<uint4*>(c->dCost.p), backstop_word(c)};
    c->costValid = false;
    RZ_HIP(c, hipMemsetAsync(c->dCostCounters.p, 0, sizeof(DevCounters), c->stream));
    launch_cost_pixels(K, C, c->stream);
    RZ_HIP(c, hipGetLastError());
    c->costValid = true;
    c->costW = f.width; c->costH = f.height; c->costSpp = spp;
    if (cost) RZ_HIP(c, hipMemcpyAsync(cost, c->dCost.p, bCost, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    if (totals) {
        DevCounters h{};
        RZ_HIP(c, hipMemcpyAsync(&h, c->dCostCounters.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
        RZ_HIP(c, hipStreamSynchronize(c->stream));
        totals->samples = h.samples; totals->traversals = h.traversals; totals->tlas_nodes = h.tlas_nodes;
        totals->tlas_leaf_indices = h.tlas_leaf_indices; totals->instances = h.instances; totals->blas_nodes = h.blas_nodes;
        totals->triangles = h.triangles; totals->materials = h.materials; totals->light_fetches = h.light_fetches;
        totals->pixels = h.pixels;
        totals->scatters = h.scatters; totals->diffuse_scatters = h.diffuse_scatters; totals->hemi_draws = h.hemi_draws;
        totals->lit_lights = h.lit_lights; totals->triangles_past_u = h.triangles_past_u;
    }
    if (!host) return RZ_OK;
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return report_backstop(c, what, "the cost map may be short of what the cut walks would have touched");
}

// Reduces the metric over `cost` (device) and maps it: the rz_cost_stats land in dCostStats; rgb (3 floats per pixel) and out4
// ((colour, 1) per pixel) are device outputs, each optional.
static int cost_view_run(rz_ctx* c, const rz_cost_view_params& V, const uint4* cost, float* rgb, float4* out4) {
    const rz_frame_params& f = c->frame;
    CostReduceLaunch R{};
    R.cost = cost;
    R.n = (long long)f.width * f.height;
    R.width = f.width;
    R.metric = V.metric;
    R.scale = V.scale;
    R.blocks = cost_reduce_blocks(R.n);
    int rc = ensure(c, c->dCostPartials, (size_t)RZ_COST_REDUCE_BLOCKS * 3 * sizeof(unsigned long long));
    if (rc == RZ_OK) rc = ensure(c, c->dCostStats, sizeof(rz_cost_stats));
    if (rc != RZ_OK) return rc;
    R.partials = static_cast<unsigned long long*>(c->dCostPartials.p);
    R.stats = static_cast<rz_cost_stats*>(c->dCostStats.p);
    launch_cost_reduce(R, c->stream);
    RZ_HIP(c, hipGetLastError());
    if (!rgb && !out4) return RZ_OK;
    CostViewLaunch L{};
    L.cost = cost;
    L.stats = R.stats;
    L.width = f.width; L.height = f.height;
    L.metric = V.metric; L.curve = V.curve;
    L.dst = out4;
    L.rgb = rgb;
    launch_cost_view(L, c->stream);
    RZ_HIP(c, hipGetLastError());
    return RZ_OK;
}

static int cost_view_impl(rz_ctx* c, const rz_cost_view_params* pp, const rz_pixel_cost* cost, size_t cost_bytes, float* rgb32f,
                          size_t rgb32f_bytes, rz_cost_stats* stats, unsigned flags) {
    const char* what = "rz_cost_view";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~RZ_COST_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const rz_cost_view_params& V = pp ? *pp : kCostViewDefaults;
    int rc = cost_view_check(c, what, V);
    if (rc != RZ_OK) return rc;
    const bool host = (flags & RZ_COST_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(cost) & 15u) || (reinterpret_cast<uintptr_t>(stats) & 7u) || (reinterpret_cast<uintptr_t>(rgb32f) & 3u)))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte (cost), 8-byte (stats) or 4-byte (rgb32f) aligned", what);
    const size_t np = (size_t)c->frame.width * c->frame.height;
    const size_t bCost = np * sizeof(rz_pixel_cost), bRgb = np * 3 * sizeof(float);
    if (cost && cost_bytes < bCost) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: cost needs %zu bytes, got %zu", what, bCost, cost_bytes);
    if (!cost) {
        rc = cost_kept(c, what);
        if (rc != RZ_OK) return rc;
    }
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (!rgb32f && !stats) return RZ_OK;
    const uint4* in = cost ? reinterpret_cast<const uint4*>(cost) : static_cast<const uint4*>(c->dCost.p);
    HostStage stage(c, host);
    const int sRgb = stage.add(rgb32f, bRgb);
    rc = stage.input(reinterpret_cast<const uint4*>(cost), bCost, in);
    if (rc == RZ_OK) rc = stage.place();
    if (rc != RZ_OK) return rc;
    rc = cost_view_run(c, V, in, stage.dev<float>(sRgb), nullptr);
    if (rc != RZ_OK) return rc;
    if (stats) RZ_HIP(c, hipMemcpyAsync(stats, c->dCostStats.p, sizeof(rz_cost_stats), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    return host ? stage.fetch() : RZ_OK;
}

static int present_cost_impl(rz_ctx* c, const rz_present_params* pp, const rz_cost_view_params* vp, uint8_t* rgba8, size_t rgba8_bytes,
                             float* rgb32f, size_t rgb32f_bytes) {
    const char* what = "rz_present_cost";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!pp) return fail(c, RZ_ERR_INVALID_ARG, "%s: null present params", what);
    const rz_cost_view_params& V = vp ? *vp : kCostViewDefaults;
    int rc = cost_view_check(c, what, V);
    if (rc == RZ_OK) rc = cost_kept(c, what);
    if (rc != RZ_OK) return rc;
    const size_t np = (size_t)c->frame.width * c->frame.height;
    if (rgba8 && rgba8_bytes < np * 4) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba8 buffer needs %zu bytes", what, np * 4);
    if (rgb32f && rgb32f_bytes < np * 12) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f buffer needs %zu bytes", what, np * 12);
    rc = ensure(c, c->dCostOut, np * 16);
    if (rc != RZ_OK) return rc;
    float4* out4 = static_cast<float4*>(c->dCostOut.p);
    rc = cost_view_run(c, V, static_cast<const uint4*>(c->dCost.p), nullptr, out4);
    if (rc != RZ_OK) return rc;
    return present_impl(c, pp, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, out4);
}

// rz_coverage (rz_coverage.hip).  Like rz_render_editor it reads the device scene as finalize left it and, of the frame, only what
// the call is given (width, height, inv_view, inv_proj, cam_pos); it touches no render state and not the frame of rz_set_frame.
static int coverage_impl(rz_ctx* c, const rz_frame_params* f, const rz_coverage_params* pp, rz_instance_coverage* coverage,
                         size_t coverage_bytes, int32_t* ids, size_t ids_bytes, unsigned flags) {
    const char* what = "rz_coverage";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!f) return fail(c, RZ_ERR_INVALID_ARG, "%s: null frame", what);
    if (flags & ~RZ_COVERAGE_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (f->width <= 0 || f->height <= 0) return fail(c, RZ_ERR_INVALID_ARG, "%s: bad size %dx%d", what, f->width, f->height);
    const size_t np = (size_t)f->width * (size_t)f->height;
    if (np > (size_t)std::numeric_limits<int32_t>::max())
        return fail(c, RZ_ERR_INVALID_ARG, "%s: %zu pixels, at most %d per frame", what, np, std::numeric_limits<int32_t>::max());
    if (pp) {
        if (pp->x1 < pp->x0 || pp->y1 < pp->y0)
            return fail(c, RZ_ERR_INVALID_ARG, "%s: rectangle [%d, %d) x [%d, %d)", what, pp->x0, pp->x1, pp->y0, pp->y1);
        for (int r : pp->reserved) if (r) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    }
    if (!coverage && !ids) return fail(c, RZ_ERR_INVALID_ARG, "%s: neither coverage nor ids given", what);
    const bool host = (flags & RZ_COVERAGE_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(coverage) & 15u) || (reinterpret_cast<uintptr_t>(ids) & 3u)))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte (coverage) or 4-byte (ids) aligned", what);
    int rc = scene_ready(c, what, false);
    if (rc != RZ_OK) return rc;
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    const size_t bCov = (nInst + 1) * sizeof(rz_instance_coverage), bIds = np * sizeof(int32_t);
    if (coverage && coverage_bytes < bCov)
        return fail(c, RZ_ERR_BUFFER_SIZE, "%s: coverage needs %zu bytes (%zu instances and the misses), got %zu", what, bCov, nInst, coverage_bytes);
    if (ids && ids_bytes < bIds) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: ids needs %zu bytes, got %zu", what, bIds, ids_bytes);
    CoverageLaunch V{};
    V.x0 = pp ? std::max(pp->x0, 0) : 0;
    V.y0 = pp ? std::max(pp->y0, 0) : 0;
    V.x1 = pp ? std::min(pp->x1, f->width) : f->width;
    V.y1 = pp ? std::min(pp->y1, f->height) : f->height;
    const bool empty = V.x0 >= V.x1 || V.y0 >= V.y1;
    if (empty && !coverage) return RZ_OK;               // no pixel to write an id for
    // host outputs are staged through dRayOut: coverage, then the id image (of which only the rectangle travels back)
    HostStage stage(c, host);
    const int sCov = stage.add(coverage, bCov), sIds = stage.add(empty ? nullptr : ids, bIds);
    rc = stage.place();
    if (rc != RZ_OK) return rc;
    unsigned* out = stage.dev<unsigned>(sCov);
    V.ids = stage.dev<int32_t>(sIds);
    if (!empty) {
        rc = finalize(c);
        if (rc == RZ_OK) rc = ensure_group_counter(c);      // (only its backstop word)
        if (rc != RZ_OK) return rc;
    }
    KParams K{};
    if (!empty) {
        camera_kparams(c, K, f->width, f->height, f->inv_view, f->inv_proj, f->cam_pos);
        V.unitsX = (V.x1 - V.x0 + 63) / 64;
        V.units = (long long)V.unitsX * (V.y1 - V.y0);
        V.grid = rays_grid(V.units * 64);
        if (const char* e = std::getenv("RZ_COVERAGE_GRID")) V.grid = std::max<long long>(1, std::min<long long>(V.grid, std::atoi(e)));   // test aid: several runs per wave on a small frame; same bytes
        V.nInst = (int)nInst;
        V.errWord = backstop_word(c);
        V.tableCap = 64;
        if (const char* e = std::getenv("RZ_COVERAGE_TABLE")) V.tableCap = std::max(1, std::min(64, std::atoi(e)));    // test aid: same bytes
        rc = size_blas_stack(c, K, 0, RZ_RAYS_WAVES_PER_CU, V.grid, c->dRayOvf);
        if (rc != RZ_OK) return rc;
    }
    if (out) {
        // the private sets: one per workgroup up to RZ_COVERAGE_SETS, 256 bytes apart at least, RZ_COVERAGE_SCRATCH at most
        const size_t stride = (bCov + 255) & ~size_t(255);
        const long long fit = std::max<long long>(1, (long long)(RZ_COVERAGE_SCRATCH / stride));
        long long sets = empty ? 1 : std::min<long long>({V.grid, RZ_COVERAGE_SETS, fit});
        if (const char* e = std::getenv("RZ_COVERAGE_SETS"))                    // A/B aid, same bytes: within the grid and the scratch too
            sets = empty ? 1 : std::max<long long>(1, std::min<long long>({V.grid, fit, std::atoi(e)}));
        const bool clean = c->dCovSets.p && c->covSets == sets && c->covStride == stride && c->covCount == nInst + 1;
        rc = ensure(c, c->dCovSets, (size_t)sets * stride);
        if (rc != RZ_OK) return rc;
        V.records = static_cast<unsigned*>(c->dCovSets.p);
        V.copies = (int)sets;
        V.strideWords = (int)(stride / 4);
        c->covSets = 0;                     // (until the merge below is queued)
        if (!clean) {
            launch_coverage_init(V.records, V.copies, V.strideWords, (int)nInst + 1, c->stream);
            RZ_HIP(c, hipGetLastError());
        }
    }
    if (!empty) {
        launch_coverage(K, V, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    if (out) {
        launch_coverage_merge(V.records, V.copies, V.strideWords, out, (int)nInst + 1, c->stream);
        RZ_HIP(c, hipGetLastError());
        c->covSets = V.copies; c->covStride = (size_t)V.strideWords * 4; c->covCount = nInst + 1;
    }
    if (!host) return RZ_OK;
    if (coverage) RZ_HIP(c, hipMemcpyAsync(coverage, out, bCov, hipMemcpyDeviceToHost, c->stream));
    if (V.ids) {
        const size_t pitch = (size_t)f->width * sizeof(int32_t), first = (size_t)V.y0 * f->width + V.x0;
        RZ_HIP(c, hipMemcpy2DAsync(ids + first, pitch, V.ids + first, pitch, (size_t)(V.x1 - V.x0) * sizeof(int32_t), (size_t)(V.y1 - V.y0),
                                   hipMemcpyDeviceToHost, c->stream));
    }
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return empty ? RZ_OK : report_backstop(c, what, "records and ids may be wrong");
}

// rz_ambient_occlusion (rz_ao.hip).  Like rz_coverage it reads the device scene as finalize left it and, of the frame, only what
// the call is given (width, height, inv_view, inv_proj, cam_pos); it touches no render state and not the frame of rz_set_frame.
static const rz_ao_params kAoDefaults = {4, 1.0f, 1, 1.0f, 0.9f, 2.0f, {0, 0}};

static int ao_impl(rz_ctx* c, const rz_frame_params* f, const rz_ao_params* pp, const float* rgb_in, size_t rgb_in_bytes, float* ao,
                   size_t ao_bytes, float* rgb32f, size_t rgb32f_bytes, uint8_t* rgba8, size_t rgba8_bytes, unsigned flags) {
    const char* what = "rz_ambient_occlusion";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!f) return fail(c, RZ_ERR_INVALID_ARG, "%s: null frame", what);
    if (flags & ~RZ_AO_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (f->width <= 0 || f->height <= 0) return fail(c, RZ_ERR_INVALID_ARG, "%s: bad size %dx%d", what, f->width, f->height);
    const size_t np = (size_t)f->width * (size_t)f->height;
    if (np > (size_t)std::numeric_limits<int32_t>::max())
        return fail(c, RZ_ERR_INVALID_ARG, "%s: %zu pixels, at most %d per frame", what, np, std::numeric_limits<int32_t>::max());
    const rz_ao_params& P = pp ? *pp : kAoDefaults;
    int log2n = 0;
    while ((1 << log2n) < P.samples && log2n < 4) ++log2n;
    if (P.samples != (1 << log2n)) return fail(c, RZ_ERR_INVALID_ARG, "%s: samples %d (1, 2, 4, 8 or 16)", what, P.samples);
    if (!(P.radius > 0.0f && P.radius < INFINITY)) return fail(c, RZ_ERR_INVALID_ARG, "%s: radius %g (finite, > 0)", what, (double)P.radius);
    if (P.smooth != 0 && P.smooth != 1) return fail(c, RZ_ERR_INVALID_ARG, "%s: smooth %d (0 or 1)", what, P.smooth);
    if (!(P.strength >= 0.0f && P.strength <= 1.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: strength %g outside [0, 1]", what, (double)P.strength);
    if (!(P.normal_cos >= -1.0f && P.normal_cos <= 1.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: normal_cos %g outside [-1, 1]", what, (double)P.normal_cos);
    if (!(P.plane_tol > 0.0f && P.plane_tol < INFINITY)) return fail(c, RZ_ERR_INVALID_ARG, "%s: plane_tol %g (finite, > 0)", what, (double)P.plane_tol);
    if (P.reserved[0] || P.reserved[1]) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    if (!ao && !rgb32f && !rgba8) return fail(c, RZ_ERR_INVALID_ARG, "%s: none of ao, rgb32f and rgba8 given", what);
    const bool host = (flags & RZ_AO_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(rgb_in) | reinterpret_cast<uintptr_t>(ao) | reinterpret_cast<uintptr_t>(rgb32f) |
                   reinterpret_cast<uintptr_t>(rgba8)) & 3u))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 4-byte aligned", what);
    int rc = scene_ready(c, what, true);
    if (rc != RZ_OK) return rc;
    const size_t bAo = np * sizeof(float), bRgb = np * 3 * sizeof(float), bRgba = np * 4;
    if (rgb_in && rgb_in_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb_in needs %zu bytes, got %zu", what, bRgb, rgb_in_bytes);
    if (ao && ao_bytes < bAo) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: ao needs %zu bytes, got %zu", what, bAo, ao_bytes);
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (rgba8 && rgba8_bytes < bRgba) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba8 needs %zu bytes, got %zu", what, bRgba, rgba8_bytes);
    // host buffers are staged as rz_denoise stages them: the input in dRayIn; ao, then rgb32f, then rgba8 in dRayOut
    HostStage stage(c, host);
    const int sAo = stage.add(ao, bAo), sRgb = stage.add(rgb32f, bRgb), sRgba = stage.add(rgba8, bRgba);
    const float* in = rgb_in;
    rc = stage.input(rgb_in, bRgb, in);
    if (rc == RZ_OK) rc = stage.place();
    if (rc == RZ_OK) rc = finalize(c);
    if (rc == RZ_OK) rc = cast_ready(c);
    if (rc == RZ_OK) rc = ensure(c, c->dDnGuide, np * 32);
    if (rc == RZ_OK) rc = ensure(c, c->dAoClaim, (size_t)RZ_AO_COUNTERS * 128);
    if (rc != RZ_OK) return rc;
    float* aoDev = stage.dev<float>(sAo);
    const bool smooth = P.smooth != 0;
    // without smoothing ao_p is raw_p: the walks write the caller's image, and nothing is left to resolve unless a colour is asked
    float* raw = (!smooth && aoDev) ? aoDev : nullptr;
    if (!raw) {
        rc = ensure(c, c->dAoRaw, bAo);
        if (rc != RZ_OK) return rc;
        raw = static_cast<float*>(c->dAoRaw.p);
    }
    if (!c->dAoDirs.p) {
        rc = upload_vec(c, c->dAoDirs, ao_direction_table(), RZ_AO_DIRS * 3 * sizeof(float));       // (static storage: it outlives the copy)
        if (rc != RZ_OK) return rc;
    }
    // the guide cast: rz_denoise's kernel through this call's camera, a wave per 64-pixel run of a row
    KParams KG{};
    camera_kparams(c, KG, f->width, f->height, f->inv_view, f->inv_proj, f->cam_pos);
    DenoiseGuideLaunch G{};
    G.unitsX = (f->width + 63) / 64;
    G.units = (long long)G.unitsX * f->height;
    G.grid = rays_grid(G.units * 64);
    G.instTriOff = static_cast<const int32_t*>(c->dRayInstOff.p);
    G.errWord = backstop_word(c);
    G.guide = static_cast<float4*>(c->dDnGuide.p);
    // the walks: a wave per 8 x 8 tile, its records beside the BLAS stack
    KParams KW = KG;
    AoWalkLaunch A{};
    A.guide = G.guide;
    A.dirs = static_cast<const float*>(c->dAoDirs.p);
    A.raw = raw;
    A.samples = P.samples; A.log2Samples = log2n;
    A.radius = P.radius;
    A.tilesX = (f->width + 7) / 8;
    A.tiles = (long long)A.tilesX * ((f->height + 7) / 8);
    A.grid = rays_grid(A.tiles * 64);
    A.claim = static_cast<unsigned*>(c->dAoClaim.p);
    // 64 sequences of trips, a counter each: measured against a sequence per wave, one counter, 16 and 256, and whole tiles as
    // units (profiles/ao/README.md)
    A.counters = 64;
    A.perTrip = 1;
    if (const char* e = std::getenv("RZ_AO_COUNTERS")) A.counters = std::max(0, std::min(RZ_AO_COUNTERS, std::atoi(e)));    // A/B aids, same bytes
    if (const char* e = std::getenv("RZ_AO_PER_TRIP")) A.perTrip = std::atoi(e) != 0;
    A.counters = (int)std::min<long long>(A.counters, A.grid);         // (a sequence no wave serves would never be walked)
    A.errWord = G.errWord;
    // (one overflow buffer serves both launches: sized for the larger need before either is queued)
    rc = size_blas_stack(c, KW, RZ_AO_WALK_LDS, RZ_RAYS_WAVES_PER_CU, A.grid, c->dRayOvf);
    if (rc == RZ_OK && KW.blasOvfCap > 0)
        rc = ensure(c, c->dRayOvf, (size_t)std::max(G.grid, A.grid) * KW.blasOvfCap * 64 * sizeof(uint2));
    if (rc == RZ_OK) rc = size_blas_stack(c, KG, 0, RZ_RAYS_WAVES_PER_CU, G.grid, c->dRayOvf);
    if (rc != RZ_OK) return rc;
    if (KW.blasOvfCap > 0) KW.blasOvf = static_cast<uint2*>(c->dRayOvf.p);
    launch_denoise_guides(KG, G, c->stream);
    RZ_HIP(c, hipGetLastError());
    if (A.counters > 0) RZ_HIP(c, hipMemsetAsync(A.claim, 0, (size_t)A.counters * 128, c->stream));
    launch_ao_walks(KW, A, c->stream);
    RZ_HIP(c, hipGetLastError());
    AoResolveLaunch R{};
    R.raw = raw;
    R.guide = G.guide;
    R.rgbIn = in;
    R.width = f->width; R.height = f->height;
    R.strength = P.strength; R.normalCos = P.normal_cos; R.planeTol = P.plane_tol;
    R.f = (float)(2.0 * std::fabs((double)f->inv_proj[5]) / (double)f->height);
    R.ao = raw == aoDev ? nullptr : aoDev;
    R.rgb = stage.dev<float>(sRgb);
    R.rgba8 = stage.dev<uchar4>(sRgba);
    if (R.ao || R.rgb || R.rgba8) {
        launch_ao_resolve(R, smooth, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    if (!host) return RZ_OK;
    rc = stage.fetch();
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the occlusion may be wrong");
}

// rz_outline (rz_outline.hip): no scene, no frame; the images are blended in place.
static int outline_impl(rz_ctx* c, const rz_outline_params* P, const int32_t* ids, size_t ids_bytes, const uint32_t* selected,
                        size_t n_instances, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes, unsigned flags) {
    const char* what = "rz_outline";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!P) return fail(c, RZ_ERR_INVALID_ARG, "%s: null params", what);
    if (flags & ~RZ_OUTLINE_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (P->width <= 0 || P->height <= 0) return fail(c, RZ_ERR_INVALID_ARG, "%s: bad size %dx%d", what, P->width, P->height);
    const size_t np = (size_t)P->width * (size_t)P->height;
    if (np > (size_t)std::numeric_limits<int32_t>::max())
        return fail(c, RZ_ERR_INVALID_ARG, "%s: %zu pixels, at most %d per image", what, np, std::numeric_limits<int32_t>::max());
    if (P->radius < 1 || P->radius > RZ_OUTLINE_MAX_RADIUS)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: radius %d outside 1..%d", what, P->radius, RZ_OUTLINE_MAX_RADIUS);
    for (float v : P->color)
        if (!(std::fabs(v) < INFINITY)) return fail(c, RZ_ERR_INVALID_ARG, "%s: color (%g, %g, %g) is not finite", what, (double)P->color[0], (double)P->color[1], (double)P->color[2]);
    if (!(P->alpha >= 0.0f && P->alpha <= 1.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: alpha %g outside [0, 1]", what, (double)P->alpha);
    if (P->reserved) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    // an id is an int32: no word past the one that holds bit 2^31 - 1 can be asked for
    const size_t nSel = std::min<size_t>(n_instances, (size_t)1 << 31), bSel = (nSel + 31) / 32 * sizeof(uint32_t);
    if (!ids) return fail(c, RZ_ERR_INVALID_ARG, "%s: null ids", what);
    if (!selected && nSel) return fail(c, RZ_ERR_INVALID_ARG, "%s: null selected", what);
    if (!rgba8 && !rgb32f) return fail(c, RZ_ERR_INVALID_ARG, "%s: neither rgba8 nor rgb32f given", what);
    const bool host = (flags & RZ_OUTLINE_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(selected) | reinterpret_cast<uintptr_t>(rgba8) |
                   reinterpret_cast<uintptr_t>(rgb32f)) & 3u))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 4-byte aligned", what);
    const size_t bIds = np * sizeof(int32_t), bRgba = np * 4, bRgb = np * 3 * sizeof(float);
    if (ids_bytes < bIds) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: ids needs %zu bytes, got %zu", what, bIds, ids_bytes);
    if (rgba8 && rgba8_bytes < bRgba) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba8 needs %zu bytes, got %zu", what, bRgba, rgba8_bytes);
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    OutlineLaunch O{};
    O.ids = ids;
    O.selected = selected;
    O.nInstances = nSel;
    O.width = P->width; O.height = P->height; O.radius = P->radius;
    std::memcpy(O.color, P->color, sizeof O.color);
    O.alpha = P->alpha;
    // host buffers: the ids, then the bit set in dRayIn; the images in dRayOut, copied in, blended there and copied back
    HostStage stage(c, host);
    const int sRgba = stage.add(rgba8, bRgba), sRgb = stage.add(rgb32f, bRgb);
    int rc = stage.place();
    if (rc != RZ_OK) return rc;
    O.rgba8 = stage.dev<uchar4>(sRgba);
    O.rgb = stage.dev<float>(sRgb);
    if (host) {
        const size_t offSel = (bIds + 15) & ~size_t(15);
        rc = ensure(c, c->dRayIn, offSel + bSel);
        if (rc != RZ_OK) return rc;
        char* in = static_cast<char*>(c->dRayIn.p);
        RZ_HIP(c, hipMemcpyAsync(in, ids, bIds, hipMemcpyHostToDevice, c->stream));
        if (bSel) RZ_HIP(c, hipMemcpyAsync(in + offSel, selected, bSel, hipMemcpyHostToDevice, c->stream));
        if (rgba8) RZ_HIP(c, hipMemcpyAsync(O.rgba8, rgba8, bRgba, hipMemcpyHostToDevice, c->stream));
        if (rgb32f) RZ_HIP(c, hipMemcpyAsync(O.rgb, rgb32f, bRgb, hipMemcpyHostToDevice, c->stream));
        O.ids = reinterpret_cast<const int32_t*>(in);
        O.selected = reinterpret_cast<const uint32_t*>(in + offSel);
    }
    launch_outline(O, c->stream);
    RZ_HIP(c, hipGetLastError());
    return host ? stage.fetch() : RZ_OK;
}

// rz_draw_lines (rz_lines.hip): no frame of rz_set_frame, and a scene only for the lines that name an instance; the images are
// blended in place.  Everything that can fail without the counts is done before the first launch; in the one case where the
// lists' size has to be waited for, the kernels queued by then have written the context's workspace only.
static const rz_lines_params kLinesDefaults = {1.5f, 0.01f, 0x1p-8f, 0.0f, 0, {0, 0, 0}};

static int lines_impl(rz_ctx* c, const rz_frame_params* f, const rz_lines_params* pp, const rz_line* lines, size_t n, const rz_hit* hits,
                      size_t hits_bytes, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes, unsigned flags) {
    const char* what = "rz_draw_lines";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!f) return fail(c, RZ_ERR_INVALID_ARG, "%s: null frame", what);
    if (flags & ~RZ_LINES_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (f->width <= 0 || f->height <= 0 || f->width > (1 << 23) || f->height > (1 << 23))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: bad size %dx%d", what, f->width, f->height);
    const size_t np = (size_t)f->width * (size_t)f->height;
    if (np > (size_t)std::numeric_limits<int32_t>::max())
        return fail(c, RZ_ERR_INVALID_ARG, "%s: %zu pixels, at most %d per frame", what, np, std::numeric_limits<int32_t>::max());
    const rz_lines_params& P = pp ? *pp : kLinesDefaults;
    if (!(P.width >= 1.0f && P.width <= 16.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: width %g outside [1, 16]", what, (double)P.width);
    if (!(P.near_w > 0.0f && P.near_w < INFINITY)) return fail(c, RZ_ERR_INVALID_ARG, "%s: near_w %g (finite, > 0)", what, (double)P.near_w);
    if (!(P.depth_bias >= 0.0f && P.depth_bias < 1.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: depth_bias %g outside [0, 1)", what, (double)P.depth_bias);
    if (!(P.hidden_alpha >= 0.0f && P.hidden_alpha <= 1.0f))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: hidden_alpha %g outside [0, 1]", what, (double)P.hidden_alpha);
    if (P.smooth != 0 && P.smooth != 1) return fail(c, RZ_ERR_INVALID_ARG, "%s: smooth %d (0 or 1)", what, P.smooth);
    if (P.reserved[0] || P.reserved[1] || P.reserved[2]) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    if (!lines && n) return fail(c, RZ_ERR_INVALID_ARG, "%s: null lines", what);
    if (n > RZ_LINES_MAX) return fail(c, RZ_ERR_INVALID_ARG, "%s: %zu lines, at most %zu per call", what, n, RZ_LINES_MAX);
    if (!rgba8 && !rgb32f) return fail(c, RZ_ERR_INVALID_ARG, "%s: neither rgba8 nor rgb32f given", what);
    const bool host = (flags & RZ_LINES_HOST) != 0;
    if (!host && (((reinterpret_cast<uintptr_t>(lines) | reinterpret_cast<uintptr_t>(hits)) & 15u) ||
                  ((reinterpret_cast<uintptr_t>(rgba8) | reinterpret_cast<uintptr_t>(rgb32f)) & 3u)))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte (lines, hits) or 4-byte (rgba8, rgb32f) aligned", what);
    const size_t bLines = n * sizeof(rz_line), bHits = np * sizeof(rz_hit), bRgba = np * 4, bRgb = np * 3 * sizeof(float);
    if (hits && hits_bytes < bHits) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: hits needs %zu bytes, got %zu", what, bHits, hits_bytes);
    if (rgba8 && rgba8_bytes < bRgba) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba8 needs %zu bytes, got %zu", what, bRgba, rgba8_bytes);
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    // the instances a line may name: those of a complete scene.  Host lines are checked here; device lines in the kernel
    bool scene = true;
    for (int b : {RZ_BIND_TRIANGLES, RZ_BIND_MATERIALS, RZ_BIND_LIGHTS, RZ_BIND_TLAS_NODES, RZ_BIND_TLAS_INDICES, RZ_BIND_BLAS_NODES,
                  RZ_BIND_BLAS_INDICES, RZ_BIND_INSTANCES})
        scene = scene && c->present[b];
    size_t nInst = scene ? hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES) : 0;
    bool named = !host;
    if (host)
        for (size_t i = 0; i < n; ++i) {
            if (lines[i].instance < 0) continue;
            if (!scene) return fail(c, RZ_ERR_NOT_READY, "%s: line %zu names instance %d and no scene has been uploaded", what, i, lines[i].instance);
            if ((size_t)lines[i].instance >= nInst)
                return fail(c, RZ_ERR_INVALID_ARG, "%s: line %zu names instance %d of %zu", what, i, lines[i].instance, nInst);
            named = true;
        }
    if (n == 0) return RZ_OK;
    int rc = RZ_OK;
    if (scene && named) rc = finalize(c);           // the transforms as the last upload / rz_update_transforms left them
    else nInst = 0;
    if (rc != RZ_OK) return rc;
    LinesLaunch V{};
    V.n = (int)n;
    V.instances = static_cast<const DevInstance*>(c->dInst.p);
    V.nInst = (int)std::min<size_t>(nInst, (size_t)std::numeric_limits<int32_t>::max());
    // proj * view as rz_present sums it
    const float* A = f->proj; const float* B = f->view;
    for (int col = 0; col < 4; ++col)
        for (int row = 0; row < 4; ++row)
            V.viewProj[col * 4 + row] = ((A[0 * 4 + row] * B[col * 4 + 0] + A[1 * 4 + row] * B[col * 4 + 1]) +
                                         A[2 * 4 + row] * B[col * 4 + 2]) + A[3 * 4 + row] * B[col * 4 + 3];
    V.width = f->width; V.height = f->height;
    V.halfWidth = P.width * 0.5f;
    V.nearW = P.near_w;
    V.depthKeep = 1.0f - P.depth_bias;
    V.hiddenAlpha = P.hidden_alpha;
    V.smooth = P.smooth;
    V.cellsX = (f->width + RZ_LINES_CELL - 1) / RZ_LINES_CELL;
    V.cells = V.cellsX * ((f->height + RZ_LINES_CELL - 1) / RZ_LINES_CELL);
    V.nSeg = (int)((n + RZ_LINES_SEG - 1) / RZ_LINES_SEG);
    const size_t slots = (size_t)V.cells * V.nSeg, offOffsets = (slots * sizeof(unsigned) + 15) & ~size_t(15);
    // the workspace: records, counts and offsets; and the lists at once if they fit whatever the counts will be -- the context
    // holds that much already, or it is little (RZ_LINES_DIRECT_BYTES; the variable: a test aid, same bytes)
    const char* unbinnedEnv = std::getenv("RZ_LINES_UNBINNED");     // A/B aid (profiles/lines/): no lists, same bytes
    const bool binned = !(unbinnedEnv && std::atoi(unbinnedEnv) != 0);
    size_t direct = RZ_LINES_DIRECT_BYTES;
    if (const char* e = std::getenv("RZ_LINES_DIRECT_BYTES")) direct = (size_t)std::max<long long>(0, std::atoll(e));
    const size_t worst = n * (size_t)V.cells * sizeof(int32_t);
    const bool wait = binned && worst > direct && !(c->dLnList.p && worst <= c->dLnList.cap);
    alloc_point(c);
    rc = ensure(c, c->dLnRec, n * 52);
    if (rc != RZ_OK) return rc;
    alloc_point(c);
    rc = ensure(c, c->dLnCells, offOffsets + (slots + 1) * sizeof(unsigned long long));
    if (rc != RZ_OK) return rc;
    if (binned && !wait) {
        alloc_point(c);
        if (ensure(c, c->dLnList, worst) != RZ_OK) {
            (void)hipGetLastError();
            return fail(c, RZ_ERR_NO_MEMORY, "%s: no device memory for the lists (%zu bytes)", what, worst);
        }
    }
    char* rec = static_cast<char*>(c->dLnRec.p);
    V.geo = reinterpret_cast<float4*>(rec);
    V.misc = reinterpret_cast<float4*>(rec + n * 16);
    V.rect = reinterpret_cast<float4*>(rec + n * 32);
    V.reach = reinterpret_cast<float*>(rec + n * 48);
    V.counts = static_cast<unsigned*>(c->dLnCells.p);
    V.offsets = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->dLnCells.p) + offOffsets);
    // host buffers: the lines, then the hits in dRayIn; the images in dRayOut, copied in, blended there and copied back
    HostStage stage(c, host);
    const int sRgba = stage.add(rgba8, bRgba), sRgb = stage.add(rgb32f, bRgb);
    rc = stage.place();
    if (rc != RZ_OK) return rc;
    V.rgba8 = stage.dev<uchar4>(sRgba);
    V.rgb = stage.dev<float>(sRgb);
    V.lines = lines;
    V.hits = reinterpret_cast<const float4*>(hits);
    if (host) {
        const size_t offHits = (bLines + 15) & ~size_t(15);
        rc = ensure(c, c->dRayIn, offHits + (hits ? bHits : 0));
        if (rc != RZ_OK) return rc;
        char* in = static_cast<char*>(c->dRayIn.p);
        RZ_HIP(c, hipMemcpyAsync(in, lines, bLines, hipMemcpyHostToDevice, c->stream));
        if (hits) RZ_HIP(c, hipMemcpyAsync(in + offHits, hits, bHits, hipMemcpyHostToDevice, c->stream));
        if (rgba8) RZ_HIP(c, hipMemcpyAsync(V.rgba8, rgba8, bRgba, hipMemcpyHostToDevice, c->stream));
        if (rgb32f) RZ_HIP(c, hipMemcpyAsync(V.rgb, rgb32f, bRgb, hipMemcpyHostToDevice, c->stream));
        V.lines = in;
        V.hits = hits ? reinterpret_cast<const float4*>(in + offHits) : nullptr;
    }
    launch_lines_project(V, c->stream);
    RZ_HIP(c, hipGetLastError());
    if (binned) {
        launch_lines_count(V, c->stream);
        RZ_HIP(c, hipGetLastError());
        if (wait) {
            unsigned long long total = 0;
            RZ_HIP(c, hipMemcpyAsync(&total, V.offsets + slots, sizeof total, hipMemcpyDeviceToHost, c->stream));
            RZ_HIP(c, hipStreamSynchronize(c->stream));
            alloc_point(c);
            if (ensure(c, c->dLnList, (size_t)total * sizeof(int32_t)) != RZ_OK) {
                (void)hipGetLastError();
                return fail(c, RZ_ERR_NO_MEMORY, "%s: no device memory for the lists (%llu entries)", what, total);
            }
        }
        V.list = static_cast<int*>(c->dLnList.p);
        launch_lines_fill(V, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    launch_lines_draw(V, c->stream);
    RZ_HIP(c, hipGetLastError());
    return host ? stage.fetch() : RZ_OK;
}

// rz_denoise_temporal / rz_present_temporal (rz_temporal.hip).  They read what rz_denoise reads and touch no render state; the
// history they keep is the context's own (rz_ctx: dTmp*).
static const rz_temporal_params kTemporalDefaults = {0.2f, 0.2f, 32, 0.9f, 2.0f, 5, 0.5f, 128.0f, 1.0f, 1, {0, 0, 0, 0, 0, 0}};

static int temporal_check(rz_ctx* c, const char* what, const rz_temporal_params& P) {
    if (!(P.alpha >= 0.0f && P.alpha <= 1.0f) || !(P.alpha_moments >= 0.0f && P.alpha_moments <= 1.0f))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: alpha %g, alpha_moments %g outside [0, 1]", what, (double)P.alpha, (double)P.alpha_moments);
    if (P.max_history < 1) return fail(c, RZ_ERR_INVALID_ARG, "%s: max_history %d < 1", what, P.max_history);
    if (!(P.normal_cos >= -1.0f && P.normal_cos <= 1.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: normal_cos %g outside [-1, 1]", what, (double)P.normal_cos);
    if (!(P.plane_tol > 0.0f && P.plane_tol < INFINITY) || !(P.sigma_l > 0.0f && P.sigma_l < INFINITY))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: plane_tol %g, sigma_l %g (finite, > 0)", what, (double)P.plane_tol, (double)P.sigma_l);
    for (int r : P.reserved)
        if (r) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    // the rest is rz_denoise's (sigma_color has no counterpart: any valid value)
    const rz_denoise_params D = {P.iterations, 1.0f, P.sigma_normal, P.sigma_plane, P.demodulate, {0, 0, 0}};
    return denoise_check(c, what, D);
}

// Casts the guide, accumulates, filters, and commits the history unless `keep`.  in: RGBA32F sum and count (device); outputs
// (device, each optional): rgb, out4 ((colour, 1)), hits (rz_hit), stats (N, variance).
static int temporal_run(rz_ctx* c, const rz_temporal_params& P, const float4* in, float* rgb, float4* out4, float4* hits,
                        float* stats, bool keep) {
    const rz_frame_params& f = c->frame;
    const size_t np = (size_t)f.width * f.height;
    int rc = finalize(c);
    if (rc != RZ_OK) return rc;
    const size_t nInst = hostCount<rz_bvh_instance>(c, RZ_BIND_INSTANCES);
    const bool havePrev = c->tmpValid && c->tmpW == f.width && c->tmpH == f.height && c->tmpInst == nInst;
    const int cur = c->tmpCur, nxt = cur ^ 1;
    rc = ensure(c, c->dTmpCol[nxt], np * 16);
    if (rc == RZ_OK) rc = ensure(c, c->dTmpMom[nxt], np * 8);
    if (rc == RZ_OK) rc = ensure(c, c->dTmpHits[nxt], np * sizeof(rz_hit));
    if (rc == RZ_OK) rc = ensure(c, c->dTmpInst[nxt], nInst * 96);
    if (rc == RZ_OK) rc = ensure(c, c->dTmpSame, nInst * sizeof(int));
    if (rc == RZ_OK) rc = ensure(c, c->dDnGuide, np * 32);
    const bool filter = (rgb || out4) && P.iterations > 0;
    if (rc == RZ_OK && filter) rc = ensure(c, c->dDnPong, np * 16);
    if (rc == RZ_OK && filter && P.iterations > 1) rc = ensure(c, c->dDnPing, np * 16);
    if (rc == RZ_OK) rc = cast_ready(c);
    if (rc != RZ_OK) return rc;
    // the guide: rz_denoise's kernel, its rz_hit records straight into the history being written
    float4* guide = static_cast<float4*>(c->dDnGuide.p);
    float4* hitsNext = static_cast<float4*>(c->dTmpHits[nxt].p);
    rc = guide_cast(c, f.width, f.height, guide, hitsNext);
    if (rc != RZ_OK) return rc;
    const DevInstance* instances = static_cast<const DevInstance*>(c->dInst.p);
    const DevMaterial* materials = static_cast<const DevMaterial*>(c->dMat.p);
    if (hits) RZ_HIP(c, hipMemcpyAsync(hits, hitsNext, np * sizeof(rz_hit), hipMemcpyDeviceToDevice, c->stream));
    launch_temporal_instances(instances, static_cast<const float*>(c->dTmpInst[cur].p), static_cast<float*>(c->dTmpInst[nxt].p),
                              static_cast<int*>(c->dTmpSame.p), (int)nInst, havePrev, c->stream);
    RZ_HIP(c, hipGetLastError());
    const double fpx = 2.0 * std::fabs((double)f.inv_proj[5]) / (double)f.height;
    TemporalLaunch T{};
    T.accum = in;
    T.hits = hitsNext;
    T.materials = materials;
    T.instances = instances;
    T.colPrev = static_cast<const float4*>(c->dTmpCol[cur].p);
    T.momPrev = static_cast<const float2*>(c->dTmpMom[cur].p);
    T.hitsPrev = static_cast<const float4*>(c->dTmpHits[cur].p);
    T.instPrev = static_cast<const float*>(c->dTmpInst[cur].p);
    T.instSame = static_cast<const int*>(c->dTmpSame.p);
    T.colNext = static_cast<float4*>(c->dTmpCol[nxt].p);
    T.momNext = static_cast<float2*>(c->dTmpMom[nxt].p);
    T.dst = P.iterations == 0 ? out4 : nullptr;
    T.rgb = P.iterations == 0 ? rgb : nullptr;
    T.width = f.width; T.height = f.height;
    T.nMaterials = (int)hostCount<rz_material>(c, RZ_BIND_MATERIALS);
    T.demodulate = P.demodulate;
    T.havePrev = havePrev ? 1 : 0;
    T.cameraSame = havePrev && std::memcmp(c->tmpView, f.view, 64) == 0 && std::memcmp(c->tmpProj, f.proj, 64) == 0;
    T.alpha = P.alpha; T.alphaMoments = P.alpha_moments; T.maxHistory = (float)P.max_history;
    T.normalCos = P.normal_cos; T.planeTol = P.plane_tol;
    T.fPrev = 2.0f * std::fabs(c->tmpInvProj[5]) / (float)f.height;
    std::memcpy(T.viewPrev, c->tmpView, 64);
    std::memcpy(T.projPrev, c->tmpProj, 64);
    std::memcpy(T.camPrev, c->tmpCam, 12);
    std::memcpy(T.invView, f.inv_view, 64);
    std::memcpy(T.invProj, f.inv_proj, 64);
    launch_temporal_accumulate(T, c->stream);
    RZ_HIP(c, hipGetLastError());
    if (filter || stats) {
        TemporalVarLaunch V{};
        V.col = T.colNext;
        V.mom = T.momNext;
        V.guide = guide;
        V.dst = filter ? static_cast<float4*>(c->dDnPong.p) : nullptr;
        V.stats = stats;
        V.width = f.width; V.height = f.height;
        V.sigmaNormal = P.sigma_normal;
        V.planeScale = (float)(1.0 / ((double)P.sigma_plane * fpx));
        launch_temporal_variance(V, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    if (filter) {
        TemporalFilterLaunch F{};
        F.guide = guide;
        F.materials = materials;
        F.width = f.width; F.height = f.height;
        F.sigmaL = P.sigma_l;
        F.sigmaNormal = P.sigma_normal;
        F.demodulate = P.demodulate;
        float4* ping = static_cast<float4*>(c->dDnPing.p);
        float4* pong = static_cast<float4*>(c->dDnPong.p);
        for (int i = 0; i < P.iterations; ++i) {
            const bool last = i == P.iterations - 1;
            F.step = 1 << i;
            F.planeScale = (float)(1.0 / ((double)P.sigma_plane * fpx * (double)(1 << i)));
            F.src = (i % 2 == 1) ? ping : pong;         // pass 0 reads what the variance kernel wrote
            F.dst = last ? out4 : ((i % 2 == 0) ? ping : pong);
            F.rgb = last ? rgb : nullptr;
            launch_temporal_pass(F, last, c->stream);
            RZ_HIP(c, hipGetLastError());
        }
    }
    if (!keep) {            // the set just written becomes the history
        c->tmpCur = nxt;
        c->tmpValid = true;
        c->tmpW = f.width; c->tmpH = f.height; c->tmpInst = nInst;
        std::memcpy(c->tmpView, f.view, 64);
        std::memcpy(c->tmpProj, f.proj, 64);
        std::memcpy(c->tmpInvProj, f.inv_proj, 64);
        std::memcpy(c->tmpCam, f.cam_pos, 12);
    }
    return RZ_OK;
}

static int temporal_impl(rz_ctx* c, const rz_temporal_params* pp, const float* rgba_in, size_t rgba_in_bytes, float* rgb32f,
                         size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, float* stats, size_t stats_bytes, unsigned flags) {
    const char* what = "rz_denoise_temporal";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~(RZ_TEMPORAL_HOST | RZ_TEMPORAL_KEEP)) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const rz_temporal_params& P = pp ? *pp : kTemporalDefaults;
    int rc = temporal_check(c, what, P);
    if (rc != RZ_OK) return rc;
    const bool host = (flags & RZ_TEMPORAL_HOST) != 0;
    if (!host && (((reinterpret_cast<uintptr_t>(rgba_in) | reinterpret_cast<uintptr_t>(guides)) & 15u) ||
                  ((reinterpret_cast<uintptr_t>(rgb32f) | reinterpret_cast<uintptr_t>(stats)) & 3u)))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte (rgba_in, guides) or 4-byte (rgb32f, stats) aligned", what);
    const size_t np = (size_t)c->frame.width * c->frame.height;
    const size_t bIn = np * 16, bRgb = np * 3 * sizeof(float), bHits = np * sizeof(rz_hit), bStats = np * 2 * sizeof(float);
    if (rgba_in && rgba_in_bytes < bIn) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba_in needs %zu bytes, got %zu", what, bIn, rgba_in_bytes);
    if (!rgba_in) {
        rc = accum_fits(c, what);
        if (rc != RZ_OK) return rc;
    }
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (guides && guides_bytes < bHits) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: guides needs %zu bytes, got %zu", what, bHits, guides_bytes);
    if (stats && stats_bytes < bStats) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: stats needs %zu bytes, got %zu", what, bStats, stats_bytes);
    const float4* in = rgba_in ? reinterpret_cast<const float4*>(rgba_in) : static_cast<const float4*>(rz_accum_device_ptr(c));
    // host buffers are staged as rz_denoise stages them: the input in dRayIn; hits, rgb32f, then stats in dRayOut
    HostStage stage(c, host);
    const int sHits = stage.add(guides, bHits), sRgb = stage.add(rgb32f, bRgb), sStats = stage.add(stats, bStats);
    rc = stage.input(reinterpret_cast<const float4*>(rgba_in), bIn, in);
    if (rc == RZ_OK) rc = stage.place();
    if (rc != RZ_OK) return rc;
    rc = temporal_run(c, P, in, stage.dev<float>(sRgb), nullptr, stage.dev<float4>(sHits), stage.dev<float>(sStats),
                      (flags & RZ_TEMPORAL_KEEP) != 0);
    if (rc != RZ_OK) return rc;
    if (!host) return RZ_OK;
    rc = stage.fetch();
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the guide may be wrong");
}

static int present_temporal_impl(rz_ctx* c, const rz_present_params* pp, const rz_temporal_params* tp, uint8_t* rgba8,
                                 size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    const char* what = "rz_present_temporal";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!pp) return fail(c, RZ_ERR_INVALID_ARG, "%s: null present params", what);
    const rz_temporal_params& P = tp ? *tp : kTemporalDefaults;
    int rc = temporal_check(c, what, P);
    if (rc != RZ_OK) return rc;
    const size_t np = (size_t)c->frame.width * c->frame.height;
    rc = present_sizes(c, what, np, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dDnOut, np * 16);
    if (rc != RZ_OK) return rc;
    float4* out4 = static_cast<float4*>(c->dDnOut.p);
    rc = temporal_run(c, P, static_cast<const float4*>(rz_accum_device_ptr(c)), nullptr, out4, nullptr, nullptr, false);
    if (rc != RZ_OK) return rc;
    rc = present_impl(c, pp, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, out4);
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the guide may be wrong");
}

// rz_display / rz_present_display (rz_display.hip).  Of the frame they read the size only; they need no scene (rz_present_display
// needs what its source and rz_present need) and touch no render state.  What they keep is one DisplayState on the device.
static const rz_display_params kDisplayDefaults = {0, 1.0f, 0.18f, 1.0f / 64.0f, 64.0f, 1.0f, 0, 0, 0, 4.0f, 0, {0, 0, 0, 0, 0}};

static int display_check(rz_ctx* c, const char* what, const rz_display_params& P) {
    auto positive = [](float v) { return v > 0.0f && v < INFINITY; };
    if (P.exposure_mode != 0 && P.exposure_mode != 1) return fail(c, RZ_ERR_INVALID_ARG, "%s: exposure_mode %d (0 manual, 1 auto)", what, P.exposure_mode);
    if (P.exposure_mode == 0 && !positive(P.exposure)) return fail(c, RZ_ERR_INVALID_ARG, "%s: exposure %g (finite, > 0)", what, (double)P.exposure);
    if (P.exposure_mode == 1) {
        if (!positive(P.key)) return fail(c, RZ_ERR_INVALID_ARG, "%s: key %g (finite, > 0)", what, (double)P.key);
        if (!positive(P.min_exposure) || !positive(P.max_exposure) || !(P.min_exposure <= P.max_exposure))
            return fail(c, RZ_ERR_INVALID_ARG, "%s: min_exposure %g, max_exposure %g (finite, 0 < min <= max)", what, (double)P.min_exposure, (double)P.max_exposure);
        if (!(P.adapt >= 0.0f && P.adapt <= 1.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: adapt %g outside [0, 1]", what, (double)P.adapt);
        if (P.low_permille < 0 || P.high_permille < 0 || (long long)P.low_permille + P.high_permille >= 1000)
            return fail(c, RZ_ERR_INVALID_ARG, "%s: low_permille %d, high_permille %d (>= 0, sum < 1000)", what, P.low_permille, P.high_permille);
    }
    if (P.curve < 0 || P.curve > 2) return fail(c, RZ_ERR_INVALID_ARG, "%s: curve %d (0 clamp, 1 Reinhard, 2 ACES)", what, P.curve);
    if (P.curve == 1 && !positive(P.white)) return fail(c, RZ_ERR_INVALID_ARG, "%s: white %g (finite, > 0)", what, (double)P.white);
    if (P.transfer != 0 && P.transfer != 1) return fail(c, RZ_ERR_INVALID_ARG, "%s: transfer %d (0 linear, 1 sRGB)", what, P.transfer);
    for (int r : P.reserved)
        if (r) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "%s: rz_set_frame has not been called", what);
    return RZ_OK;
}

static int ensure_display_state(rz_ctx* c) {
    if (c->dDisplay.p) return RZ_OK;
    int rc = ensure(c, c->dDisplay, sizeof(DisplayState));
    if (rc != RZ_OK) return rc;
    RZ_HIP(c, hipMemsetAsync(c->dDisplay.p, 0, sizeof(DisplayState), c->stream));     // fresh: no exposure yet, an empty histogram
    return RZ_OK;
}

// Meters and adapts (auto) or commits the manual exposure, then tones, on the stream.  The input (device) is rgb (3 floats per
// pixel) or in4 (RGBA32F sum and count); outputs (device, each optional): rgb, rgba8, out4 ((colour, 1); may be in4 itself).
// pixels: how many the buffers hold -- the frame's when 0; rz_present_upscaled passes the high size.
static int display_run(rz_ctx* c, const rz_display_params& P, const float* in, const float4* in4, float* rgb, uchar4* rgba8,
                       float4* out4, bool keep, long long pixels = 0) {
    const long long np = pixels > 0 ? pixels : (long long)c->frame.width * c->frame.height;
    const bool metered = P.exposure_mode == 1;
    DisplayState* S = nullptr;
    if (metered || !keep) {
        int rc = ensure_display_state(c);
        if (rc != RZ_OK) return rc;
        S = static_cast<DisplayState*>(c->dDisplay.p);
    }
    if (metered) {
        launch_display_meter(in, in4, np, S, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    if (S) {
        DisplayExpose X{};
        X.mode = metered ? 1 : 0;
        X.keep = keep ? 1 : 0;
        X.manual = P.exposure;
        X.key = P.key; X.minExposure = P.min_exposure; X.maxExposure = P.max_exposure; X.adapt = P.adapt;
        X.lowPermille = P.low_permille; X.highPermille = P.high_permille;
        launch_display_expose(S, X, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    if (!rgb && !rgba8 && !out4) return RZ_OK;
    DisplayTone T{};
    T.in = in; T.in4 = in4;
    T.state = metered ? S : nullptr;
    T.exposure = P.exposure;
    T.curve = P.curve;
    T.white2 = P.white * P.white;
    T.transfer = P.transfer;
    T.n = np;
    T.rgb = rgb; T.rgba8 = rgba8; T.out4 = out4;
    launch_display_tone(T, c->stream);
    RZ_HIP(c, hipGetLastError());
    return RZ_OK;
}

static int display_impl(rz_ctx* c, const rz_display_params* pp, const float* rgb_in, size_t rgb_in_bytes, float* rgb32f,
                        size_t rgb32f_bytes, uint8_t* rgba8, size_t rgba8_bytes, unsigned flags) {
    const char* what = "rz_display";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~(RZ_DISPLAY_HOST | RZ_DISPLAY_KEEP)) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const rz_display_params& P = pp ? *pp : kDisplayDefaults;
    int rc = display_check(c, what, P);
    if (rc != RZ_OK) return rc;
    if (!rgb_in && c->frame.tile_nranks > 1)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: the frame is tile %d of %d; the accumulation is not the whole frame", what, c->frame.tile_rank, c->frame.tile_nranks);
    const bool host = (flags & RZ_DISPLAY_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(rgb_in) | reinterpret_cast<uintptr_t>(rgb32f) | reinterpret_cast<uintptr_t>(rgba8)) & 3u))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 4-byte aligned", what);
    const size_t np = (size_t)c->frame.width * c->frame.height;
    const size_t bRgb = np * 3 * sizeof(float), bRgba8 = np * 4;
    if (rgb_in && rgb_in_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb_in needs %zu bytes, got %zu", what, bRgb, rgb_in_bytes);
    if (!rgb_in) {
        rc = accum_fits(c, what);
        if (rc != RZ_OK) return rc;
    }
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (rgba8 && rgba8_bytes < bRgba8) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgba8 needs %zu bytes, got %zu", what, bRgba8, rgba8_bytes);
    const float* in = rgb_in;
    const float4* in4 = rgb_in ? nullptr : static_cast<const float4*>(rz_accum_device_ptr(c));
    // host buffers are staged as rz_denoise stages them: the input in dRayIn; rgb32f, then rgba8 in dRayOut
    HostStage stage(c, host);
    const int sRgb = stage.add(rgb32f, bRgb), sRgba8 = stage.add(rgba8, bRgba8);
    rc = stage.input(rgb_in, bRgb, in);
    if (rc == RZ_OK) rc = stage.place();
    if (rc != RZ_OK) return rc;
    rc = display_run(c, P, in, in4, stage.dev<float>(sRgb), stage.dev<uchar4>(sRgba8), nullptr, (flags & RZ_DISPLAY_KEEP) != 0);
    if (rc != RZ_OK) return rc;
    if (!host) return RZ_OK;
    return stage.fetch();
}

// What rz_present_display and rz_present_upscaled tone: (source, filter_params) as given, the filter's defaults filled in.
struct FilterSource {
    int source = 0;         // 0 accumulation, 1 rz_denoise, 2 rz_denoise_temporal
    rz_denoise_params P1 = kDenoiseDefaults;
    rz_temporal_params P2 = kTemporalDefaults;
};

// The checks both calls open with, in the order their header documents: the source, the display parameters, the filter's own.
static int source_check(rz_ctx* c, const char* what, int source, const void* filter_params, const rz_display_params& D, FilterSource& F) {
    if (source < 0 || source > 2) return fail(c, RZ_ERR_INVALID_ARG, "%s: source %d (0 accumulation, 1 rz_denoise, 2 rz_denoise_temporal)", what, source);
    if (source == 0 && filter_params) return fail(c, RZ_ERR_INVALID_ARG, "%s: filter_params must be NULL for source 0", what);
    int rc = display_check(c, what, D);
    if (rc != RZ_OK) return rc;
    F.source = source;
    if (source == 1 && filter_params) F.P1 = *static_cast<const rz_denoise_params*>(filter_params);
    if (source == 2 && filter_params) F.P2 = *static_cast<const rz_temporal_params*>(filter_params);
    if (source == 1) rc = denoise_check(c, what, F.P1);
    if (source == 2) rc = temporal_check(c, what, F.P2);
    return rc;
}

// Sources 1 and 2 filter `accum` (at the frame's size) into out4 as (colour, 1); source 0 runs nothing.
static int source_run(rz_ctx* c, const FilterSource& F, const float4* accum, float4* out4) {
    if (F.source == 1) return denoise_run(c, F.P1, accum, nullptr, out4, nullptr);
    if (F.source == 2) return temporal_run(c, F.P2, accum, nullptr, out4, nullptr, nullptr, false);
    return RZ_OK;
}

static int present_display_impl(rz_ctx* c, const rz_present_params* pp, const rz_display_params* dp, int source,
                                const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    const char* what = "rz_present_display";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!pp) return fail(c, RZ_ERR_INVALID_ARG, "%s: null present params", what);
    const rz_display_params& D = dp ? *dp : kDisplayDefaults;
    FilterSource F;
    int rc = source_check(c, what, source, filter_params, D, F);
    if (rc != RZ_OK) return rc;
    if (source == 0 && D.exposure_mode == 1 && c->frame.tile_nranks > 1)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: the frame is tile %d of %d; metering needs the whole frame", what, c->frame.tile_rank, c->frame.tile_nranks);
    const size_t np = (size_t)c->frame.width * c->frame.height;
    rc = present_sizes(c, what, np, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dDnOut, np * 16);
    if (rc != RZ_OK) return rc;
    float4* out4 = static_cast<float4*>(c->dDnOut.p);
    const float4* accum = static_cast<const float4*>(rz_accum_device_ptr(c));
    // sources 1 and 2 leave (colour, 1) in out4, which the tone kernel then rewrites in place: (colour, 1) resolves to colour
    rc = source_run(c, F, accum, out4);
    if (rc != RZ_OK) return rc;
    rc = display_run(c, D, nullptr, source == 0 ? accum : out4, nullptr, nullptr, out4, false);
    if (rc != RZ_OK) return rc;
    rc = present_impl(c, pp, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, out4);
    if (rc != RZ_OK) return rc;
    return source == 0 ? RZ_OK : report_backstop(c, what, "the guide may be wrong");
}

// rz_bloom / rz_present_bloomed (rz_bloom.hip).  Of the frame they read the size only; rz_bloom needs no scene.  They touch no
// render, temporal or display state of their own; what they keep is the pyramid.
static const rz_bloom_params kBloomDefaults = {1.0f, 0.5f, 64.0f, 0.25f, 1.0f, 6, {0, 0}};

static int bloom_check(rz_ctx* c, const char* what, const rz_bloom_params& P) {
    auto finite0 = [](float v) { return v >= 0.0f && v < INFINITY; };
    if (!finite0(P.threshold)) return fail(c, RZ_ERR_INVALID_ARG, "%s: threshold %g (finite, >= 0)", what, (double)P.threshold);
    if (!finite0(P.knee)) return fail(c, RZ_ERR_INVALID_ARG, "%s: knee %g (finite, >= 0)", what, (double)P.knee);
    if (!(P.limit > 0.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: limit %g (> 0; +Inf: none)", what, (double)P.limit);
    if (!finite0(P.intensity)) return fail(c, RZ_ERR_INVALID_ARG, "%s: intensity %g (finite, >= 0)", what, (double)P.intensity);
    if (!(P.spread > 0.0f && P.spread <= 4.0f)) return fail(c, RZ_ERR_INVALID_ARG, "%s: spread %g outside (0, 4]", what, (double)P.spread);
    if (P.levels < 1 || P.levels > RZ_BLOOM_MAX_LEVELS) return fail(c, RZ_ERR_INVALID_ARG, "%s: levels %d outside 1..%d", what, P.levels, RZ_BLOOM_MAX_LEVELS);
    if (P.reserved[0] || P.reserved[1]) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "%s: rz_set_frame has not been called", what);
    if (((long long)c->frame.height + 3) / 4 > 65535) return fail(c, RZ_ERR_INVALID_ARG, "%s: a frame of %d rows is more than 262140", what, c->frame.height);
    return RZ_OK;
}

// step 1 of the definition: the sizes of the levels, and where each starts in the workspace (in texels)
struct BloomLevels {
    int n = 0;
    int w[RZ_BLOOM_MAX_LEVELS] = {}, h[RZ_BLOOM_MAX_LEVELS] = {};
    size_t off[RZ_BLOOM_MAX_LEVELS] = {}, texels = 0;
};

static BloomLevels bloom_levels(int W, int H, int levels) {
    BloomLevels L;
    int w = W, h = H;
    do {
        w = (w + 1) / 2; h = (h + 1) / 2;
        L.w[L.n] = w; L.h[L.n] = h; L.off[L.n] = L.texels;
        L.texels += (size_t)w * h;
        ++L.n;
    } while (L.n < levels && !(w == 1 && h == 1));
    return L;
}

// Whether a call with these parameters and outputs builds the pyramid at all (step 6: with intensity 0 only `glare` needs it).
static bool bloom_needs_pyramid(const rz_bloom_params& P, bool glare) { return glare || P.intensity != 0.0f; }

// The workspace of a call, before anything is queued: a failure here leaves nothing launched and nothing written.
static int bloom_workspace(rz_ctx* c, const char* what, const rz_bloom_params& P) {
    const BloomLevels L = bloom_levels(c->frame.width, c->frame.height, P.levels);
    alloc_point(c);
    if (ensure(c, c->dBloom, L.texels * sizeof(float4)) != RZ_OK) {
        (void)hipGetLastError();
        return fail(c, RZ_ERR_NO_MEMORY, "%s: no device memory for the pyramid (%zu bytes)", what, L.texels * sizeof(float4));
    }
    return RZ_OK;
}

// The pass on the stream, bloom_workspace done.  The input (device) is `in` (3 floats per pixel) or in4 (RGBA32F sum and count);
// outputs (device, each optional): rgb (may be `in`), glare, out4 ((out, 1); may be in4).
static int bloom_run(rz_ctx* c, const rz_bloom_params& P, const float* in, const float4* in4, float* rgb, float* glare, float4* out4) {
    const int W = c->frame.width, H = c->frame.height;
    BloomCombine C{};
    C.in = in; C.in4 = in4;
    C.w = W; C.h = H;
    C.intensity = P.intensity;
    C.copy = P.intensity == 0.0f ? 1 : 0;
    C.rgb = rgb; C.glare = glare; C.out4 = out4;
    if (!bloom_needs_pyramid(P, glare != nullptr)) {        // out = c: nothing in place, a copy of the rgb frame, or the resolve
        if (in && !out4) {
            if (rgb != in) RZ_HIP(c, hipMemcpyAsync(rgb, in, (size_t)W * H * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            return RZ_OK;
        }
        launch_bloom_combine(C, c->stream);
        RZ_HIP(c, hipGetLastError());
        return RZ_OK;
    }
    const BloomLevels L = bloom_levels(W, H, P.levels);
    float4* ws = static_cast<float4*>(c->dBloom.p);
    for (int k = 0; k < L.n; ++k) {
        BloomDown K{};
        if (k == 0) { K.rgb = in; K.src4 = in4; K.prefilter = 1; K.sw = W; K.sh = H; }
        else { K.src4 = ws + L.off[k - 1]; K.sw = L.w[k - 1]; K.sh = L.h[k - 1]; }
        K.dst = ws + L.off[k];
        K.dw = L.w[k]; K.dh = L.h[k];
        K.threshold = P.threshold; K.knee = P.knee; K.limit = P.limit;
        launch_bloom_down(K, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    for (int k = L.n - 2; k >= 0; --k) {
        BloomUp U{};
        U.coarse = ws + L.off[k + 1]; U.cw = L.w[k + 1]; U.ch = L.h[k + 1];
        U.fine = ws + L.off[k]; U.w = L.w[k]; U.h = L.h[k];
        U.spread = P.spread;
        launch_bloom_up(U, c->stream);
        RZ_HIP(c, hipGetLastError());
    }
    double N = 0.0, pw = 1.0;       // N = sum of spread^k, the powers by repeated multiplication, ascending k
    for (int k = 0; k < L.n; ++k) { N += pw; pw *= (double)P.spread; }
    C.u0 = ws; C.cw = L.w[0]; C.ch = L.h[0];
    C.n = (float)(1.0 / N);
    launch_bloom_combine(C, c->stream);
    RZ_HIP(c, hipGetLastError());
    return RZ_OK;
}

static bool ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return a && b && p < q + bytes && q < p + bytes;
}

static int bloom_impl(rz_ctx* c, const rz_bloom_params* pp, const float* rgb_in, size_t rgb_in_bytes, float* rgb32f, size_t rgb32f_bytes,
                      float* glare, size_t glare_bytes, unsigned flags) {
    const char* what = "rz_bloom";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~RZ_BLOOM_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const rz_bloom_params& P = pp ? *pp : kBloomDefaults;
    int rc = bloom_check(c, what, P);
    if (rc != RZ_OK) return rc;
    if (!rgb_in && c->frame.tile_nranks > 1)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: the frame is tile %d of %d; the accumulation is not the whole frame", what, c->frame.tile_rank, c->frame.tile_nranks);
    const bool host = (flags & RZ_BLOOM_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(rgb_in) | reinterpret_cast<uintptr_t>(rgb32f) | reinterpret_cast<uintptr_t>(glare)) & 3u))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 4-byte aligned", what);
    if (!rgb32f && !glare) return fail(c, RZ_ERR_INVALID_ARG, "%s: neither rgb32f nor glare is given", what);
    const size_t np = (size_t)c->frame.width * c->frame.height;
    const size_t bRgb = np * 3 * sizeof(float);
    if (ranges_overlap(glare, rgb_in, bRgb) || ranges_overlap(glare, rgb32f, bRgb))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: glare must not alias rgb_in or rgb32f", what);
    if (rgb_in && rgb_in_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb_in needs %zu bytes, got %zu", what, bRgb, rgb_in_bytes);
    if (!rgb_in) {
        rc = accum_fits(c, what);
        if (rc != RZ_OK) return rc;
    }
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (glare && glare_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: glare needs %zu bytes, got %zu", what, bRgb, glare_bytes);
    if (bloom_needs_pyramid(P, glare != nullptr)) {
        rc = bloom_workspace(c, what, P);
        if (rc != RZ_OK) return rc;
    }
    const float* in = rgb_in;
    const float4* in4 = rgb_in ? nullptr : static_cast<const float4*>(rz_accum_device_ptr(c));
    // host buffers are staged as rz_display stages them: the input in dRayIn; rgb32f, then glare in dRayOut
    HostStage stage(c, host);
    const int sRgb = stage.add(rgb32f, bRgb), sGlare = stage.add(glare, bRgb);
    rc = stage.input(rgb_in, bRgb, in);
    if (rc == RZ_OK) rc = stage.place();
    if (rc != RZ_OK) return rc;
    rc = bloom_run(c, P, in, in4, stage.dev<float>(sRgb), stage.dev<float>(sGlare), nullptr);
    if (rc != RZ_OK) return rc;
    if (!host) return RZ_OK;
    return stage.fetch();
}

static int present_bloomed_impl(rz_ctx* c, const rz_present_params* pp, const rz_display_params* dp, const rz_bloom_params* bp,
                                int source, const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f,
                                size_t rgb32f_bytes) {
    const char* what = "rz_present_bloomed";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!pp) return fail(c, RZ_ERR_INVALID_ARG, "%s: null present params", what);
    const rz_display_params& D = dp ? *dp : kDisplayDefaults;
    const rz_bloom_params& B = bp ? *bp : kBloomDefaults;
    FilterSource F;
    int rc = source_check(c, what, source, filter_params, D, F);
    if (rc != RZ_OK) return rc;
    rc = bloom_check(c, what, B);
    if (rc != RZ_OK) return rc;
    const bool bloomed = B.intensity != 0.0f;       // intensity 0: out = c, the call IS rz_present_display
    if (source == 0 && (D.exposure_mode == 1 || bloomed) && c->frame.tile_nranks > 1)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: the frame is tile %d of %d; %s needs the whole frame", what, c->frame.tile_rank,
                    c->frame.tile_nranks, D.exposure_mode == 1 ? "metering" : "the glare");
    const size_t np = (size_t)c->frame.width * c->frame.height;
    rc = present_sizes(c, what, np, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dDnOut, np * 16);
    if (rc == RZ_OK && bloomed) rc = bloom_workspace(c, what, B);
    if (rc != RZ_OK) return rc;
    float4* out4 = static_cast<float4*>(c->dDnOut.p);
    const float4* accum = static_cast<const float4*>(rz_accum_device_ptr(c));
    rc = source_run(c, F, accum, out4);
    if (rc != RZ_OK) return rc;
    // the source's colour -- the accumulation, or the (colour, 1) a denoiser left in out4 -- becomes (bloomed colour, 1) in out4,
    // which the tone kernel then rewrites in place
    const float4* colour = source == 0 ? accum : out4;
    if (bloomed) {
        rc = bloom_run(c, B, nullptr, colour, nullptr, nullptr, out4);
        if (rc != RZ_OK) return rc;
        colour = out4;
    }
    rc = display_run(c, D, nullptr, colour, nullptr, nullptr, out4, false);
    if (rc != RZ_OK) return rc;
    rc = present_impl(c, pp, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, out4);
    if (rc != RZ_OK) return rc;
    return source == 0 ? RZ_OK : report_backstop(c, what, "the guide may be wrong");
}

// rz_upscale / rz_present_upscaled (rz_upscale.hip).  The frame rz_set_frame set is the LOW one; they read its size and camera,
// the device scene as finalize left it, and touch no render state.  What they keep is buffers of the high size.
static const rz_upscale_params kUpscaleDefaults = {2, 128.0f, 1.0f, 1, {0, 0, 0, 0}};

static int upscale_check(rz_ctx* c, const char* what, const rz_upscale_params& P) {
    if (P.factor < 1 || P.factor > 4) return fail(c, RZ_ERR_INVALID_ARG, "%s: factor %d outside 1..4", what, P.factor);
    if (P.reserved[0] || P.reserved[1] || P.reserved[2] || P.reserved[3]) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words must be 0", what);
    // the rest is rz_denoise's: the sigmas, demodulate, the frame, the scene, the whole frame (no colour sigma, no passes here)
    const rz_denoise_params D = {1, 1.0f, P.sigma_normal, P.sigma_plane, P.demodulate, {0, 0, 0}};
    const int rc = denoise_check(c, what, D);
    if (rc != RZ_OK) return rc;
    if ((long long)c->frame.width * P.factor * ((long long)c->frame.height * P.factor) > 0x7fffffffLL)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: %d x %d times %d is more than INT32_MAX pixels", what, c->frame.width, c->frame.height, P.factor);
    return RZ_OK;
}

// rz_upscale_seethrough / rz_present_upscaled_seethrough (rz_seethrough.hip): the same calls with the guide cast along the
// pixel's deterministic chain.  `st` below is null for the first-hit entry points, whose launches and buffers are unchanged.
static const rz_seethrough_params kSeethroughDefaults = {8, {0, 0, 0, 0, 0, 0, 0}};

static int seethrough_check(rz_ctx* c, const char* what, const rz_seethrough_params& S) {
    if (S.max_depth < 0 || S.max_depth > 8) return fail(c, RZ_ERR_INVALID_ARG, "%s: max_depth %d outside 0..8", what, S.max_depth);
    for (int k = 0; k < 7; ++k)
        if (S.reserved[k]) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words of rz_seethrough_params must be 0", what);
    return RZ_OK;
}

// One launch of rz_seethrough_guides at width x height with the frame's camera: the 48-B records, and the rz_hit and rz_chain
// records when asked.
static int seethrough_cast(rz_ctx* c, int width, int height, int maxDepth, float4* rec, float4* hits, float4* chains) {
    KParams K{};
    SeethroughGuideLaunch G{};
    const int rc = cast_wiring(c, width, height, K, G);
    if (rc != RZ_OK) return rc;
    G.maxDepth = maxDepth;
    G.rec = rec;
    G.hits = hits;
    G.chains = chains;
    launch_seethrough_guides(K, G, c->stream);
    RZ_HIP(c, hipGetLastError());
    return RZ_OK;
}

// Casts a guide of either kind at width x height into the buffer that kind keeps, which it sizes first: the chain records (48 B,
// seethrough_cast) into the see-through pair with `st`, rz_denoise's (32 B, guide_cast; `chains` is then null) into the
// upsampler's pair without.  hi: the pair's high-size buffer.  `guide` receives the records' address.
static int either_cast(rz_ctx* c, const rz_seethrough_params* st, bool hi, int width, int height, float4* hits, float4* chains,
                       const float4*& guide) {
    DevBuf& buf = st ? (hi ? c->dStGuideHi : c->dStGuideLo) : (hi ? c->dUpGuideHi : c->dUpGuideLo);
    const int rc = ensure(c, buf, (size_t)width * height * (st ? 48 : 32));
    if (rc != RZ_OK) return rc;
    float4* rec = static_cast<float4*>(buf.p);
    guide = rec;
    return st ? seethrough_cast(c, width, height, st->max_depth, rec, hits, chains) : guide_cast(c, width, height, rec, hits);
}

// The world size of a frame pixel at unit distance.
static double frame_fpx(const rz_frame_params& f) { return 2.0 * std::fabs((double)f.inv_proj[5]) / (double)f.height; }

// What rz_upscale_gather and the antialias kernels read and write, at the frame rz_set_frame set (the upsampler's LOW frame): the
// colour in3 or in4, the guides, the outputs and the filter's terms.
static UpscaleLaunch upscale_wiring(rz_ctx* c, const rz_upscale_params& P, const float* in3, const float4* in4, const float4* guideLo,
                                    const float4* guideHi, float* rgb, float4* out4) {
    const rz_frame_params& f = c->frame;
    UpscaleLaunch U{};
    U.in3 = in4 ? nullptr : in3;
    U.in4 = in4;
    U.guideLo = guideLo;
    U.guideHi = guideHi;
    U.materials = static_cast<const DevMaterial*>(c->dMat.p);
    U.dst = out4;
    U.rgb = rgb;
    U.w = f.width; U.h = f.height;
    U.s = P.factor;
    U.sigmaNormal = P.sigma_normal;
    U.planeScale = (float)(1.0 / ((double)P.sigma_plane * frame_fpx(f)));
    U.demodulate = P.demodulate;
    return U;
}

// Factor 1 of rz_upscale and rz_antialias, c_p itself: in4 resolved into out4 and rgb, or in3 copied to rgb unless it is rgb.
static int colour_itself(rz_ctx* c, const float* in3, const float4* in4, float* rgb, float4* out4) {
    if (in4) {
        DenoiseLaunch D{};
        D.accum = in4;
        D.dst = out4;
        D.rgb = rgb;
        D.width = c->frame.width; D.height = c->frame.height;
        launch_denoise_resolve(D, c->stream);
        RZ_HIP(c, hipGetLastError());
    } else if (rgb && rgb != in3) {
        RZ_HIP(c, hipMemcpyAsync(rgb, in3, (size_t)c->frame.width * c->frame.height * 12, hipMemcpyDeviceToDevice, c->stream));
    }
    return RZ_OK;
}

// Casts both guides and gathers, on the stream; factor >= 2.  The low frame (device) is in3 (3 floats per pixel) or in4 (RGBA32F
// sum and count); outputs (device, high size, each optional): rgb (3 floats per pixel), out4 ((colour, 1)), hits (rz_hit).
static int upscale_run(rz_ctx* c, const rz_upscale_params& P, const float* in3, const float4* in4, float* rgb, float4* out4, float4* hits,
                       const rz_seethrough_params* st = nullptr, float4* chains = nullptr) {
    if (!rgb && !out4 && !hits && !chains) return RZ_OK;
    const rz_frame_params& f = c->frame;
    const int W = f.width * P.factor, H = f.height * P.factor;
    int rc = finalize(c);
    if (rc != RZ_OK) return rc;
    rc = cast_ready(c);
    if (rc != RZ_OK) return rc;
    // the high cast first: its overflow columns (size_blas_stack) are the larger ones, so the low cast finds them in place
    const float4 *guideHi = nullptr, *guideLo = nullptr;
    rc = either_cast(c, st, true, W, H, hits, chains, guideHi);
    if (rc != RZ_OK) return rc;
    if (!rgb && !out4) return RZ_OK;
    rc = either_cast(c, st, false, f.width, f.height, nullptr, nullptr, guideLo);
    if (rc != RZ_OK) return rc;
    const UpscaleLaunch U = upscale_wiring(c, P, in3, in4, guideLo, guideHi, rgb, out4);
    if (st) launch_seethrough_gather(U, c->stream);
    else launch_upscale_gather(U, c->stream);
    RZ_HIP(c, hipGetLastError());
    return RZ_OK;
}

static int upscale_impl(rz_ctx* c, const rz_upscale_params* pp, const float* rgb_in, size_t rgb_in_bytes, float* rgb32f,
                        size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, unsigned flags,
                        const rz_seethrough_params* st = nullptr, rz_chain* chains = nullptr, size_t chains_bytes = 0) {
    const char* what = st ? "rz_upscale_seethrough" : "rz_upscale";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~RZ_UPSCALE_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const rz_upscale_params& P = pp ? *pp : kUpscaleDefaults;
    int rc = upscale_check(c, what, P);
    if (rc != RZ_OK) return rc;
    if (st) {
        rc = seethrough_check(c, what, *st);
        if (rc != RZ_OK) return rc;
    }
    const bool host = (flags & RZ_UPSCALE_HOST) != 0;
    if (!host && (((reinterpret_cast<uintptr_t>(guides) | reinterpret_cast<uintptr_t>(chains)) & 15u) ||
                  ((reinterpret_cast<uintptr_t>(rgb_in) | reinterpret_cast<uintptr_t>(rgb32f)) & 3u)))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte (guides%s) or 4-byte (rgb_in, rgb32f) aligned", what,
                    st ? ", chains" : "");
    const size_t np = (size_t)c->frame.width * c->frame.height, nP = np * P.factor * P.factor;
    const size_t bIn = np * 3 * sizeof(float), bRgb = nP * 3 * sizeof(float), bHits = nP * sizeof(rz_hit), bChains = nP * sizeof(rz_chain);
    if (rgb_in && rgb_in_bytes < bIn) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb_in needs %zu bytes, got %zu", what, bIn, rgb_in_bytes);
    if (!rgb_in) {
        rc = accum_fits(c, what);
        if (rc != RZ_OK) return rc;
    }
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (guides && guides_bytes < bHits) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: guides needs %zu bytes, got %zu", what, bHits, guides_bytes);
    if (chains && chains_bytes < bChains) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: chains needs %zu bytes, got %zu", what, bChains, chains_bytes);
    if (!rgb32f && !guides && !chains) return RZ_OK;
    const float* in3 = rgb_in;
    const float4* in4 = rgb_in ? nullptr : static_cast<const float4*>(rz_accum_device_ptr(c));
    // host buffers are staged as rz_denoise stages them: the input in dRayIn; hits, then chains, then rgb32f in dRayOut
    HostStage stage(c, host);
    const int sHits = stage.add(guides, bHits), sChains = stage.add(chains, bChains), sRgb = stage.add(rgb32f, bRgb);
    rc = stage.input(rgb_in, bIn, in3);
    if (rc == RZ_OK) rc = stage.place();
    if (rc != RZ_OK) return rc;
    float* dRgb = stage.dev<float>(sRgb);
    float4* dHits = stage.dev<float4>(sHits);
    float4* dChains = stage.dev<float4>(sChains);
    if (P.factor == 1) {                    // c_p itself, and nothing is cast unless the guide is asked for
        if (dRgb) rc = colour_itself(c, in3, in4, dRgb, nullptr);
        if (rc == RZ_OK && (dHits || dChains)) {
            const float4* guide = nullptr;
            rc = finalize(c);
            if (rc == RZ_OK) rc = cast_ready(c);
            if (rc == RZ_OK) rc = either_cast(c, st, true, c->frame.width, c->frame.height, dHits, dChains, guide);
        }
    } else {
        rc = upscale_run(c, P, in3, in4, dRgb, nullptr, dHits, st, dChains);
    }
    if (rc != RZ_OK) return rc;
    if (!host) return RZ_OK;
    rc = stage.fetch();
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the guide may be wrong");
}

static int present_upscaled_impl(rz_ctx* c, const rz_present_params* pp, const rz_upscale_params* up, const rz_display_params* dp,
                                 int source, const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f,
                                 size_t rgb32f_bytes, const rz_seethrough_params* st = nullptr) {
    const char* what = st ? "rz_present_upscaled_seethrough" : "rz_present_upscaled";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!pp) return fail(c, RZ_ERR_INVALID_ARG, "%s: null present params", what);
    const rz_upscale_params& U = up ? *up : kUpscaleDefaults;
    const rz_display_params& D = dp ? *dp : kDisplayDefaults;
    FilterSource F;
    int rc = source_check(c, what, source, filter_params, D, F);
    if (rc != RZ_OK) return rc;
    rc = upscale_check(c, what, U);
    if (rc != RZ_OK) return rc;
    if (st) {
        rc = seethrough_check(c, what, *st);
        if (rc != RZ_OK) return rc;
    }
    // factor 1: nothing to reconstruct, the call IS rz_present_display (its bytes exactly, for every source)
    if (U.factor == 1) return present_display_impl(c, pp, dp, source, filter_params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    const int W = c->frame.width * U.factor, H = c->frame.height * U.factor;
    const size_t np = (size_t)c->frame.width * c->frame.height, nP = (size_t)W * H;
    rc = present_sizes(c, what, nP, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dUpOut, nP * 16);
    if (rc != RZ_OK) return rc;
    float4* hi4 = static_cast<float4*>(c->dUpOut.p);
    const float4* low4 = static_cast<const float4*>(rz_accum_device_ptr(c));
    if (source != 0) {                      // the denoisers run at the low size and leave (colour, 1), which resolves to the colour
        rc = ensure(c, c->dDnOut, np * 16);
        if (rc != RZ_OK) return rc;
        float4* out4 = static_cast<float4*>(c->dDnOut.p);
        rc = source_run(c, F, low4, out4);
        if (rc != RZ_OK) return rc;
        low4 = out4;
    }
    rc = upscale_run(c, U, nullptr, low4, nullptr, hi4, nullptr, st);
    if (rc != RZ_OK) return rc;
    rc = display_run(c, D, nullptr, hi4, nullptr, nullptr, hi4, false, (long long)nP);
    if (rc != RZ_OK) return rc;
    rc = present_impl(c, pp, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, hi4, W, H);
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the guide may be wrong");
}

// rz_antialias / rz_present_antialiased (rz_antialias.hip).  The frame rz_set_frame set is the frame that was rendered; they
// read its size and camera, the device scene as finalize left it, and touch no render state.  The frame-size guide lives in the
// upsampler's low-guide buffer, which every call that reads it casts anew.
static const rz_antialias_params kAntialiasDefaults = {2, 128.0f, 1.0f, 1, 0.9f, 1.0f, {0, 0}};

static int antialias_check(rz_ctx* c, const char* what, const rz_antialias_params& P) {
    // the factor, the sigmas, demodulate, the frame, the scene, the whole frame: rz_upscale's
    const rz_upscale_params U = {P.factor, P.sigma_normal, P.sigma_plane, P.demodulate, {0, 0, 0, 0}};
    const int rc = upscale_check(c, what, U);
    if (rc != RZ_OK) return rc;
    if (!(P.edge_normal >= -1.0f && P.edge_normal <= 1.0f))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: edge_normal %g outside -1..1", what, (double)P.edge_normal);
    if (!(P.edge_plane >= 0.0f && P.edge_plane < INFINITY))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: edge_plane %g (finite, >= 0)", what, (double)P.edge_plane);
    if (P.reserved[0] || P.reserved[1]) return fail(c, RZ_ERR_INVALID_ARG, "%s: reserved words of rz_antialias_params must be 0", what);
    return RZ_OK;
}

// Casts the frame-size guide, classifies and anti-aliases, on the stream.  The frame (device) is in3 (3 floats per pixel) or in4
// (RGBA32F sum and count); outputs (device, frame size, each optional): rgb (3 floats per pixel), out4 ((colour, 1)), hits
// (rz_hit), edges (a byte per pixel).  Factor 1 without `edges` casts nothing unless hits are asked for.
// rz_antialias_seethrough / rz_present_antialiased_seethrough (rz_antialias_seethrough.hip) pass `st`: the frame-size records are
// then the chain records (48 B, in the see-through low-guide buffer), `chains` (rz_chain) is one more optional output, and the
// kernel is the one that follows the chains.  With `st` null every launch and buffer is the first-hit call's, unchanged.
static int antialias_run(rz_ctx* c, const rz_antialias_params& P, const float* in3, const float4* in4, float* rgb, float4* out4,
                         float4* hits, uint8_t* edges, const rz_seethrough_params* st = nullptr, float4* chains = nullptr) {
    if (!rgb && !out4 && !hits && !edges && !chains) return RZ_OK;
    const rz_frame_params& f = c->frame;
    int rc = finalize(c);
    if (rc != RZ_OK) return rc;
    const bool kernel = edges || ((rgb || out4) && P.factor > 1);
    if (!kernel && (rgb || out4)) {         // factor 1: c_p itself
        rc = colour_itself(c, in3, in4, rgb, out4);
        if (rc != RZ_OK) return rc;
    }
    if (!kernel && !hits && !chains) return RZ_OK;
    rc = cast_ready(c);
    if (rc != RZ_OK) return rc;
    const float4* guide = nullptr;
    rc = either_cast(c, st, false, f.width, f.height, hits, chains, guide);
    if (rc != RZ_OK || !kernel) return rc;
    KParams K{};
    AntialiasSeethroughLaunch A{};          // (AntialiasLaunch and the chain's bound; the first-hit kernel takes the base)
    rc = cast_wiring(c, f.width, f.height, K, A, st ? 0 : RZ_AA_QUEUE * sizeof(int));
    if (rc != RZ_OK) return rc;
    A.U = upscale_wiring(c, {P.factor, P.sigma_normal, P.sigma_plane, P.demodulate, {0, 0, 0, 0}}, in3, in4, guide, nullptr, rgb, out4);
    A.edges = edges;
    A.edgeNormal = P.edge_normal;
    A.edgePlane = (float)((double)P.edge_plane * frame_fpx(f));
    A.maxDepth = st ? st->max_depth : 0;
    if (st) {                               // the list between the two kernels: a segment per wave of the grid
        A.segCap = (int)((A.units + A.grid - 1) / A.grid) * 64;
        rc = ensure(c, c->dAasList, (size_t)A.grid * A.segCap * sizeof(int));
        if (rc == RZ_OK) rc = ensure(c, c->dAasCounts, (size_t)A.grid * sizeof(int));
        if (rc != RZ_OK) return rc;
        A.list = static_cast<int*>(c->dAasList.p);
        A.counts = static_cast<int*>(c->dAasCounts.p);
    }
    if (st) launch_antialias_seethrough(K, A, c->stream);
    else launch_antialias(K, A, c->stream);
    RZ_HIP(c, hipGetLastError());
    return RZ_OK;
}

static int antialias_impl(rz_ctx* c, const rz_antialias_params* pp, const float* rgb_in, size_t rgb_in_bytes, float* rgb32f,
                          size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, uint8_t* edges, size_t edges_bytes, unsigned flags,
                          const rz_seethrough_params* st = nullptr, rz_chain* chains = nullptr, size_t chains_bytes = 0) {
    const char* what = st ? "rz_antialias_seethrough" : "rz_antialias";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (flags & ~RZ_ANTIALIAS_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    const rz_antialias_params& P = pp ? *pp : kAntialiasDefaults;
    int rc = antialias_check(c, what, P);
    if (rc != RZ_OK) return rc;
    if (st) {
        rc = seethrough_check(c, what, *st);
        if (rc != RZ_OK) return rc;
    }
    const bool host = (flags & RZ_ANTIALIAS_HOST) != 0;
    if (!host && (((reinterpret_cast<uintptr_t>(guides) | reinterpret_cast<uintptr_t>(chains)) & 15u) ||
                  ((reinterpret_cast<uintptr_t>(rgb_in) | reinterpret_cast<uintptr_t>(rgb32f)) & 3u)))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 16-byte (guides%s) or 4-byte (rgb_in, rgb32f) aligned", what,
                    st ? ", chains" : "");
    if (!host && rgb32f && rgb32f == rgb_in)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: rgb32f must not be rgb_in (an edge pixel reads its neighbours)", what);
    const size_t np = (size_t)c->frame.width * c->frame.height;
    const size_t bRgb = np * 3 * sizeof(float), bHits = np * sizeof(rz_hit), bChains = np * sizeof(rz_chain);
    if (rgb_in && rgb_in_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb_in needs %zu bytes, got %zu", what, bRgb, rgb_in_bytes);
    if (!rgb_in) {
        rc = accum_fits(c, what);
        if (rc != RZ_OK) return rc;
    }
    if (rgb32f && rgb32f_bytes < bRgb) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: rgb32f needs %zu bytes, got %zu", what, bRgb, rgb32f_bytes);
    if (guides && guides_bytes < bHits) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: guides needs %zu bytes, got %zu", what, bHits, guides_bytes);
    if (edges && edges_bytes < np) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: edges needs %zu bytes, got %zu", what, np, edges_bytes);
    if (chains && chains_bytes < bChains) return fail(c, RZ_ERR_BUFFER_SIZE, "%s: chains needs %zu bytes, got %zu", what, bChains, chains_bytes);
    if (!rgb32f && !guides && !edges && !chains) return RZ_OK;
    const float* in3 = rgb_in;
    const float4* in4 = rgb_in ? nullptr : static_cast<const float4*>(rz_accum_device_ptr(c));
    // host buffers are staged as rz_upscale stages them: the input in dRayIn; guides, then rgb32f, then edges, then chains in dRayOut
    HostStage stage(c, host);
    const int sHits = stage.add(guides, bHits), sRgb = stage.add(rgb32f, bRgb), sEdges = stage.add(edges, np);
    const int sChains = stage.add(chains, bChains);
    rc = stage.input(rgb_in, bRgb, in3);
    if (rc == RZ_OK) rc = stage.place();
    if (rc != RZ_OK) return rc;
    rc = antialias_run(c, P, in3, in4, stage.dev<float>(sRgb), nullptr, stage.dev<float4>(sHits), stage.dev<uint8_t>(sEdges), st,
                       stage.dev<float4>(sChains));
    if (rc != RZ_OK) return rc;
    if (!host) return RZ_OK;
    rc = stage.fetch();
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the guide may be wrong");
}

static int present_antialiased_impl(rz_ctx* c, const rz_present_params* pp, const rz_antialias_params* ap, const rz_display_params* dp,
                                    int source, const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f,
                                    size_t rgb32f_bytes, const rz_seethrough_params* st = nullptr) {
    const char* what = st ? "rz_present_antialiased_seethrough" : "rz_present_antialiased";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    if (!pp) return fail(c, RZ_ERR_INVALID_ARG, "%s: null present params", what);
    const rz_antialias_params& A = ap ? *ap : kAntialiasDefaults;
    const rz_display_params& D = dp ? *dp : kDisplayDefaults;
    FilterSource F;
    int rc = source_check(c, what, source, filter_params, D, F);
    if (rc != RZ_OK) return rc;
    rc = antialias_check(c, what, A);
    if (rc != RZ_OK) return rc;
    if (st) {
        rc = seethrough_check(c, what, *st);
        if (rc != RZ_OK) return rc;
    }
    // factor 1: nothing to average, the call IS rz_present_display (its bytes exactly, for every source)
    if (A.factor == 1) return present_display_impl(c, pp, dp, source, filter_params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    const size_t np = (size_t)c->frame.width * c->frame.height;
    rc = present_sizes(c, what, np, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    if (rc != RZ_OK) return rc;
    rc = ensure(c, c->dUpOut, np * 16);
    if (rc != RZ_OK) return rc;
    float4* aa4 = static_cast<float4*>(c->dUpOut.p);
    const float4* in4 = static_cast<const float4*>(rz_accum_device_ptr(c));
    if (source != 0) {                      // the denoisers leave (colour, 1), which resolves to the colour
        rc = ensure(c, c->dDnOut, np * 16);
        if (rc != RZ_OK) return rc;
        float4* out4 = static_cast<float4*>(c->dDnOut.p);
        rc = source_run(c, F, in4, out4);
        if (rc != RZ_OK) return rc;
        in4 = out4;
    }
    rc = antialias_run(c, A, nullptr, in4, nullptr, aa4, nullptr, nullptr, st);
    if (rc != RZ_OK) return rc;
    rc = display_run(c, D, nullptr, aa4, nullptr, nullptr, aa4, false);
    if (rc != RZ_OK) return rc;
    rc = present_impl(c, pp, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, aa4);
    if (rc != RZ_OK) return rc;
    return report_backstop(c, what, "the guide may be wrong");
}

static int display_reset_impl(rz_ctx* c) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "rz_display_reset: null context");
    if (!c->dDisplay.p) return RZ_OK;       // (nothing to drop)
    RZ_HIP(c, hipMemsetAsync(c->dDisplay.p, 0, sizeof(DisplayState), c->stream));
    return RZ_OK;
}

static int display_state_impl(rz_ctx* c, rz_display_info* out) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "rz_display_state: null context");
    if (!out) return fail(c, RZ_ERR_INVALID_ARG, "rz_display_state: null out");
    std::memset(out, 0, sizeof *out);
    out->exposure = out->target = 1.0f;     // a fresh state
    if (!c->dDisplay.p) return RZ_OK;
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    struct { float exposure; unsigned have; float call; unsigned pad; rz_display_info info; } head;
    static_assert(sizeof head == offsetof(DisplayState, work), "the head of DisplayState");
    RZ_HIP(c, hipMemcpy(&head, c->dDisplay.p, sizeof head, hipMemcpyDeviceToHost));
    if (head.have || head.info.exposure != 0.0f) *out = head.info;      // (else: zeroed by rz_display_reset, or never written)
    return RZ_OK;
}

static int debug_read_temporal_impl(rz_ctx* c, int which, void* out, size_t bytes, size_t* needed) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (which < 0 || which > 4) return fail(c, RZ_ERR_INVALID_ARG, "which = %d", which);
    const size_t np = c->tmpValid ? (size_t)c->tmpW * c->tmpH : 0;
    const int cur = c->tmpCur;
    float cam[51];
    size_t have = 0;
    const void* src = nullptr;
    switch (which) {
        case 0: have = np * 16; src = c->dTmpCol[cur].p; break;
        case 1: have = np * 8; src = c->dTmpMom[cur].p; break;
        case 2: have = np * sizeof(rz_hit); src = c->dTmpHits[cur].p; break;
        case 3: have = c->tmpValid ? sizeof cam : 0; break;
        default: have = c->tmpValid ? c->tmpInst * 96 : 0; src = c->dTmpInst[cur].p; break;
    }
    if (needed) *needed = have;
    if (!out || have == 0) return RZ_OK;
    if (bytes < have) return fail(c, RZ_ERR_BUFFER_SIZE, "rz_debug_read_temporal: %zu bytes held, buffer has %zu", have, bytes);
    if (which == 3) {
        std::memcpy(cam, c->tmpView, 64);
        std::memcpy(cam + 16, c->tmpProj, 64);
        std::memcpy(cam + 32, c->tmpInvProj, 64);
        std::memcpy(cam + 48, c->tmpCam, 12);
        std::memcpy(out, cam, sizeof cam);
        return RZ_OK;
    }
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    RZ_HIP(c, hipMemcpy(out, src, have, hipMemcpyDeviceToHost));
    return RZ_OK;
}

// ---- exported wrappers: no exception leaves the library (guarded(), above) ----
int rz_upload(rz_ctx* c, rz_binding binding, const void* data, size_t bytes) {
    return guarded(c, "rz_upload", [&] { return upload_impl(c, binding, data, bytes); });
}
int rz_update(rz_ctx* c, rz_binding binding, size_t offset, const void* data, size_t bytes) {
    return guarded(c, "rz_update", [&] { return update_impl(c, binding, offset, data, bytes); });
}
int rz_update_transforms(rz_ctx* c, const float* transforms, size_t n) {
    return guarded(c, "rz_update_transforms", [&] { return update_transforms_impl(c, transforms, n); });
}
int rz_refit_geometry(rz_ctx* c, const rz_triangle* triangles, size_t first_triangle, size_t n_triangles, unsigned flags) {
    return guarded(c, "rz_refit_geometry", [&] { return refit_geometry_impl(c, triangles, first_triangle, n_triangles, flags); });
}
int rz_skin_create(rz_ctx* c, size_t first_triangle, size_t n_triangles, const rz_triangle* rest, const rz_skin_triangle* skin, int n_bones,
                   const rz_morph_triangle* morphs, int n_morphs, int* rig_out) {
    return guarded(c, "rz_skin_create", [&] { return skin_create_impl(c, first_triangle, n_triangles, rest, skin, n_bones, morphs, n_morphs, rig_out); });
}
int rz_skin_pose(rz_ctx* c, int rig, const float* bones, const float* morph_weights, unsigned flags) {
    return guarded(c, "rz_skin_pose", [&] { return skin_pose_impl(c, rig, bones, morph_weights, flags); });
}
int rz_skin_destroy(rz_ctx* c, int rig) {
    return guarded(c, "rz_skin_destroy", [&] { return skin_destroy_impl(c, rig); });
}
int rz_skin_last_kernel_ms(rz_ctx* c, float* ms) {
    return guarded(c, "rz_skin_last_kernel_ms", [&] { return skin_last_kernel_ms_impl(c, ms); });
}
int rz_geometry_quality(rz_ctx* c, rz_mesh_quality* out, size_t cap, size_t* n_meshes) {
    return guarded(c, "rz_geometry_quality", [&] { return geometry_quality_impl(c, out, cap, n_meshes); });
}
int rz_rebuild_geometry(rz_ctx* c, double max_ratio, rz_mesh_quality* out, size_t cap, size_t* n_meshes, unsigned flags) {
    return guarded(c, "rz_rebuild_geometry", [&] { return rebuild_geometry_impl(c, max_ratio, out, cap, n_meshes, flags); });
}
int rz_build_blas(rz_ctx* c, const rz_triangle* tris, size_t n, rz_bvh_node* nodes_out, size_t nodes_cap, int32_t* indices_out, size_t* n_nodes, int* depth, float* device_ms) {
    return guarded(c, "rz_build_blas", [&] { return build_blas_impl(c, tris, n, nodes_out, nodes_cap, indices_out, n_nodes, depth, device_ms); });
}
int rz_read_binding(rz_ctx* c, rz_binding binding, void* out, size_t bytes, size_t* needed) {
    return guarded(c, "rz_read_binding", [&] { return read_binding_impl(c, binding, out, bytes, needed); });
}
int rz_set_frame(rz_ctx* c, const rz_frame_params* p) {
    return guarded(c, "rz_set_frame", [&] { return set_frame_impl(c, p); });
}
int rz_present(rz_ctx* c, const rz_present_params* pp, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present", [&] { return present_impl(c, pp, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes); });
}
int rz_resolve_rgba8(rz_ctx* c, uint8_t* rgba8, size_t bytes) {
    return guarded(c, "rz_resolve_rgba8", [&] { return resolve_rgba8_impl(c, rgba8, bytes); });
}
int rz_bind_accum(rz_ctx* c, void* device_rgba, size_t bytes) {
    return guarded(c, "rz_bind_accum", [&] { return bind_accum_impl(c, device_rgba, bytes); });
}
int rz_read_accum(rz_ctx* c, float* rgba, size_t bytes) {
    return guarded(c, "rz_read_accum", [&] { return read_accum_impl(c, rgba, bytes); });
}
int rz_clear_accum(rz_ctx* c) {
    return guarded(c, "rz_clear_accum", [&] { return clear_accum_impl(c); });
}

int rz_build_geometry(rz_ctx* c, const rz_triangle* triangles, size_t n_triangles, rz_mesh_build* meshes, size_t n_meshes) {
    return guarded(c, "rz_build_geometry", [&] { return build_geometry_impl(c, triangles, n_triangles, meshes, n_meshes); });
}

int rz_trace_rays(rz_ctx* c, const rz_ray* rays, rz_hit* hits, size_t n, unsigned flags) {
    return guarded(c, "rz_trace_rays", [&] { return rays_impl(c, rays, hits, n, flags, false); });
}
int rz_shadow_rays(rz_ctx* c, const rz_ray* rays, rz_visibility* out, size_t n, unsigned flags) {
    return guarded(c, "rz_shadow_rays", [&] { return rays_impl(c, rays, out, n, flags, true); });
}
int rz_render_editor(rz_ctx* c, const rz_frame_params* frame, const rz_editor_params* params, uint8_t* rgba8, size_t rgba8_bytes,
                     float* rgb32f, size_t rgb32f_bytes, rz_hit* hits, size_t hits_bytes, unsigned flags) {
    return guarded(c, "rz_render_editor", [&] {
        return editor_impl(c, frame, params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, hits, hits_bytes, flags);
    });
}

int rz_denoise(rz_ctx* c, const rz_denoise_params* params, const float* rgba_in, size_t rgba_in_bytes, float* rgb32f,
               size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, unsigned flags) {
    return guarded(c, "rz_denoise", [&] {
        return denoise_impl(c, params, rgba_in, rgba_in_bytes, rgb32f, rgb32f_bytes, guides, guides_bytes, flags);
    });
}
int rz_present_denoised(rz_ctx* c, const rz_present_params* present, const rz_denoise_params* params, uint8_t* rgba8,
                        size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_denoised", [&] {
        return present_denoised_impl(c, present, params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    });
}
int rz_denoise_temporal(rz_ctx* c, const rz_temporal_params* params, const float* rgba_in, size_t rgba_in_bytes, float* rgb32f,
                        size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, float* stats, size_t stats_bytes, unsigned flags) {
    return guarded(c, "rz_denoise_temporal", [&] {
        return temporal_impl(c, params, rgba_in, rgba_in_bytes, rgb32f, rgb32f_bytes, guides, guides_bytes, stats, stats_bytes, flags);
    });
}
int rz_present_temporal(rz_ctx* c, const rz_present_params* present, const rz_temporal_params* params, uint8_t* rgba8,
                        size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_temporal", [&] {
        return present_temporal_impl(c, present, params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    });
}
int rz_temporal_reset(rz_ctx* c) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "rz_temporal_reset: null context");
    c->tmpValid = false;
    return RZ_OK;
}
int rz_debug_read_temporal(rz_ctx* c, int which, void* out, size_t bytes, size_t* needed) {
    return guarded(c, "rz_debug_read_temporal", [&] { return debug_read_temporal_impl(c, which, out, bytes, needed); });
}
int rz_display(rz_ctx* c, const rz_display_params* params, const float* rgb_in, size_t rgb_in_bytes, float* rgb32f,
               size_t rgb32f_bytes, uint8_t* rgba8, size_t rgba8_bytes, unsigned flags) {
    return guarded(c, "rz_display", [&] {
        return display_impl(c, params, rgb_in, rgb_in_bytes, rgb32f, rgb32f_bytes, rgba8, rgba8_bytes, flags);
    });
}
int rz_present_display(rz_ctx* c, const rz_present_params* present, const rz_display_params* display, int source,
                       const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_display", [&] {
        return present_display_impl(c, present, display, source, filter_params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    });
}
int rz_bloom(rz_ctx* c, const rz_bloom_params* params, const float* rgb_in, size_t rgb_in_bytes, float* rgb32f, size_t rgb32f_bytes,
             float* glare, size_t glare_bytes, unsigned flags) {
    return guarded(c, "rz_bloom", [&] {
        return bloom_impl(c, params, rgb_in, rgb_in_bytes, rgb32f, rgb32f_bytes, glare, glare_bytes, flags);
    });
}
int rz_present_bloomed(rz_ctx* c, const rz_present_params* present, const rz_display_params* display, const rz_bloom_params* bloom,
                       int source, const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_bloomed", [&] {
        return present_bloomed_impl(c, present, display, bloom, source, filter_params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    });
}
int rz_upscale(rz_ctx* c, const rz_upscale_params* params, const float* rgb_in, size_t rgb_in_bytes, float* rgb32f,
               size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, unsigned flags) {
    return guarded(c, "rz_upscale", [&] {
        return upscale_impl(c, params, rgb_in, rgb_in_bytes, rgb32f, rgb32f_bytes, guides, guides_bytes, flags);
    });
}
int rz_present_upscaled(rz_ctx* c, const rz_present_params* present, const rz_upscale_params* upscale, const rz_display_params* display,
                        int source, const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_upscaled", [&] {
        return present_upscaled_impl(c, present, upscale, display, source, filter_params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    });
}
int rz_upscale_seethrough(rz_ctx* c, const rz_upscale_params* params, const rz_seethrough_params* seethrough, const float* rgb_in,
                          size_t rgb_in_bytes, float* rgb32f, size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, rz_chain* chains,
                          size_t chains_bytes, unsigned flags) {
    return guarded(c, "rz_upscale_seethrough", [&] {
        return upscale_impl(c, params, rgb_in, rgb_in_bytes, rgb32f, rgb32f_bytes, guides, guides_bytes, flags,
                            seethrough ? seethrough : &kSeethroughDefaults, chains, chains_bytes);
    });
}
int rz_present_upscaled_seethrough(rz_ctx* c, const rz_present_params* present, const rz_upscale_params* upscale,
                                   const rz_seethrough_params* seethrough, const rz_display_params* display, int source,
                                   const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_upscaled_seethrough", [&] {
        return present_upscaled_impl(c, present, upscale, display, source, filter_params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes,
                                     seethrough ? seethrough : &kSeethroughDefaults);
    });
}
int rz_antialias(rz_ctx* c, const rz_antialias_params* params, const float* rgb_in, size_t rgb_in_bytes, float* rgb32f, size_t rgb32f_bytes,
                 rz_hit* guides, size_t guides_bytes, uint8_t* edges, size_t edges_bytes, unsigned flags) {
    return guarded(c, "rz_antialias", [&] {
        return antialias_impl(c, params, rgb_in, rgb_in_bytes, rgb32f, rgb32f_bytes, guides, guides_bytes, edges, edges_bytes, flags);
    });
}
int rz_present_antialiased(rz_ctx* c, const rz_present_params* present, const rz_antialias_params* antialias,
                           const rz_display_params* display, int source, const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes,
                           float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_antialiased", [&] {
        return present_antialiased_impl(c, present, antialias, display, source, filter_params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes);
    });
}
int rz_antialias_seethrough(rz_ctx* c, const rz_antialias_params* params, const rz_seethrough_params* seethrough, const float* rgb_in,
                            size_t rgb_in_bytes, float* rgb32f, size_t rgb32f_bytes, rz_hit* guides, size_t guides_bytes, rz_chain* chains,
                            size_t chains_bytes, uint8_t* edges, size_t edges_bytes, unsigned flags) {
    return guarded(c, "rz_antialias_seethrough", [&] {
        return antialias_impl(c, params, rgb_in, rgb_in_bytes, rgb32f, rgb32f_bytes, guides, guides_bytes, edges, edges_bytes, flags,
                              seethrough ? seethrough : &kSeethroughDefaults, chains, chains_bytes);
    });
}
int rz_present_antialiased_seethrough(rz_ctx* c, const rz_present_params* present, const rz_antialias_params* antialias,
                                      const rz_seethrough_params* seethrough, const rz_display_params* display, int source,
                                      const void* filter_params, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_antialiased_seethrough", [&] {
        return present_antialiased_impl(c, present, antialias, display, source, filter_params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes,
                                        seethrough ? seethrough : &kSeethroughDefaults);
    });
}
int rz_render_cost(rz_ctx* c, const rz_cost_params* params, rz_pixel_cost* cost, size_t cost_bytes, rz_counters* totals, unsigned flags) {
    return guarded(c, "rz_render_cost", [&] { return render_cost_impl(c, params, cost, cost_bytes, totals, flags); });
}
int rz_cost_view(rz_ctx* c, const rz_cost_view_params* params, const rz_pixel_cost* cost, size_t cost_bytes, float* rgb32f,
                 size_t rgb32f_bytes, rz_cost_stats* stats, unsigned flags) {
    return guarded(c, "rz_cost_view", [&] { return cost_view_impl(c, params, cost, cost_bytes, rgb32f, rgb32f_bytes, stats, flags); });
}
int rz_present_cost(rz_ctx* c, const rz_present_params* present, const rz_cost_view_params* params, uint8_t* rgba8, size_t rgba8_bytes,
                    float* rgb32f, size_t rgb32f_bytes) {
    return guarded(c, "rz_present_cost", [&] { return present_cost_impl(c, present, params, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes); });
}
int rz_coverage(rz_ctx* c, const rz_frame_params* frame, const rz_coverage_params* params, rz_instance_coverage* coverage,
                size_t coverage_bytes, int32_t* ids, size_t ids_bytes, unsigned flags) {
    return guarded(c, "rz_coverage", [&] { return coverage_impl(c, frame, params, coverage, coverage_bytes, ids, ids_bytes, flags); });
}
int rz_ambient_occlusion(rz_ctx* c, const rz_frame_params* frame, const rz_ao_params* params, const float* rgb_in, size_t rgb_in_bytes,
                         float* ao, size_t ao_bytes, float* rgb32f, size_t rgb32f_bytes, uint8_t* rgba8, size_t rgba8_bytes, unsigned flags) {
    return guarded(c, "rz_ambient_occlusion", [&] {
        return ao_impl(c, frame, params, rgb_in, rgb_in_bytes, ao, ao_bytes, rgb32f, rgb32f_bytes, rgba8, rgba8_bytes, flags);
    });
}
int rz_ao_directions(float* out, size_t bytes) {
    const size_t need = RZ_AO_DIRS * 3 * sizeof(float);
    if (!out) return fail(nullptr, RZ_ERR_INVALID_ARG, "rz_ao_directions: null output");
    if (bytes < need) return fail(nullptr, RZ_ERR_BUFFER_SIZE, "rz_ao_directions: out needs %zu bytes, got %zu", need, bytes);
    std::memcpy(out, ao_direction_table(), need);
    return RZ_OK;
}
int rz_outline(rz_ctx* c, const rz_outline_params* params, const int32_t* ids, size_t ids_bytes, const uint32_t* selected,
               size_t n_instances, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes, unsigned flags) {
    return guarded(c, "rz_outline", [&] {
        return outline_impl(c, params, ids, ids_bytes, selected, n_instances, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, flags);
    });
}
int rz_draw_lines(rz_ctx* c, const rz_frame_params* frame, const rz_lines_params* params, const rz_line* lines, size_t n,
                  const rz_hit* hits, size_t hits_bytes, uint8_t* rgba8, size_t rgba8_bytes, float* rgb32f, size_t rgb32f_bytes,
                  unsigned flags) {
    return guarded(c, "rz_draw_lines", [&] {
        return lines_impl(c, frame, params, lines, n, hits, hits_bytes, rgba8, rgba8_bytes, rgb32f, rgb32f_bytes, flags);
    });
}
int rz_display_reset(rz_ctx* c) {
    return guarded(c, "rz_display_reset", [&] { return display_reset_impl(c); });
}
int rz_display_state(rz_ctx* c, rz_display_info* out) {
    return guarded(c, "rz_display_state", [&] { return display_state_impl(c, out); });
}
int rz_debug_read_layout(rz_ctx* c, int which, void* out, size_t bytes, size_t* needed) {
    return guarded(c, "rz_debug_read_layout", [&]() -> int {
        if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
        if (which < 0 || which > 2) return fail(c, RZ_ERR_INVALID_ARG, "which = %d", which);
        RZ_HIP(c, hipSetDevice(c->device));
        int rc = finalize(c);
        if (rc != RZ_OK) return rc;
        size_t have;
        const void* src;
        if (which == 0) { have = (c->layoutOnDevice ? (size_t)c->devPairsUsed : c->hPairs.size()) * sizeof(DevPair); src = c->dPairs.p; }
        else if (which == 1) { have = (c->layoutOnDevice ? (size_t)c->devTrisUsed : c->hTris.size()) * sizeof(DevTri); src = c->dTris.p; }
        else { have = (size_t)c->nTlasDfs * sizeof(TlasDfs); src = c->dTlasDfs.p; }     // whoever made it: finalize's upload or rz_tlas_refit
        if (needed) *needed = have;
        if (!out) return RZ_OK;
        if (bytes < have) return fail(c, RZ_ERR_BUFFER_SIZE, "layout %d holds %zu bytes, buffer has %zu", which, have, bytes);
        if (have) {
            RZ_HIP(c, hipMemcpyAsync(out, src, have, hipMemcpyDeviceToHost, c->stream));
            RZ_HIP(c, hipStreamSynchronize(c->stream));
        }
        return RZ_OK;
    });
}

int rz_debug_last_plan(rz_ctx* c, rz_launch_plan* out) {
    if (!c || !out) return fail(c, RZ_ERR_INVALID_ARG, "rz_debug_last_plan: null argument");
    if (!c->timed) return fail(c, RZ_ERR_NOT_READY, "rz_debug_last_plan: nothing has been rendered yet");
    *out = c->lastPlan;
    return RZ_OK;
}

int rz_debug_fail_alloc(rz_ctx* c, int nth) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    c->failAllocCountdown = nth > 0 ? nth : 0;
    return RZ_OK;
}

}  // extern "C"

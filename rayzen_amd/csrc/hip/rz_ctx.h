// rz_ctx.h -- struct rz_ctx and what the host files behind the C-ABI of include/rayzen_hip.h share: rz_context.hip and
// rz_ctx_render.hip.  Host code only; nothing else includes it, and no kernel file names the struct.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <tuple>
#include <limits>
#include <vector>

#include "rayzen_hip.h"
#include "rz_internal.h"

namespace rz {

// Device memory and its owner: move-only, freed with the object (a context's buffers with the context, a rig's with the rig,
// a local's at scope exit -- after whatever on the stream still reads it has been waited for).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Where a group of the caller's arrays is current (DESIGN.md 4.3 has the table).  The context keeps a host copy and a device
// copy of each group, several calls write only one of the two, and at least one of them always holds the bytes in force.
//   kTris: host[0] | dRawTris.   kBlas: host[7], [8] | dRawNodes, dRawIdx, described by devNodes, devIdx, devRoots.
//   kTlas: host[9], [5], [6] | dInstRef, dTlasNodes, dTlasIdx, described by tlasHostCounts, devTlasNodes; dXforms holds the transforms in force.
struct Residency { bool host = true, dev = false; };
enum Group { kTris, kBlas, kTlas, kNumGroups, kNoGroup = -1 };

// One BLAS as seen from an instance: RayZen lets every instance name its own
// node / index / triangle offsets (include/BVH.h:14-21); distinct triples are
// laid out once each.
struct BlasView {
    int pairBase = 0, triBase = 0;
    int rootEnc = 0;
    float rootMin[3] = {0, 0, 0}, rootMax[3] = {0, 0, 0};
    int depth = 1;
    bool empty = false;
    bool mayGlass = true;       // a triangle of the view may use a transparent material (a scheduling hint for the kernels: DevInstance.flags bit 1)
    bool irregular = false;     // device re-layout: one of its child boxes has min > max or a NaN plane
    int nPairs = 0, nSlots = 0; // what the view occupies behind pairBase / triBase
};

// What rz_refit_geometry needs of a laid-out view beyond the arrays (refit_topology): the breadth-first ranks of its
// internal nodes, level by level.  Derived once per layout, kept until the views are laid out again.
struct RefitView {
    std::tuple<int, int, int> key;
    int rankBase = 0;               // where its rankToNode entries start in dRefitRank
    std::vector<int> levelStart;    // ranks of tree level d: [levelStart[d], levelStart[d + 1]); empty: the root is a leaf
    int maxNode = 0;                // the largest node index (relative to the view) its root reaches
};

// One rig of rz_skin_create: the device copies rz_skin_pose's kernel reads (rz_skin.hip)
struct SkinRig {
    size_t first = 0, n = 0;        // its triangle range of binding 0
    int nBones = 0, nMorphs = 0;    // nBones == 0: a morph-only rig (dSkin is empty)
    DevBuf dRest, dSkin, dMorphs;
};

constexpr int kNumBindings = 10;

}  // namespace rz

// (struct rz_ctx is the C-ABI's global name; it spells the types it is made of as they are spelt inside namespace rz)
using rz::DevBuf; using rz::Residency; using rz::kNumGroups; using rz::BlasView; using rz::RefitView; using rz::SkinRig;
using rz::kNumBindings; using rz::DevPair; using rz::DevTri;

struct rz_ctx {
    int device = 0;
    unsigned flags = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    // a ring of event pairs: every render launch is bracketed on its stream, and the durations can be
    // collected later without synchronising inside a timed loop
    static constexpr int kRing = 64;
    hipEvent_t evStart[kRing] = {}, evStop[kRing] = {};
    int ringHead = 0;       // next slot to record into
    int ringCount = 0;      // launches recorded since the history was last drained (<= kRing)
    bool timed = false;
    int lastLaunches = 0;
    float hemi0[3] = {0.0f, 0.0f, 0.0f};   // KParams::hemi0, computed at rz_create
    long long triNValid = -1;       // triangles dTriN holds normals for (-1: none; reset with the geometry)
    long long lastGrid = 0;         // workgroups of the last render launch (RZ_PROF: how many wave-log entries are valid)
    rz_launch_plan lastPlan{};      // rz_debug_last_plan
    bool lastCompact = false;       // the last launch took compacting claims (rz_kernels.hip: render_claim_compact)
    bool lastGlobalPool = false;    // the last launch's waves kept their pools of parked paths across claims (rz_kernels.hip: pool_process)
    std::string err;

    // host copies of the caller's arrays (the re-layout needs them; rz_update patches them)
    std::vector<unsigned char> host[kNumBindings];
    bool present[kNumBindings] = {};
    Residency where[kNumGroups];    // triangles, BLAS nodes + indices, instances + TLAS: which copy is current
    bool geomDirty = true, instDirty = true, tlasDirty = true, matDirty = true, lightDirty = true;

    // device scene
    DevBuf dPairs, dTris, dInst, dTlasNodes, dTlasIdx, dMat, dLight, dCounters, dResolve, dGroupCtr, dBlasOvf;
    std::map<std::tuple<int, int, int>, BlasView> views;
    std::vector<DevPair> hPairs;
    std::vector<DevTri> hTris;
    int maxBlasDepth = 1, tlasDepth = 1;

    // frame
    bool haveFrame = false;
    rz_frame_params frame{};
    DevBuf ownAccum, dIor;
    // device-side dynamic update (rz_update_transforms)
    DevBuf dXforms, dInstRef, dTlasScratch, dProjBoxes, dBuildWs, dTlasDfs, dTriN;
    int nTlasDfs = 0;               // pop positions of the TLAS (rz_trace.h: trace_closest)
    int tlasEntry = 0;              // the verdict of whoever made dTlasDfs: queries may enter the list behind its root (rz_scene_dev.h: tlas_entry_verdict)
    int* tlasHostCounts = nullptr;      // pinned: node count, index count, depth, entry verdict
    int devTlasNodes = 0;
    bool sceneHasTransparency = true;   // some triangle uses a material with transparency > 0
    const char* lastKernel = "";
    void* extAccum = nullptr;
    size_t extAccumBytes = 0;
    int failAllocCountdown = 0;         // rz_debug_fail_alloc (test hook)
    // device re-layout (rz_relayout.hip): the caller's raw arrays on the device, the fill of dPairs / dTris, scratch
    DevBuf dRawNodes, dRawIdx, dRawTris, dRelayoutWs, dClaimScratch;
    DevBuf dSnap;                                  // transparent scenes: the resident waves' sample prefixes (rz_path.h: snapshot_store)
    DevBuf dWavePools, dWaitMeta;     // the resident waves' pools of parked paths and the bookkeeping of their wait slots (rz_kernels.hip: pool_process; the slots themselves: behind the claim scratch in dClaimScratch)
    size_t lastScratchBytes = 0;                   // what the last compacting launch's waves had in scratch (pools + wait slots + bookkeeping)
    int* relayoutPinned = nullptr;
    bool layoutOnDevice = false;        // dPairs / dTris were produced on the device (hPairs / hTris are empty)
    long long devPairsUsed = 0, devTrisUsed = 0;
    bool matChangedSinceLayout = false; // materials were uploaded after the BLAS views were laid out: their per-view transparency hints are stale
    unsigned devTransparent = 0;       // device re-layout: bit 0 a transparent material is in use, bit 1 an irregular child box
    bool irregularBoxes = false;       // some BLAS child box has min > max or a NaN plane: the traversal keeps the generic slab test
    // what describes dRawNodes / dRawIdx while only they are current (rz_build_geometry, a device refit, rz_rebuild_geometry)
    size_t devNodes = 0, devIdx = 0;
    std::map<int, rz_bvh_node> devRoots;    // node offset of a mesh -> its root node
    // ray queries (rz_trace_rays / rz_shadow_rays, rz_rays.hip): their own BLAS overflow columns, the staging buffers of
    // RZ_RAYS_HOST calls and the globalTriOffset of every instance (re-uploaded after the instances change)
    DevBuf dRayOvf, dRayIn, dRayOut, dRayInstOff;
    bool rayInstOffStale = true;
    // the denoiser (rz_denoise / rz_present_denoised, rz_denoise.hip): the guide (2 float4 per pixel), the two float4 buffers
    // its passes ping-pong between, and the (colour, 1) buffer rz_present_denoised presents
    DevBuf dDnGuide, dDnPing, dDnPong, dDnOut;
    // rz_denoise_temporal (rz_temporal.hip): two sets of history buffers (colour | N, moments, guide, instance transforms) that
    // swap roles at every committing call -- set tmpCur is the stored history, the other one is written -- the per-instance
    // "transform unchanged" flags, and the frame the history was made for
    DevBuf dTmpCol[2], dTmpMom[2], dTmpHits[2], dTmpInst[2], dTmpSame;
    int tmpCur = 0;
    bool tmpValid = false;
    int tmpW = 0, tmpH = 0;
    size_t tmpInst = 0;
    float tmpView[16] = {}, tmpProj[16] = {}, tmpInvProj[16] = {}, tmpCam[3] = {};
    // the display stage (rz_display / rz_present_display, rz_display.hip): one DisplayState -- the exposure last applied, the
    // rz_display_info record and the working histogram -- allocated and zeroed by the first call that needs it
    DevBuf dDisplay;
    // rz_upscale / rz_present_upscaled (rz_upscale.hip): the guides cast at the low and at the high size (2 float4 per pixel
    // each) and the high-size (colour, 1) buffer rz_present_upscaled presents; allocated on first use and kept
    DevBuf dUpGuideLo, dUpGuideHi, dUpOut;
    // rz_upscale_seethrough / rz_present_upscaled_seethrough (rz_seethrough.hip): the chain guides at both sizes (3 float4 per
    // pixel each); allocated on first use and kept.  The first-hit buffers above are not touched by those calls.
    DevBuf dStGuideLo, dStGuideHi;
    // rz_antialias_seethrough (rz_antialias_seethrough.hip): the edge pixels its classifying waves found, a segment per wave,
    // and the segments' counts; allocated on first use and kept
    DevBuf dAasList, dAasCounts;
    // rz_refit_geometry (rz_refit.hip)
    unsigned long long layoutGen = 0;   // counts the times the views / instances were laid out
    unsigned long long refitGen = ~0ull; // the layout the refit topology below was derived from
    std::vector<RefitView> refitViews;  // in the order of `views`
    DevBuf dRefitRank, dRefitInstView, dRefitViewOff, dRefitFlags, dRefitRoots;
    unsigned char* refitPinned = nullptr;   // per view: 4 flag words, then per view: its root node
    size_t refitPinnedCap = 0;
    // rz_skin_create / rz_skin_pose (rz_skin.hip): the rigs by id, the posed triangles the refit is given, the bones and morph
    // weights of a host-argument pose, and the events around the last pose's kernel
    std::map<int, SkinRig> rigs;
    int nextRig = 0;
    DevBuf dSkinOut, dSkinBones, dSkinWeights;
    hipEvent_t evSkin[2] = {nullptr, nullptr};
    bool skinTimed = false;
    // rz_geometry_quality (rz_quality.hip): the views as its kernels see them (derived with the refit topology), the
    // per-workgroup partial sums and the costs; and the cost of every laid-out mesh's tree as it was when it was last handed
    // over or built -- measured at the library's first look at it (note_built_costs), dropped with the tree
    DevBuf dQualViews, dQualPartials, dQualCost;
    int qualBlocks = 0;
    std::map<std::tuple<int, int, int>, double> costBuilt;
    unsigned long long costGen = ~0ull;  // the layout whose views all have their entry in costBuilt
    // rz_render_cost / rz_cost_view / rz_present_cost (rz_cost.hip): the last cost buffer (rz_pixel_cost per pixel) with the size
    // and spp it was measured at, the call's own counters, the reduction's partial records and its rz_cost_stats, and the
    // (colour, 1) buffer rz_present_cost presents; allocated on first use and kept
    DevBuf dCost, dCostCounters, dCostPartials, dCostStats, dCostOut;
    bool costValid = false;
    int costW = 0, costH = 0, costSpp = 0;
    // rz_coverage (rz_coverage.hip): the private sets of records its workgroups merge into, and the layout (sets, stride in
    // bytes, records per set) at which they are all empty -- rz_coverage_merge leaves them so; 0 sets: not known to be
    DevBuf dCovSets;
    long long covSets = 0;
    size_t covStride = 0, covCount = 0;
    // rz_ambient_occlusion (rz_ao.hip): the direction table (uploaded by the first call), raw_p of every pixel and the counter
    // its waves claim tiles from (zeroed by every call); the guide it casts goes to dDnGuide, which every pass that casts one
    // rewrites before it reads it
    DevBuf dAoDirs, dAoRaw, dAoClaim;
    // rz_render_adaptive (rz_adaptive.hip): per pixel, tile by tile, the accumulation after the tile's previous batch and the
    // luminance moments; per tile its error, the batches it has received and its flags; the list of the tiles a batch rendered;
    // the pinned block the flags come back to and the list goes up from; the events around a batch's render launches and its
    // metering launch.  Allocated by the first call and kept; every call starts them afresh
    DevBuf dAdPrev, dAdMoments, dAdError, dAdBatches, dAdFlags, dAdList;
    uint8_t* adPinned = nullptr;
    size_t adPinnedCap = 0;
    hipEvent_t evAdaptive[3] = {nullptr, nullptr, nullptr};
    // rz_draw_lines (rz_lines.hip): the projected records (52 B per line), the counts and offsets of the coarse lists (12 B per
    // cell and segment, and the total) and the lists themselves; allocated by the first call, grown on demand and kept
    DevBuf dLnRec, dLnCells, dLnList;
    // rz_bloom / rz_present_bloomed (rz_bloom.hip): the pyramid, level after level, a float4 per texel; allocated by the first
    // call that needs one, grown on demand and kept
    DevBuf dBloom;

    ~rz_ctx();      // the events and the pinned blocks (rz_context.hip, with rz_destroy); the DevBufs and the rigs free themselves
};

namespace rz {

// All defined in rz_context.hip.  (fail: sets the context's error text and the thread's; returns `code`)
int fail(rz_ctx* c, int code, const char* fmt, ...);

// No C++ exception crosses the C-ABI: every exported entry point that can reach a std::vector / std::map /
// std::string growth runs its body through guarded(), which turns std::bad_alloc into RZ_ERR_NO_MEMORY and anything
// else into RZ_ERR_HIP.  (rz_debug_fail_alloc arms a countdown that makes alloc_point() throw std::bad_alloc at the
// n-th host allocation site reached -- the test hook that proves the conversion.)
// It also makes the context's device the calling thread's current one: a context may be driven while another device is
// current (a group of several devices in one process, rz_group.hip: a member reached through rz_group_ctx), and every
// hipMalloc, kernel launch and event below would otherwise land on THAT device.
template <class F>
int guarded(rz_ctx* c, const char* what, F&& body) {
    try {
        if (c) {
            const hipError_t e = hipSetDevice(c->device);
            if (e != hipSuccess) return fail(c, RZ_ERR_HIP, "%s: hipSetDevice(%d): %s", what, c->device, hipGetErrorString(e));
        }
        return body();
    } catch (const std::bad_alloc&) {
        return fail(c, RZ_ERR_NO_MEMORY, "%s: out of host memory", what);
    } catch (const std::exception& e) {
        return fail(c, RZ_ERR_HIP, "%s: %s", what, e.what());
    } catch (...) {
        return fail(c, RZ_ERR_HIP, "%s: unknown C++ exception", what);
    }
}
void alloc_point(rz_ctx* c);

#define RZ_HIP(c, call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return fail((c), RZ_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

int ensure(rz_ctx* c, DevBuf& b, size_t bytes);
bool ensure_optional(DevBuf& b, size_t bytes);
int finalize(rz_ctx* c);
int ensure_group_counter(rz_ctx* c);
int size_blas_stack(rz_ctx* c, KParams& K, size_t fixedLds, int wavesPerCu, long long residentWaves, DevBuf& ovf);
int frame_kparams(rz_ctx* c, KParams& K, int spp, int sampleBase);

}  // namespace rz

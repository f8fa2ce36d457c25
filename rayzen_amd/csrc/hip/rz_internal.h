// rz_internal.h -- what the translation units of librayzen_hip.so share besides the device data layout
// (rz_scene_dev.h): the structs that cross file boundaries and the launch / helper entry points, declared ONCE.
// (Round 1 repeated some of these structs in the files that use them; two copies of one struct are an ODR violation
// waiting for the day one of them changes.)
#pragma once
#include <hip/hip_runtime.h>

#include "rayzen_hip.h"
#include "rz_scene_dev.h"

namespace rz {

// ---- the colour outputs of the passes that run outside a frame (rz_denoise.hip, rz_temporal.hip, rz_upscale_body.h,
// rz_antialias_body.h): pixel p as (c, w) in `dst` and as three floats in `rgb`, each optional.  C: a colour with x, y, z (v3).
template <class C>
__device__ __forceinline__ void store_colour(float4* dst, float* rgb, size_t p, const C& c, float w) {
    if (dst) dst[p] = make_float4(c.x, c.y, c.z, w);
    if (rgb) {
        rgb[3 * p] = c.x;
        rgb[3 * p + 1] = c.y;
        rgb[3 * p + 2] = c.z;
    }
}

// ---- rz_kernels.hip
// The launch shape of rz_render_pixels, which rz_cost_pixels (rz_cost.hip) takes as it stands.
#ifndef RZ_WAVES_PER_BLOCK
#define RZ_WAVES_PER_BLOCK 1   // measured on C2: 4 -> 98.9 ms, 2 -> 88.5 ms, 1 -> 88.0 ms (a 4-wave group holds its CU slots until its slowest tile ends)
#endif
constexpr int WAVES_PER_BLOCK = RZ_WAVES_PER_BLOCK;
#ifndef RZ_MIN_WAVES_PER_SIMD
#define RZ_MIN_WAVES_PER_SIMD 2
#endif
void launch_render_pixels(const KParams& K, bool counted, hipStream_t stream);
SamplesPlan plan_render_samples(int spp, int nSlots, bool glass);
size_t samples_lds_extra(bool glass, bool compact);
void launch_render_samples(const KParams& K, bool counted, bool glass, hipStream_t stream);
void launch_resolve(const float4* accum, uchar4* out, int n, hipStream_t stream);
int compute_hemi0(float out[3], hipStream_t stream);
#ifdef RZ_PROF
void dump_wave_log(int nWaves);
#endif
#ifdef RZ_GSTATS
void dump_gstats();
#endif

// ---- rz_rays.hip
constexpr int RZ_RAYS_WAVES_PER_CU = 16;         // resident waves per CU of a ray-query launch (one wave per workgroup)
struct RaysLaunch {
    const void* rays;           // device: n x rz_ray
    void* out;                  // device: n x rz_hit (trace) or n x rz_visibility (shadow)
    int n;
    long long grid;             // rays_grid(n)
    bool shadow, spread;        // which query; the lane-by-lane walk (trace_spread) instead of the wave-cursor one
    const int32_t* instTriOff;  // trace: globalTriOffset of every instance
    unsigned* errWord;          // the context's backstop word
};
long long rays_grid(long long n);
void launch_rays(const KParams& K, const RaysLaunch& R, hipStream_t stream);

// ---- rz_editor.hip
struct EditorLaunch {
    float view[16], proj[16];   // rz_frame_params.view / proj (the clip test of a hit)
    float ambient[3];           // rz_editor_params.ambient
    float clear[4];             // rz_editor_params.clear
    long long units;            // 64-pixel units of the frame: 64-pixel runs of a row (rows = 1), or 8 x 8 tiles
    int unitsX;                 // units per row of units
    int rows;                   // 1: a wave covers 64 pixels of one row (the default); 0: an 8 x 8 tile (RZ_EDITOR_TILES=1, an A/B aid)
    long long grid;             // rays_grid(width * height)
    bool spread;                // the lane-by-lane walk (trace_spread)
    uchar4* rgba8;              // device outputs, each optional (nullptr: not written); row 0 = bottom
    float* rgb32f;              // width x height x 3
    float4* hits;               // width x height rz_hit (3 float4)
    const int32_t* instTriOff;  // globalTriOffset of every instance (as RaysLaunch)
    unsigned* errWord;          // the context's backstop word
};
void launch_editor(const KParams& K, const EditorLaunch& E, hipStream_t stream);

// ---- rz_denoise.hip
struct DenoiseGuideLaunch {
    long long units;            // 64-pixel runs of a row
    int unitsX;                 // runs per row
    long long grid;             // rays_grid(units * 64)
    float4* guide;              // width x height x 2 float4: (normal, t), (point, hit word: material index, -1 = miss)
    float4* hits;               // width x height rz_hit (3 float4), optional
    const int32_t* instTriOff;  // globalTriOffset of every instance (as RaysLaunch)
    unsigned* errWord;          // the context's backstop word
};
void launch_denoise_guides(const KParams& K, const DenoiseGuideLaunch& G, hipStream_t stream);
struct DenoiseLaunch {
    const float4* accum;        // pass 0 (and the K = 0 resolve): RGBA32F sum and count
    const float4* src;          // later passes: the previous pass's output
    const float4* guide;        // DenoiseGuideLaunch::guide
    const DevMaterial* materials;
    float4* dst;                // the pass's output (the last pass: (colour, 1)); may be null on the last pass
    float* rgb;                 // the last pass: width x height x 3 floats, optional
    int width, height;
    int step;                   // s = 2^i
    float invColor;             // 2^i / sigma_color^2
    float sigmaNormal;
    float planeScale;           // 1 / (sigma_plane f s)
    int demodulate;
};
void launch_denoise_pass(const DenoiseLaunch& D, bool first, bool last, hipStream_t stream);
void launch_denoise_resolve(const DenoiseLaunch& D, hipStream_t stream);

// ---- rz_upscale.hip
struct UpscaleLaunch {          // rz_upscale_gather
    const float* in3;           // the low frame: w x h x 3 linear colour, or
    const float4* in4;          // RGBA32F sum and count (then `in3` is unused)
    const float4* guideLo;      // DenoiseGuideLaunch::guide cast at w x h
    const float4* guideHi;      // ... and at W x H = s w x s h
    const DevMaterial* materials;
    float4* dst;                // W x H (colour, 1), optional
    float* rgb;                 // W x H x 3 floats, optional
    int w, h;                   // the low frame
    int s;                      // the factor, 2..4
    float sigmaNormal;
    float planeScale;           // 1 / (sigma_plane f), f = 2 |inv_proj[5]| / h
    int demodulate;
};
void launch_upscale_gather(const UpscaleLaunch& U, hipStream_t stream);

// ---- rz_antialias.hip
constexpr int RZ_AA_QUEUE = 128;        // entries of a wave's edge queue in LDS: fewer than 64 / s^2 left over plus one unit's 64
struct AntialiasLaunch {        // rz_antialias_edges: DenoiseGuideLaunch's shape at the frame's size
    long long units;            // 64-pixel runs of a row
    int unitsX;                 // runs per row
    long long grid;             // rays_grid(units * 64)
    const int32_t* instTriOff;  // (cast_wiring's; the kernel writes no rz_hit)
    unsigned* errWord;          // the context's backstop word
    UpscaleLaunch U;            // the frame (in3 / in4, w, h), its guide (guideLo), s = the factor (1: classify only), the
                                // sigmas; dst / rgb: the w x h outputs, each optional; guideHi is unused
    uint8_t* edges;             // w x h bytes, 1 = edge, optional
    float edgeNormal;           // rz_antialias_params.edge_normal
    float edgePlane;            // k_e = (float)(edge_plane * f)
};
void launch_antialias(const KParams& K, const AntialiasLaunch& A, hipStream_t stream);

// ---- rz_seethrough.hip
struct SeethroughGuideLaunch {  // rz_seethrough_guides: DenoiseGuideLaunch with the chain's bound and outputs
    long long units;            // 64-pixel runs of a row
    int unitsX;                 // runs per row
    long long grid;             // rays_grid(units * 64)
    int maxDepth;               // rz_seethrough_params.max_depth, 0..8
    float4* rec;                // width x height x 3 float4: (n, L), (x, final hit word: material index, -1 = miss), (T, cls)
    float4* hits;               // width x height rz_hit (3 float4) of the final hit with t = L, optional
    float4* chains;             // width x height rz_chain, optional
    const int32_t* instTriOff;  // globalTriOffset of every instance (as RaysLaunch)
    unsigned* errWord;          // the context's backstop word
};
void launch_seethrough_guides(const KParams& K, const SeethroughGuideLaunch& G, hipStream_t stream);
void launch_seethrough_gather(const UpscaleLaunch& U, hipStream_t stream);     // guideLo / guideHi: SeethroughGuideLaunch::rec

// ---- rz_antialias_seethrough.hip
struct AntialiasSeethroughLaunch : AntialiasLaunch {    // both kernels: U.guideLo = SeethroughGuideLaunch::rec at w x h
    int maxDepth;               // rz_seethrough_params.max_depth, 0..8
    int segCap;                 // entries of a wave's segment of `list`: 64 x ceil(units / grid)
    int* list;                  // grid x segCap pixel indices: the edge pixels each classifying wave found
    int* counts;                // grid: how many
};
void launch_antialias_seethrough(const KParams& K, const AntialiasSeethroughLaunch& A, hipStream_t stream);

// ---- rz_temporal.hip
struct TemporalLaunch {         // rz_temporal_accumulate
    const float4* accum;        // RGBA32F sum and count
    const float4* hits;         // this frame's guide: width x height rz_hit (3 float4)
    const DevMaterial* materials;
    const DevInstance* instances;
    const float4* colPrev;      // the history: colour | N
    const float2* momPrev;      // ... the luminance moments
    const float4* hitsPrev;     // ... the guide
    const float* instPrev;      // ... per instance inverseTransform[12], transform[12] (DevInstance's packing)
    const int* instSame;        // per instance: 1 = its transform is the stored one bit for bit
    float4* colNext;            // the history this call writes
    float2* momNext;
    float4* dst;                // K = 0 only: (colour, 1), optional
    float* rgb;                 // K = 0 only: width x height x 3, optional
    int width, height;
    int nMaterials;
    int demodulate;
    int havePrev;               // 0: no history, every pixel starts at N = 1
    int cameraSame;             // view and proj equal the stored ones bit for bit
    float alpha, alphaMoments, maxHistory, normalCos, planeTol;
    float fPrev;                // 2 |inv_proj_prev[5]| / height
    float viewPrev[16], projPrev[16], camPrev[3];
    float invView[16], invProj[16];     // this frame's (the direction of a miss)
};
struct TemporalVarLaunch {      // rz_temporal_variance
    const float4* col;          // colour | N, as the accumulate kernel left it
    const float2* mom;
    const float4* guide;        // DenoiseGuideLaunch::guide
    float4* dst;                // colour | variance: the filter's input, optional
    float* stats;               // width x height x 2 (N, variance), optional
    int width, height;
    float sigmaNormal;
    float planeScale;           // 1 / (sigma_plane f)
};
struct TemporalFilterLaunch {   // rz_temporal_atrous
    const float4* src;          // colour | variance
    const float4* guide;
    const DevMaterial* materials;
    float4* dst;                // the pass's output (the last pass: (colour, 1)); may be null on the last pass
    float* rgb;                 // the last pass: width x height x 3 floats, optional
    int width, height;
    int step;                   // s = 2^i
    float sigmaL;
    float sigmaNormal;
    float planeScale;           // 1 / (sigma_plane f s)
    int demodulate;
};
void launch_temporal_instances(const DevInstance* inst, const float* prev, float* next, int* same, int n, bool havePrev, hipStream_t stream);
void launch_temporal_accumulate(const TemporalLaunch& T, hipStream_t stream);
void launch_temporal_variance(const TemporalVarLaunch& V, hipStream_t stream);
void launch_temporal_pass(const TemporalFilterLaunch& F, bool last, hipStream_t stream);

// ---- rz_display.hip
constexpr int RZ_DISPLAY_BINS = 128;    // rz_display_info::histogram
struct DisplayState {           // the context's display state, device memory (zeroed = fresh: no exposure yet)
    float exposure;             // the exposure last committed
    unsigned have;              // 1: `exposure` holds one
    float call;                 // the exposure of the auto call in flight (what its tone kernel reads; RZ_DISPLAY_KEEP commits nothing else)
    unsigned pad;
    rz_display_info info;       // what rz_display_state reports
    unsigned work[RZ_DISPLAY_BINS + 2];   // the working histogram: the bins, below, above; zero between calls
};
struct DisplayExpose {          // rz_display_expose
    int mode;                   // 0: commit `manual`; 1: meter-driven (steps 3 and 4)
    int keep;                   // RZ_DISPLAY_KEEP
    float manual;
    float key, minExposure, maxExposure, adapt;
    int lowPermille, highPermille;
};
struct DisplayTone {            // rz_display_tone
    const float* in;            // width x height x 3 linear colour, or
    const float4* in4;          // RGBA32F sum and count (then `in` is unused)
    const DisplayState* state;  // auto: the exposure is state->call; null: `exposure`
    float exposure;
    int curve;
    float white2;               // white * white
    int transfer;
    long long n;                // pixels
    float* rgb;                 // outputs, each optional: width x height x 3,
    uchar4* rgba8;              //   width x height,
    float4* out4;               //   (colour, 1) per pixel
};
void launch_display_meter(const float* rgb, const float4* rgba, long long n, DisplayState* S, hipStream_t s);
void launch_display_expose(DisplayState* S, const DisplayExpose& X, hipStream_t s);
void launch_display_tone(const DisplayTone& T, hipStream_t s);

// ---- rz_bloom.hip
constexpr int RZ_BLOOM_MAX_LEVELS = 8;  // rz_bloom_params::levels
struct BloomDown {              // rz_bloom_down: dst (dw x dh) from a source of sw x sh, dw = ceil(sw / 2), dh = ceil(sh / 2)
    const float* rgb;           // the frame as 3 floats per pixel (prefiltered at staging), or
    const float4* src4;         // prefilter: the RGBA32F sum and count (resolved, prefiltered); else a pyramid level
    int prefilter;
    float4* dst;
    int sw, sh, dw, dh;
    float threshold, knee, limit;
};
struct BloomUp {                // rz_bloom_up: fine (w x h) += spread * Up(coarse (cw x ch))
    const float4* coarse;
    float4* fine;
    int cw, ch, w, h;
    float spread;
};
struct BloomCombine {           // rz_bloom_combine, w x h pixels
    const float* in;            // 3 floats per pixel, or
    const float4* in4;          // RGBA32F sum and count (then `in` is unused)
    const float4* u0;           // U_0 (cw x ch); null: no glare is computed (copy, nothing asks for the glare)
    int cw, ch, w, h;
    float n, intensity;         // 1 / N; the weight
    int copy;                   // intensity == 0: out = c, bit for bit
    float* rgb;                 // outputs, each optional: out as 3 floats per pixel (may be `in`),
    float* glare;               //   the normalised glare as 3 floats per pixel,
    float4* out4;               //   (out, 1) per pixel (may be in4)
};
void launch_bloom_down(const BloomDown& K, hipStream_t s);
void launch_bloom_up(const BloomUp& U, hipStream_t s);
void launch_bloom_combine(const BloomCombine& C, hipStream_t s);

// ---- rz_tlas_device.hip
void launch_tlas_refit(const TlasWork& W, hipStream_t s);

// ---- rz_blas_device.hip
size_t blas_build_workspace_bytes(size_t n);
int blas_build_device(const rz_triangle* hostTris, size_t n, void* workspace, size_t workspaceBytes, rz_bvh_node* nodes_out,
                      int32_t* idx_out, int* nNodesOut, int* depthOut, float* ms, hipStream_t s);

// ---- rz_relayout.hip
struct RelayoutView {           // in: the three offsets; out: everything else
    int nodeOff, triOff, gTriOff;
    int pairBase, triBase;      // where this view's pairs / triangles start in the global arrays (in)
    int nPairs, nSlots, depth, rootEnc, empty;
    float rootMin[3], rootMax[3];
};
size_t relayout_workspace_bytes(size_t nNodes);
int relayout_view_device(const rz_bvh_node* nodes, long long nNodes, const int32_t* idx, long long nIdx, const rz_triangle* tris,
                         long long nTris, const rz_material* mats, int nMat, const rz_bvh_node& hostRoot, RelayoutView& V,
                         DevPair* pairs, long long pairCap, DevTri* trisOut, long long triCap, void* workspace, size_t workspaceBytes,
                         int* pinned, unsigned* transparentOut, hipStream_t s);
int tri_normals_device(const DevTri* tris, long long n, DevTriN* out, hipStream_t s);
int relayout_check_materials_device(const DevTri* tris, long long n, const rz_material* mats, int nMat, void* workspace, int* pinned,
                                    unsigned* transparentOut, int* detail, hipStream_t s);

// ---- rz_refit.hip
struct RefitViewWork {          // one BLAS view to refit; every pointer is the VIEW's part of its array unless it says otherwise
    rz_bvh_node* nodes;         // dRawNodes + blasNodeOffset
    const int32_t* idx;         // dRawIdx + blasTriOffset
    const rz_triangle* rawTris; // the WHOLE triangle array (already patched) and its length
    long long nTris;
    int gTriOff;                // globalTriOffset
    int nSlots;                 // leaf slots of the view
    DevTri* tris;               // dTris + triBase
    DevTriN* triN;              // dTriN + triBase
    DevPair* pairs;             // dPairs + pairBase
    const int32_t* rankToNode;  // device: pair index (breadth-first rank of an internal node) -> node index in the view
    const int* levelStart;      // HOST: ranks of tree level d are [levelStart[d], levelStart[d + 1]); nLevels + 1 entries
    int nLevels;                // 0: the root is a leaf
    const rz_material* mats;
    int nMat;
    unsigned* vflags;           // device, 4 words, zeroed by the caller: [0] bit 0 transparent, bit 1 irregular child box, bit 2 bad material index; [1] one such triangle
};
int refit_view_device(const RefitViewWork& W, hipStream_t s);
int refit_roots_device(DevInstance* inst, int nInst, const int32_t* instView, const int32_t* viewNodeOff, int nViews,
                       const rz_bvh_node* nodes, const unsigned* vflags, rz_bvh_node* rootsOut, hipStream_t s);

// ---- rz_quality.hip
struct QualityView {            // one BLAS view as the cost kernels see it; the array ends with a sentinel that carries the total block count
    int32_t nodeOff;            // blasNodeOffset
    int32_t rankBase;           // where its rankToNode entries start (RefitViewWork::rankToNode)
    int32_t nPairs;             // its internal nodes
    int32_t blockBase;          // the first of its ceil(nPairs / 256) workgroups in rz_quality_partials' grid
};
int quality_device(const rz_bvh_node* nodes, const int32_t* rank, const QualityView* views, int nViews, int nBlocks, double* partials,
                   double* cost, hipStream_t s);

// ---- rz_skin.hip
struct SkinWork {               // one rig posed: every pointer is device memory
    const rz_triangle* rest;            // n rest triangles
    const rz_skin_triangle* skin;       // n, or null: a morph-only rig
    const float* bones;                 // nBones x 16, column-major, 16-byte aligned (unused without `skin`)
    int nBones;
    const rz_morph_triangle* morphs;    // target-major [nMorphs][n]
    const float* morphWeights;          // nMorphs
    int nMorphs;
    long long n;
    rz_triangle* out;                   // n posed triangles
};
int skin_device(const SkinWork& W, hipStream_t s);

// ---- rz_cost.hip
constexpr int RZ_COST_REDUCE_BLOCKS = 1024;     // the most workgroups of rz_cost_reduce's first stage (= partial records)
struct CostLaunch {             // rz_cost_pixels (beside the KParams of a one-lane-per-pixel render at sample 0)
    uint4* cost;                // width x height rz_pixel_cost (2 uint4)
    unsigned* errWord;          // the context's backstop word
};
struct CostReduceLaunch {       // rz_cost_reduce_partials, rz_cost_reduce_final
    const uint4* cost;          // width x height rz_pixel_cost
    long long n;                // pixels
    int width;
    int metric;                 // rz_cost_view_params.metric
    float scale;                // rz_cost_view_params.scale
    int blocks;                 // workgroups of the first stage, <= RZ_COST_REDUCE_BLOCKS
    unsigned long long* partials;   // blocks x (maximum, its lowest pixel index, sum)
    rz_cost_stats* stats;       // what the second stage writes
};
struct CostViewLaunch {         // rz_cost_view
    const uint4* cost;
    const rz_cost_stats* stats; // scale_used: the top of the ramp
    int width, height;
    int metric, curve;
    float4* dst;                // (colour, 1), optional
    float* rgb;                 // width x height x 3 floats, optional
};
void launch_cost_pixels(const KParams& K, const CostLaunch& C, hipStream_t stream);
int cost_reduce_blocks(long long n);
void launch_cost_reduce(const CostReduceLaunch& R, hipStream_t stream);
void launch_cost_view(const CostViewLaunch& V, hipStream_t stream);

// ---- rz_coverage.hip
struct CoverageLaunch {         // rz_coverage_runs (beside the KParams of camera_kparams)
    int x0, y0, x1, y1;         // the rectangle clipped to the frame, not empty
    int unitsX;                 // 64-pixel runs per row of the rectangle
    long long units;            // runs
    long long grid;             // rays_grid(units * 64)
    int nInst;                  // instances of binding 9: the key of a miss, and the record it is counted in
    unsigned* records;          // `copies` private sets of nInst + 1 rz_instance_coverage (8 words each), strideWords apart, all
    int copies, strideWords;    //   empty; a workgroup sends its table to set blockIdx.x % copies; optional
    int tableCap;               // entries of a wave's table of groups, 1..64 (64; fewer: RZ_COVERAGE_TABLE, a test aid)
    int32_t* ids;               // width x height, optional
    unsigned* errWord;          // the context's backstop word
};
constexpr size_t RZ_COVERAGE_SCRATCH = (size_t)32 << 20;        // the most the private sets may take, and
constexpr int RZ_COVERAGE_SETS = 256;                           // the most there are (measured: profiles/coverage/README.md)
void launch_coverage_init(unsigned* sets, int copies, int strideWords, int count, hipStream_t stream);
void launch_coverage(const KParams& K, const CoverageLaunch& V, hipStream_t stream);
void launch_coverage_merge(unsigned* sets, int copies, int strideWords, unsigned* out, int count, hipStream_t stream);

// ---- rz_outline.hip
constexpr int RZ_OUTLINE_MAX_RADIUS = 4;        // rz_outline_params.radius: 1..4 (the halo the kernel stages)
struct OutlineLaunch {          // rz_outline_kernel
    const int32_t* ids;         // width x height
    const uint32_t* selected;   // (nInstances + 31) / 32 words
    unsigned long long nInstances;
    int width, height, radius;
    int tilesX;                 // (set by launch_outline)
    float color[3], alpha;
    uchar4* rgba8;              // images blended in place, each optional
    float* rgb;
};
void launch_outline(OutlineLaunch O, hipStream_t stream);

// ---- rz_lines.hip
constexpr int RZ_LINES_CELL = 128;              // pixels per side of a cell of the coarse lists
constexpr int RZ_LINES_SEG = 4096;              // lines a workgroup of the coarse pass scans: a cell's list is made by ceil(n / SEG) of them
constexpr size_t RZ_LINES_MAX = (size_t)1 << 20;        // lines per call
constexpr size_t RZ_LINES_DIRECT_BYTES = (size_t)4 << 20;   // a list workspace that is no larger even if every line meets every cell is
                                                            // taken whole, and the call never waits for the counts
struct LinesLaunch {            // rz_lines_project, rz_lines_bin, rz_lines_draw
    const void* lines;          // n x rz_line
    int n;
    const DevInstance* instances;   // step 1 reads fwd; nInst 0: no scene
    int nInst;
    float viewProj[16];         // proj * view, summed as rz_present's
    int width, height;
    float halfWidth;            // hw = width * 0.5f
    float nearW;
    float depthKeep;            // 1.0f - depth_bias
    float hiddenAlpha;
    int smooth;
    float4* geo;                // the projected records, n each: (A_s.x, A_s.y, ab.x, ab.y),
    float4* misc;               //   (ia, ib - ia, colour bits, L),
    float4* rect;               //   the cull rectangle (lox, loy, hix, hiy), empty for a dropped line,
    float* reach;               //   and what a cell or a tile adds to its own radius (rz_lines.hip: LINE CULL)
    int cellsX, cells;          // cells of RZ_LINES_CELL^2 pixels, row by row
    int nSeg;                   // ceil(n / RZ_LINES_SEG)
    unsigned* counts;           // cells x nSeg: lines of segment s that meet cell c at [c * nSeg + s]
    unsigned long long* offsets;    // their exclusive scan, cells * nSeg + 1 entries
    int* list;                  // the lists, offsets[cells * nSeg] indices; null: no lists, every tile walks all n lines
    const float4* hits;         // width x height rz_hit (3 float4), optional
    uchar4* rgba8;              // images blended in place, each optional
    float* rgb;
    int tilesX;                 // (set by launch_lines_draw)
};
void launch_lines_project(const LinesLaunch& V, hipStream_t stream);
void launch_lines_count(const LinesLaunch& V, hipStream_t stream);      // the counts and their scan
void launch_lines_fill(const LinesLaunch& V, hipStream_t stream);
void launch_lines_draw(LinesLaunch V, hipStream_t stream);

// ---- rz_ao.hip
constexpr int RZ_AO_DIRS = 256;                 // points of the direction table (rz_ao_directions)
constexpr int RZ_AO_COUNTERS = 256;              // the most counters rz_ao_walks' waves claim units from (128 B apart)
constexpr size_t RZ_AO_WALK_LDS = 2048;         // what rz_ao_walks keeps in LDS per wave beside the BLAS stack: 64 records of 32 B
const float* ao_direction_table();              // host: RZ_AO_DIRS x 3 floats, built on first use
struct AoWalkLaunch {           // rz_ao_walks (beside the KParams of camera_kparams)
    const float4* guide;        // DenoiseGuideLaunch::guide at the frame's size
    const float* dirs;          // device: the direction table
    float* raw;                 // width x height: raw_p, 1 for a miss
    int samples, log2Samples;   // N = 1, 2, 4, 8, 16
    float radius;
    int tilesX;                 // 8 x 8 tiles per row of tiles
    long long tiles;
    long long grid;             // rays_grid(tiles * 64)
    unsigned* claim;            // `counters` words, 32 words apart, zero when the kernel starts: the next unit of each sequence
    int counters;               // 1..RZ_AO_COUNTERS sequences of units, each with a counter; 0: a sequence per wave, no counter
    int perTrip;                // a unit is one trip of a tile, not a tile
    unsigned* errWord;          // the context's backstop word
};
struct AoResolveLaunch {        // rz_ao_resolve
    const float* raw;           // AoWalkLaunch::raw
    const float4* guide;        // smooth: the guide
    const float* rgbIn;         // width x height x 3, optional: (1, 1, 1)
    int width, height;
    float strength, normalCos, planeTol;
    float f;                    // 2 |inv_proj[5]| / height, rounded to binary32
    float* ao;                  // outputs, each optional
    float* rgb;
    uchar4* rgba8;
};
void launch_ao_walks(const KParams& K, const AoWalkLaunch& A, hipStream_t stream);
void launch_ao_resolve(const AoResolveLaunch& R, bool smooth, hipStream_t stream);

// ---- rz_adaptive.hip
constexpr unsigned RZ_ADAPTIVE_ACTIVE = 1u;     // a tile's flags: it still takes samples;
constexpr unsigned RZ_ADAPTIVE_CURRENT = 2u;    // it has received every batch so far
struct AdaptiveMeterLaunch {    // rz_adaptive_meter
    const float4* accum;        // the accumulation after batch `batch`
    float4* prev;               // tiles x 64, lane l of tile t at t * 64 + l: the accumulation after the tile's previous batch
    float2* moments;            // tiles x 64: (S1, S2)
    const int32_t* tiles;       // the nSlots tiles the batch rendered; null: tile k is slot k (batch 1)
    int nSlots;
    int width, height, tilesX;
    int spp, batch;             // s and B (1-based)
    int minBatches;
    float threshold, floor;
    float* tileError;           // per tile: E,
    int32_t* tileBatches;       //   the batches it has received (read unless batch is 1),
    uint8_t* tileFlags;         //   RZ_ADAPTIVE_ACTIVE | RZ_ADAPTIVE_CURRENT (read unless batch is 1)
};
void launch_adaptive_meter(const AdaptiveMeterLaunch& A, hipStream_t stream);

// ---- rz_present.hip
struct ProjBox;               // screen-space corners of one box (rz_present.hip)
struct PresentParams {
    const float4* accum;
    uchar4* rgba8;              // may be null
    float* rgb;                 // may be null: 3 floats per pixel, the colour before quantisation
    const TlasNode* tlasNodes;
    const int32_t* tlasIndices;
    const DevInstance* instances;
    const DevLight* lights;
    int width, height;
    int nTlasNodes, nInstances, nLights;
    float viewProj[16];         // projectionMatrix * viewMatrix
    float fps;
    int showFps, showLights, showBvh, bvhMode;
    int pathLen;                // bvhMode 1: nodes on the branch to the selected triangle
    float pathMin[32][3], pathMax[32][3];   // their object-space boxes
    float selTransform[16];     // the selected instance's transform
    ProjBox* boxes;             // screen-space corners of every box a pixel may have to draw, projected ONCE
};
void launch_present(const PresentParams& P, hipStream_t s);

}  // namespace rz

// rz_ctx_render.hip -- the frame of rz_set_frame on the render kernels (rz_kernels.hip): rz_render, rz_render_counted,
// rz_render_adaptive and its plan, and the timing ring of the render launches.  Host code; calls into rz_context.hip only
// through rz_ctx.h.
#include "rz_ctx.h"

using namespace rz;

namespace {

#ifndef RZ_WPOOL_CHUNK
#define RZ_WPOOL_CHUNK 256         // paths a wave collects across claims before it traces them together
#endif
#ifndef RZ_CLAIM_STRIDE_PAD
#define RZ_CLAIM_STRIDE_PAD 0      // extra dwords between the scratch regions of neighbouring resident waves
#endif

// One lane per sample: independent samples when no triangle is transparent, speculated currentIor otherwise
// (rz_kernels.hip).  The one-lane-per-pixel kernel remains as RZ_FLAG_MEGAKERNEL (the literal, sequential form).
bool use_samples(const rz_ctx* c) { return (c->flags & RZ_FLAG_MEGAKERNEL) == 0; }

// (evSlot: the pair of the ring that brackets the launch; negative: none -- rz_render_adaptive brackets its batches itself)
int render_samples(rz_ctx* c, KParams K, bool counted, int evSlot) {
    K.nSlots = K.nLocalTiles * 64;
    int rc = ensure_group_counter(c);
    if (rc != RZ_OK) return rc;
    K.groupCounter = static_cast<unsigned*>(c->dGroupCtr.p);
    // (16 waves per CU for the opaque variant = its VGPR limit, and for the transparent one too: 5.4 KB of versions leave it a
    // 9-entry window -- measured 40.2 -> 34.3 ms on the glass+mirror scene against 12 waves with the whole stack in LDS)
    const SamplesPlan plan = plan_render_samples(K.spp, K.nSlots, c->sceneHasTransparency);
#ifndef RZ_GLASS_WAVES_PER_CU
#define RZ_GLASS_WAVES_PER_CU 16
#endif
#ifndef RZ_OPAQUE_WAVES_PER_CU
#define RZ_OPAQUE_WAVES_PER_CU 16
#endif
    rc = size_blas_stack(c, K, samples_lds_extra(c->sceneHasTransparency, plan.compact) + (size_t)K.tlasStackCap * 256,
                         c->sceneHasTransparency ? RZ_GLASS_WAVES_PER_CU : RZ_OPAQUE_WAVES_PER_CU,
                         plan.perClaim > 0 ? plan.grid : 0, c->dBlasOvf);
    if (rc != RZ_OK) return rc;
    // Compacting launches: every resident wave's scratch (rz_kernels.hip: WAIT SLOTS, pool_process) --
    //   * its pool of parked paths: room for the chunk it collects before it traces them + the most one more claim can park;
    //   * its claim scratch (the addends of the claim it is running, 1.5 KB per unit) and behind it its wait slots, one waiting
    //     group's addends (batches x 1.5 KB) each: twice the groups of a claim by default (a claim that
    //     finds fewer free ones than it has groups makes the wave trace its pool first; RZ_WAIT_SLOTS overrides);
    //   * 2 ints of bookkeeping per slot.
    // C2: 80 + 12 + 24 KB per wave, 470 MiB for the grid (round 3: 3.7 GB, of which 3.2 GB an array of 1.5 KB per unit of the launch).
    // The scratch is optional: a launch that cannot have it (or is told so: RZ_DEBUG_NO_POOL_MEMORY=1, a test aid) runs the
    // plain persistent loop instead, same image.
    K.wslots = nullptr; K.wslotStride = 0; K.slotFloats = 0; K.nWaitSlots = 0; K.wmeta = nullptr; K.drainEachClaim = 0; K.claimUnits = 0; K.claimScratchFloats = 0;
    K.wpool = nullptr; K.wpoolStride = 0; K.wpoolChunk = 0;
    if (plan.compact && K.maxBounces < 32768) {     // (a pool entry keeps its path's bounce in 15 bits: rz_kernels.hip, BACK)
        long long chunk = RZ_WPOOL_CHUNK;
        if (const char* e = std::getenv("RZ_WPOOL_CHUNK")) chunk = std::max<long long>(1, std::atoll(e));      // tuning / test aid
        const int nBatches = (K.spp + 63) / 64;
        const int groupsPerClaim = std::max(1, plan.perClaim);
        // (twice a claim's groups: measured on the final build against 24 and 32 slots, C2 / C3 / C4 / C5 / glass all within
        //  0.4 % -- profiles/r04_wait_slots/slots_chunk_final.log -- and 24 KB per wave less to keep: C2's scratch 553 -> 470 MiB)
        int nSlots = std::max(2 * groupsPerClaim, 16 / nBatches);
        if (const char* e = std::getenv("RZ_WAIT_SLOTS")) nSlots = std::max(2 * groupsPerClaim, std::atoi(e));  // tuning / test aid
        nSlots = std::min(nSlots, 64);
        // a pool's capacity: what a wave may hold when it starts a pass -- fewer than `chunk` paths plus a whole claim's -- and what a
        // pass can ADD to that: nothing in an opaque scene (a path survives in place or ends); in a transparent one every sample on the
        // wave's late list (at most RZ_GLATE_CAP, listed in this pass or earlier ones) can be released into the pool behind the survivors
        const size_t stride = (size_t)chunk + (size_t)plan.claimUnits * 64 + 64 + (c->sceneHasTransparency ? (size_t)RZ_GLATE_CAP : 0);
        // (a group's addends; transparent scenes: + one row, the currentIor each pixel ends with)
        const size_t slotFloats = (size_t)nBatches * 384 + (c->sceneHasTransparency ? 64 : 0);
        const size_t claimScratchFloats = (size_t)groupsPerClaim * slotFloats;
        bool snapOn = true;                 // transparent scenes resolve currentIor from the samples' snapshots: no snapshots, no claims
        if (const char* e = std::getenv("RZ_GLASS_SNAPSHOT")) snapOn = std::atoi(e) != 0;
        size_t slotPad = 0;                                                                                      // floats between neighbouring waves' slot regions
        if (const char* e = std::getenv("RZ_SLOT_STRIDE_PAD")) slotPad = (size_t)std::max(0, std::atoi(e));     // tuning aid
        const char* forceNo = std::getenv("RZ_DEBUG_NO_POOL_MEMORY");      // test aid: as if the device had no room for it
        if (nSlots >= groupsPerClaim && !(forceNo && std::atoi(forceNo) != 0) && (!c->sceneHasTransparency || snapOn) &&
            ensure_optional(c->dWavePools, (size_t)plan.grid * stride * RZ_GPOOL_FIELDS * sizeof(unsigned)) &&
            ensure_optional(c->dClaimScratch, (size_t)plan.grid * (claimScratchFloats + nSlots * slotFloats + slotPad) * sizeof(float)) &&
            ensure_optional(c->dWaitMeta, (size_t)plan.grid * 4 * nSlots * sizeof(int32_t))) {
            K.wpool = static_cast<unsigned*>(c->dWavePools.p);
            K.wpoolStride = (uint32_t)stride;
            K.wpoolChunk = (uint32_t)chunk;
            K.wslots = static_cast<float*>(c->dClaimScratch.p);
            K.wslotStride = (uint32_t)(claimScratchFloats + nSlots * slotFloats + slotPad);
            K.claimUnits = plan.claimUnits;
            K.claimScratchFloats = (uint32_t)claimScratchFloats;
            K.glassBoxHint = 1;
            if (const char* e = std::getenv("RZ_GLASS_BOX_HINT")) K.glassBoxHint = std::atoi(e) != 0 ? 1 : 0;      // A/B and test aid
            K.slotFloats = (uint32_t)slotFloats;
            K.nWaitSlots = nSlots;
            K.wmeta = static_cast<int32_t*>(c->dWaitMeta.p);
            K.drainEachClaim = plan.drainEachClaim ? 1 : 0;
        }
    }
    c->lastGlobalPool = K.wpool != nullptr && K.drainEachClaim == 0;
    c->lastCompact = K.wpool != nullptr;
    c->lastScratchBytes = K.wpool ? (size_t)plan.grid * ((size_t)K.wpoolStride * RZ_GPOOL_FIELDS * 4 + (size_t)K.wslotStride * 4 + (size_t)16 * K.nWaitSlots) : 0;
    // transparent scenes, persistent launches: room for every resident wave's sample prefixes (19 + 14 dwords per lane, 34 MB for
    // the grid), so that a sample's second version starts at its first transparent scatter instead of at the camera.
    // RZ_GLASS_SNAPSHOT=0 switches it off (A/B aid: same image either way).
    K.snap = nullptr; K.snapStride = 0;
    if (c->sceneHasTransparency && plan.perClaim > 0) {
        bool on = true;
        if (const char* e = std::getenv("RZ_GLASS_SNAPSHOT")) on = std::atoi(e) != 0;
        const size_t stride = (size_t)(RZ_SNAP_FIELDS + RZ_SNAP_TALLY + RZ_GVER_ROWS) * 64 + (size_t)RZ_GLATE_FIELDS * RZ_GLATE_CAP;
        if (on) {
            rc = ensure(c, c->dSnap, (size_t)plan.grid * stride * sizeof(float));
            if (rc != RZ_OK) return rc;
            K.snap = static_cast<float*>(c->dSnap.p);
            K.snapStride = (uint32_t)stride;
        }
    }
    if (evSlot >= 0) RZ_HIP(c, hipEventRecord(c->evStart[evSlot], c->stream));
    if (K.nSlots > 0) launch_render_samples(K, counted, c->sceneHasTransparency, c->stream);
    if (evSlot >= 0) RZ_HIP(c, hipEventRecord(c->evStop[evSlot], c->stream));
    c->lastLaunches = K.nSlots > 0 ? 1 : 0;
    c->lastGrid = plan.grid;
    c->lastPlan = rz_launch_plan{plan.groups, plan.grid, plan.perClaim, (plan.compact && K.wpool) ? plan.claimUnits : 0,
                                 (K.spp + 63) / 64, K.spp >= 64 ? 1 : 64 / K.spp, K.blasStackCap, K.blasOvfCap,
                                 c->sceneHasTransparency ? 1 : 0, (int32_t)((c->lastScratchBytes + (1u << 20) - 1) >> 20)};
    return RZ_OK;
}

int do_render(rz_ctx* c, bool counted, rz_counters* out) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "rz_set_frame has not been called");
    RZ_HIP(c, hipSetDevice(c->device));
    int rc = finalize(c);
    if (rc != RZ_OK) return rc;
    const rz_frame_params& f = c->frame;
    const size_t nPix = (size_t)f.width * f.height;
    float4* accum = nullptr;
    if (c->extAccum) {
        if (c->extAccumBytes < nPix * 16) return fail(c, RZ_ERR_BUFFER_SIZE, "bound accumulation buffer holds %zu bytes, frame needs %zu", c->extAccumBytes, nPix * 16);
        accum = static_cast<float4*>(c->extAccum);
    } else {
        accum = static_cast<float4*>(c->ownAccum.p);
    }
    KParams K{};
    K.accum = accum;
    K.ior = static_cast<float*>(c->dIor.p);
    rc = frame_kparams(c, K, f.spp, f.sample_base);
    if (rc != RZ_OK) return rc;
    if (counted) {
        rc = ensure(c, c->dCounters, sizeof(DevCounters) + 160 * sizeof(unsigned long long));
        if (rc != RZ_OK) return rc;
        RZ_HIP(c, hipMemsetAsync(c->dCounters.p, 0, sizeof(DevCounters) + 160 * sizeof(unsigned long long), c->stream));
        K.counters = static_cast<DevCounters*>(c->dCounters.p);
    }
    // The event pair brackets the render kernels of this call (for the one-lane-per-sample path: the
    // rz_render_samples launches; its small ordered-sum kernel runs after the stop event when unchunked).
    const int slot = c->ringHead;
    if (use_samples(c)) {
        rc = render_samples(c, K, counted, slot);
        if (rc != RZ_OK) return rc;
        c->lastKernel = c->sceneHasTransparency ? (c->lastCompact ? "rz_render_samples<glass>+pool" : "rz_render_samples<glass>")
                                                : (c->lastGlobalPool ? "rz_render_samples+pool" : "rz_render_samples");
    } else {
        RZ_HIP(c, hipEventRecord(c->evStart[slot], c->stream));
        launch_render_pixels(K, counted, c->stream);
        RZ_HIP(c, hipEventRecord(c->evStop[slot], c->stream));
        c->lastLaunches = 1;
        c->lastKernel = "rz_render_pixels";
        c->lastPlan = rz_launch_plan{K.nLocalTiles, K.nLocalTiles, 0, 0, (K.spp + 63) / 64, 64, K.blasStackCap, 0, c->sceneHasTransparency ? 1 : 0, 0};
    }
    RZ_HIP(c, hipGetLastError());
    c->ringHead = (slot + 1) % rz_ctx::kRing;
    c->ringCount = std::min(c->ringCount + 1, (int)rz_ctx::kRing);
    c->timed = true;
    if (counted && out) {
        DevCounters h{};
        RZ_HIP(c, hipMemcpyAsync(&h, c->dCounters.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
        RZ_HIP(c, hipStreamSynchronize(c->stream));
        out->samples = h.samples; out->traversals = h.traversals; out->tlas_nodes = h.tlas_nodes;
        out->tlas_leaf_indices = h.tlas_leaf_indices; out->instances = h.instances; out->blas_nodes = h.blas_nodes;
        out->triangles = h.triangles; out->materials = h.materials; out->light_fetches = h.light_fetches;
        out->pixels = h.pixels;
        out->scatters = h.scatters; out->diffuse_scatters = h.diffuse_scatters; out->hemi_draws = h.hemi_draws; out->lit_lights = h.lit_lights; out->triangles_past_u = h.triangles_past_u;
#ifdef RZ_PROF
        unsigned long long pr[160];
        RZ_HIP(c, hipMemcpy(pr, static_cast<char*>(c->dCounters.p) + sizeof(DevCounters), sizeof pr, hipMemcpyDeviceToHost));
        for (int r = 0; r < 8; ++r) {       // per query round of a path: 0 primary, 1-2 shadow, 3 first bounce, ...
            const unsigned long long* q = pr + 32 + 11 * r;
            auto avg = [](unsigned long long l, unsigned long long e) { return e ? (double)l / (double)e : 0.0; };
            fprintf(stderr, "[rz_prof] round %d: queries %10llu x %4.1f lanes | descend steps %11llu x %4.1f (uniform %11llu) | triangle tests %11llu x %4.1f | instance entries %10llu x %4.1f | trace wave-cycles %llu\n",
                    r, q[8], avg(q[9], q[8]), q[0], avg(q[1], q[0]), q[6], q[2], avg(q[3], q[2]), q[4], avg(q[5], q[4]), q[10]);
        }
        dump_wave_log(use_samples(c) ? (int)std::min<long long>(c->lastGrid, 1 << 17) : K.nLocalTiles);
        static const char* namesPx[] = {"blas loop iter", "leaf branch", "triangle test", "internal branch", "tlas pop", "instance enter", "outer iter", "uniform pair"};
        const char** names = namesPx;
        for (int k = 0; k < 8; ++k)
            fprintf(stderr, "[rz_prof] %-16s wave-execs %12llu  lanes %14llu  avg active lanes %.1f\n", names[k], pr[2 * k], pr[2 * k + 1], pr[2 * k] ? (double)pr[2 * k + 1] / (double)pr[2 * k] : 0.0);
        fprintf(stderr, "[rz_prof] wave cycles: begin %llu  trace %llu  advance %llu | inside trace: descend loops %llu  leaf phases %llu  whole BLAS walks %llu\n", pr[16], pr[17], pr[18], pr[19], pr[20], pr[21]);
        fprintf(stderr, "[rz_prof] compacting claims: phase 1 (units) %llu  pool rounds %llu wave cycles; %llu rounds with %llu paths = %.1f lanes per round\n", pr[23], pr[28], pr[29], pr[30], pr[29] ? (double)pr[30] / (double)pr[29] : 0.0);
        fprintf(stderr, "[rz_prof] cross-claim pools: %llu traced, %llu queries in them, shade rounds %llu wave cycles\n", pr[29], pr[30], pr[28]);
        fprintf(stderr, "[rz_prof] pool_trace (a claim's pooled queries traced together): %llu wave cycles = T phases %llu + B phases %llu (of which refills %llu); round 7 above = its steps\n", pr[120], pr[121], pr[122], pr[123]);
        fprintf(stderr, "[rz_prof] descend steps of the general (per-lane) walk by children entered: none %llu  one %llu  both %llu (lane-level; the scalar-unit steps are not in here); in the pools' walks: none %llu  one %llu  both %llu\n", pr[132], pr[133], pr[134], pr[136], pr[137], pr[138]);
        fprintf(stderr, "[rz_prof] wait slots: end-of-claim sections %llu wave cycles (of which the claim-end sums %llu); slot_sums inside pool_process %llu\n", pr[124], pr[126], pr[125]);
        // (this build's counted frame takes the shortcut, as the product's uncounted one does: rz_path.h, shadow_exit)
        for (int r = 0; r < 3; ++r) {
            const unsigned long long* q = pr + 140 + 6 * r;
            fprintf(stderr, "[rz_prof] shadow exit, round %d%s: eligible queries %llu | walks cut short %llu | refused: hit within 2 EPS %llu, not clearly nearer than the light %llu | held %llu | traced again %llu\n",
                    r + 1, r == 2 ? " and later" : "", q[0], q[1], q[2], q[3], q[4], q[5]);
        }
        fprintf(stderr, "[rz_prof] inside advance: sky %llu  hit %llu  start_light %llu  shade_light %llu  scatter %llu (hemisphere %llu)  shadow step %llu\n", pr[22], pr[23], pr[24], pr[25], pr[26], pr[27], pr[28]);
#endif
    }
    return RZ_OK;
}

// ---- rz_render_adaptive / rz_adaptive_plan (rz_adaptive.hip; include/rayzen_hip.h states the rule) -----------------------------
// The runs of the next batch.  A merge changes no other gap, so step 3's "smallest all-current gap first, lowest index among
// equals" is a stable sort of the gaps step 2 left open.
void adaptive_plan(const uint8_t* active, const uint8_t* current, size_t n, int mergeGap, int maxRuns, std::vector<rz_tile_run>& out) {
    out.clear();
    for (size_t i = 0; i < n;) {
        if (!active[i]) { ++i; continue; }
        size_t j = i;
        while (j < n && active[j]) ++j;
        out.push_back(rz_tile_run{(int32_t)i, (int32_t)(j - i)});
        i = j;
    }
    if (out.size() < 2) return;
    std::vector<char> join(out.size() - 1, 0);
    std::vector<std::pair<int32_t, int32_t>> open;          // (length, the run in front) of the all-current gaps step 2 leaves
    size_t runs = out.size();
    for (size_t k = 0; k + 1 < out.size(); ++k) {
        const int32_t g0 = out[k].first + out[k].len, g1 = out[k + 1].first;
        bool allCurrent = true;
        for (int32_t t = g0; t < g1 && allCurrent; ++t) allCurrent = current[t] != 0;
        if (!allCurrent) continue;
        if (g1 - g0 <= mergeGap) { join[k] = 1; --runs; }
        else open.emplace_back(g1 - g0, (int32_t)k);
    }
    if (runs > (size_t)maxRuns) {
        std::stable_sort(open.begin(), open.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (size_t k = 0; k < open.size() && runs > (size_t)maxRuns; ++k, --runs) join[open[k].second] = 1;
    }
    size_t w = 0;
    for (size_t k = 1; k < out.size(); ++k) {
        if (join[k - 1]) out[w].len = out[k].first + out[k].len - out[w].first;
        else out[++w] = out[k];
    }
    out.resize(w + 1);
}

// The frame of rz_set_frame in batches of s samples over runs of tiles.  Every launch is a launch of do_render's kernels with
// three fields of its KParams overridden -- tileNRanks 1, tileRank the run's first tile, nLocalTiles its length -- which
// render_samples and launch_render_pixels size everything else from; sampleBase continues the pixels from the accumulation and
// currentIor.  The launches record no event pair of the ring, which therefore keeps the renders' history.
int render_adaptive(rz_ctx* c, const rz_adaptive_params* pp, rz_adaptive_info* info, int32_t* tileBatches, size_t tileBatchesBytes,
                    float* tileError, size_t tileErrorBytes) {
    const char* what = "rz_render_adaptive";
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null context", what);
    rz_adaptive_params P{};
    if (pp) P = *pp;
    if (P.flags & ~RZ_ADAPTIVE_HOST) return fail(c, RZ_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, P.flags);
    if (P.batch_spp == 0) P.batch_spp = 8;
    if (P.min_batches == 0) P.min_batches = 4;
    if (P.max_batches == 0) P.max_batches = std::max(8, P.min_batches);
    if (P.threshold == 0.0f) P.threshold = 0.02f;
    if (P.luminance_floor == 0.0f) P.luminance_floor = 0.01f;
    if (P.merge_gap == 0) P.merge_gap = 8;
    if (P.max_runs == 0) P.max_runs = 1;         // (every further launch of a batch cost more than it saved: profiles/adaptive/README.md)
    if (P.batch_spp < 1 || P.batch_spp > 1024) return fail(c, RZ_ERR_INVALID_ARG, "%s: batch_spp %d outside 1..1024", what, P.batch_spp);
    if (P.min_batches < 2 || P.min_batches > RZ_ADAPTIVE_MAX_BATCHES)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: min_batches %d outside 2..%d", what, P.min_batches, RZ_ADAPTIVE_MAX_BATCHES);
    if (P.max_batches < P.min_batches || P.max_batches > RZ_ADAPTIVE_MAX_BATCHES)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: max_batches %d outside %d..%d", what, P.max_batches, P.min_batches, RZ_ADAPTIVE_MAX_BATCHES);
    if (P.threshold != P.threshold) return fail(c, RZ_ERR_INVALID_ARG, "%s: threshold is not a number", what);
    if (!(P.luminance_floor > 0.0f && P.luminance_floor < INFINITY))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: luminance_floor %g (finite, > 0)", what, (double)P.luminance_floor);
    if (P.merge_gap < -1) return fail(c, RZ_ERR_INVALID_ARG, "%s: merge_gap %d (-1: none, 0: the default, or a number of tiles)", what, P.merge_gap);
    if (P.max_runs < 0) return fail(c, RZ_ERR_INVALID_ARG, "%s: max_runs %d", what, P.max_runs);
    const int mergeGap = std::max(0, P.merge_gap);
    const bool host = (P.flags & RZ_ADAPTIVE_HOST) != 0;
    if (!host && ((reinterpret_cast<uintptr_t>(tileBatches) | reinterpret_cast<uintptr_t>(tileError)) & 3u))
        return fail(c, RZ_ERR_INVALID_ARG, "%s: device pointers must be 4-byte aligned", what);
    if (!c->haveFrame) return fail(c, RZ_ERR_NOT_READY, "%s: rz_set_frame has not been called", what);
    const rz_frame_params& f = c->frame;
    if (f.tile_nranks > 1)
        return fail(c, RZ_ERR_INVALID_ARG, "%s: the frame is tile %d of %d; an adaptive frame is rendered whole", what, f.tile_rank, f.tile_nranks);
    const int tilesX = (f.width + RZ_TILE_W - 1) / RZ_TILE_W, tilesY = (f.height + RZ_TILE_H - 1) / RZ_TILE_H;
    const int nTiles = tilesX * tilesY;
    const size_t nPix = (size_t)f.width * f.height;
    if (tileBatches && tileBatchesBytes < (size_t)nTiles * 4)
        return fail(c, RZ_ERR_BUFFER_SIZE, "%s: tile_batches needs %zu bytes, got %zu", what, (size_t)nTiles * 4, tileBatchesBytes);
    if (tileError && tileErrorBytes < (size_t)nTiles * 4)
        return fail(c, RZ_ERR_BUFFER_SIZE, "%s: tile_error needs %zu bytes, got %zu", what, (size_t)nTiles * 4, tileErrorBytes);
    if (c->extAccum && c->extAccumBytes < nPix * 16)
        return fail(c, RZ_ERR_BUFFER_SIZE, "%s: bound accumulation buffer holds %zu bytes, frame needs %zu", what, c->extAccumBytes, nPix * 16);
    RZ_HIP(c, hipSetDevice(c->device));
    int rc = finalize(c);
    if (rc != RZ_OK) return rc;
    KParams K{};
    K.accum = static_cast<float4*>(c->extAccum ? c->extAccum : c->ownAccum.p);
    K.ior = static_cast<float*>(c->dIor.p);
    rc = frame_kparams(c, K, P.batch_spp, 0);
    if (rc == RZ_OK) rc = ensure(c, c->dAdPrev, (size_t)nTiles * 64 * sizeof(float4));
    if (rc == RZ_OK) rc = ensure(c, c->dAdMoments, (size_t)nTiles * 64 * sizeof(float2));
    if (rc == RZ_OK) rc = ensure(c, c->dAdError, (size_t)nTiles * sizeof(float));
    if (rc == RZ_OK) rc = ensure(c, c->dAdBatches, (size_t)nTiles * sizeof(int32_t));
    if (rc == RZ_OK) rc = ensure(c, c->dAdFlags, (size_t)nTiles);
    if (rc == RZ_OK) rc = ensure(c, c->dAdList, (size_t)nTiles * sizeof(int32_t));
    if (rc != RZ_OK) return rc;
    // pinned: the tiles' flags as they come back, then the list of the tiles a batch rendered as it goes up
    const size_t listOff = ((size_t)nTiles + 15) & ~size_t(15), pinnedBytes = listOff + (size_t)nTiles * sizeof(int32_t);
    if (c->adPinnedCap < pinnedBytes) {
        if (c->adPinned) (void)hipHostFree(c->adPinned);
        c->adPinned = nullptr; c->adPinnedCap = 0;
        RZ_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->adPinned), pinnedBytes, hipHostMallocDefault));
        c->adPinnedCap = pinnedBytes;
    }
    for (hipEvent_t* e : {&c->evAdaptive[0], &c->evAdaptive[1], &c->evAdaptive[2]})
        if (!*e) RZ_HIP(c, hipEventCreate(e));
    const uint8_t* hFlags = c->adPinned;
    int32_t* hList = reinterpret_cast<int32_t*>(c->adPinned + listOff);

    AdaptiveMeterLaunch M{};
    M.accum = K.accum;
    M.prev = static_cast<float4*>(c->dAdPrev.p);
    M.moments = static_cast<float2*>(c->dAdMoments.p);
    M.width = f.width; M.height = f.height; M.tilesX = tilesX;
    M.spp = P.batch_spp;
    M.minBatches = P.min_batches;
    M.threshold = P.threshold; M.floor = P.luminance_floor;
    M.tileError = static_cast<float*>(c->dAdError.p);
    M.tileBatches = static_cast<int32_t*>(c->dAdBatches.p);
    M.tileFlags = static_cast<uint8_t*>(c->dAdFlags.p);

    auto tilePixels = [&](int t) {
        const int tx = t % tilesX, ty = t / tilesX;
        return (uint64_t)(std::min<int>(RZ_TILE_W, f.width - tx * RZ_TILE_W) * std::min<int>(RZ_TILE_H, f.height - ty * RZ_TILE_H));
    };
    rz_adaptive_info I{};
    I.n_tiles = nTiles;
    I.samples_uniform = (uint64_t)nPix * (uint64_t)P.max_batches * (uint64_t)P.batch_spp;
    alloc_point(c);
    std::vector<uint8_t> active((size_t)nTiles, 1), current((size_t)nTiles, 1), rendered((size_t)nTiles, 1);
    std::vector<rz_tile_run> runs(1, rz_tile_run{0, nTiles});
    for (int B = 1;; ++B) {
        RZ_HIP(c, hipEventRecord(c->evAdaptive[0], c->stream));
        int nRendered = 0;
        for (const rz_tile_run& r : runs) {
            KParams KR = K;
            KR.sampleBase = (B - 1) * P.batch_spp;
            KR.tileNRanks = 1; KR.tileRank = r.first; KR.nLocalTiles = r.len;
            if (use_samples(c)) {
                rc = render_samples(c, KR, false, -1);
                if (rc != RZ_OK) return rc;
            } else {
                launch_render_pixels(KR, false, c->stream);
                c->lastLaunches = 1;
                c->lastPlan = rz_launch_plan{KR.nLocalTiles, KR.nLocalTiles, 0, 0, (KR.spp + 63) / 64, 64, KR.blasStackCap, 0, c->sceneHasTransparency ? 1 : 0, 0};
            }
            RZ_HIP(c, hipGetLastError());
            if (B > 1) for (int t = r.first; t < r.first + r.len; ++t) { hList[nRendered++] = t; rendered[t] = 1; }
            else nRendered += r.len;
        }
        RZ_HIP(c, hipEventRecord(c->evAdaptive[1], c->stream));
        M.batch = B;
        M.nSlots = nRendered;
        M.tiles = nullptr;
        if (nRendered < nTiles) {       // (a batch of the whole frame needs no list: tile k is slot k)
            RZ_HIP(c, hipMemcpyAsync(c->dAdList.p, hList, (size_t)nRendered * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            M.tiles = static_cast<const int32_t*>(c->dAdList.p);
        }
        launch_adaptive_meter(M, c->stream);
        RZ_HIP(c, hipGetLastError());
        RZ_HIP(c, hipEventRecord(c->evAdaptive[2], c->stream));
        RZ_HIP(c, hipMemcpyAsync(c->adPinned, c->dAdFlags.p, (size_t)nTiles, hipMemcpyDeviceToHost, c->stream));
        RZ_HIP(c, hipStreamSynchronize(c->stream));
        float msRender = 0.0f, msMeter = 0.0f;
        RZ_HIP(c, hipEventElapsedTime(&msRender, c->evAdaptive[0], c->evAdaptive[1]));
        RZ_HIP(c, hipEventElapsedTime(&msMeter, c->evAdaptive[1], c->evAdaptive[2]));
        I.render_ms += msRender; I.meter_ms += msMeter;
        int nActive = 0;
        for (int t = 0; t < nTiles; ++t) {
            if (rendered[t]) {
                active[t] = (hFlags[t] & RZ_ADAPTIVE_ACTIVE) != 0;
                current[t] = (hFlags[t] & RZ_ADAPTIVE_CURRENT) != 0;
                I.samples_traced += tilePixels(t) * (uint64_t)P.batch_spp;
            } else {
                current[t] = 0;
            }
            nActive += active[t];
            rendered[t] = 0;
        }
        I.batches = B;
        I.tiles_active[B - 1] = nActive;
        I.tiles_rendered[B - 1] = nRendered;
        I.runs[B - 1] = (int32_t)runs.size();
        if (nActive == 0 || B == P.max_batches) break;
        adaptive_plan(active.data(), current.data(), (size_t)nTiles, mergeGap, P.max_runs, runs);
    }
    c->lastKernel = !use_samples(c) ? "rz_render_pixels"
                  : c->sceneHasTransparency ? (c->lastCompact ? "rz_render_samples<glass>+pool" : "rz_render_samples<glass>")
                                            : (c->lastGlobalPool ? "rz_render_samples+pool" : "rz_render_samples");
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (tileBatches) RZ_HIP(c, hipMemcpyAsync(tileBatches, c->dAdBatches.p, (size_t)nTiles * 4, kind, c->stream));
    if (tileError) RZ_HIP(c, hipMemcpyAsync(tileError, c->dAdError.p, (size_t)nTiles * 4, kind, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    if (info) *info = I;
    return RZ_OK;
}

}  // namespace

extern "C" {

int rz_render(rz_ctx* c) {
    return guarded(c, "rz_render", [&] { return do_render(c, false, nullptr); });
}
int rz_render_counted(rz_ctx* c, rz_counters* out) {
    return guarded(c, "rz_render_counted", [&] { return do_render(c, true, out); });
}
int rz_render_adaptive(rz_ctx* c, const rz_adaptive_params* params, rz_adaptive_info* info, int32_t* tile_batches,
                       size_t tile_batches_bytes, float* tile_error, size_t tile_error_bytes) {
    return guarded(c, "rz_render_adaptive", [&] {
        return render_adaptive(c, params, info, tile_batches, tile_batches_bytes, tile_error, tile_error_bytes);
    });
}
int rz_adaptive_plan(const uint8_t* active, const uint8_t* current, size_t n_tiles, int merge_gap, int max_runs, rz_tile_run* runs,
                     size_t cap, size_t* n_runs) {
    const char* what = "rz_adaptive_plan";
    if (!n_runs) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null n_runs", what);
    if ((!active || !current) && n_tiles > 0) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null active or current", what);
    if (!runs && cap > 0) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: null runs", what);
    if (merge_gap < 0 || max_runs < 1) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: merge_gap %d, max_runs %d", what, merge_gap, max_runs);
    if (n_tiles > ((size_t)1 << 30)) return fail(nullptr, RZ_ERR_INVALID_ARG, "%s: %zu tiles, at most 2^30", what, n_tiles);
    return guarded(nullptr, what, [&]() -> int {
        std::vector<rz_tile_run> out;
        adaptive_plan(active, current, n_tiles, merge_gap, max_runs, out);
        *n_runs = out.size();
        if (out.size() > cap) return fail(nullptr, RZ_ERR_BUFFER_SIZE, "%s: %zu runs, room for %zu", what, out.size(), cap);
        if (!out.empty()) std::memcpy(runs, out.data(), out.size() * sizeof(rz_tile_run));
        return RZ_OK;
    });
}

int rz_last_render_ms(rz_ctx* c, float* ms, int* launches) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (!c->timed) return fail(c, RZ_ERR_NOT_READY, "nothing rendered yet");
    return guarded(c, "rz_last_render_ms", [&]() -> int {
        const int slot = (c->ringHead + rz_ctx::kRing - 1) % rz_ctx::kRing;
        RZ_HIP(c, hipEventSynchronize(c->evStop[slot]));
        float t = 0.0f;
        RZ_HIP(c, hipEventElapsedTime(&t, c->evStart[slot], c->evStop[slot]));
        if (ms) *ms = t;
        if (launches) *launches = c->lastLaunches;
        return RZ_OK;
    });
}

const char* rz_last_kernel_name(const rz_ctx* c) { return c ? c->lastKernel : ""; }

int rz_render_history_ms(rz_ctx* c, float* ms, int cap) {
    if (!c) return fail(nullptr, RZ_ERR_INVALID_ARG, "null context");
    if (cap < 0 || (cap > 0 && !ms)) return fail(c, RZ_ERR_INVALID_ARG, "bad history buffer");
    return guarded(c, "rz_render_history_ms", [&]() -> int {
        const int n = std::min(c->ringCount, cap);
        for (int i = 0; i < n; ++i) {     // oldest of the last n first
            const int slot = (c->ringHead + 2 * rz_ctx::kRing - n + i) % rz_ctx::kRing;
            RZ_HIP(c, hipEventSynchronize(c->evStop[slot]));
            RZ_HIP(c, hipEventElapsedTime(&ms[i], c->evStart[slot], c->evStop[slot]));
        }
        c->ringCount = 0;
        return n;
    });
}

}  // extern "C"

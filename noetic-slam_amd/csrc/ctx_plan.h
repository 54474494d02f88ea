// ctx_plan.h -- what tsdf_create decides before it allocates (tsdf_capi.cpp): whether the params
// are valid, the band a ray's walk covers, the per-ray slot bounds and the sizes of one batch.
// Pure integer and double arithmetic on tsdf_params.  Plain C++ like host_pack.h, checked and
// sanitized on the CPU (tests/test_ctx_plan.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/tsdf_hip.h"

namespace tsdf {

// The device constants the plan depends on (tsdf_device.h: RPB, MAX_BATCH, WLK_THREADS, SPAN,
// VOX_LIMIT), handed in by the caller so that this header needs no device header
struct PlanConsts { uint32_t rpb, max_batch, wlk_threads, span; int vox_limit; };

// What tsdf_create accepts; anything else is TSDF_EINVAL, with no text.
inline bool params_valid(const tsdf_params& p) {
    return p.voxel_size > 0 && p.sdf_trunc > 0 && p.brick_side == TSDF_BRICK_SIDE &&
           p.weight_mode == TSDF_WEIGHT_CONSTANT && p.max_bricks != 0 &&
           p.max_bricks < 0xFFFFFFF0ull && p.max_points != 0 && p.min_range >= 0 &&
           p.max_range > p.min_range && p.max_batch != 0 && p.max_batch <= TSDF_MAX_BATCH &&
           (p.semantics == TSDF_SEM_VDBFUSION || p.semantics == TSDF_SEM_VOXBLOX ||
            p.semantics == TSDF_SEM_VDBFUSION_F64) &&
           (p.semantics != TSDF_SEM_VOXBLOX || p.max_weight > 0.0f) &&
           (p.voxblox_method == TSDF_VB_SIMPLE || p.voxblox_method == TSDF_VB_MERGED) &&
           p.sector_input >= TSDF_SECTOR_INPUT_FANOUT && p.sector_input <= TSDF_SECTOR_INPUT_SPLIT &&
           (p.sector_rule == TSDF_SECTOR_RULE_WORLD || p.sector_rule == TSDF_SECTOR_RULE_INDEX) &&
           (p.n_sectors <= 1 || p.sector < p.n_sectors) && std::isfinite(p.sector_yaw0) &&
           (!p.max_bricks_hard || p.max_bricks_hard >= p.max_bricks) &&
           (!p.space_carving || std::isfinite(p.max_range));
}

// The kernels' semantics: TSDF_SEM_*, or 3 for Voxblox with per-sample weights (the 1/z^2 weight;
// MergedTsdfIntegrator, whose bundles carry summed weights)
inline bool plan_merged(const tsdf_params& p) {
    return p.semantics == TSDF_SEM_VOXBLOX && p.voxblox_method == TSDF_VB_MERGED;
}
inline int plan_sem(const tsdf_params& p) {
    const bool depth_w = p.semantics == TSDF_SEM_VOXBLOX && p.depth_weight;
    return depth_w || plan_merged(p) ? 3 : p.semantics;
}

// Band length in voxels along the ray: the truncation band around the hit, and what a ray's walk
// covers (with space carving, from the sensor's max_range to behind the hit).
inline double trunc_band_voxels(const tsdf_params& p) { return 2.0 * p.sdf_trunc / p.voxel_size; }
inline double band_voxels(const tsdf_params& p) {
    return p.space_carving ? (p.max_range + p.sdf_trunc) / p.voxel_size : trunc_band_voxels(p);
}

// Pair slots per ray: the distinct bricks a DDA over the band can visit.  A segment of length L
// (voxels) covers at most E = floor(L) + 2 cells along an axis, E cells cross at most
// floor((E - 1) / 8) + 1 brick boundaries, and a line crosses them monotonically, one axis per
// step: 1 + 3 * crossings bricks.  (A 6-voxel band: 4.)  Exceeding it is reported (OVF_PAIRS).
inline uint32_t pairs_per_ray(const tsdf_params& p) {
    const double e = std::floor(band_voxels(p)) + 2.0;
    const double crossings = std::floor((e - 1.0) / TSDF_BRICK_SIDE) + 1.0;
    return (uint32_t)(1.0 + 3.0 * crossings);
}

// Sample slots per ray: a ray's gated voxels are among its DDA voxels, at most
// 1 + 3 (floor(band) + 2).  (A 6-voxel band: 25.  The doubles 0.05 and 0.15 give 2 * 0.15 / 0.05 =
// 5.999..., as do the floats the kernels gate with: 22.)
inline uint32_t samples_per_ray(const tsdf_params& p) {
    return (uint32_t)(1.0 + 3.0 * (std::floor(band_voxels(p)) + 2.0));
}

// The smallest double x >= 0 with (float)sqrt(x) >= tau (bisection over the ordered bit patterns
// of non-negative doubles): behind the hit, VDBFusion's gate -(float)dist > -tau holds iff
// d2 < this threshold (TSDF_SEM_VDBFUSION_F64; the oracle gates on the sqrt itself).
inline double gate_threshold(float tau) {
    auto ok = [&](uint64_t b) {
        double x;
        std::memcpy(&x, &b, 8);
        return (float)std::sqrt(x) >= tau;
    };
    double hi_d = 4.0 * (double)tau * (double)tau + 1.0;
    uint64_t lo = 0, hi;
    std::memcpy(&hi, &hi_d, 8);
    while (hi - lo > 1) {  // ok(lo) false, ok(hi) true
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ok(mid)) hi = mid;
        else lo = mid;
    }
    double x;
    std::memcpy(&x, &hi, 8);
    return x;
}

// One batch's sizes.  refusal: why no context can be created with these params (TSDF_EINVAL), or
// empty; the sizes after the refusing step are then unset.
struct CtxPlan {
    uint32_t maxp = 0, spr = 0;  // pair and sample slots per ray
    int band_vox = 0;            // RayConst::band_vox
    // single walk: k_walk + k_spans instead of k_count + k_place, when asked for
    // (tsdf_params.walk) and the band's walk fits nstep register slots per ray
    bool fused = false;
    int nstep = 0;
    uint64_t batch_points = 0, slots = 0;  // points one batch may hold; its pair slots
    // k_count / k_place workgroups it may need; Table::cell_stride
    uint32_t max_blocks = 0, cell_stride = 0;
    uint32_t max_smp = 0, max_spn = 0, max_fb = 0;  // entries of the growable lists at create
    std::string refusal;
};

inline CtxPlan ctx_plan(const tsdf_params& p, const PlanConsts& K) {
    CtxPlan P;
    auto refuse = [&P](const char* fmt, auto... a) {
        char text[256];
        std::snprintf(text, sizeof text, fmt, a...);
        P.refusal = text;
        return P;
    };
    P.band_vox = (int)std::min(std::ceil(band_voxels(p)) + 4.0, (double)(K.vox_limit / 2));
    // Points one batch may hold: max_batch full scans, unless the per-ray worst cases (pair slots,
    // sample slots — large with space carving) exceed the u32 index space or the sample budget;
    // the host queue then cuts batches by points.  A single scan must always fit.
    P.maxp = pairs_per_ray(p);
    P.spr = samples_per_ray(p);
    uint64_t bp = p.max_points * p.max_batch;
    bp = std::min<uint64_t>(bp, 0xFFFFFFF0ull / P.maxp);
    if (p.max_pairs) bp = std::min<uint64_t>(bp, p.max_pairs / P.maxp);  // caller-imposed cap
    if (bp < p.max_points)
        return refuse("max_points %llu exceeds what one batch can hold (%llu: %u pair and %u sample "
                      "slots per ray)", (unsigned long long)p.max_points, (unsigned long long)bp,
                      P.maxp, P.spr);
    // Single walk: k_walk keeps a ray's samples in one register slot per DDA step,
    // so the band's walk must have a proven bound: a segment of L voxels crosses at most
    // floor(L |u_a|) + 1 boundaries per axis, i.e. visits <= sqrt(3) L + 4 voxels.  Carving and
    // Voxblox clearing rays (length up to max_range) keep the two-walk path, the default.
    const double steps = std::floor(std::sqrt(3.0) * trunc_band_voxels(p) * (1.0 + 1e-4)) + 5.0;
    const bool clearing = p.semantics == TSDF_SEM_VOXBLOX && p.allow_clear && std::isfinite(p.max_range);
    P.fused = p.walk == TSDF_WALK_SINGLE && !p.space_carving && !clearing && P.maxp <= 4 &&
              plan_sem(p) != 3 && steps <= 32.0;
    P.nstep = steps <= 16.0 ? 16 : 32;
    const uint64_t stg = (uint64_t)K.wlk_threads * (uint64_t)P.nstep;  // samples per k_walk region
    if (P.fused) {
        // the span record addresses 2^30 samples: at most 2^30 / stg k_walk workgroups per batch
        const uint64_t lim = ((1ull << 30) / (2 * stg) - K.max_batch - 1) * K.rpb;
        bp = std::min<uint64_t>(bp, lim);
        if (bp < p.max_points)
            return refuse("max_points %llu exceeds a single-walk batch (%llu)",
                          (unsigned long long)p.max_points, (unsigned long long)bp);
    }
    P.batch_points = bp;
    P.slots = bp * P.maxp;
    P.max_blocks = (uint32_t)(bp / K.rpb + K.max_batch + 1);
    const uint32_t nsec = std::max<uint32_t>(1u, p.n_sectors);
    if (P.fused) {
        // 64-bit cells and a totals cell after the last scan; the pair and fallback lists are not
        // used; one region of stg samples per k_walk workgroup (sharded: this GPU's share of the
        // blocks, grown on OVF_SMP); span records ~ samples / SPAN + one partial span per run
        P.cell_stride = (p.max_batch + 2u) & ~1u;
        const uint64_t reg_blocks = nsec > 1 ? std::min<uint64_t>(
            P.max_blocks, P.max_blocks * 5ull / (4ull * nsec) + 2ull * p.max_batch + 64) : P.max_blocks;
        P.max_smp = (uint32_t)std::min<uint64_t>(2 * reg_blocks * stg, 1ull << 30);
        P.max_spn = (uint32_t)std::min<uint64_t>(
            bp * P.spr / K.span / nsec + 2 * reg_blocks * 256, 0xFFFFFFF0ull);
        P.max_fb = 4;
    } else {
        // sample list: the worst case (spr per ray) of the rays a context keeps — 1 / n_sectors of
        // them when sharded — capped at 2^30 samples (8 GiB); an overflow grows it (OVF_SMP,
        // DESIGN.md §4b)
        const uint64_t smp_budget = 1ull << 30;
        P.cell_stride = (p.max_batch + 3u) & ~3u;
        P.max_smp = (uint32_t)std::min<uint64_t>(
            std::min<uint64_t>(bp * P.spr / nsec, smp_budget), 0xFFFFFFF0ull);
        // fallback pairs (a workgroup's LDS brick hash is full): rare without carving, the rule with
        // it (the fallback index has 26 bits; past it pairs are dropped and OVF_FB reported)
        P.max_fb = (uint32_t)std::min<uint64_t>(
            p.space_carving ? P.slots : std::max<uint64_t>(P.slots / 16, 1u << 20), 1u << 26);
        P.max_spn = 4;
    }
    return P;
}

}  // namespace tsdf

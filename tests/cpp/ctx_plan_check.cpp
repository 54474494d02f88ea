// Check of the context's sizing plan (noetic-slam_amd/csrc/ctx_plan.h) on the CPU:
//   * ctx_plan against a straight-line restatement of the arithmetic tsdf_create used before the
//     plan had a header of its own, field by field, refusals and their texts included, over a grid:
//     voxel 0.02 / 0.05 / 0.10; trunc 1-6 voxels; carving off, and on with max_range 5 / 40 / 120;
//     the three semantics and both Voxblox methods; walk two / single; max_batch 1 / 2 / 64 / 512;
//     max_points 2^10 / 2^18 / 2^22; n_sectors 0 / 4; max_pairs 0 and a binding value;
//   * the known answers of the comments: 5 cm voxels with a 15 cm truncation (three voxels: a band
//     of 6) give 4 pair and 25 sample slots per ray -- the double literals 0.05 and 0.15 make a band
//     of 5.999... voxels and give 4 and 22, as the restatement does; the single walk is taken only
//     when its step bound is <= 32, with nstep 16 exactly when the bound is <= 16; the single
//     walk's own refusal and its text;
//   * gate_threshold: for tau in {0.02, 0.06, 0.15, 0.3, 1.0} and 1000 random floats in [1e-3, 10],
//     (float)sqrt(x) >= tau holds for the returned double and fails for the next double below it;
//   * params_valid: the defaults pass, and each rule of tsdf_create's validation refuses.
// Exits non-zero on the first misses.  Built plain and with -fsanitize=address,undefined
// (tests/test_ctx_plan.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../../noetic-slam_amd/csrc/ctx_plan.h"

using namespace tsdf;

static int fails = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            if (++fails > 10) return;     \
        }                                 \
    } while (0)

// the device constants (tsdf_device.h), as literals
static const uint32_t kRPB = 1024, kMAX_BATCH = 512, kWLK_THREADS = 512, kSPAN = 4;
static const int kVOX_LIMIT = 1 << 23;
static const PlanConsts kConsts{kRPB, kMAX_BATCH, kWLK_THREADS, kSPAN, kVOX_LIMIT};

// The library's defaults (tsdf_default_params), restated: the program links no library
static tsdf_params defaults() {
    tsdf_params p;
    std::memset(&p, 0, sizeof p);
    p.voxel_size = 0.05;
    p.sdf_trunc = 0.15;
    p.weight_mode = TSDF_WEIGHT_CONSTANT;
    p.max_range = INFINITY;
    p.max_bricks = 1u << 20;
    p.max_points = 1u << 18;
    p.brick_side = TSDF_BRICK_SIDE;
    p.max_batch = 32;
    p.semantics = TSDF_SEM_VDBFUSION_F64;
    p.voxblox_method = TSDF_VB_SIMPLE;
    p.sector_input = TSDF_SECTOR_INPUT_FANOUT;
    p.sector_rule = TSDF_SECTOR_RULE_INDEX;
    p.allow_clear = 1;
    p.use_weight_dropoff = 1;
    p.max_weight = 10000.0f;
    p.depth_weight = 1;
    return p;
}

// ---- the restatement: tsdf_create's sizing as one straight line ----------------------------------

struct Ref {
    uint32_t maxp, spr;
    int band_vox;
    bool fused;
    int nstep;
    uint64_t batch_points, slots;
    uint32_t max_blocks, cell_stride, max_smp, max_spn, max_fb;
    std::string refusal;
};

static uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
static uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

static Ref restate(const tsdf_params& p) {
    Ref r{};
    char text[256];
    double band1;  // pairs_per_ray's band
    if (p.space_carving) band1 = (p.max_range + p.sdf_trunc) / p.voxel_size;
    else band1 = 2.0 * p.sdf_trunc / p.voxel_size;
    const double e = std::floor(band1) + 2.0;
    const double crossings = std::floor((e - 1.0) / 8.0) + 1.0;
    r.maxp = (uint32_t)(1.0 + 3.0 * crossings);
    double band2;  // samples_per_ray's
    if (p.space_carving) band2 = (p.max_range + p.sdf_trunc) / p.voxel_size;
    else band2 = 2.0 * p.sdf_trunc / p.voxel_size;
    r.spr = (uint32_t)(1.0 + 3.0 * (std::floor(band2) + 2.0));
    const double band3 = p.space_carving ? (p.max_range + p.sdf_trunc) / p.voxel_size
                                         : 2.0 * p.sdf_trunc / p.voxel_size;
    r.band_vox = (int)std::fmin(std::ceil(band3) + 4.0, (double)(kVOX_LIMIT / 2));
    uint64_t bp = p.max_points * (uint64_t)p.max_batch;
    bp = min64(bp, 0xFFFFFFF0ull / r.maxp);
    if (p.max_pairs) bp = min64(bp, p.max_pairs / r.maxp);
    if (bp < p.max_points) {
        std::snprintf(text, sizeof text,
                      "max_points %llu exceeds what one batch can hold (%llu: %u pair and %u sample "
                      "slots per ray)", (unsigned long long)p.max_points, (unsigned long long)bp,
                      r.maxp, r.spr);
        r.refusal = text;
        return r;
    }
    const bool depth_w = p.semantics == TSDF_SEM_VOXBLOX && p.depth_weight;
    const bool merged = p.semantics == TSDF_SEM_VOXBLOX && p.voxblox_method == TSDF_VB_MERGED;
    const int sem = depth_w || merged ? 3 : p.semantics;
    const double band4 = 2.0 * p.sdf_trunc / p.voxel_size;
    const double steps = std::floor(std::sqrt(3.0) * band4 * (1.0 + 1e-4)) + 5.0;
    const bool clearing = p.semantics == TSDF_SEM_VOXBLOX && p.allow_clear && std::isfinite(p.max_range);
    r.fused = p.walk == TSDF_WALK_SINGLE && !p.space_carving && !clearing && r.maxp <= 4 && sem != 3 &&
              steps <= 32.0;
    r.nstep = steps <= 16.0 ? 16 : 32;
    const uint64_t stg = (uint64_t)kWLK_THREADS * (uint64_t)r.nstep;
    if (r.fused) {
        const uint64_t lim = ((1ull << 30) / (2 * stg) - kMAX_BATCH - 1) * kRPB;
        bp = min64(bp, lim);
        if (bp < p.max_points) {
            std::snprintf(text, sizeof text, "max_points %llu exceeds a single-walk batch (%llu)",
                          (unsigned long long)p.max_points, (unsigned long long)bp);
            r.refusal = text;
            return r;
        }
    }
    r.batch_points = bp;
    const uint64_t slots = bp * r.maxp;
    r.slots = slots;
    r.max_blocks = (uint32_t)(bp / kRPB + kMAX_BATCH + 1);
    const uint32_t nsec = p.n_sectors > 1u ? p.n_sectors : 1u;
    if (r.fused) {
        r.cell_stride = (p.max_batch + 2u) & ~1u;
        const uint64_t reg_blocks =
            nsec > 1 ? min64(r.max_blocks, r.max_blocks * 5ull / (4ull * nsec) + 2ull * p.max_batch + 64)
                     : r.max_blocks;
        r.max_smp = (uint32_t)min64(2 * reg_blocks * stg, 1ull << 30);
        r.max_spn = (uint32_t)min64(bp * r.spr / kSPAN / nsec + 2 * reg_blocks * 256, 0xFFFFFFF0ull);
        r.max_fb = 4;
    } else {
        r.cell_stride = (p.max_batch + 3u) & ~3u;
        r.max_smp = (uint32_t)min64(min64(bp * r.spr / nsec, 1ull << 30), 0xFFFFFFF0ull);
        r.max_fb = (uint32_t)min64(p.space_carving ? slots : max64(slots / 16, 1u << 20), 1u << 26);
        r.max_spn = 4;
    }
    return r;
}

static void check_grid(long* n_cases, long* n_refused, long* n_fused) {
    const double voxels[] = {0.02, 0.05, 0.10};
    const double ranges[] = {0.0 /* carving off */, 5.0, 40.0, 120.0};
    const int modes[][2] = {{TSDF_SEM_VDBFUSION, TSDF_VB_SIMPLE}, {TSDF_SEM_VDBFUSION_F64, TSDF_VB_SIMPLE},
                            {TSDF_SEM_VOXBLOX, TSDF_VB_SIMPLE}, {TSDF_SEM_VOXBLOX, TSDF_VB_MERGED}};
    const uint32_t batches[] = {1, 2, 64, 512};
    const uint64_t points[] = {1ull << 10, 1ull << 18, 1ull << 22};
    for (double vs : voxels)
    for (int tv = 1; tv <= 6; tv++)
    for (double range : ranges)
    for (auto& mode : modes)
    for (int depth_w = 0; depth_w < 2; depth_w++)
    for (int walk : {TSDF_WALK_TWO, TSDF_WALK_SINGLE})
    for (uint32_t mb : batches)
    for (uint64_t mp : points)
    for (uint32_t nsec : {0u, 4u})
    for (int capped = 0; capped < 2; capped++) {
        tsdf_params p = defaults();
        p.voxel_size = vs;
        p.sdf_trunc = tv * vs;
        p.space_carving = range > 0.0;
        if (range > 0.0) p.max_range = range;
        p.semantics = mode[0];
        p.voxblox_method = mode[1];
        p.depth_weight = depth_w;
        p.walk = walk;
        p.max_batch = mb;
        p.max_points = mp;
        p.n_sectors = nsec;
        p.sector = nsec ? 1 : 0;
        // a binding cap: room for three scans' worth of points at four pair slots per ray
        p.max_pairs = capped ? 12 * mp : 0;
        CHECK(params_valid(p), "grid params refused");
        const CtxPlan P = ctx_plan(p, kConsts);
        const Ref r = restate(p);
        ++*n_cases;
        *n_refused += !r.refusal.empty();
        *n_fused += r.fused;
        const bool same_head = P.maxp == r.maxp && P.spr == r.spr && P.band_vox == r.band_vox &&
                               P.refusal == r.refusal;
        // (after a refusal the later fields are not part of the plan)
        const bool same_tail = !r.refusal.empty() ||
            (P.fused == r.fused && P.nstep == r.nstep && P.batch_points == r.batch_points &&
             P.slots == r.slots && P.max_blocks == r.max_blocks && P.cell_stride == r.cell_stride &&
             P.max_smp == r.max_smp && P.max_spn == r.max_spn && P.max_fb == r.max_fb);
        CHECK(same_head && same_tail,
              "plan differs: vs %.2f trunc %dv range %.0f sem %d method %d dw %d walk %d batch %u "
              "points %llu sectors %u capped %d: maxp %u/%u spr %u/%u band %d/%d fused %d/%d nstep "
              "%d/%d bp %llu/%llu slots %llu/%llu blocks %u/%u stride %u/%u smp %u/%u spn %u/%u fb "
              "%u/%u refusal '%s'/'%s'",
              vs, tv, range, mode[0], mode[1], depth_w, walk, mb, (unsigned long long)mp, nsec, capped,
              P.maxp, r.maxp, P.spr, r.spr, P.band_vox, r.band_vox, (int)P.fused, (int)r.fused,
              P.nstep, r.nstep, (unsigned long long)P.batch_points,
              (unsigned long long)r.batch_points, (unsigned long long)P.slots,
              (unsigned long long)r.slots, P.max_blocks, r.max_blocks, P.cell_stride, r.cell_stride,
              P.max_smp, r.max_smp, P.max_spn, r.max_spn, P.max_fb, r.max_fb, P.refusal.c_str(),
              r.refusal.c_str());
    }
}

// ---- known answers -------------------------------------------------------------------------------

static void check_known() {
    // 5 cm voxels and a truncation of three of them, formed like the grid's: a band of 6 voxels
    tsdf_params p = defaults();
    p.sdf_trunc = 3 * p.voxel_size;
    CHECK(pairs_per_ray(p) == 4, "5 cm / 15 cm: %u pair slots", pairs_per_ray(p));
    CHECK(samples_per_ray(p) == 25, "5 cm / 15 cm: %u sample slots", samples_per_ray(p));
    CHECK(std::floor(band_voxels(p)) == 6.0 && band_voxels(p) == trunc_band_voxels(p), "5 cm / 15 cm: band");
    // the literals 0.05 and 0.15 as doubles: 2 * 0.15 / 0.05 rounds to 5.999..., a hair under 6
    // voxels (as do the floats the kernels gate with), so the bound is one voxel's 3 samples lower
    p = defaults();
    CHECK(band_voxels(p) < 6.0 && pairs_per_ray(p) == 4 && samples_per_ray(p) == 22,
          "0.05 / 0.15: band %.17g, %u pair and %u sample slots", band_voxels(p), pairs_per_ray(p),
          samples_per_ray(p));
    CHECK(restate(p).maxp == 4 && restate(p).spr == 22, "0.05 / 0.15: the restatement differs");
    p.space_carving = 1;
    p.max_range = 40.0;
    CHECK(band_voxels(p) == (40.0 + 0.15) / 0.05 && trunc_band_voxels(p) == 2.0 * 0.15 / 0.05,
          "carving band");
    // the single walk against its step bound, the band swept in sixteenths of a voxel
    p = defaults();
    p.walk = TSDF_WALK_SINGLE;
    p.voxel_size = 0.0625;
    int n16 = 0, n32 = 0, n_two = 0;
    for (int k = 1; k <= 384; k++) {
        p.sdf_trunc = k * 0.0625 / 32.0;  // band = k / 16 voxels, exactly
        const double bound = std::floor(std::sqrt(3.0) * (k / 16.0) * (1.0 + 1e-4)) + 5.0;
        const CtxPlan P = ctx_plan(p, kConsts);
        CHECK(P.refusal.empty(), "sweep refused at band %g", k / 16.0);
        // (a band under 7 voxels has 4 pair slots; from there on the two walks)
        const bool want = bound <= 32.0 && pairs_per_ray(p) <= 4;
        CHECK(P.fused == want, "band %g: fused %d, bound %g, %u pair slots", k / 16.0, (int)P.fused, bound,
              pairs_per_ray(p));
        CHECK(!(P.fused && bound > 32.0), "band %g: single walk past its bound %g", k / 16.0, bound);
        CHECK(P.nstep == (bound <= 16.0 ? 16 : 32), "band %g: nstep %d, bound %g", k / 16.0, P.nstep, bound);
        n16 += P.fused && P.nstep == 16;
        n32 += P.fused && P.nstep == 32;
        n_two += !P.fused;
    }
    CHECK(n16 > 0 && n32 > 0 && n_two > 0, "sweep misses a case: %d / %d / %d", n16, n32, n_two);
    // the single walk's own refusal (the grid's scans are too small for it): a scan of 2^27 points
    // against the 2^30 samples a span record addresses
    p = defaults();
    p.walk = TSDF_WALK_SINGLE;
    p.max_batch = 2;
    p.max_points = 1ull << 27;
    const CtxPlan P = ctx_plan(p, kConsts);
    CHECK(P.refusal == "max_points 134217728 exceeds a single-walk batch (66583552)", "refusal '%s'",
          P.refusal.c_str());
    CHECK(P.refusal == restate(p).refusal, "refusal '%s' / '%s'", P.refusal.c_str(),
          restate(p).refusal.c_str());
    p.walk = TSDF_WALK_TWO;
    CHECK(ctx_plan(p, kConsts).refusal.empty(), "two walks refused: %s", ctx_plan(p, kConsts).refusal.c_str());
}

// ---- gate_threshold ------------------------------------------------------------------------------

static double next_below(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    b--;  // x > 0: the next double towards zero
    std::memcpy(&x, &b, 8);
    return x;
}

static void check_gate_one(float tau) {
    const double x = gate_threshold(tau);
    CHECK(x > 0.0, "tau %.9g: threshold %g", tau, x);
    CHECK((float)std::sqrt(x) >= tau, "tau %.9g: (float)sqrt(%.17g) < tau", tau, x);
    const double y = next_below(x);
    CHECK(!((float)std::sqrt(y) >= tau), "tau %.9g: the double below %.17g passes too", tau, x);
}

static void check_gate() {
    for (float tau : {0.02f, 0.06f, 0.15f, 0.3f, 1.0f}) check_gate_one(tau);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 1000; i++) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const double u = (double)(s >> 11) * 0x1p-53;  // [0, 1)
        check_gate_one((float)(1e-3 * std::pow(1e4, u)));  // log-uniform in [1e-3, 10]
        if (fails) return;
    }
}

// ---- params_valid --------------------------------------------------------------------------------

static void check_valid() {
    const tsdf_params d = defaults();
    CHECK(params_valid(d), "defaults refused");
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    int k = 0;
    auto bad = [&](auto&& change) {
        tsdf_params p = d;
        change(p);
        k++;
        if (params_valid(p)) {
            std::printf("invalid params %d accepted\n", k);
            fails++;
        }
    };
    bad([&](tsdf_params& p) { p.voxel_size = 0; });
    bad([&](tsdf_params& p) { p.voxel_size = nan; });
    bad([&](tsdf_params& p) { p.sdf_trunc = -1; });
    bad([&](tsdf_params& p) { p.brick_side = 4; });
    bad([&](tsdf_params& p) { p.weight_mode = TSDF_WEIGHT_CONSTANT + 1; });
    bad([&](tsdf_params& p) { p.max_bricks = 0; });
    bad([&](tsdf_params& p) { p.max_bricks = 0xFFFFFFF0ull; });
    bad([&](tsdf_params& p) { p.max_points = 0; });
    bad([&](tsdf_params& p) { p.min_range = -0.5; });
    bad([&](tsdf_params& p) { p.min_range = nan; });
    bad([&](tsdf_params& p) { p.min_range = 2; p.max_range = 2; });
    bad([&](tsdf_params& p) { p.max_range = nan; });
    bad([&](tsdf_params& p) { p.max_batch = 0; });
    bad([&](tsdf_params& p) { p.max_batch = TSDF_MAX_BATCH + 1; });
    bad([&](tsdf_params& p) { p.semantics = 3; });
    bad([&](tsdf_params& p) { p.semantics = TSDF_SEM_VOXBLOX; p.max_weight = 0.0f; });
    bad([&](tsdf_params& p) { p.voxblox_method = 2; });
    bad([&](tsdf_params& p) { p.sector_input = TSDF_SECTOR_INPUT_SPLIT + 1; });
    bad([&](tsdf_params& p) { p.sector_rule = 7; });
    bad([&](tsdf_params& p) { p.n_sectors = 4; p.sector = 4; });
    bad([&](tsdf_params& p) { p.sector_yaw0 = inf; });
    bad([&](tsdf_params& p) { p.max_bricks_hard = p.max_bricks - 1; });
    bad([&](tsdf_params& p) { p.space_carving = 1; });  // max_range is infinite
}

int main() {
    long n_cases = 0, n_refused = 0, n_fused = 0;
    check_grid(&n_cases, &n_refused, &n_fused);
    if (!fails && (n_refused == 0 || n_fused == 0 || n_refused == n_cases)) {
        std::printf("the grid misses a branch: %ld cases, %ld refused, %ld single-walk\n", n_cases,
                    n_refused, n_fused);
        fails++;
    }
    check_known();
    check_gate();
    check_valid();
    if (fails) {
        std::printf("FAILED (%d)\n", fails);
        return 1;
    }
    std::printf("ok: %ld plans (%ld refused, %ld single-walk)\n", n_cases, n_refused, n_fused);
    return 0;
}

/*
 * tsdf_oracle.c — CPU ORACLE for the TSDF integration hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library,
 * and only as the checker / the timed CPU baseline.  The product path (libtsdf_hip.so) never
 * links or calls it.
 *
 * What it restates.  The reference's TSDF node and all four of its backends are absent from
 * /root/reference (README.md:44-50 names src/tsdf_map/src/tsdf_map_node.cpp with
 * MAP_BACKEND_IDX 0 CHAD TSDF / 1 Octomap / 2 Voxblox / 3 VDBFusion; none is committed or
 * vendored, and no version is pinned anywhere).  This file restates the published algorithm of
 * the backend the north star names as the parity target, VDBFusion (PRBonn/vdbfusion,
 * `VDBVolume::Integrate`, unpinned version; README.md:48,75), in plain C, scalar and serial the
 * way upstream loops over points with std::for_each:
 *
 *   for each point p (origin o):  d = |p - o|, u = (p - o)/d
 *       band t in [t0, t1], t0 = space_carving ? 0 : d - tau, t1 = d + tau
 *       Amanatides-Woo DDA in voxel index space (OpenVDB math::DDA, ties -> higher axis)
 *       for each voxel v: c = (v + 1/2) vs          (GetVoxelCenter)
 *           sdf = sign((c - o).(p - c)) |p - c|     (ComputeSDF; sign of 0 is NaN -> skipped)
 *           if sdf > -tau: s = min(tau, sdf), w = 1  (constant weighting_function)
 *               S <- (S W + s w)/(W + w), W <- W + w
 *
 * and the input contract of the reference's producer: points are DLIO's world-frame deskewed
 * cloud (dlio::Point, src/dlio/include/dlio/dlio.h:85-106: x,y,z float32 at offsets 0,4,8,
 * point_step 32), origin = the scan pose (src/dlio/src/dlio/odom.cc:434-451, 315-356).
 *
 * Two accumulation modes:
 *   ORACLE_MODE_SCAN_FUSED (default) — the backend's documented per-scan semantics: all samples
 *     of one scan hitting voxel v are summed as exact 64-bit fixed point (q = trunc(s * 2^32)) and
 *     count, then fused once:  S <- (S W + A 2^-32) / (W + B),  W <- W + B.  Order-independent,
 *     so the GPU backend must reproduce it BIT FOR BIT.
 *   ORACLE_MODE_SEQUENTIAL — VDBFusion's literal per-sample fp32 running average, in input order.
 *     Equal to SCAN_FUSED in exact arithmetic; the fp32 difference is the parity tolerance
 *     reported against "the reference CPU backend" (DESIGN.md §4).
 *   ORACLE_MODE_VDB_LITERAL — VDBFusion's Integrate with upstream's own precisions (walk_ray_vdb):
 *     double points / origin, the Ray<float> built from them and mapped to index space through the
 *     grid transform (double scale), openvdb's DDA in float, GetVoxelCenter / ComputeSDF in double,
 *     and the per-sample float running average in input order.  The distance of the GPU field from
 *     this mode is what "matches VDBFusion" means quantitatively (tests/test_literal.py).
 *
 * Parity pinning: no reference test pins values at this boundary, so this oracle
 * is pinned by closed-form known-answer tests (tests/test_oracle_kat.py: single rays, planes,
 * spheres) and committed golden vectors generated from it (tests/golden/make_golden.py).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/tsdf_hip.h"
#include "../include/tsdf_mc_tables.h"

#define ORACLE_MODE_SCAN_FUSED 0
#define ORACLE_MODE_SEQUENTIAL 1
#define ORACLE_MODE_VDB_LITERAL 2

/* voxel domain: |index| < 2^23 on every axis (the GPU packs 21-bit brick coordinates) */
#define VOX_LIMIT (1 << 23)
#define MAX_DDA_STEPS (1 << 20)

typedef struct {
    int32_t x, y, z;
    int32_t used;
    float S, W;     /* persistent field */
    int64_t A;      /* per-scan fixed-point sum of w*s (scale 2^32) */
    int64_t B;      /* per-scan sum of w: a count (VDBFusion, w = 1) or fixed point 2^32 (Voxblox) */
    uint32_t stamp; /* last scan that touched it (for the touched list) */
} vox_t;

struct tsdf_ctx {
    tsdf_params p;
    float vs, inv_vs, tau;
    float bg;   /* background distance: tau (VDBFusion) or 0 (Voxblox TsdfVoxel) */
    int sem;    /* TSDF_SEM_* */
    float zax[3]; /* the current scan's sensor z axis (tsdf_integrate_pose; else world z) */
    /* azimuth-sector filter (tsdf_params.n_sectors > 1): pseudo-angle interval [sec_lo, sec_hi),
     * cyclic when sec_wrap (include/tsdf_hip.h tsdf_sector_of) */
    int sec_on, sec_wrap;
    float sec_lo, sec_hi;
    vox_t* tab;
    uint64_t cap, n;
    uint32_t* touched; /* indices into tab of voxels touched this scan */
    uint64_t n_touched, touched_cap;
    uint32_t scan_id;
    int mode;
    tsdf_stats st;
    char err[256];
    /* multi-threaded scan-fused mode (tsdf_oracle_set_threads, n_thr > 1): the field is split into
     * n_thr partitions by brick hash, each a full context of its own (sub[p]); tab is then only a
     * read-out snapshot, rebuilt from the partitions when mt_dirty */
    int n_thr, mt_dirty;
    /* Voxblox MergedTsdfIntegrator (voxblox_method == TSDF_VB_MERGED): while mg_on, the "points"
     * walked are the scan's bundled rays, 16-B records (x, y, z, w) with w < 0 for a clearing ray */
    int mg_on;
    struct tsdf_ctx** sub;
    struct mt_bucket* bk; /* n_thr x n_thr: samples of ray-thread t for partition p at [t n_thr + p] */
    /* border-reduce transaction (ABI v9; the GPU library's brd_*): the bricks the open reduce's pack
     * sent (reset at commit), and the voxels its merges touched as they were (restored at abort) */
    int brd_open;
    int32_t* brd_sent; /* brick coordinates, 3 per brick */
    uint64_t brd_n_sent;
    struct brd_vox* brd_bk;
    uint64_t brd_n_bk, brd_cap_bk;
};

struct brd_vox { int32_t x, y, z; float S, W; };

typedef struct { int32_t x, y, z; float s, w; } mt_sample;
struct mt_bucket { mt_sample* v; uint64_t n, cap; };

static uint64_t mix3(int32_t x, int32_t y, int32_t z) {
    uint64_t h = (uint64_t)(uint32_t)x * 0x9E3779B97F4A7C15ull;
    h ^= (uint64_t)(uint32_t)y * 0xC2B2AE3D27D4EB4Full + (h << 6) + (h >> 2);
    h ^= (uint64_t)(uint32_t)z * 0x165667B19E3779F9ull + (h << 6) + (h >> 2);
    h ^= h >> 31;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
    return h;
}

static int set_err(tsdf_ctx* c, int code, const char* msg) {
    if (c) snprintf(c->err, sizeof c->err, "%s", msg);
    return code;
}

static int grow(tsdf_ctx* c);

/* ---- azimuth sectors (include/tsdf_hip.h tsdf_sector_of: the multi-GPU shard rule) ---------- */

/* fp32 pseudo-angle of (x, y) in [0, 4), monotone in atan2; one IEEE division */
static float pseudo_angle(float x, float y) {
    if (y >= 0.0f) {
        if (x >= 0.0f) {
            const float d = x + y;
            return d > 0.0f ? y / d : 0.0f;
        }
        return 1.0f - x / (y - x);
    }
    if (x < 0.0f) return 2.0f - y / (-x - y);
    return 3.0f + x / (x - y);
}

/* sector k of n starts at the pseudo-angle of yaw0 + 2 pi k / n (cos/sin in double) */
static float sector_start(double yaw0, uint32_t k, uint32_t n) {
    const double th = yaw0 + 6.283185307179586476925286766559 * (double)k / (double)n;
    return pseudo_angle((float)cos(th), (float)sin(th));
}

typedef struct { int on, wrap; float lo, hi; } sector_t;

static sector_t sector_bounds(double yaw0, uint32_t sector, uint32_t n) {
    sector_t r = {0, 0, 0.0f, 0.0f};
    if (n <= 1) return r;
    r.on = 1;
    r.lo = sector_start(yaw0, sector, n);
    r.hi = sector_start(yaw0, (sector + 1) % n, n);
    r.wrap = r.hi <= r.lo;
    return r;
}

static int sector_has(const sector_t* r, float dx, float dy) {
    if (!r->on) return 1;
    const float a = pseudo_angle(dx, dy);
    return r->wrap ? (a >= r->lo || a < r->hi) : (a >= r->lo && a < r->hi);
}

static int ctx_in_sector(const tsdf_ctx* c, float dx, float dy) {
    const sector_t r = {c->sec_on, c->sec_wrap, c->sec_lo, c->sec_hi};
    return sector_has(&r, dx, dy);
}

/* find-or-insert voxel (x,y,z); returns index or -1 on allocation failure */
static int64_t vox_get(tsdf_ctx* c, int32_t x, int32_t y, int32_t z) {
    if (2 * (c->n + 1) > c->cap)
        if (grow(c)) return -1;
    uint64_t m = c->cap - 1, h = mix3(x, y, z) & m;
    for (;;) {
        vox_t* v = &c->tab[h];
        if (!v->used) {
            v->used = 1;
            v->x = x; v->y = y; v->z = z;
            v->S = c->bg; /* background: (sdf_trunc, 0) VDBFusion, (0, 0) Voxblox */
            v->W = 0.0f;
            v->A = 0; v->B = 0; v->stamp = 0;
            c->n++;
            return (int64_t)h;
        }
        if (v->x == x && v->y == y && v->z == z) return (int64_t)h;
        h = (h + 1) & m;
    }
}

static const vox_t* vox_find(const tsdf_ctx* c, int32_t x, int32_t y, int32_t z) {
    if (!c->cap) return NULL;
    uint64_t m = c->cap - 1, h = mix3(x, y, z) & m;
    for (;;) {
        const vox_t* v = &c->tab[h];
        if (!v->used) return NULL;
        if (v->x == x && v->y == y && v->z == z) return v;
        h = (h + 1) & m;
    }
}

static int grow(tsdf_ctx* c) {
    uint64_t ncap = c->cap ? c->cap * 2 : (1u << 16);
    vox_t* nt = (vox_t*)calloc(ncap, sizeof(vox_t));
    if (!nt) return 1;
    /* touched indices refer to old slots: re-map them */
    uint32_t* remap = NULL;
    if (c->n_touched) {
        remap = (uint32_t*)malloc(c->n_touched * sizeof(uint32_t));
        if (!remap) { free(nt); return 1; }
    }
    uint64_t m = ncap - 1;
    for (uint64_t i = 0; i < c->cap; i++) {
        if (!c->tab[i].used) continue;
        uint64_t h = mix3(c->tab[i].x, c->tab[i].y, c->tab[i].z) & m;
        while (nt[h].used) h = (h + 1) & m;
        nt[h] = c->tab[i];
        /* stash new position in old slot's A? no: use a linear search through touched below */
        c->tab[i].stamp = (uint32_t)h; /* old table is discarded; reuse field as forward pointer */
    }
    for (uint64_t k = 0; k < c->n_touched; k++) remap[k] = c->tab[c->touched[k]].stamp;
    for (uint64_t k = 0; k < c->n_touched; k++) c->touched[k] = remap[k];
    free(remap);
    free(c->tab);
    c->tab = nt;
    c->cap = ncap;
    return 0;
}

void tsdf_default_params(tsdf_params* p) {
    memset(p, 0, sizeof *p);
    p->voxel_size = 0.05;
    p->sdf_trunc = 0.15;
    p->space_carving = 0;
    p->weight_mode = TSDF_WEIGHT_CONSTANT;
    p->min_range = 0.0;
    p->max_range = INFINITY;
    p->max_bricks = 1u << 20;
    p->max_points = 1u << 18;
    p->max_pairs = 0;
    p->device_id = 0;
    p->brick_side = TSDF_BRICK_SIDE;
    p->max_batch = 32; /* accepted for ABI parity; the oracle integrates scan by scan */
    p->semantics = TSDF_SEM_VDBFUSION_F64; /* ABI v8 default */
    p->allow_clear = 1;        /* voxblox TsdfIntegratorBase::Config defaults */
    p->use_weight_dropoff = 1;
    p->max_weight = 10000.0f;
    p->depth_weight = 1; /* voxblox use_const_weight = false (upstream's default) */
    p->voxblox_method = TSDF_VB_SIMPLE;
    p->sector_input = TSDF_SECTOR_INPUT_FANOUT;
    p->sector_rule = TSDF_SECTOR_RULE_INDEX; /* ABI v10 */
}

int tsdf_abi_version(void) { return TSDF_ABI_VERSION; }

int tsdf_create(const tsdf_params* params, tsdf_ctx** out) {
    if (!params || !out) return TSDF_EINVAL;
    if (!(params->voxel_size > 0) || !(params->sdf_trunc > 0) ||
        params->brick_side != TSDF_BRICK_SIDE || params->weight_mode != TSDF_WEIGHT_CONSTANT ||
        (params->semantics != TSDF_SEM_VDBFUSION && params->semantics != TSDF_SEM_VOXBLOX &&
         params->semantics != TSDF_SEM_VDBFUSION_F64) ||
        (params->semantics == TSDF_SEM_VOXBLOX && !(params->max_weight > 0.0f)) ||
        (params->voxblox_method != TSDF_VB_SIMPLE && params->voxblox_method != TSDF_VB_MERGED) ||
        (params->sector_input < TSDF_SECTOR_INPUT_FANOUT ||
         params->sector_input > TSDF_SECTOR_INPUT_SPLIT) ||
        (params->sector_rule != TSDF_SECTOR_RULE_WORLD &&
         params->sector_rule != TSDF_SECTOR_RULE_INDEX) ||
        (params->n_sectors > 1 && params->sector >= params->n_sectors) ||
        !isfinite(params->sector_yaw0))
        return TSDF_EINVAL;
    tsdf_ctx* c = (tsdf_ctx*)calloc(1, sizeof *c);
    if (!c) return TSDF_ENOMEM;
    c->p = *params;
    c->vs = (float)params->voxel_size;
    c->inv_vs = 1.0f / c->vs;
    c->tau = (float)params->sdf_trunc;
    c->sem = params->semantics;
    c->zax[0] = 0.0f; c->zax[1] = 0.0f; c->zax[2] = 0.0f; /* no orientation: weight 1 */
    c->bg = c->sem == TSDF_SEM_VOXBLOX ? 0.0f : c->tau;
    c->mode = ORACLE_MODE_SCAN_FUSED;
    if (params->sector_rule == TSDF_SECTOR_RULE_WORLD) { /* the index rule slices at entry */
        const sector_t r = sector_bounds(params->sector_yaw0, params->sector, params->n_sectors);
        c->sec_on = r.on; c->sec_wrap = r.wrap; c->sec_lo = r.lo; c->sec_hi = r.hi;
    }
    *out = c;
    return TSDF_OK;
}

void tsdf_destroy(tsdf_ctx* c) {
    if (!c) return;
    if (c->sub)
        for (int p = 0; p < c->n_thr; p++) tsdf_destroy(c->sub[p]);
    if (c->bk)
        for (int k = 0; k < c->n_thr * c->n_thr; k++) free(c->bk[k].v);
    free(c->sub);
    free(c->bk);
    free(c->tab);
    free(c->touched);
    free(c->brd_sent);
    free(c->brd_bk);
    free(c);
}

const char* tsdf_last_error(const tsdf_ctx* c) { return c ? c->err : "null context"; }

int tsdf_oracle_set_mode(tsdf_ctx* c, int mode) {
    if (!c || (mode != ORACLE_MODE_SCAN_FUSED && mode != ORACLE_MODE_SEQUENTIAL &&
               mode != ORACLE_MODE_VDB_LITERAL))
        return TSDF_EINVAL;
    if (mode == ORACLE_MODE_VDB_LITERAL && c->sem == TSDF_SEM_VOXBLOX) return TSDF_EINVAL;
    if (c->n_thr > 1 && mode != ORACLE_MODE_SCAN_FUSED) return TSDF_EINVAL;
    c->mode = mode;
    return TSDF_OK;
}

/* ---- the ray walk (VDBFusion Integrate body, one point) ---------------------------------- */

typedef void (*visit_fn)(tsdf_ctx* c, int32_t vx, int32_t vy, int32_t vz, float s, float w,
                         void* user);

/* The far-ray rule (include/tsdf_hip.h "Index domain"; the kernels' far_ok): a ray is dropped whole,
 * like a range-filtered one, unless every index-space coordinate handed to a float -> int
 * conversion is finite and of magnitude < 2^30.  Decided on the floats, before the conversion (an
 * out-of-range conversion is undefined in C and differs between targets); 2^30 leaves MAX_DDA_STEPS
 * steps without int overflow and lies far outside the domain's bands. */
#define FAR_LIMIT 1073741824.0f /* 2^30 */

static int far_ok(float x, float y, float z) {
    return fabsf(x) < FAR_LIMIT && fabsf(y) < FAR_LIMIT && fabsf(z) < FAR_LIMIT; /* false for NaN */
}

/* Returns the number of voxels visited by the DDA (gated or not), -1 for a dropped ray; calls
 * visit() for every voxel with sdf > -tau, in DDA order.  All arithmetic fp32, no contraction (built -ffp-contract=off). */
static int64_t walk_ray(tsdf_ctx* c, float px, float py, float pz, float ox, float oy, float oz,
                        visit_fn visit, void* user) {
    const float vs = c->vs, inv_vs = c->inv_vs, tau = c->tau;
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    if (!ctx_in_sector(c, dx, dy)) return -1; /* another GPU's azimuth sector */
    const float depth = sqrtf(dx * dx + dy * dy + dz * dz);
    /* range filter (VDBFusion pipelines drop r < min_range / r > max_range before Integrate);
     * NaN / zero-length rays are dropped (Ouster r = 0 -> (0,0,0), cartesian.h:64-65) */
    if (!(depth > 0.0f)) return -1;
    if (!(depth >= (float)c->p.min_range) || !(depth <= (float)c->p.max_range)) return -1;
    const float ux = dx / depth, uy = dy / depth, uz = dz / depth;
    const float t0 = c->p.space_carving ? 0.0f : depth - tau;
    const float t1 = depth + tau;
    /* Ray::worldToIndex: eye/vs, same unit direction, times scaled by 1/vs */
    const float t0i = t0 * inv_vs, t1i = t1 * inv_vs;
    const float sx = ox * inv_vs + ux * t0i;
    const float sy = oy * inv_vs + uy * t0i;
    const float sz = oz * inv_vs + uz * t0i;
    if (!far_ok(sx, sy, sz) || !(t1i < INFINITY)) return -1; /* the far-ray rule */
    int32_t v[3] = {(int32_t)floorf(sx), (int32_t)floorf(sy), (int32_t)floorf(sz)};
    const float s3[3] = {sx, sy, sz}, u3[3] = {ux, uy, uz};
    float tn[3], td[3];
    int32_t st[3];
    for (int a = 0; a < 3; a++) {
        if (u3[a] > 0.0f) {
            const float inv = 1.0f / u3[a];
            st[a] = 1;
            td[a] = inv;
            tn[a] = t0i + ((float)(v[a] + 1) - s3[a]) * inv;
        } else if (u3[a] < 0.0f) {
            const float inv = 1.0f / u3[a];
            st[a] = -1;
            td[a] = -inv;
            tn[a] = t0i + ((float)v[a] - s3[a]) * inv;
        } else {
            st[a] = 0;
            td[a] = INFINITY;
            tn[a] = INFINITY;
        }
    }
    int64_t visited = 0;
    for (int it = 0; it < MAX_DDA_STEPS; it++) {
        visited++;
        if (v[0] > -VOX_LIMIT && v[0] < VOX_LIMIT && v[1] > -VOX_LIMIT && v[1] < VOX_LIMIT &&
            v[2] > -VOX_LIMIT && v[2] < VOX_LIMIT) {
            /* GetVoxelCenter + ComputeSDF */
            const float cx = ((float)v[0] + 0.5f) * vs;
            const float cy = ((float)v[1] + 0.5f) * vs;
            const float cz = ((float)v[2] + 0.5f) * vs;
            const float ax = cx - ox, ay = cy - oy, az = cz - oz; /* voxel - origin */
            const float bx = px - cx, by = py - cy, bz = pz - cz; /* point - voxel */
            const float dist = sqrtf(bx * bx + by * by + bz * bz);
            const float proj = ax * bx + ay * by + az * bz;
            if (proj > 0.0f || proj < 0.0f) {
                const float sdf = proj > 0.0f ? dist : -dist;
                if (sdf > -tau) visit(c, v[0], v[1], v[2], sdf < tau ? sdf : tau, 1.0f, user);
            }
        }
        /* math::MinIndex tie-break: equal entries resolve to the higher axis */
        int a;
        if (tn[0] < tn[1]) a = (tn[0] < tn[2]) ? 0 : 2;
        else a = (tn[1] < tn[2]) ? 1 : 2;
        if (!(tn[a] <= t1i)) break;
        tn[a] += td[a];
        v[a] += st[a];
    }
    return visited;
}

/* ---- VDBFusion's Integrate body at upstream's own precisions (ORACLE_MODE_VDB_LITERAL) -------
 *
 * PRBonn/vdbfusion VDBVolume::Integrate (unpinned; not in /root/reference — SURVEY §8a8) on
 * std::vector<Eigen::Vector3d> points, restated step by step:
 *   direction = point - origin (double);  depth = (float)direction.norm()  (Eigen: x + (y + z))
 *   Vec3R dir = direction; dir.normalize()  (openvdb: len = sqrt((x x + y y) + z z), dir *= 1/len)
 *   t0 = carving ? 0 : depth - tau;  t1 = depth + tau  (float)
 *   Ray<float>(eye, dir, t0, t1): eye, dir rounded to float;  .worldToIndex(grid):
 *       eye_i = (float)(eye * (1/vs)), d = (float)(dir * (1/vs)) (double scale map), L = |d| (float),
 *       dir_i = d / L, t0_i = L t0, t1_i = L t1, inv = 1 / dir_i (float)
 *   math::DDA: pos = eye_i + dir_i t0_i; v = floor(pos); per axis: dir_i == 0 -> next = FLT_MAX;
 *       inv > 0 -> next = t0_i + ((v + 1) - pos) inv, delta = inv; else next = t0_i + (v - pos) inv,
 *       delta = -inv;  step(): a = MinIndex(next) (ties -> higher axis); stop when next[a] > t1_i
 *   GetVoxelCenter: c = v vs + vs / 2 (double);  ComputeSDF: sign((c - o).(p - c)) |p - c| (double,
 *       Eigen x + (y + z) reductions), cast to float;  gate sdf > -tau, then the float update.
 * All float ops are evaluated without contraction (-ffp-contract=off), as an x86-64 build without
 * FMA instructions evaluates them. */
static int64_t walk_ray_vdb(tsdf_ctx* c, const double p[3], const double o[3], visit_fn visit,
                            void* user) {
    const float tau = c->tau;
    const double vs_d = (double)c->vs;
    const double dx = p[0] - o[0], dy = p[1] - o[1], dz = p[2] - o[2];
    if (!ctx_in_sector(c, (float)p[0] - (float)o[0], (float)p[1] - (float)o[1])) return -1;
    const float depth = (float)sqrt(dx * dx + (dy * dy + dz * dz));
    if (!(depth > 0.0f)) return -1;
    if (!(depth >= (float)c->p.min_range) || !(depth <= (float)c->p.max_range)) return -1;
    const double len = sqrt((dx * dx + dy * dy) + dz * dz);
    const double il = 1.0 / len;
    const double dir_d[3] = {dx * il, dy * il, dz * il};
    const float t0 = c->p.space_carving ? 0.0f : depth - tau;
    const float t1 = depth + tau;
    const double inv_s = 1.0 / vs_d;
    float eye_i[3], dj[3];
    for (int a = 0; a < 3; a++) {
        eye_i[a] = (float)((double)(float)o[a] * inv_s);
        dj[a] = (float)((double)(float)dir_d[a] * inv_s);
    }
    const float L = (float)sqrt((double)((dj[0] * dj[0] + dj[1] * dj[1]) + dj[2] * dj[2]));
    float dir_i[3], inv[3], pos[3];
    for (int a = 0; a < 3; a++) {
        dir_i[a] = dj[a] / L;
        inv[a] = 1.0f / dir_i[a];
    }
    const float t0_i = L * t0, t1_i = L * t1;
    int32_t v[3], st[3];
    float tn[3], td[3];
    for (int a = 0; a < 3; a++) pos[a] = eye_i[a] + dir_i[a] * t0_i;
    if (!far_ok(pos[0], pos[1], pos[2]) || !(t1_i < INFINITY)) return -1; /* the far-ray rule */
    for (int a = 0; a < 3; a++) v[a] = (int32_t)floorf(pos[a]);
    for (int a = 0; a < 3; a++) {
        if (dir_i[a] == 0.0f) {
            st[a] = 0;
            tn[a] = 3.402823466e+38f;
            td[a] = 3.402823466e+38f;
        } else if (inv[a] > 0.0f) {
            st[a] = 1;
            tn[a] = t0_i + ((float)(v[a] + 1) - pos[a]) * inv[a];
            td[a] = inv[a];
        } else {
            st[a] = -1;
            tn[a] = t0_i + ((float)v[a] - pos[a]) * inv[a];
            td[a] = -inv[a];
        }
    }
    int64_t visited = 0;
    for (int it = 0; it < MAX_DDA_STEPS; it++) {
        visited++;
        if (v[0] > -VOX_LIMIT && v[0] < VOX_LIMIT && v[1] > -VOX_LIMIT && v[1] < VOX_LIMIT &&
            v[2] > -VOX_LIMIT && v[2] < VOX_LIMIT) {
            double cc[3], va[3], vb[3];
            for (int a = 0; a < 3; a++) {
                cc[a] = (double)v[a] * vs_d + vs_d / 2.0;
                va[a] = cc[a] - o[a];
                vb[a] = p[a] - cc[a];
            }
            const double dist = sqrt(vb[0] * vb[0] + (vb[1] * vb[1] + vb[2] * vb[2]));
            const double proj = va[0] * vb[0] + (va[1] * vb[1] + va[2] * vb[2]);
            const float sdf = (float)((proj / fabs(proj)) * dist);
            if (sdf > -tau) visit(c, v[0], v[1], v[2], tau < sdf ? tau : sdf, 1.0f, user);
        }
        int a; /* math::MinIndex */
        if (tn[0] < tn[1] && tn[0] < tn[2]) a = 0;
        else a = (tn[1] < tn[2]) ? 1 : 2;
        if (!(tn[a] <= t1_i)) break; /* a NaN entry time ends the walk, as the kernels' ray_step */
        v[a] += st[a];
        tn[a] += td[a];
    }
    return visited;
}

/* ---- the Voxblox ray walk (SimpleTsdfIntegrator::integrateFunction body, one point) ----------
 *
 * voxblox (ethz-asl/voxblox, unpinned version; not in /root/reference — SURVEY §8a9), restated:
 *   isPointValid:   d = |p - o|; d < min_ray_length -> dropped; d > max_ray_length -> a clearing
 *                   ray if allow_clear, else dropped
 *   RayCaster ctor: u = (p - o).normalized();
 *                   clearing: len = min(max(d - tau, 0), max_ray_length), end = o + u len,
 *                             start = carving ? o : end
 *                   else:     end = p + u tau, start = carving ? o : p - u tau
 *                   start/end scaled by 1/voxel_size
 *   setupRayCaster: cur = floor(start_s + kCoordinateEpsilon) (getGridIndexFromPoint, 1e-6),
 *                   steps = |floor(end_s + eps) - cur|_1; r = end_s - start_s; sign = signum(r);
 *                   t_next = (max(0, sign) - (start_s - cur)) / r; t_step = sign / r
 *   nextRayIndex:   steps + 1 voxels; after each, the axis of the FIRST minimum of t_next
 *                   (Eigen minCoeff: ties -> lower axis) advances by its sign
 *   getVoxelWeight: use_const_weight -> w = 1; else w = 1 / z^2, z the point's sensor-frame depth
 *                   (|z| <= 1e-6 -> 0; tsdf_params.depth_weight, the axis from the scan's pose)
 *   updateTsdfVoxel: c = (v + 1/2) vs;
 *                   sdf = |p - o| - ((c - o).(p - o)) / |p - o|     (computeDistance, projective)
 *                   dropoff: sdf < -vs -> w = (w (tau + sdf)) / (tau - vs), max(w, 0)
 *                   W' = W + w (W' < kFloatEpsilon: no update); S' = (sdf w + S W) / W'
 *                   S = S' > 0 ? min(tau, S') : max(-tau, S');  W = min(max_weight, W')
 * Stated deviations:
 *   - a zero component of r gets t_next = t_step = +inf (the axis never advances).  Upstream's
 *     guard `std::abs(r) < 0.0` is never true, so it divides by zero and the NaN/-inf entry
 *     stalls the walk on that axis; the +inf is the guard's evident intent;
 *   - samples of weight < 2^-16 are dropped whole (no allocation, no fuse): upstream allocates the
 *     block and applies the (negligible) update;
 *   - zero-length rays (p == o) are dropped;
 *   - validity uses |p - o| of the world-frame cloud (upstream: |point_C|, the same in exact
 *     arithmetic).
 * All fp32, -ffp-contract=off, the GPU's op order (tsdf_ray.h vb_*). */
#define VB_MIN_WEIGHT (1.0f / 65536.0f)

/* bw: 0 for a point's own ray (SimpleTsdfIntegrator); else a MergedTsdfIntegrator bundle's ray,
 * weight |bw|, a clearing ray when bw < 0: integrateVoxel hands the RayCaster the clearing flag and
 * updateTsdfVoxel the bundle's summed point weight, without re-testing the ray's length */
static int64_t walk_ray_vb(tsdf_ctx* c, float px, float py, float pz, float ox, float oy,
                           float oz, float bw, visit_fn visit, void* user) {
    const float vs = c->vs, inv_vs = c->inv_vs, tau = c->tau;
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    if (!ctx_in_sector(c, dx, dy)) return -1; /* another GPU's azimuth sector */
    /* Eigen's fixed-size-3 reductions (squaredNorm, dot) associate as x + (y + z) */
    const float depth = sqrtf(dx * dx + (dy * dy + dz * dz));
    if (!(depth > 0.0f)) return -1;
    int clearing = 0;
    if (bw != 0.0f) {
        clearing = bw < 0.0f;
    } else {
        if (depth < (float)c->p.min_range) return -1;
        if (depth > (float)c->p.max_range) {
            if (!c->p.allow_clear) return -1;
            clearing = 1;
        }
    }
    const float ux = dx / depth, uy = dy / depth, uz = dz / depth;
    /* TsdfIntegratorBase::getVoxelWeight: use_const_weight -> 1; else 1 / z^2 of the point's
     * sensor-frame depth z = zaxis . (p - o) (Eigen's x + (y + z)), 0 for |z| <= kEpsilon 1e-6 */
    float w0 = 1.0f;
    if (bw != 0.0f) {
        w0 = fabsf(bw);
    } else if (c->p.depth_weight && (c->zax[0] != 0.0f || c->zax[1] != 0.0f || c->zax[2] != 0.0f)) {
        /* capped at min(max_weight, 2^16): the int64 fixed-point sums cannot overflow (the GPU
         * library's RayConst::w0_cap); an origin-only scan (zero axis) keeps the weight 1 */
        const float cap = c->p.max_weight > 0.0f && c->p.max_weight < TSDF_W0_CAP
                              ? c->p.max_weight : TSDF_W0_CAP;
        const float z = fabsf(c->zax[0] * dx + (c->zax[1] * dy + c->zax[2] * dz));
        w0 = z > 1e-6f ? fminf(1.0f / (z * z), cap) : 0.0f;
    }
    float ex, ey, ez, sx, sy, sz;
    if (clearing) {
        float len = depth - tau;
        len = len > 0.0f ? len : 0.0f;
        len = (float)c->p.max_range < len ? (float)c->p.max_range : len;
        ex = ox + ux * len; ey = oy + uy * len; ez = oz + uz * len;
        if (c->p.space_carving) { sx = ox; sy = oy; sz = oz; }
        else { sx = ex; sy = ey; sz = ez; }
    } else {
        ex = px + ux * tau; ey = py + uy * tau; ez = pz + uz * tau;
        if (c->p.space_carving) { sx = ox; sy = oy; sz = oz; }
        else { sx = px - ux * tau; sy = py - uy * tau; sz = pz - uz * tau; }
    }
    const float ss[3] = {sx * inv_vs, sy * inv_vs, sz * inv_vs};
    const float es[3] = {ex * inv_vs, ey * inv_vs, ez * inv_vs};
    /* the far-ray rule, on the hit point as well: a far point makes no clearing ray either */
    if (!far_ok(ss[0], ss[1], ss[2]) || !far_ok(es[0], es[1], es[2]) ||
        !far_ok(px * inv_vs, py * inv_vs, pz * inv_vs) || !(depth < INFINITY))
        return -1;
    int32_t v[3], st[3];
    float tn[3], td[3];
    int64_t steps = 0;
    for (int a = 0; a < 3; a++) {
        v[a] = (int32_t)floorf(ss[a] + 1e-6f);
        const int32_t e = (int32_t)floorf(es[a] + 1e-6f);
        steps += e > v[a] ? (int64_t)e - v[a] : (int64_t)v[a] - e;
        const float r = es[a] - ss[a];
        st[a] = (0.0f < r) - (r < 0.0f);
        if (st[a] == 0) {
            tn[a] = INFINITY;
            td[a] = INFINITY;
        } else {
            const float corr = st[a] > 0 ? 1.0f : 0.0f;
            tn[a] = (corr - (ss[a] - (float)v[a])) / r;
            td[a] = (float)st[a] / r;
        }
    }
    /* at most MAX_DDA_STEPS voxels, as the other walks (the kernels' vb_init: rem) */
    if (steps > MAX_DDA_STEPS - 1) steps = MAX_DDA_STEPS - 1;
    for (int64_t k = 0;; k++) {
        if (v[0] > -VOX_LIMIT && v[0] < VOX_LIMIT && v[1] > -VOX_LIMIT && v[1] < VOX_LIMIT &&
            v[2] > -VOX_LIMIT && v[2] < VOX_LIMIT) {
            const float cx = ((float)v[0] + 0.5f) * vs;
            const float cy = ((float)v[1] + 0.5f) * vs;
            const float cz = ((float)v[2] + 0.5f) * vs;
            const float ax = cx - ox, ay = cy - oy, az = cz - oz; /* v_voxel_origin */
            const float proj = (ax * dx + (ay * dy + az * dz)) / depth; /* dist_G_V */
            const float sdf = depth - proj;
            float w = w0;
            if (c->p.use_weight_dropoff && sdf < -vs) {
                w = (w * (tau + sdf)) / (tau - vs);
                w = w > 0.0f ? w : 0.0f;
            }
            if (w >= VB_MIN_WEIGHT) visit(c, v[0], v[1], v[2], sdf, w, user);
        }
        if (k >= steps) break;
        /* Eigen minCoeff: the first minimum wins */
        int a = 0;
        if (tn[1] < tn[a]) a = 1;
        if (tn[2] < tn[a]) a = 2;
        v[a] += st[a];
        tn[a] += td[a];
    }
    return steps + 1;
}

static void visit_accum(tsdf_ctx* c, int32_t x, int32_t y, int32_t z, float s, float w,
                        void* user) {
    int* fail = (int*)user;
    int64_t i = vox_get(c, x, y, z);
    if (i < 0) { *fail = 1; return; }
    vox_t* v = &c->tab[i];
    if (c->mode == ORACLE_MODE_SEQUENTIAL && c->sem == TSDF_SEM_VOXBLOX) {
        /* updateTsdfVoxel, literally, in input order */
        const float nw = v->W + w;
        if (!(nw < 1e-6f)) { /* kFloatEpsilon */
            const float ns = (s * w + v->S * v->W) / nw;
            const float tau = c->tau;
            v->S = ns > 0.0f ? (ns < tau ? ns : tau) : (-tau < ns ? ns : -tau);
            v->W = nw < c->p.max_weight ? nw : c->p.max_weight;
        }
        if (v->stamp != c->scan_id) { v->stamp = c->scan_id; c->st.n_voxels_last++; }
        return;
    }
    if (c->mode != ORACLE_MODE_SCAN_FUSED) { /* SEQUENTIAL / VDB_LITERAL: VDBVolume's update */
        const float nw = v->W + w;
        v->S = (v->S * v->W + s * w) / nw;
        v->W = nw;
        if (v->stamp != c->scan_id) { v->stamp = c->scan_id; c->st.n_voxels_last++; }
        return;
    }
    if (v->stamp != c->scan_id) {
        v->stamp = c->scan_id;
        if (c->n_touched == c->touched_cap) {
            uint64_t nc = c->touched_cap ? 2 * c->touched_cap : 4096;
            uint32_t* t = (uint32_t*)realloc(c->touched, nc * sizeof(uint32_t));
            if (!t) { *fail = 1; return; }
            c->touched = t;
            c->touched_cap = nc;
        }
        c->touched[c->n_touched++] = (uint32_t)i;
    }
    if (c->sem == TSDF_SEM_VOXBLOX) {
        v->A += (int64_t)((s * w) * 4294967296.0f); /* trunc(s w 2^32) */
        v->B += (int64_t)(w * 4294967296.0f);       /* trunc(w 2^32) */
        return;
    }
    v->A += (int64_t)(s * 4294967296.0f); /* trunc(s * 2^32): exact scaling, C truncation */
    v->B += 1;
}

static void fuse_scan(tsdf_ctx* c) {
    for (uint64_t k = 0; k < c->n_touched; k++) {
        vox_t* v = &c->tab[c->touched[k]];
        const float a = (float)((double)v->A * (1.0 / 4294967296.0));
        if (c->sem == TSDF_SEM_VOXBLOX) {
            /* updateTsdfVoxel with the scan's samples applied together: (a, b) = (sum s w, sum w) */
            const float b = (float)((double)v->B * (1.0 / 4294967296.0));
            const float nw = v->W + b;
            if (!(nw < 1e-6f)) {
                const float ns = (a + v->S * v->W) / nw;
                const float tau = c->tau;
                v->S = ns > 0.0f ? (ns < tau ? ns : tau) : (-tau < ns ? ns : -tau);
                v->W = nw < c->p.max_weight ? nw : c->p.max_weight;
            }
            v->A = 0;
            v->B = 0;
            continue;
        }
        const float b = (float)v->B;
        const float nw = v->W + b;
        v->S = (v->S * v->W + a) / nw;
        v->W = nw;
        v->A = 0;
        v->B = 0;
    }
    c->st.n_voxels_last = c->n_touched;
    c->n_touched = 0;
}

/* ---- multi-threaded scan-fused mode (the CPU baseline's multi-core leg) ------
 * Bit-identical to the serial scan-fused mode: a voxel's scan update is an exact integer sum
 * (order-free) followed by one fuse per scan, and every voxel lives in exactly one partition.
 *   phase 1  threads walk contiguous ray ranges and bucket each gated sample by its brick's
 *            partition (hash of the 8^3 brick coordinates);
 *   phase 2  thread p accumulates partition p's samples into its own context and fuses them. */
#include <pthread.h>

typedef struct {
    tsdf_ctx* c;
    int t;
    const char* base;
    uint64_t i0, i1;
    uint32_t point_step, xyz_offset;
    int32_t xyz_is_f64;
    float ox, oy, oz;
    const double* origin;
    uint64_t rays;
    int fail;
} mt_job;

static void mt_point(const char* q, int32_t f64, float* px, float* py, float* pz) {
    if (f64) {
        double d[3];
        memcpy(d, q, sizeof d);
        *px = (float)d[0]; *py = (float)d[1]; *pz = (float)d[2];
    } else {
        float f[3];
        memcpy(f, q, sizeof f);
        *px = f[0]; *py = f[1]; *pz = f[2];
    }
}

static void visit_bucket(tsdf_ctx* c, int32_t x, int32_t y, int32_t z, float s, float w,
                         void* user) {
    mt_job* j = (mt_job*)user;
    const int T = c->n_thr;
    /* floor division by the brick side (arithmetic shift) */
    const int p = (int)(mix3(x >> 3, y >> 3, z >> 3) % (uint64_t)T);
    struct mt_bucket* b = &c->bk[j->t * T + p];
    if (b->n == b->cap) {
        const uint64_t nc = b->cap ? 2 * b->cap : 4096;
        mt_sample* v = (mt_sample*)realloc(b->v, nc * sizeof(mt_sample));
        if (!v) { j->fail = 1; return; }
        b->v = v;
        b->cap = nc;
    }
    b->v[b->n++] = (mt_sample){x, y, z, s, w};
}

static void* mt_walk(void* arg) {
    mt_job* j = (mt_job*)arg;
    tsdf_ctx* c = j->c;
    for (uint64_t i = j->i0; i < j->i1 && !j->fail; i++) {
        float px, py, pz, bw = 0.0f;
        const char* q = j->base + i * j->point_step + j->xyz_offset;
        mt_point(q, j->xyz_is_f64, &px, &py, &pz);
        if (c->mg_on) memcpy(&bw, q + 12, sizeof bw);
        int64_t r;
        if (c->sem == TSDF_SEM_VDBFUSION_F64) {
            double pd[3] = {px, py, pz};
            if (j->xyz_is_f64) memcpy(pd, q, sizeof pd);
            r = walk_ray_vdb(c, pd, j->origin, visit_bucket, j);
        } else {
            r = c->sem == TSDF_SEM_VOXBLOX
                    ? walk_ray_vb(c, px, py, pz, j->ox, j->oy, j->oz, bw, visit_bucket, j)
                    : walk_ray(c, px, py, pz, j->ox, j->oy, j->oz, visit_bucket, j);
        }
        if (r >= 0) j->rays++;
    }
    return NULL;
}

static void* mt_fuse(void* arg) {
    mt_job* j = (mt_job*)arg;
    tsdf_ctx* c = j->c;
    const int T = c->n_thr, p = j->t;
    tsdf_ctx* sc = c->sub[p];
    sc->scan_id = c->scan_id;
    sc->st.n_voxels_last = 0;
    for (int t = 0; t < T && !j->fail; t++) {
        struct mt_bucket* b = &c->bk[t * T + p];
        for (uint64_t k = 0; k < b->n && !j->fail; k++)
            visit_accum(sc, b->v[k].x, b->v[k].y, b->v[k].z, b->v[k].s, b->v[k].w, &j->fail);
        b->n = 0;
    }
    fuse_scan(sc);
    return NULL;
}

static int mt_integrate(tsdf_ctx* c, const char* base, uint64_t n, uint32_t point_step,
                        uint32_t xyz_offset, int32_t xyz_is_f64, float ox, float oy, float oz,
                        const double* origin) {
    const int T = c->n_thr;
    mt_job job[64];
    pthread_t th[64];
    for (int phase = 0; phase < 2; phase++) {
        for (int t = 0; t < T; t++) {
            job[t] = (mt_job){c, t, base, n * (uint64_t)t / T, n * (uint64_t)(t + 1) / T,
                              point_step, xyz_offset, xyz_is_f64, ox, oy, oz, origin, 0, 0};
            if (pthread_create(&th[t], NULL, phase ? mt_fuse : mt_walk, &job[t])) {
                for (int k = 0; k < t; k++) pthread_join(th[k], NULL);
                return set_err(c, TSDF_ENOMEM, "oracle thread creation failed");
            }
        }
        int fail = 0;
        for (int t = 0; t < T; t++) {
            pthread_join(th[t], NULL);
            fail |= job[t].fail;
            if (phase == 0) c->st.n_rays_total += job[t].rays;
            else c->st.n_voxels_last += c->sub[t]->st.n_voxels_last;
        }
        if (fail) return set_err(c, TSDF_ENOMEM, "oracle allocation failed");
    }
    c->mt_dirty = 1;
    return TSDF_OK;
}

/* tab <- the union of the partitions (read-outs of the multi-threaded mode) */
static void mt_collect(const tsdf_ctx* cc) {
    tsdf_ctx* c = (tsdf_ctx*)cc;
    if (c->n_thr <= 1 || !c->mt_dirty) return;
    /* sized once for the union (the partitions hold disjoint voxels), not grown insert by insert */
    uint64_t total = 0, ncap = c->cap ? c->cap : (1u << 16);
    for (int p = 0; p < c->n_thr; p++) total += c->sub[p]->n;
    while (2 * (total + 1) > ncap) ncap *= 2;
    if (ncap > c->cap && c->n_touched == 0) {
        vox_t* nt = (vox_t*)calloc(ncap, sizeof(vox_t));
        if (nt) {
            free(c->tab);
            c->tab = nt;
            c->cap = ncap;
        }
    }
    if (c->cap) memset(c->tab, 0, c->cap * sizeof(vox_t));
    c->n = 0;
    for (int p = 0; p < c->n_thr; p++) {
        const tsdf_ctx* sc = c->sub[p];
        for (uint64_t i = 0; i < sc->cap; i++) {
            if (!sc->tab[i].used) continue;
            const int64_t h = vox_get(c, sc->tab[i].x, sc->tab[i].y, sc->tab[i].z);
            if (h < 0) return;
            c->tab[h].S = sc->tab[i].S;
            c->tab[h].W = sc->tab[i].W;
        }
    }
    c->mt_dirty = 0;
}

/* n >= 1 threads; n > 1 selects the partitioned scan-fused mode (before the first scan only) */
int tsdf_oracle_set_threads(tsdf_ctx* c, int n) {
    if (!c || n < 1 || n > 64) return TSDF_EINVAL;
    if (n == 1 && !c->sub) return TSDF_OK;
    if (c->n || c->mode != ORACLE_MODE_SCAN_FUSED || c->sub) return TSDF_EINVAL;
    c->sub = (tsdf_ctx**)calloc((size_t)n, sizeof(tsdf_ctx*));
    c->bk = (struct mt_bucket*)calloc((size_t)n * n, sizeof(struct mt_bucket));
    if (!c->sub || !c->bk) return set_err(c, TSDF_ENOMEM, "oracle allocation failed");
    c->n_thr = n;
    for (int p = 0; p < n; p++)
        if (tsdf_create(&c->p, &c->sub[p]) != TSDF_OK)
            return set_err(c, TSDF_ENOMEM, "oracle allocation failed");
    return TSDF_OK;
}


/* ---- Voxblox MergedTsdfIntegrator: the bundling pre-pass (tsdf_params.voxblox_method) ----------
 *
 * voxblox (ethz-asl/voxblox, unpinned; not in /root/reference -- SURVEY §8a9), restated:
 *   bundleRays:     for every point (index order: integration_order_mode "sorted"):
 *                   isPointValid (as walk_ray_vb: d = |p - o|, < min_range dropped, > max_range a
 *                   clearing point if allow_clear, else dropped); its voxel
 *                   getGridIndexFromPoint(p, 1/vs) = floor(p / vs + kCoordinateEpsilon) goes to
 *                   clear_map or voxel_map, each voxel keeping its points in visiting order
 *   integrateVoxel: per map entry: merged = 0, W = 0; for each point: w = getVoxelWeight (1 or
 *                   1/z^2, walk_ray_vb's w0); w < kEpsilon (1e-6) -> skipped;
 *                   merged = (merged W + (p - o) w) / (W + w) per component; W += w;
 *                   a clearing entry stops after its first kept point.  Then ONE ray from o to
 *                   o + merged, clearing as its map, carrying the weight W (updateTsdfVoxel's
 *                   `weight`; the dropoff multiplies it per voxel)
 *   enable_anti_grazing = false (voxblox's default): no ray skips voxels of other bundles.
 * Stated deviations: the merge runs on p - o in the world frame (upstream on the
 * sensor-frame point_C, rotated back: equal in exact arithmetic); bundles are formed in cloud
 * order (upstream's default "mixed" order visits a bundle's points in another fixed order, which
 * only changes the rounding of the running mean); voxel indices beyond +-2^20 drop the point; a
 * bundle's weight is capped at TSDF_MG_W_CAP (2^20) so the exact fixed-point sums cannot overflow;
 * the bundles' rays update the field in the order of their first points, through the same
 * scan-fused fuse as SimpleTsdfIntegrator (deviation 4). */
#define MG_W_CAP 1048576.0f
#define MG_VOX_LIM (1 << 20)

typedef struct { uint64_t key; uint32_t i; } mg_ent;

static int cmp_mg(const void* a, const void* b) {
    const mg_ent* x = (const mg_ent*)a;
    const mg_ent* y = (const mg_ent*)b;
    if (x->key != y->key) return x->key < y->key ? -1 : 1;
    return x->i < y->i ? -1 : (x->i > y->i);
}

/* the scan's bundled rays as 16-B records (x, y, z, w), w < 0: clearing; *nb of them */
static float* mg_bundle(tsdf_ctx* c, const char* base, uint64_t n, uint32_t point_step,
                        uint32_t xyz_offset, int32_t xyz_is_f64, float ox, float oy, float oz,
                        uint64_t* nb) {
    mg_ent* e = (mg_ent*)malloc((n ? n : 1) * sizeof(mg_ent));
    float* w = (float*)malloc((n ? n : 1) * sizeof(float));
    float* d = (float*)malloc((n ? n : 1) * 3 * sizeof(float));
    float* out = (float*)malloc((n ? n : 1) * 4 * sizeof(float));
    *nb = 0;
    if (!e || !w || !d || !out) {
        free(e); free(w); free(d); free(out);
        return NULL;
    }
    const int have_axis = c->zax[0] != 0.0f || c->zax[1] != 0.0f || c->zax[2] != 0.0f;
    const float cap = c->p.max_weight > 0.0f && c->p.max_weight < TSDF_W0_CAP ? c->p.max_weight
                                                                            : TSDF_W0_CAP;
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; i++) {
        float p[3];
        mt_point(base + i * point_step + xyz_offset, xyz_is_f64, &p[0], &p[1], &p[2]);
        const float dx = p[0] - ox, dy = p[1] - oy, dz = p[2] - oz;
        const float depth = sqrtf(dx * dx + (dy * dy + dz * dz));
        if (!(depth > 0.0f) || depth < (float)c->p.min_range) continue;
        int clearing = 0;
        if (depth > (float)c->p.max_range) {
            if (!c->p.allow_clear) continue;
            clearing = 1;
        }
        int32_t v[3];
        int ok = 1;
        for (int a = 0; a < 3; a++) {
            const float f = floorf(p[a] * c->inv_vs + 1e-6f);
            ok &= f > -(float)MG_VOX_LIM && f < (float)MG_VOX_LIM;
            v[a] = ok ? (int32_t)f : 0;
        }
        if (!ok) continue;
        float pw = 1.0f;
        if (c->p.depth_weight && have_axis) {
            const float z = fabsf(c->zax[0] * dx + (c->zax[1] * dy + c->zax[2] * dz));
            pw = z > 1e-6f ? fminf(1.0f / (z * z), cap) : 0.0f;
        }
        w[i] = pw;
        d[3 * i] = dx; d[3 * i + 1] = dy; d[3 * i + 2] = dz;
        /* key: clearing bit, then the biased 21-bit axes (z, y, x), as the GPU pre-pass */
        e[m].key = ((uint64_t)clearing << 63) | ((uint64_t)(uint32_t)(v[2] + MG_VOX_LIM) << 42) |
                   ((uint64_t)(uint32_t)(v[1] + MG_VOX_LIM) << 21) | (uint64_t)(uint32_t)(v[0] + MG_VOX_LIM);
        e[m].i = (uint32_t)i;
        m++;
    }
    qsort(e, m, sizeof(mg_ent), cmp_mg);
    /* bundles in the order of their first points */
    uint64_t nr = 0;
    for (uint64_t j = 0; j < m;) {
        uint64_t q = j;
        const int clearing = (int)(e[j].key >> 63);
        float mx = 0.0f, my = 0.0f, mz = 0.0f, mw = 0.0f;
        for (; q < m && e[q].key == e[j].key; q++) {
            const uint32_t i = e[q].i;
            const float pw = w[i];
            if (pw < 1e-6f || (clearing && mw > 0.0f)) continue; /* kEpsilon; clearing: first only */
            const float nw = mw + pw;
            mx = (mx * mw + d[3 * i] * pw) / nw;
            my = (my * mw + d[3 * i + 1] * pw) / nw;
            mz = (mz * mw + d[3 * i + 2] * pw) / nw;
            mw = mw + pw;
        }
        if (mw > 0.0f) {
            float* r = out + 4 * nr;
            r[0] = ox + mx; r[1] = oy + my; r[2] = oz + mz;
            const float bw = mw < MG_W_CAP ? mw : MG_W_CAP;
            r[3] = clearing ? -bw : bw;
            e[nr].i = e[j].i; /* reuse: first point of bundle nr */
            e[nr].key = nr;
            nr++;
        }
        j = q;
    }
    /* order the bundles by first point (a stable order independent of the voxel keys) */
    for (uint64_t k = 0; k < nr; k++) e[k].key = ((uint64_t)e[k].i << 32) | e[k].key;
    qsort(e, nr, sizeof(mg_ent), cmp_mg);
    float* res = (float*)malloc((nr ? nr : 1) * 4 * sizeof(float));
    if (res)
        for (uint64_t k = 0; k < nr; k++) memcpy(res + 4 * k, out + 4 * (e[k].key & 0xFFFFFFFFull), 16);
    free(e); free(w); free(d); free(out);
    *nb = nr;
    return res;
}

static int integrate_scan(tsdf_ctx* c, const void* pts, uint64_t n, uint32_t point_step,
                          uint32_t xyz_offset, int32_t xyz_is_f64, const double origin[3]);

int tsdf_integrate(tsdf_ctx* c, const void* pts, uint64_t n, uint32_t point_step,
                   uint32_t xyz_offset, int32_t xyz_is_f64, const double origin[3]) {
    if (!c) return TSDF_EINVAL;
    c->zax[0] = 0.0f; c->zax[1] = 0.0f; c->zax[2] = 0.0f; /* no orientation: weight 1 */
    return integrate_scan(c, pts, n, point_step, xyz_offset, xyz_is_f64, origin);
}

/* pose = (x, y, z, qx, qy, qz, qw): the scan's sensor z axis is the third column of the rotation
 * of the normalised quaternion, in double, rounded to float (the GPU library's pose_of) */
int tsdf_integrate_pose(tsdf_ctx* c, const void* pts, uint64_t n, uint32_t point_step,
                        uint32_t xyz_offset, int32_t xyz_is_f64, const double pose[7]) {
    if (!c) return TSDF_EINVAL;
    if (!pose) return set_err(c, TSDF_EINVAL, "null argument");
    const double qn = pose[3] * pose[3] + pose[4] * pose[4] + pose[5] * pose[5] + pose[6] * pose[6];
    if (!(qn > 0.0) || !isfinite(qn)) return set_err(c, TSDF_EINVAL, "pose quaternion is zero");
    const double nn = sqrt(pose[3] * pose[3] + pose[4] * pose[4] + pose[5] * pose[5] + pose[6] * pose[6]);
    const double x = pose[3] / nn, y = pose[4] / nn, z = pose[5] / nn, w = pose[6] / nn;
    c->zax[0] = (float)(2.0 * (x * z + w * y));
    c->zax[1] = (float)(2.0 * (y * z - w * x));
    c->zax[2] = (float)(1.0 - 2.0 * (x * x + y * y));
    return integrate_scan(c, pts, n, point_step, xyz_offset, xyz_is_f64, pose);
}

static int integrate_scan(tsdf_ctx* c, const void* pts, uint64_t n, uint32_t point_step,
                          uint32_t xyz_offset, int32_t xyz_is_f64, const double origin[3]) {
    if (!c || (!pts && n) || !origin) return set_err(c, TSDF_EINVAL, "null argument");
    if (c->brd_open)
        return set_err(c, TSDF_EINVAL, "a border reduce is open on this context: commit or abort it first");
    const uint32_t need = xyz_is_f64 ? 24u : 12u;
    if (point_step < need || xyz_offset > point_step - need)
        return set_err(c, TSDF_EINVAL, "point_step/xyz_offset inconsistent");
    if (c->p.n_sectors > 1 && c->p.sector_rule == TSDF_SECTOR_RULE_INDEX && !c->mg_on) {
        /* ABI v10, SURVEY §8e: sector k of N takes points [floor(k n / N), floor((k + 1) n / N)) --
           for DLIO's time-sorted cloud (reference odom.cc:635-636) contiguous column ranges (the
           merged bundles of the share are not sliced again) */
        const unsigned __int128 N = c->p.n_sectors, k = c->p.sector;
        const uint64_t lo = (uint64_t)((unsigned __int128)n * k / N);
        const uint64_t hi = (uint64_t)((unsigned __int128)n * (k + 1) / N);
        if (pts) pts = (const char*)pts + lo * point_step;
        n = hi - lo;
    }
    const float ox = (float)origin[0], oy = (float)origin[1], oz = (float)origin[2];
    if (c->sem == TSDF_SEM_VOXBLOX && c->p.voxblox_method == TSDF_VB_MERGED && !c->mg_on) {
        /* MergedTsdfIntegrator: walk the scan's bundled rays instead of its points */
        uint64_t nb = 0;
        float* b = mg_bundle(c, (const char*)pts, n, point_step, xyz_offset, xyz_is_f64, ox, oy, oz,
                             &nb);
        if (!b) return set_err(c, TSDF_ENOMEM, "oracle allocation failed");
        c->mg_on = 1;
        for (int t = 0; t < c->n_thr; t++) c->sub[t]->mg_on = 1;
        const int rc = integrate_scan(c, b, nb, 16, 0, 0, origin);
        c->mg_on = 0;
        for (int t = 0; t < c->n_thr; t++) c->sub[t]->mg_on = 0;
        free(b);
        if (rc == TSDF_OK) c->st.n_points_in += n - nb; /* count the scan's points, not bundles */
        return rc;
    }
    c->scan_id++;
    c->st.n_voxels_last = 0;
    int fail = 0;
    const char* base = (const char*)pts;
    if (c->n_thr > 1) {
        const int rc = mt_integrate(c, base, n, point_step, xyz_offset, xyz_is_f64, ox, oy, oz,
                                     origin);
        if (rc != TSDF_OK) return rc;
        c->st.n_scans++;
        c->st.n_points_in += n;
        c->st.n_voxels_total += c->st.n_voxels_last;
        return TSDF_OK;
    }
    /* TSDF_SEM_VDBFUSION_F64 (scan-fused or sequential) and the VDB_LITERAL mode walk as upstream */
    const int vdb_walk = c->sem == TSDF_SEM_VDBFUSION_F64 || c->mode == ORACLE_MODE_VDB_LITERAL;
    for (uint64_t i = 0; i < n && !fail && vdb_walk; i++) {
        const char* q = base + i * point_step + xyz_offset;
        double pd[3];
        if (xyz_is_f64) {
            memcpy(pd, q, sizeof pd);
        } else {
            float f[3];
            memcpy(f, q, sizeof f);
            pd[0] = f[0]; pd[1] = f[1]; pd[2] = f[2];
        }
        if (walk_ray_vdb(c, pd, origin, visit_accum, &fail) >= 0) c->st.n_rays_total++;
    }
    for (uint64_t i = 0; i < n && !fail && !vdb_walk; i++) {
        const char* q = base + i * point_step + xyz_offset;
        float px, py, pz;
        if (xyz_is_f64) {
            double d[3];
            memcpy(d, q, sizeof d);
            px = (float)d[0]; py = (float)d[1]; pz = (float)d[2];
        } else {
            float f[3];
            memcpy(f, q, sizeof f);
            px = f[0]; py = f[1]; pz = f[2];
        }
        float bw = 0.0f;
        if (c->mg_on) memcpy(&bw, q + 12, sizeof bw);
        const int64_t r = c->sem == TSDF_SEM_VOXBLOX
                              ? walk_ray_vb(c, px, py, pz, ox, oy, oz, bw, visit_accum, &fail)
                              : walk_ray(c, px, py, pz, ox, oy, oz, visit_accum, &fail);
        if (r >= 0) c->st.n_rays_total++;
    }
    if (fail) return set_err(c, TSDF_ENOMEM, "oracle allocation failed");
    if (c->mode == ORACLE_MODE_SCAN_FUSED) fuse_scan(c);
    c->st.n_scans++;
    c->st.n_points_in += n;
    c->st.n_voxels_total += c->st.n_voxels_last;
    return TSDF_OK;
}

int tsdf_sync(tsdf_ctx* c) { return c ? TSDF_OK : TSDF_EINVAL; }

/* The GPU library's diagnostics, present so that a C++ host links against either library: the
 * oracle records no kernel times and writes no per-batch metrics log. */
int tsdf_set_profiling(tsdf_ctx* c, int32_t on) {
    (void)on;
    return c ? TSDF_OK : TSDF_EINVAL;
}

int tsdf_set_profiling_period(tsdf_ctx* c, uint32_t every_mask, uint32_t period) {
    (void)every_mask;
    return c && period ? TSDF_OK : TSDF_EINVAL;
}

int tsdf_set_metrics_log(tsdf_ctx* c, const char* path) {
    if (!c) return TSDF_EINVAL;
    return path ? set_err(c, TSDF_EINVAL, "the oracle writes no metrics log") : TSDF_OK;
}

/* ABI v10: int64 bounds, the GPU library's limits (extent < 2^31, box < 2^40);
   voxels outside the index domain (|i| >= 2^23) read the background */
int tsdf_query_dense(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], float* sdf,
                     float* weight) {
    if (!c || !lo || !hi) return TSDF_EINVAL;
    mt_collect(c);
    uint64_t ext[3];
    for (int a = 0; a < 3; a++) {
        if (hi[a] < lo[a]) return set_err(c, TSDF_EINVAL, "hi < lo");
        ext[a] = (uint64_t)hi[a] - (uint64_t)lo[a];
        if (ext[a] >= (1ull << 31)) return set_err(c, TSDF_EINVAL, "query extent >= 2^31 voxels");
    }
    uint64_t total = 0;
    if (__builtin_mul_overflow(ext[0] * ext[1], ext[2], &total) || total >= (1ull << 40))
        return set_err(c, TSDF_EINVAL, "query box >= 2^40 voxels");
    uint64_t i = 0;
    const int64_t lim = VOX_LIMIT;
    for (int64_t z = lo[2]; z < hi[2]; z++)
        for (int64_t y = lo[1]; y < hi[1]; y++)
            for (int64_t x = lo[0]; x < hi[0]; x++, i++) {
                const int in = x > -lim && x < lim && y > -lim && y < lim && z > -lim && z < lim;
                const vox_t* v = in ? vox_find(c, (int32_t)x, (int32_t)y, (int32_t)z) : NULL;
                if (sdf) sdf[i] = v ? v->S : c->bg;
                if (weight) weight[i] = v ? v->W : 0.0f;
            }
    return TSDF_OK;
}

/* ---- brick view of the voxel map (same shape as the GPU export) ------------------------- */

static int32_t fdiv8(int32_t v) { return (v >= 0) ? v / 8 : -((-v + 7) / 8); }

typedef struct { int32_t b[3]; uint64_t first; } brick_ent;

static int cmp_brick(const void* a, const void* b) {
    const int32_t* x = ((const brick_ent*)a)->b;
    const int32_t* y = ((const brick_ent*)b)->b;
    for (int k = 2; k >= 0; k--) {
        if (x[k] != y[k]) return x[k] < y[k] ? -1 : 1;
    }
    return 0;
}

/* unique bricks holding at least one voxel with W > 0, sorted by (z, y, x): deduplicated through
   an open-addressing set of brick indices first (one entry per brick, not per voxel), then sorted */
static brick_ent* list_bricks(const tsdf_ctx* c, uint64_t* nb) {
    mt_collect(c);
    uint64_t cap = 1024, u = 0;
    while (cap < 2 * (c->n / 64 + 1)) cap *= 2;
    brick_ent* e = (brick_ent*)malloc(cap / 2 * sizeof(brick_ent));
    uint32_t* set = (uint32_t*)malloc(cap * sizeof(uint32_t)); /* entry index + 1; 0 = free */
    if (!e || !set) { free(e); free(set); return NULL; }
    memset(set, 0, cap * sizeof(uint32_t));
    for (uint64_t i = 0; i < c->cap; i++) {
        const vox_t* v = &c->tab[i];
        if (!v->used || !(v->W > 0.0f)) continue;
        const int32_t b[3] = {fdiv8(v->x), fdiv8(v->y), fdiv8(v->z)};
        uint64_t h = mix3(b[0], b[1], b[2]) & (cap - 1);
        for (;; h = (h + 1) & (cap - 1)) {
            if (!set[h]) break;
            const int32_t* q = e[set[h] - 1].b;
            if (q[0] == b[0] && q[1] == b[1] && q[2] == b[2]) break;
        }
        if (set[h]) continue;
        if (2 * (u + 1) > cap) { /* rehash into a set twice the size */
            const uint64_t nc = 2 * cap;
            brick_ent* ne = (brick_ent*)realloc(e, nc / 2 * sizeof(brick_ent));
            uint32_t* ns = (uint32_t*)calloc(nc, sizeof(uint32_t));
            if (!ne || !ns) { free(ne ? ne : e); free(ns); free(set); return NULL; }
            e = ne;
            for (uint64_t j = 0; j < u; j++) {
                uint64_t g = mix3(e[j].b[0], e[j].b[1], e[j].b[2]) & (nc - 1);
                while (ns[g]) g = (g + 1) & (nc - 1);
                ns[g] = (uint32_t)(j + 1);
            }
            free(set);
            set = ns;
            cap = nc;
            h = mix3(b[0], b[1], b[2]) & (cap - 1);
            while (set[h]) h = (h + 1) & (cap - 1);
        }
        e[u].b[0] = b[0]; e[u].b[1] = b[1]; e[u].b[2] = b[2];
        set[h] = (uint32_t)(++u);
    }
    free(set);
    qsort(e, u, sizeof(brick_ent), cmp_brick);
    *nb = u;
    return e;
}

/* index of the sorted brick list by brick coordinates: an open-addressing set of (index + 1) */
typedef struct { uint32_t* slot; uint64_t cap; const brick_ent* e; } brick_index;

static int brick_index_build(brick_index* x, const brick_ent* e, uint64_t nb) {
    x->cap = 1024;
    while (x->cap < 2 * nb) x->cap *= 2;
    x->e = e;
    x->slot = (uint32_t*)calloc(x->cap, sizeof(uint32_t));
    if (!x->slot) return TSDF_ENOMEM;
    for (uint64_t i = 0; i < nb; i++) {
        uint64_t g = mix3(e[i].b[0], e[i].b[1], e[i].b[2]) & (x->cap - 1);
        while (x->slot[g]) g = (g + 1) & (x->cap - 1);
        x->slot[g] = (uint32_t)(i + 1);
    }
    return TSDF_OK;
}

/* the brick's index in the list, -1 when it is not listed */
static int64_t brick_index_find(const brick_index* x, int32_t bx, int32_t by, int32_t bz) {
    for (uint64_t g = mix3(bx, by, bz) & (x->cap - 1); x->slot[g]; g = (g + 1) & (x->cap - 1)) {
        const int32_t* q = x->e[x->slot[g] - 1].b;
        if (q[0] == bx && q[1] == by && q[2] == bz) return (int64_t)x->slot[g] - 1;
    }
    return -1;
}

/* in-brick index z*64 + y*8 + x of voxel (x, y, z) */
static int vox_local(int32_t x, int32_t y, int32_t z) {
    return ((z - 8 * fdiv8(z)) << 6) | ((y - 8 * fdiv8(y)) << 3) | (x - 8 * fdiv8(x));
}

int tsdf_num_bricks(tsdf_ctx* c, uint64_t* n) {
    if (!c || !n) return TSDF_EINVAL;
    uint64_t nb = 0;
    brick_ent* e = list_bricks(c, &nb);
    if (!e) return TSDF_ENOMEM;
    free(e);
    *n = nb;
    return TSDF_OK;
}

int tsdf_export_bricks(tsdf_ctx* c, int32_t* coords, float* sdf, float* weight, uint64_t cap,
                       uint64_t* n_out) {
    if (!c || !n_out) return TSDF_EINVAL;
    uint64_t nb = 0;
    brick_ent* e = list_bricks(c, &nb);
    if (!e) return TSDF_ENOMEM;
    *n_out = nb;
    if (nb > cap) { free(e); return TSDF_EOVERFLOW; }
    for (uint64_t i = 0; i < nb; i++) {
        if (coords) { coords[3 * i] = e[i].b[0]; coords[3 * i + 1] = e[i].b[1]; coords[3 * i + 2] = e[i].b[2]; }
        for (int l = 0; l < 512; l++) {
            if (sdf) sdf[512 * i + l] = c->bg; /* absent voxels: the background */
            if (weight) weight[512 * i + l] = 0.0f;
        }
    }
    if (nb && (sdf || weight)) { /* every stored voxel of a listed brick, in one pass over the table */
        brick_index x;
        if (brick_index_build(&x, e, nb)) { free(e); return TSDF_ENOMEM; }
        for (uint64_t i = 0; i < c->cap; i++) {
            const vox_t* v = &c->tab[i];
            if (!v->used) continue;
            const int64_t bi = brick_index_find(&x, fdiv8(v->x), fdiv8(v->y), fdiv8(v->z));
            if (bi < 0) continue;
            const uint64_t o = 512 * (uint64_t)bi + vox_local(v->x, v->y, v->z);
            if (sdf) sdf[o] = v->S;
            if (weight) weight[o] = v->W;
        }
        free(x.slot);
    }
    free(e);
    return TSDF_OK;
}

static int import_impl(tsdf_ctx* c, const int32_t* coords, const float* sdf, const float* weight,
                       uint64_t n);

int tsdf_import_bricks(tsdf_ctx* c, const int32_t* coords, const float* sdf, const float* weight,
                       uint64_t n) {
    if (!c || (n && (!coords || !sdf || !weight))) return TSDF_EINVAL;
    if (c->brd_open)
        return set_err(c, TSDF_EINVAL, "a border reduce is open on this context: commit or abort it first");
    return import_impl(c, coords, sdf, weight, n);
}

static int import_impl(tsdf_ctx* c, const int32_t* coords, const float* sdf, const float* weight,
                       uint64_t n) {
    if (c->n_thr > 1) return set_err(c, TSDF_EINVAL, "import is not supported in the threaded mode");
    for (uint64_t i = 0; i < n; i++)
        for (int l = 0; l < 512; l++) {
            const float wi = weight[512 * i + l];
            if (!(wi > 0.0f)) continue;
            const int lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
            int64_t k = vox_get(c, coords[3 * i] * 8 + lx, coords[3 * i + 1] * 8 + ly,
                                coords[3 * i + 2] * 8 + lz);
            if (k < 0) return TSDF_ENOMEM;
            vox_t* v = &c->tab[k];
            if (v->W == 0.0f) { /* unobserved: copy (keeps single-owner voxels bit-exact) */
                v->S = sdf[512 * i + l];
                v->W = wi;
                continue;
            }
            const float nw = v->W + wi;
            v->S = (v->S * v->W + sdf[512 * i + l] * wi) / nw;
            /* Voxblox semantics never lets a weight pass max_weight (updateTsdfVoxel's cap): the
             * merged replica weight is capped the same way (an approximation of Voxblox's
             * order-dependent update) */
            v->W = (c->sem == TSDF_SEM_VOXBLOX && nw > c->p.max_weight) ? c->p.max_weight : nw;
        }
    return TSDF_OK;
}

int tsdf_get_stats(tsdf_ctx* c, tsdf_stats* out) {
    if (!c || !out) return TSDF_EINVAL;
    *out = c->st;
    uint64_t nb = 0;
    brick_ent* e = list_bricks(c, &nb);
    if (e) free(e);
    out->n_bricks = nb;
    return TSDF_OK;
}

int tsdf_reset_stats(tsdf_ctx* c) {
    if (!c) return TSDF_EINVAL;
    memset(&c->st, 0, sizeof c->st);
    return TSDF_OK;
}

/* ---- oracle-only helpers for the tests ------------------------------------------------------ */

/* number of voxels with W > 0 */
uint64_t tsdf_oracle_num_voxels(const tsdf_ctx* c) {
    mt_collect(c);
    uint64_t k = 0;
    for (uint64_t i = 0; i < c->cap; i++)
        if (c->tab[i].used && c->tab[i].W > 0.0f) k++;
    return k;
}

typedef struct { int32_t x, y, z; float S, W; } vrec;

static int cmp_vrec(const void* a, const void* b) {
    const vrec* p = (const vrec*)a;
    const vrec* q = (const vrec*)b;
    if (p->z != q->z) return p->z < q->z ? -1 : 1;
    if (p->y != q->y) return p->y < q->y ? -1 : 1;
    if (p->x != q->x) return p->x < q->x ? -1 : 1;
    return 0;
}

/* (z, y, x) order of cmp_vrec by a stable LSD radix sort over the biased coordinates (|index| <
   2^23: 24 bits each), x's bytes first; a byte every record shares is skipped (qsort when the
   scratch buffer cannot be had) */
static void sort_vrec(vrec* r, uint64_t n) {
    vrec* tmp = n > 1 ? (vrec*)malloc(n * sizeof(vrec)) : NULL;
    if (!tmp) {
        if (n > 1) qsort(r, n, sizeof(vrec), cmp_vrec);
        return;
    }
    vrec *src = r, *dst = tmp;
    for (int pass = 0; pass < 9; pass++) {
        const int axis = pass / 3, shift = 8 * (pass % 3);
        uint64_t cnt[256] = {0};
#define VREC_DIGIT(v) \
    (((uint32_t)((axis == 0 ? (v).x : axis == 1 ? (v).y : (v).z) + VOX_LIMIT) >> shift) & 255u)
        for (uint64_t i = 0; i < n; i++) cnt[VREC_DIGIT(src[i])]++;
        int same = 0;
        for (int d = 0; d < 256; d++) same |= cnt[d] == n;
        if (same) continue;
        uint64_t o = 0;
        for (int d = 0; d < 256; d++) {
            const uint64_t k = cnt[d];
            cnt[d] = o;
            o += k;
        }
        for (uint64_t i = 0; i < n; i++) dst[cnt[VREC_DIGIT(src[i])]++] = src[i];
#undef VREC_DIGIT
        vrec* t = src;
        src = dst;
        dst = t;
    }
    if (src != r) memcpy(r, src, n * sizeof(vrec));
    free(tmp);
}

/* every voxel with W > 0, sorted by (z, y, x): ijk[3*i..], sdf[i], w[i] */
int tsdf_oracle_export_voxels(const tsdf_ctx* c, int32_t* ijk, float* sdf, float* w, uint64_t cap,
                              uint64_t* n_out) {
    const uint64_t n = tsdf_oracle_num_voxels(c);
    *n_out = n;
    if (n > cap) return TSDF_EOVERFLOW;
    vrec* r = (vrec*)malloc((n ? n : 1) * sizeof(vrec));
    if (!r) return TSDF_ENOMEM;
    uint64_t k = 0;
    for (uint64_t i = 0; i < c->cap; i++) {
        const vox_t* v = &c->tab[i];
        if (!v->used || !(v->W > 0.0f)) continue;
        r[k].x = v->x; r[k].y = v->y; r[k].z = v->z; r[k].S = v->S; r[k].W = v->W;
        k++;
    }
    sort_vrec(r, n);
    for (uint64_t i = 0; i < n; i++) {
        ijk[3 * i] = r[i].x; ijk[3 * i + 1] = r[i].y; ijk[3 * i + 2] = r[i].z;
        sdf[i] = r[i].S;
        w[i] = r[i].W;
    }
    free(r);
    return TSDF_OK;
}

typedef struct { int32_t* ijk; float* s; uint64_t n, cap; } ray_rec;

static void visit_record(tsdf_ctx* c, int32_t x, int32_t y, int32_t z, float s, float w,
                         void* user) {
    (void)c;
    (void)w;
    ray_rec* r = (ray_rec*)user;
    if (r->n < r->cap) {
        r->ijk[3 * r->n] = x; r->ijk[3 * r->n + 1] = y; r->ijk[3 * r->n + 2] = z;
        r->s[r->n] = s;
    }
    r->n++;
}

/* The gated voxels of ONE ray in DDA order (for closed-form KATs); returns the count, or -1 if
 * the ray is filtered out.  Does not modify the map. */
int64_t tsdf_oracle_ray_voxels(tsdf_ctx* c, const float p[3], const double origin[3],
                               int32_t* ijk, float* sdf, uint64_t cap) {
    ray_rec r = {ijk, sdf, 0, cap};
    const float ox = (float)origin[0], oy = (float)origin[1], oz = (float)origin[2];
    const double pd[3] = {p[0], p[1], p[2]};
    int64_t v = c->sem == TSDF_SEM_VOXBLOX
                    ? walk_ray_vb(c, p[0], p[1], p[2], ox, oy, oz, 0.0f, visit_record, &r)
                : c->mode == ORACLE_MODE_VDB_LITERAL
                    ? walk_ray_vdb(c, pd, origin, visit_record, &r)
                    : walk_ray(c, p[0], p[1], p[2], ox, oy, oz, visit_record, &r);
    if (v < 0) return -1;
    return (int64_t)r.n;
}

/* Per-ray facts of one scan, walked as tsdf_integrate / tsdf_integrate_pose would walk it (the
 * walk of the context's semantics -- TSDF_SEM_VDBFUSION_F64 at upstream's precisions, which
 * tsdf_oracle_ray_voxels does not take --, the pose's z axis for 1/z^2 weights, the bundles of
 * TSDF_VB_MERGED) without touching the map.  Row r is the scan's r-th point (merged: bundle):
 * visited[r] the DDA's voxels, gated or not (-1: the ray is dropped), gated[r] the voxels handed to
 * the fuse, runs[r] the runs of consecutive gated voxels in one brick (k_count's pairs).  Returns
 * the rows written (the points; merged: the bundles), -1 on a failed allocation or a short cap. */
typedef struct {
    int32_t n, runs, b[3];
} facts_rec;

static void visit_facts(tsdf_ctx* c, int32_t x, int32_t y, int32_t z, float s, float w,
                        void* user) {
    (void)c;
    (void)s;
    (void)w;
    facts_rec* r = (facts_rec*)user;
    const int32_t bx = x >> 3, by = y >> 3, bz = z >> 3;
    if (r->n == 0 || bx != r->b[0] || by != r->b[1] || bz != r->b[2]) r->runs++;
    r->b[0] = bx; r->b[1] = by; r->b[2] = bz;
    r->n++;
}

int64_t tsdf_oracle_ray_facts(tsdf_ctx* c, const float* xyz, uint64_t n, const double* ext,
                              int32_t has_pose, int32_t* visited, int32_t* gated, int32_t* runs,
                              uint64_t cap) {
    if (!c || (!xyz && n) || !ext || !visited || !gated || !runs) return -1;
    c->zax[0] = 0.0f; c->zax[1] = 0.0f; c->zax[2] = 0.0f;
    if (has_pose) { /* tsdf_integrate_pose's axis */
        const double nn = sqrt(ext[3] * ext[3] + ext[4] * ext[4] + ext[5] * ext[5] + ext[6] * ext[6]);
        if (!(nn > 0.0) || !isfinite(nn)) return -1;
        const double x = ext[3] / nn, y = ext[4] / nn, z = ext[5] / nn, w = ext[6] / nn;
        c->zax[0] = (float)(2.0 * (x * z + w * y));
        c->zax[1] = (float)(2.0 * (y * z - w * x));
        c->zax[2] = (float)(1.0 - 2.0 * (x * x + y * y));
    }
    const float ox = (float)ext[0], oy = (float)ext[1], oz = (float)ext[2];
    const int merged = c->sem == TSDF_SEM_VOXBLOX && c->p.voxblox_method == TSDF_VB_MERGED;
    const float* rows = xyz;
    uint32_t step = 3;
    float* b = NULL;
    if (merged) {
        uint64_t nb = 0;
        b = mg_bundle(c, (const char*)xyz, n, 12, 0, 0, ox, oy, oz, &nb);
        if (!b) return -1;
        rows = b;
        step = 4;
        n = nb;
    }
    if (n > cap) {
        free(b);
        return -1;
    }
    const int vdb_walk = c->sem == TSDF_SEM_VDBFUSION_F64 || c->mode == ORACLE_MODE_VDB_LITERAL;
    for (uint64_t i = 0; i < n; i++) {
        const float* q = rows + i * step;
        facts_rec r = {0, 0, {0, 0, 0}};
        int64_t v;
        if (vdb_walk) {
            const double pd[3] = {q[0], q[1], q[2]};
            v = walk_ray_vdb(c, pd, ext, visit_facts, &r);
        } else if (c->sem == TSDF_SEM_VOXBLOX) {
            v = walk_ray_vb(c, q[0], q[1], q[2], ox, oy, oz, merged ? q[3] : 0.0f, visit_facts, &r);
        } else {
            v = walk_ray(c, q[0], q[1], q[2], ox, oy, oz, visit_facts, &r);
        }
        visited[i] = v < 0 ? -1 : (int32_t)(v > 0x7fffffff ? 0x7fffffff : v);
        gated[i] = v < 0 ? 0 : r.n;
        runs[i] = v < 0 ? 0 : r.runs;
    }
    free(b);
    return (int64_t)n;
}

/* Host-side azimuth sector selection (same contract as the GPU library's). */
int32_t tsdf_sector_of(float px, float py, const double origin[3], double yaw0,
                       uint32_t n_sectors) {
    if (!origin || n_sectors == 0) return -1;
    const float dx = px - (float)origin[0], dy = py - (float)origin[1];
    if (dx != dx || dy != dy) return -1;
    if (n_sectors == 1) return 0;
    for (uint32_t k = 0; k < n_sectors; k++) {
        const sector_t r = sector_bounds(yaw0, k, n_sectors);
        if (sector_has(&r, dx, dy)) return (int32_t)k;
    }
    return -1;
}

int tsdf_select_sector(const float* xyz, uint64_t n, const double origin[3], double yaw0,
                       uint32_t sector, uint32_t n_sectors, float* out_xyz, uint64_t* n_out) {
    if (!xyz || !origin || !out_xyz || !n_out || n_sectors == 0 || sector >= n_sectors)
        return TSDF_EINVAL;
    const sector_t r = sector_bounds(yaw0, sector, n_sectors);
    const float ox = (float)origin[0], oy = (float)origin[1];
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!sector_has(&r, xyz[3 * i] - ox, xyz[3 * i + 1] - oy)) continue;
        out_xyz[3 * k] = xyz[3 * i]; out_xyz[3 * k + 1] = xyz[3 * i + 1]; out_xyz[3 * k + 2] = xyz[3 * i + 2];
        k++;
    }
    *n_out = k;
    return TSDF_OK;
}

/* ---- border-brick reduce (include/tsdf_hip.h; the GPU's tsdf_border.hip restated) ------------
 * The "device" buffers of the ABI are host memory here.  Bricks are the voxel map's bricks with
 * an observed voxel (list_bricks); a reset brick's voxels go to (bg, 0), so it drops out of the
 * list — the GPU keeps its (empty) brick allocated, which sends zero-weight tiles that merge as
 * no-ops: the two agree on the merged field. */
#define TILE_WORDS TSDF_TILE_WORDS

static uint64_t pack_key(const int32_t b[3]) {
    return (uint64_t)(b[0] + (1 << 20)) | ((uint64_t)(b[1] + (1 << 20)) << 21) |
           ((uint64_t)(b[2] + (1 << 20)) << 42);
}

static int cmp_u64(const void* a, const void* b) {
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : (x > y);
}

int tsdf_brick_keys_device(tsdf_ctx* c, uint64_t* keys, uint64_t cap, uint64_t* n_out) {
    if (!c || !n_out) return TSDF_EINVAL;
    uint64_t nb = 0;
    brick_ent* e = list_bricks(c, &nb);
    if (!e) return TSDF_ENOMEM;
    *n_out = nb;
    if (nb > cap) { free(e); return set_err(c, TSDF_EOVERFLOW, "key buffer too small"); }
    for (uint64_t i = 0; i < nb; i++) keys[i] = pack_key(e[i].b);
    free(e);
    return TSDF_OK;
}

int tsdf_border_pack_device(tsdf_ctx* c, const uint64_t* all_keys, const uint64_t* counts,
                            uint64_t stride, uint32_t world, uint32_t rank, uint32_t* send,
                            uint64_t cap_rows, uint64_t* send_counts) {
    if (!c || !counts || !send_counts || world == 0 || world > TSDF_MAX_WORLD || rank >= world)
        return set_err(c, TSDF_EINVAL, "bad world/rank or null counts");
    if (c->n_thr > 1) return set_err(c, TSDF_EINVAL, "border reduce needs the serial mode");
    if (c->brd_n_sent) return set_err(c, TSDF_EINVAL, "border pack: the open reduce has packed already");
    for (uint32_t r = 0; r < world; r++) {
        if (counts[r] > stride) return set_err(c, TSDF_EINVAL, "counts[r] > stride");
        send_counts[r] = 0;
    }
    uint64_t nb = 0;
    brick_ent* e = list_bricks(c, &nb);
    if (!e) return TSDF_ENOMEM;
    uint32_t* owner = (uint32_t*)malloc((nb ? nb : 1) * sizeof(uint32_t));
    uint64_t* sorted = (uint64_t*)malloc((stride ? stride : 1) * sizeof(uint64_t));
    if (!owner || !sorted) { free(e); free(owner); free(sorted); return TSDF_ENOMEM; }
    for (uint64_t i = 0; i < nb; i++) owner[i] = rank;
    for (uint32_t r = rank; r-- > 0;) { /* descending, so the lowest holder wins */
        memcpy(sorted, all_keys + r * stride, counts[r] * sizeof(uint64_t));
        qsort(sorted, counts[r], sizeof(uint64_t), cmp_u64);
        for (uint64_t i = 0; i < nb; i++) {
            const uint64_t k = pack_key(e[i].b);
            if (bsearch(&k, sorted, counts[r], sizeof(uint64_t), cmp_u64)) owner[i] = r;
        }
    }
    uint64_t rows = 0;
    for (uint64_t i = 0; i < nb; i++)
        if (owner[i] != rank) { send_counts[owner[i]]++; rows++; }
    int rc = TSDF_OK;
    if (send && rows > cap_rows) rc = set_err(c, TSDF_EOVERFLOW, "send buffer too small");
    if (send && rc == TSDF_OK) {
        /* ABI v9: packed WITHOUT resetting; the sent bricks are reset at commit */
        c->brd_sent = (int32_t*)malloc((rows ? rows : 1) * 3 * sizeof(int32_t));
        if (!c->brd_sent) rc = TSDF_ENOMEM;
        uint64_t row = 0;
        for (uint32_t d = 0; d < rank && rc == TSDF_OK; d++)
            for (uint64_t i = 0; i < nb; i++) {
                if (owner[i] != d) continue;
                uint32_t* t = send + row * TILE_WORDS;
                float* ts = (float*)t;
                float* tw = (float*)(t + 512);
                for (int l = 0; l < 512; l++) {
                    const int32_t x = e[i].b[0] * 8 + (l & 7), y = e[i].b[1] * 8 + ((l >> 3) & 7),
                                  z = e[i].b[2] * 8 + (l >> 6);
                    const vox_t* v = vox_find(c, x, y, z);
                    ts[l] = v ? v->S : c->bg;
                    tw[l] = v ? v->W : 0.0f;
                }
                const uint64_t key = pack_key(e[i].b);
                t[1024] = (uint32_t)key; t[1025] = (uint32_t)(key >> 32); t[1026] = 0; t[1027] = 0;
                memcpy(c->brd_sent + 3 * row, e[i].b, 3 * sizeof(int32_t));
                row++;
            }
        if (rc == TSDF_OK) {
            c->brd_n_sent = rows;
            c->brd_open = 1;
        }
    }
    free(e); free(owner); free(sorted);
    return rc;
}

static void key_brick(uint64_t key, int32_t b[3]) {
    b[0] = (int32_t)(key & 0x1FFFFF) - (1 << 20);
    b[1] = (int32_t)((key >> 21) & 0x1FFFFF) - (1 << 20);
    b[2] = (int32_t)((key >> 42) & 0x1FFFFF) - (1 << 20);
}

/* a brick holds an observed voxel here */
static int brick_observed(const tsdf_ctx* c, const int32_t b[3]) {
    for (int l = 0; l < 512; l++) {
        const vox_t* v = vox_find(c, b[0] * 8 + (l & 7), b[1] * 8 + ((l >> 3) & 7), b[2] * 8 + (l >> 6));
        if (v && v->W > 0.0f) return 1;
    }
    return 0;
}

int tsdf_border_merge_device(tsdf_ctx* c, const uint32_t* recv, const uint64_t* recv_counts,
                             uint32_t world) {
    if (!c || !recv_counts || world == 0 || world > TSDF_MAX_WORLD)
        return set_err(c, TSDF_EINVAL, "bad world or null counts");
    if (c->n_thr > 1) return set_err(c, TSDF_EINVAL, "border reduce needs the serial mode");
    uint64_t total = 0;
    for (uint32_t r = 0; r < world; r++) total += recv_counts[r];
    c->brd_open = 1;
    /* ABI v9: every received brick as it is before the merge (restored at abort) */
    if (c->brd_n_bk + 512 * total > c->brd_cap_bk) {
        const uint64_t nc = c->brd_n_bk + 512 * total + 512;
        struct brd_vox* q = (struct brd_vox*)realloc(c->brd_bk, nc * sizeof *q);
        if (!q) return TSDF_ENOMEM;
        c->brd_bk = q;
        c->brd_cap_bk = nc;
    }
    for (uint64_t row = 0; row < total; row++) {
        const uint32_t* t = recv + row * TILE_WORDS;
        int32_t b[3];
        key_brick((uint64_t)t[1024] | ((uint64_t)t[1025] << 32), b);
        for (int l = 0; l < 512; l++) {
            struct brd_vox* o = &c->brd_bk[c->brd_n_bk++];
            o->x = b[0] * 8 + (l & 7); o->y = b[1] * 8 + ((l >> 3) & 7); o->z = b[2] * 8 + (l >> 6);
            const vox_t* v = vox_find(c, o->x, o->y, o->z);
            o->S = v ? v->S : c->bg;
            o->W = v ? v->W : 0.0f;
        }
    }
    for (uint64_t row = 0; row < total; row++) { /* rows are grouped by source, ascending */
        const uint32_t* t = recv + row * TILE_WORDS;
        int32_t b[3];
        key_brick((uint64_t)t[1024] | ((uint64_t)t[1025] << 32), b);
        if (!brick_observed(c, b))
            return set_err(c, TSDF_EINVAL, "border merge: a tile's brick is not held here");
        const int rc = import_impl(c, b, (const float*)t, (const float*)(t + 512), 1);
        if (rc != TSDF_OK) return rc;
    }
    return TSDF_OK;
}

int tsdf_border_commit_device(tsdf_ctx* c, int32_t commit) {
    if (!c) return TSDF_EINVAL;
    if (commit) {
        for (uint64_t i = 0; i < c->brd_n_sent; i++) {
            const int32_t* b = c->brd_sent + 3 * i;
            for (int l = 0; l < 512; l++) {
                const vox_t* v = vox_find(c, b[0] * 8 + (l & 7), b[1] * 8 + ((l >> 3) & 7), b[2] * 8 + (l >> 6));
                if (v) { vox_t* w = &c->tab[v - c->tab]; w->S = c->bg; w->W = 0.0f; } /* mass moved out */
            }
        }
    } else {
        for (uint64_t i = c->brd_n_bk; i-- > 0;) { /* the earliest snapshot of a voxel is written last */
            const struct brd_vox* o = &c->brd_bk[i];
            const vox_t* v = vox_find(c, o->x, o->y, o->z);
            if (v) { vox_t* w = &c->tab[v - c->tab]; w->S = o->S; w->W = o->W; }
        }
    }
    free(c->brd_sent);
    c->brd_sent = NULL;
    c->brd_n_sent = 0;
    c->brd_n_bk = 0;
    c->brd_open = 0;
    return TSDF_OK;
}

/* ---- several contexts in one process (the GPU library's tsdf_create_sharded & co., host-side) */

int tsdf_create_sharded(const tsdf_params* p, uint32_t n, const int32_t* device_ids, tsdf_ctx** out) {
    (void)device_ids;
    if (!p || !out || n == 0 || n > TSDF_MAX_WORLD) return TSDF_EINVAL;
    for (uint32_t k = 0; k < n; k++) out[k] = NULL;
    for (uint32_t k = 0; k < n; k++) {
        tsdf_params q = *p;
        q.n_sectors = n > 1 ? n : 0;
        q.sector = k;
        const int rc = tsdf_create(&q, &out[k]);
        if (rc) {
            for (uint32_t j = 0; j < k; j++) { tsdf_destroy(out[j]); out[j] = NULL; }
            return rc;
        }
    }
    return TSDF_OK;
}

static int sectors_check(tsdf_ctx* const* ctxs, uint32_t n_ctx) {
    if (!ctxs || n_ctx == 0 || n_ctx > TSDF_MAX_WORLD) return TSDF_EINVAL;
    for (uint32_t k = 0; k < n_ctx; k++) {
        const tsdf_ctx* c = ctxs[k];
        if (!c) return TSDF_EINVAL;
        const int sharded = n_ctx == 1 ? c->p.n_sectors <= 1 : c->p.n_sectors == n_ctx;
        if (!sharded || (n_ctx > 1 && (c->p.sector != k || c->p.sector_yaw0 != ctxs[0]->p.sector_yaw0)))
            return set_err(ctxs[0], TSDF_EINVAL, "a context is not its sector of n (same sector_yaw0)");
        if (n_ctx > 1 && c->p.sector_rule != ctxs[0]->p.sector_rule)
            return set_err(ctxs[0], TSDF_EINVAL, "the contexts' sector_rule differs");
        if (c->brd_open)
            return set_err(ctxs[0], TSDF_EINVAL, "a border reduce is open on a context");
    }
    return TSDF_OK;
}

/* every context integrates the whole cloud and keeps its sector's rays (the world rule) or its
 * share's points (the index rule, sliced in integrate_scan): the fields the GPU library's fan-out /
 * split / per-context shares give, bit for bit */
int tsdf_integrate_sectors(tsdf_ctx* const* ctxs, uint32_t n_ctx, const void* pts, uint64_t n,
                           uint32_t point_step, uint32_t xyz_offset, int32_t xyz_is_f64,
                           const double pose[7]) {
    int rc = sectors_check(ctxs, n_ctx);
    for (uint32_t k = 0; k < n_ctx && rc == TSDF_OK; k++) {
        rc = tsdf_integrate_pose(ctxs[k], pts, n, point_step, xyz_offset, xyz_is_f64, pose);
        if (rc && k) snprintf(ctxs[0]->err, sizeof ctxs[0]->err, "%s", ctxs[k]->err);
    }
    return rc;
}

int tsdf_integrate_sectors_origin(tsdf_ctx* const* ctxs, uint32_t n_ctx, const void* pts,
                                  uint64_t n, uint32_t point_step, uint32_t xyz_offset,
                                  int32_t xyz_is_f64, const double origin[3]) {
    int rc = sectors_check(ctxs, n_ctx);
    for (uint32_t k = 0; k < n_ctx && rc == TSDF_OK; k++) {
        rc = tsdf_integrate(ctxs[k], pts, n, point_step, xyz_offset, xyz_is_f64, origin);
        if (rc && k) snprintf(ctxs[0]->err, sizeof ctxs[0]->err, "%s", ctxs[k]->err);
    }
    return rc;
}

/* the GPU library's tsdf_border_reduce_local on host buffers: keys, pack, merge per owner (sources
 * ascending), then commit everywhere, or abort everywhere on any failure */
int tsdf_border_reduce_local(tsdf_ctx* const* ctxs, uint32_t n, uint64_t* bricks_moved) {
    if (!ctxs || n == 0 || n > TSDF_MAX_WORLD) return TSDF_EINVAL;
    for (uint32_t k = 0; k < n; k++)
        if (!ctxs[k]) return TSDF_EINVAL;
    if (bricks_moved) *bricks_moved = 0;
    if (n == 1) return TSDF_OK;
    {   /* test hook (the node's fallback, tests/test_node_stub.py): TSDF_ORACLE_REDUCE_FAIL = k
           makes the first k reduces of the process fail as an aborted transaction would, every
           context unchanged */
        static int fails_left = -1;
        if (fails_left < 0) {
            const char* e = getenv("TSDF_ORACLE_REDUCE_FAIL");
            fails_left = e ? atoi(e) : 0;
        }
        if (fails_left > 0) {
            fails_left--;
            return set_err(ctxs[0], TSDF_EHIP, "injected border-reduce failure (aborted, fields unchanged)");
        }
    }
    int rc = TSDF_OK;
    uint64_t counts[TSDF_MAX_WORLD] = {0}, stride = 1;
    for (uint32_t k = 0; k < n && rc == TSDF_OK; k++) {
        if (ctxs[k]->brd_open) rc = set_err(ctxs[0], TSDF_EINVAL, "a border reduce is open on a context");
        else rc = tsdf_num_bricks(ctxs[k], &counts[k]);
        if (counts[k] > stride) stride = counts[k];
    }
    if (rc) return rc;
    uint64_t* all = (uint64_t*)malloc(stride * n * sizeof(uint64_t));
    uint32_t* send[TSDF_MAX_WORLD] = {0};
    uint64_t sc[TSDF_MAX_WORLD][TSDF_MAX_WORLD];
    memset(sc, 0, sizeof sc);
    if (!all) return TSDF_ENOMEM;
    for (uint64_t i = 0; i < stride * n; i++) all[i] = ~0ull;
    for (uint32_t k = 0; k < n && rc == TSDF_OK; k++)
        rc = tsdf_brick_keys_device(ctxs[k], all + k * stride, stride, &counts[k]);
    for (uint32_t k = 0; k < n && rc == TSDF_OK; k++) {
        send[k] = (uint32_t*)malloc((counts[k] ? counts[k] : 1) * TILE_WORDS * 4);
        if (!send[k]) { rc = TSDF_ENOMEM; break; }
        rc = tsdf_border_pack_device(ctxs[k], all, counts, stride, n, k, send[k], counts[k], sc[k]);
    }
    uint64_t moved = 0;
    for (uint32_t d = 0; d < n && rc == TSDF_OK; d++) {
        uint64_t rcnt[TSDF_MAX_WORLD] = {0}, total = 0;
        for (uint32_t r = 0; r < n; r++) { rcnt[r] = sc[r][d]; total += rcnt[r]; }
        if (!total) continue;
        uint32_t* recv = (uint32_t*)malloc(total * TILE_WORDS * 4);
        if (!recv) { rc = TSDF_ENOMEM; break; }
        uint64_t row = 0;
        for (uint32_t r = 0; r < n; r++) {
            uint64_t off = 0;
            for (uint32_t q = 0; q < d; q++) off += sc[r][q];
            memcpy(recv + row * TILE_WORDS, send[r] + off * TILE_WORDS, rcnt[r] * TILE_WORDS * 4);
            row += rcnt[r];
        }
        rc = tsdf_border_merge_device(ctxs[d], recv, rcnt, n);
        if (rc && d) snprintf(ctxs[0]->err, sizeof ctxs[0]->err, "%s", ctxs[d]->err);
        free(recv);
        moved += total;
    }
    for (uint32_t k = 0; k < n; k++) {
        const int crc = tsdf_border_commit_device(ctxs[k], rc == TSDF_OK);
        if (crc && rc == TSDF_OK) rc = crc;
        free(send[k]);
    }
    free(all);
    if (rc == TSDF_OK && bricks_moved) *bricks_moved = moved;
    return rc;
}

/* ---- mesh halo (the GPU library's tsdf_halo_* on host buffers) ---------------------------- */

int tsdf_halo_keys_device(tsdf_ctx* c, uint64_t* keys, uint64_t cap, uint64_t* n_out) {
    if (!c || !n_out) return TSDF_EINVAL;
    uint64_t nb = 0;
    brick_ent* e = list_bricks(c, &nb);
    if (!e) return TSDF_ENOMEM;
    uint64_t* have = (uint64_t*)malloc((nb ? nb : 1) * sizeof(uint64_t));
    uint64_t* need = (uint64_t*)malloc((nb ? 7 * nb : 1) * sizeof(uint64_t));
    if (!have || !need) { free(e); free(have); free(need); return TSDF_ENOMEM; }
    /* observed bricks only (list_bricks lists the bricks with a W > 0 voxel): a reset copy of a
       brick owned elsewhere (W = 0 after a border reduce) is requested like an absent one */
    for (uint64_t i = 0; i < nb; i++) have[i] = pack_key(e[i].b);
    qsort(have, nb, sizeof(uint64_t), cmp_u64);
    uint64_t m = 0;
    for (uint64_t i = 0; i < nb; i++)
        for (int d = 1; d < 8; d++) {
            const int32_t q[3] = {e[i].b[0] + (d & 1), e[i].b[1] + ((d >> 1) & 1), e[i].b[2] + (d >> 2)};
            if (q[0] >= (1 << 20) || q[1] >= (1 << 20) || q[2] >= (1 << 20)) continue;
            const uint64_t k = pack_key(q);
            if (!bsearch(&k, have, nb, sizeof(uint64_t), cmp_u64)) need[m++] = k;
        }
    qsort(need, m, sizeof(uint64_t), cmp_u64);
    uint64_t u = 0;
    for (uint64_t i = 0; i < m; i++)
        if (u == 0 || need[u - 1] != need[i]) need[u++] = need[i];
    *n_out = u;
    int rc = TSDF_OK;
    if (u > cap) rc = set_err(c, TSDF_EOVERFLOW, "halo key buffer too small");
    else if (u && !keys) rc = set_err(c, TSDF_EINVAL, "null key buffer");
    else if (u) memcpy(keys, need, u * sizeof(uint64_t));
    free(e); free(have); free(need);
    return rc;
}

/* tiles of the requested bricks observed here, in request order */
int tsdf_halo_pack_device(tsdf_ctx* c, const uint64_t* req, uint64_t n_req, uint32_t* send,
                          uint64_t cap_rows, uint64_t* n_rows) {
    if (!c || !n_rows) return TSDF_EINVAL;
    *n_rows = 0;
    if (!n_req) return TSDF_OK;
    if (!req || !send) return set_err(c, TSDF_EINVAL, "null buffer");
    /* the bricks observed here (a W > 0 voxel), as sorted keys */
    uint64_t nb = 0;
    brick_ent* e = list_bricks(c, &nb);
    uint64_t* have = (uint64_t*)malloc((nb ? nb : 1) * sizeof(uint64_t));
    if (!e || !have) { free(e); free(have); return TSDF_ENOMEM; }
    for (uint64_t i = 0; i < nb; i++) have[i] = pack_key(e[i].b);
    free(e);
    qsort(have, nb, sizeof(uint64_t), cmp_u64);
    uint64_t row = 0;
    for (uint64_t i = 0; i < n_req; i++) {
        if (req[i] == ~0ull) continue;
        if (!bsearch(&req[i], have, nb, sizeof(uint64_t), cmp_u64)) continue;
        int32_t b[3];
        key_brick(req[i], b);
        if (row < cap_rows) {
            uint32_t* t = send + row * TILE_WORDS;
            for (int l = 0; l < 512; l++) {
                const vox_t* v = vox_find(c, b[0] * 8 + (l & 7), b[1] * 8 + ((l >> 3) & 7), b[2] * 8 + (l >> 6));
                ((float*)t)[l] = v ? v->S : c->bg;
                ((float*)t)[512 + l] = v ? v->W : 0.0f;
            }
            t[1024] = (uint32_t)req[i]; t[1025] = (uint32_t)(req[i] >> 32); t[1026] = 0; t[1027] = 0;
        }
        row++;
    }
    free(have);
    *n_rows = row;
    return row > cap_rows ? set_err(c, TSDF_EOVERFLOW, "halo send buffer too small") : TSDF_OK;
}

/* ---- marching cubes (mesh extraction over the field) --------------------
 *
 * Semantics (the GPU's tsdf_extract_mesh restates the same):
 *   A cube is the 2x2x2 voxels v + {0,1}^3; it is meshed when all 8 voxels are observed
 *   (W > 0 and W >= min_weight).  Corner c = (c & 1, c >> 1 & 1, c >> 2 & 1) is INSIDE when S < 0.
 *   The case table is built, not transcribed: on every cube face the sign-change edges are paired
 *   into segments (an ambiguous face pairs the crossings around its inside corners, so the two
 *   cubes sharing a face agree), each segment directed with the face's inside corners on its right
 *   (seen from outside the cube), segments chained into cycles, cycles fan-triangulated.
 *   A vertex on edge (a, b) (b = a + axis bit) is corner a's centre + t vs along the axis,
 *   t = S_a / (S_a - S_b), corner centres at (i + 1/2) vs (fp32).
 *   Output: triangle soup, 9 floats per triangle, bricks in (z, y, x) order, cubes by their min
 *   voxel's in-brick index z*64 + y*8 + x, triangles in table order. */

static uint8_t mc_tabs[TSDF_MC_TABLES][256][32]; /* TSDF_MC_*: [case][0] = triangles, then 3 edge ids each */
static int mc_edge_a[12], mc_edge_b[12];
static int mc_ready = 0;

static int mc_edge_of(int a, int b) {
    for (int e = 0; e < 12; e++)
        if ((mc_edge_a[e] == a && mc_edge_b[e] == b) || (mc_edge_a[e] == b && mc_edge_b[e] == a))
            return e;
    return -1;
}

/* TSDF_MC_LORENSEN_RULE: the classic table's ambiguity rule -- an ambiguous face pairs its crossings
 * around the inside corners when at most 4 cube corners are inside, around the outside corners
 * otherwise (Lorensen & Cline's complement symmetry; neighbouring cubes can then disagree) */
static void mc_build_table(int lorensen, uint8_t mc_tab[256][32]) {
    for (int k = 0; k < 256; k++) {
        int nxt[12];
        for (int e = 0; e < 12; e++) nxt[e] = -1;
        for (int d = 0; d < 3; d++) {
            const int u = (d + 1) % 3, w = (d + 2) % 3;
            for (int s = 0; s < 2; s++) {
                /* face corners, counter-clockwise seen from outside (normal (2s-1) e_d) */
                static const int cu_p[4] = {0, 1, 1, 0}, cw_p[4] = {0, 0, 1, 1};
                int q[4];
                for (int i = 0; i < 4; i++) {
                    const int iu = s ? cu_p[i] : cw_p[i], iw = s ? cw_p[i] : cu_p[i];
                    q[i] = (s << d) | (iu << u) | (iw << w);
                }
                int in[4], cr[4], ncr = 0;
                for (int i = 0; i < 4; i++) in[i] = (k >> q[i]) & 1;
                for (int i = 0; i < 4; i++)
                    if (in[i] != in[(i + 1) & 3]) cr[ncr++] = i;
                int pi[2], pj[2], np = 0;
                if (ncr == 2) { pi[0] = cr[0]; pj[0] = cr[1]; np = 1; }
                else if (ncr == 4) {
                    const int around_in = !lorensen || __builtin_popcount((unsigned)k) <= 4;
                    if (in[0] == around_in) { pi[0] = 3; pj[0] = 0; pi[1] = 1; pj[1] = 2; }
                    else { pi[0] = 0; pj[0] = 1; pi[1] = 2; pj[1] = 3; }
                    np = 2;
                }
                for (int t = 0; t < np; t++) {
                    const int i = pi[t], j = pj[t];
                    const int ei = mc_edge_of(q[i], q[(i + 1) & 3]);
                    const int ej = mc_edge_of(q[j], q[(j + 1) & 3]);
                    /* corners q[i+1 .. j] lie on the right of the segment i -> j */
                    const int arc_in = in[(i + 1) & 3];
                    if (arc_in) nxt[ei] = ej; else nxt[ej] = ei;
                }
            }
        }
        int used[12] = {0}, nt = 0;
        for (int e0 = 0; e0 < 12; e0++) {
            if (nxt[e0] < 0 || used[e0]) continue;
            int poly[12], n = 0, e = e0;
            while (!used[e] && n < 12) { used[e] = 1; poly[n++] = e; e = nxt[e]; }
            for (int m = 1; m + 1 < n; m++) {
                mc_tab[k][1 + 3 * nt] = (uint8_t)poly[0];
                mc_tab[k][2 + 3 * nt] = (uint8_t)poly[m];
                mc_tab[k][3 + 3 * nt] = (uint8_t)poly[m + 1];
                nt++;
            }
        }
        mc_tab[k][0] = (uint8_t)nt;
    }
}

static void mc_build(void) {
    int ne = 0;
    for (int d = 0; d < 3; d++)
        for (int base = 0; base < 8; base++)
            if (!(base & (1 << d))) { mc_edge_a[ne] = base; mc_edge_b[ne] = base | (1 << d); ne++; }
    mc_build_table(0, mc_tabs[TSDF_MC_GENERATED]);
    mc_build_table(1, mc_tabs[TSDF_MC_LORENSEN_RULE]);
    /* TSDF_MC_LORENSEN: the published table (include/tsdf_mc_tables.h) renumbered: Bourke vertex v
     * -> corner kv[v], edge e -> edge ke[e]; triangle order and winding kept */
    {
        static const int kv[8] = {0, 1, 3, 2, 4, 5, 7, 6};
        static const int ke[12] = {0, 5, 1, 4, 2, 7, 3, 6, 8, 9, 11, 10};
        for (int b = 0; b < 256; b++) {
            int k = 0, nt = 0;
            for (int v = 0; v < 8; v++)
                if (b >> v & 1) k |= 1 << kv[v];
            memset(mc_tabs[TSDF_MC_LORENSEN][k], 0, 32);
            for (int i = 0; i < 15 && tsdf_mc_tri_table[b][i] >= 0; i += 3, nt++)
                for (int j = 0; j < 3; j++)
                    mc_tabs[TSDF_MC_LORENSEN][k][1 + 3 * nt + j] = (uint8_t)ke[tsdf_mc_tri_table[b][i + j]];
            mc_tabs[TSDF_MC_LORENSEN][k][0] = (uint8_t)nt;
        }
    }
    mc_ready = 1;
}

int tsdf_mc_table(uint8_t* out) { return tsdf_mc_table_of(TSDF_MC_GENERATED, out); }

int tsdf_mc_table_of(int32_t table, uint8_t* out) {
    if (!out || table < 0 || table >= TSDF_MC_TABLES) return TSDF_EINVAL;
    if (!mc_ready) mc_build();
    memcpy(out, mc_tabs[table], sizeof mc_tabs[table]);
    return TSDF_OK;
}

int tsdf_extract_mesh(tsdf_ctx* c, float min_weight, float* tri, uint64_t cap, uint64_t* n_tri) {
    return tsdf_extract_mesh_table(c, min_weight, TSDF_MC_GENERATED, tri, cap, n_tri);
}

/* halo tiles (ABI v9) sorted by key for the corner lookups of mesh_impl */
typedef struct { uint64_t key; const uint32_t* tile; } halo_ent;

static int cmp_halo(const void* a, const void* b) {
    const uint64_t x = ((const halo_ent*)a)->key, y = ((const halo_ent*)b)->key;
    return x < y ? -1 : (x > y);
}

static int mesh_impl(tsdf_ctx* c, float min_weight, int32_t table, const uint32_t* halo,
                     uint64_t n_halo, float* tri, uint64_t cap, uint64_t* n_tri) {
    if (!c || !n_tri) return TSDF_EINVAL;
    if (table < 0 || table >= TSDF_MC_TABLES)
        return set_err(c, TSDF_EINVAL, "unknown marching-cubes table");
    if (n_halo && !halo) return set_err(c, TSDF_EINVAL, "null halo tiles");
    if (!mc_ready) mc_build();
    const uint8_t(*mc_tab)[32] = mc_tabs[table];
    halo_ent* h = (halo_ent*)malloc((n_halo ? n_halo : 1) * sizeof(halo_ent));
    if (!h) return TSDF_ENOMEM;
    for (uint64_t i = 0; i < n_halo; i++) {
        h[i].tile = halo + i * TILE_WORDS;
        h[i].key = (uint64_t)h[i].tile[1024] | ((uint64_t)h[i].tile[1025] << 32);
    }
    qsort(h, n_halo, sizeof(halo_ent), cmp_halo);
    uint64_t nb = 0;
    brick_ent* e = list_bricks(c, &nb);
    if (!e) { free(h); return TSDF_ENOMEM; }
    const float vs = c->vs;
    uint64_t nt = 0;
    /* the observed voxels in dense per-brick tiles (one pass over the voxel table; brick i of the
       sorted list at tile i), so a cube's corners are array reads instead of hash probes */
    brick_index bx;
    float* ts = (float*)calloc((nb ? nb : 1) * 512, sizeof(float));
    float* tw = (float*)calloc((nb ? nb : 1) * 512, sizeof(float));
    if (brick_index_build(&bx, e, nb) || !ts || !tw) {
        free(bx.slot); free(ts); free(tw); free(e); free(h);
        return TSDF_ENOMEM;
    }
    for (uint64_t i = 0; i < c->cap; i++) {
        const vox_t* v = &c->tab[i];
        if (!v->used || !(v->W > 0.0f)) continue;
        const int64_t bi = brick_index_find(&bx, fdiv8(v->x), fdiv8(v->y), fdiv8(v->z));
        const int l = vox_local(v->x, v->y, v->z);
        ts[(uint64_t)bi * 512 + l] = v->S;
        tw[(uint64_t)bi * 512 + l] = v->W;
    }
    /* the brick's 9^3 corner neighbourhood: its own voxels from its tile, a neighbour brick's from
       its halo tile when there is one, else from its tile here (corner()'s precedence); cu[] =
       usable (observed, W >= min_weight) */
    float cs[729];
    uint8_t cu[729];
    for (uint64_t b = 0; b < nb; b++) {
        const int32_t x0 = e[b].b[0] * 8, y0 = e[b].b[1] * 8, z0 = e[b].b[2] * 8;
        for (int d = 0; d < 8; d++) {
            const int32_t nbk[3] = {e[b].b[0] + (d & 1), e[b].b[1] + ((d >> 1) & 1), e[b].b[2] + (d >> 2)};
            const float *S = NULL, *W = NULL;
            if (d == 0) {
                S = ts + b * 512; W = tw + b * 512;
            } else {
                if (n_halo) {
                    const halo_ent q = {pack_key(nbk), NULL};
                    const halo_ent* f = (const halo_ent*)bsearch(&q, h, n_halo, sizeof(halo_ent), cmp_halo);
                    if (f) { S = (const float*)f->tile; W = (const float*)f->tile + 512; }
                }
                if (!S) {
                    const int64_t bi = brick_index_find(&bx, nbk[0], nbk[1], nbk[2]);
                    if (bi >= 0) { S = ts + (uint64_t)bi * 512; W = tw + (uint64_t)bi * 512; }
                }
            }
            /* the part of the 9^3 block this brick covers: local 0..7 (own) or 0 (neighbour side) */
            const int nx = (d & 1) ? 1 : 8, ny = ((d >> 1) & 1) ? 1 : 8, nz = (d >> 2) ? 1 : 8;
            for (int lz = 0; lz < nz; lz++)
                for (int ly = 0; ly < ny; ly++)
                    for (int lx = 0; lx < nx; lx++) {
                        const int m = ((d >> 2) ? 8 : lz) * 81 + (((d >> 1) & 1) ? 8 : ly) * 9 + ((d & 1) ? 8 : lx);
                        const int l = (lz << 6) | (ly << 3) | lx;
                        const float wv = W ? W[l] : 0.0f;
                        cu[m] = wv > 0.0f && wv >= min_weight;
                        cs[m] = S ? S[l] : 0.0f;
                    }
        }
        for (int l = 0; l < 512; l++) {
            const int32_t x = x0 + (l & 7), y = y0 + ((l >> 3) & 7), z = z0 + (l >> 6);
            const int m0 = (l >> 6) * 81 + ((l >> 3) & 7) * 9 + (l & 7);
            float S[8];
            int ok = 1, k = 0;
            for (int q = 0; q < 8 && ok; q++) {
                const int m = m0 + ((q >> 2) & 1) * 81 + ((q >> 1) & 1) * 9 + (q & 1);
                if (!cu[m]) { ok = 0; break; }
                S[q] = cs[m];
                if (S[q] < 0.0f) k |= 1 << q;
            }
            if (!ok) continue;
            const int ntc = mc_tab[k][0];
            for (int t = 0; t < ntc; t++) {
                if (nt < cap && tri) {
                    for (int j = 0; j < 3; j++) {
                        const int ed = mc_tab[k][1 + 3 * t + j];
                        const int a = mc_edge_a[ed], bb = mc_edge_b[ed];
                        const int ax = (a ^ bb) == 1 ? 0 : ((a ^ bb) == 2 ? 1 : 2);
                        const float tt = S[a] / (S[a] - S[bb]);
                        float p[3] = {((float)(x + (a & 1)) + 0.5f) * vs,
                                      ((float)(y + ((a >> 1) & 1)) + 0.5f) * vs,
                                      ((float)(z + ((a >> 2) & 1)) + 0.5f) * vs};
                        p[ax] = p[ax] + tt * vs;
                        tri[9 * nt + 3 * j] = p[0];
                        tri[9 * nt + 3 * j + 1] = p[1];
                        tri[9 * nt + 3 * j + 2] = p[2];
                    }
                }
                nt++;
            }
        }
    }
    free(bx.slot); free(ts); free(tw);
    free(e);
    free(h);
    *n_tri = nt;
    return (tri && nt > cap) ? TSDF_EOVERFLOW : TSDF_OK;  /* tri == NULL: count only */
}

int tsdf_extract_mesh_table(tsdf_ctx* c, float min_weight, int32_t table, float* tri,
                            uint64_t cap, uint64_t* n_tri) {
    return mesh_impl(c, min_weight, table, NULL, 0, tri, cap, n_tri);
}

int tsdf_extract_mesh_halo(tsdf_ctx* c, float min_weight, int32_t table, const uint32_t* halo,
                           uint64_t n_halo, float* tri, uint64_t cap, uint64_t* n_tri) {
    return mesh_impl(c, min_weight, table, halo, n_halo, tri, cap, n_tri);
}

/* the GPU library's tsdf_extract_mesh_local: reduce, halo exchange, one mesh per context,
 * soups concatenated in context order */
int tsdf_extract_mesh_local(tsdf_ctx* const* ctxs, uint32_t n, float min_weight, int32_t table,
                            float* tri, uint64_t cap, uint64_t* n_tri) {
    if (!ctxs || n == 0 || n > TSDF_MAX_WORLD || !n_tri) return TSDF_EINVAL;
    for (uint32_t k = 0; k < n; k++)
        if (!ctxs[k]) return TSDF_EINVAL;
    *n_tri = 0;
    if (n == 1) return tsdf_extract_mesh_table(ctxs[0], min_weight, table, tri, cap, n_tri);
    int rc = tsdf_border_reduce_local(ctxs, n, NULL);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n && rc == TSDF_OK; k++) {
        uint64_t nr = 0;
        rc = tsdf_halo_keys_device(ctxs[k], NULL, 0, &nr);
        if (rc == TSDF_EOVERFLOW) rc = TSDF_OK;
        uint64_t* req = (uint64_t*)malloc((nr ? nr : 1) * sizeof(uint64_t));
        uint32_t* halo = (uint32_t*)malloc((nr ? nr : 1) * TILE_WORDS * 4);
        if (!req || !halo) rc = TSDF_ENOMEM;
        uint64_t got = 0, nh = 0;
        if (rc == TSDF_OK) rc = tsdf_halo_keys_device(ctxs[k], req, nr, &got);
        for (uint32_t j = 0; j < n && rc == TSDF_OK; j++) {
            if (j == k) continue;
            uint64_t rows = 0;
            rc = tsdf_halo_pack_device(ctxs[j], req, nr, halo + nh * TILE_WORDS, nr - nh, &rows);
            nh += rows;
        }
        uint64_t nt = 0;
        if (rc == TSDF_OK) {
            rc = mesh_impl(ctxs[k], min_weight, table, halo, nh, tri && total <= cap ? tri + 9 * total : NULL,
                           tri && total <= cap ? cap - total : 0, &nt);
            if (rc == TSDF_EOVERFLOW) rc = TSDF_OK;
        }
        total += nt;
        free(req);
        free(halo);
    }
    *n_tri = total;
    if (rc == TSDF_OK && tri && total > cap) rc = set_err(ctxs[0], TSDF_EOVERFLOW, "mesh buffer too small");
    return rc;
}

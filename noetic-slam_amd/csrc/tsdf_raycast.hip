// tsdf_raycast.hip — the map seen along rays (include/tsdf_hip_raycast.h): depth,
// surface normal and a hit flag per ray, one lane per ray.
//   k_raycast<MODE>  marches the lattice t_k = t_min + (float)k * step, samples the field at
//                    p_k = o + t_k * d exactly as tsdf_sample_device does (tsdf_sample_dev.h: the
//                    same functions), and stops at the first front-facing zero crossing between
//                    two valid samples.
//
// A lane walks its own ray: per-lane table probes, as in tsdf_sample.hip (wave-shared probes lost
// there by 1.8-2.7x).  What the march saves against sampling the whole lattice:
//   - it stops at the hit;
//   - a lane keeps the pool slots of the bricks it probed last (BrickCache): at step = voxel / 2 a
//     ray takes ~16 samples per brick and probes once;
//   - samples in bricks the map does not hold are skipped in one jump (below) -- on a lidar map
//     ~96 % of the lattice samples before the hit.
// TSDF_RAYCAST_SKIP=0 (A/B builds, `make variants`) is the plain march, one sample at a time; both
// give the same bits.
// TSDF_RAYCAST_COUNT=1 (a diagnostic build for profiles/raycast_bench.py; its outputs are counters,
// not results): depth = the lattice samples the lane evaluated in the march, normal = (the skip's
// probe evaluations, the hash-table probes, the k at which the march ended: the samples a full
// march takes).
#include "tsdf_sample_dev.h"

#ifndef TSDF_RAYCAST_SKIP
#define TSDF_RAYCAST_SKIP 1
#endif
#ifndef TSDF_RAYCAST_COUNT
#define TSDF_RAYCAST_COUNT 0
#endif
#if TSDF_RAYCAST_COUNT
#define RC_COUNT(x) ((x)++)
#else
#define RC_COUNT(x) ((void)0)
#endif

namespace tsdf {

namespace {

constexpr int RC_THREADS = 256;

// The pool slots of the bricks (bx, by, bz) + offset o a lane probed last (bit o of `have`),
// INVALID_SLOT where the map lacks the brick.  NC = 1 (nearest) or 8 (trilinear).
template <int NC>
struct BrickCache {
    int bx, by, bz;
    uint32_t have;
    uint32_t slot[NC];
#if TSDF_RAYCAST_COUNT
    uint32_t probes;
#endif
};

template <int NC>
__device__ __forceinline__ void cache_aim(BrickCache<NC>& C, int bx, int by, int bz) {
    if (C.bx != bx || C.by != by || C.bz != bz) {
        C.bx = bx;
        C.by = by;
        C.bz = bz;
        C.have = 0;
    }
}

// resolve_lane through the cache: the same bricks in the same order, probed only where the lane
// does not hold the answer yet.  Offset 0, the base brick, comes first.
template <int NC>
__device__ __forceinline__ bool resolve_cached(const Table& T, BrickCache<NC>& C, uint32_t m,
                                               uint32_t (&cslot)[NC]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < NC; c++) cslot[c] = INVALID_SLOT;
#pragma unroll
    for (uint32_t o = 0; o < (uint32_t)NC; o++) {
        if (ok && (o & ~m) == 0) {
            if (!((C.have >> o) & 1u)) {
                C.slot[o] = brick_slot(T, C.bx + (int)(o & 1), C.by + (int)((o >> 1) & 1),
                                       C.bz + (int)(o >> 2));
                C.have |= 1u << o;
                RC_COUNT(C.probes);
            }
            const uint32_t s = C.slot[o];
            if (s == INVALID_SLOT) {
                ok = false;
            } else {
#pragma unroll
                for (uint32_t c = 0; c < (uint32_t)NC; c++)
                    if ((c & m) == o) cslot[c] = s;
            }
        }
    }
    return ok;
}

struct Ray {
    float ox, oy, oz, dx, dy, dz;
};

template <int MODE>
__device__ __forceinline__ Base base_at(const Ray& r, float inv, float t) {
    const float px = r.ox + t * r.dx, py = r.oy + t * r.dy, pz = r.oz + t * r.dz;
    return MODE == 0 ? base_nearest(inv, true, px, py, pz) : base_trilinear(inv, true, px, py, pz);
}

#if TSDF_RAYCAST_SKIP
// t where the ray leaves the slab [lo, lo + w) of one axis (an estimate: any value is safe)
__device__ __forceinline__ float slab_exit(float lo, float w, float o, float d) {
    const float inf = __builtin_inff();
    if (d > 0.0f) return ((lo + w) - o) / d;
    if (d < 0.0f) return (lo - o) / d;
    return inf;
}
#endif

// One lane per ray.  n_k: the number of lattice samples, the k with t_k <= t_max (the lattice is
// the same for every ray, so the host counts it once, with the same fp32 expression).
template <int MODE>
__global__ __launch_bounds__(RC_THREADS) void k_raycast(
    Table T, Pool Pl, float inv, float vs, float bg, const float* __restrict__ org,
    const float* __restrict__ dir, uint64_t n, OsPose P, int has_pose, float t_min, float step,
    uint32_t n_k, float min_w, float* __restrict__ out_depth, float* __restrict__ out_normal,
    uint8_t* __restrict__ out_hit) {
    constexpr int NC = MODE == 0 ? 1 : 8;
    const uint64_t stride = (uint64_t)gridDim.x * RC_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < n; i += stride) {
        Ray r{org[3 * i], org[3 * i + 1], org[3 * i + 2], dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]};
        if (has_pose) {
            const float x = r.ox, y = r.oy, z = r.oz, u = r.dx, v = r.dy, w = r.dz;
            r.ox = ((P.m[0] * x + P.m[1] * y) + P.m[2] * z) + P.m[3];
            r.oy = ((P.m[4] * x + P.m[5] * y) + P.m[6] * z) + P.m[7];
            r.oz = ((P.m[8] * x + P.m[9] * y) + P.m[10] * z) + P.m[11];
            r.dx = (P.m[0] * u + P.m[1] * v) + P.m[2] * w;
            r.dy = (P.m[4] * u + P.m[5] * v) + P.m[6] * w;
            r.dz = (P.m[8] * u + P.m[9] * v) + P.m[10] * w;
        }
        BrickCache<NC> C;
        C.bx = C.by = C.bz = INT32_MIN;
        C.have = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) C.slot[c] = INVALID_SLOT;

        bool prev_valid = false, hit = false;
        float prev_s = 0.0f, depth = 0.0f;
        uint32_t k = 0;
#if TSDF_RAYCAST_COUNT
        uint32_t n_march = 0, n_jump = 0;
        C.probes = 0;
#endif
        while (k < n_k) {
            RC_COUNT(n_march);
            const float t = t_min + (float)k * step;
            const Base b = base_at<MODE>(r, inv, t);
            if (!b.inside) {  // invalid by the sampling rules (non-finite, or off the index domain)
                prev_valid = false;
                k++;
                continue;
            }
            const int bx = b.x >> 3, by = b.y >> 3, bz = b.z >> 3;
            cache_aim(C, bx, by, bz);
            uint32_t cslot[NC];
            const bool ok = resolve_cached<NC>(T, C, MODE == 0 ? 0u : straddle_mask(b), cslot);
            if (!ok) {
                prev_valid = false;
                uint32_t next = k + 1;
#if TSDF_RAYCAST_SKIP
                // The skip.  A sample whose base brick B (the brick of its base voxel: the voxel
                // itself, or corner 0 of the trilinear cube) is not in the map is invalid in both
                // modes.  For a finite ray every step from k to the base brick coordinate is
                // monotone in its input -- (float)k, fl(k * step), fl(t_min + .), fl(t * d_a),
                // fl(o_a + .), . * inv (- 0.5f), floorf, >> 3 -- so on every axis the base brick
                // coordinate of sample k is monotone in k, and the samples whose base voxel lies
                // in B form one contiguous run of k.  If sample kc > k, evaluated by the very
                // formula of the march, is inside the index domain with base brick B again, then
                // every sample of k..kc has base brick B (each coordinate lies between two equal
                // values) and is invalid, exactly as the full march finds them: the march goes on
                // at kc + 1 with "previous sample invalid".  A hit needs two consecutive valid
                // samples, so no hit lies in k..kc + 1 either way, and the result is bit for bit
                // the full march's.  How kc is guessed does not matter for that: the exit of the
                // ray from B's box is estimated in fast arithmetic, one sample is kept in hand,
                // and a guess that overshoots B is halved until it lands in B or reaches k.
                // (Only cslot[0]'s brick failing is used: a missing neighbour brick of the
                // trilinear cube invalidates this sample only, and the march steps by one.)
                if (C.slot[0] == INVALID_SLOT) {
                    const float off = MODE == 0 ? 0.0f : 0.5f, w = 8.0f * vs;
                    float te = slab_exit(((float)(bx * 8) + off) * vs, w, r.ox, r.dx);
                    te = fminf(te, slab_exit(((float)(by * 8) + off) * vs, w, r.oy, r.dy));
                    te = fminf(te, slab_exit(((float)(bz * 8) + off) * vs, w, r.oz, r.dz));
                    float kf = floorf((te - t_min) / step) - 1.0f;
                    kf = fminf(kf, (float)(n_k - 1));
                    if (kf > (float)k) {  // false for a NaN estimate
                        uint32_t kc = (uint32_t)kf;
                        while (kc > k) {
                            RC_COUNT(n_jump);
                            const Base c = base_at<MODE>(r, inv, t_min + (float)kc * step);
                            if (c.inside && (c.x >> 3) == bx && (c.y >> 3) == by &&
                                (c.z >> 3) == bz) {
                                next = kc + 1;
                                break;
                            }
                            kc = k + (kc - k) / 2;
                        }
                    }
                }
#endif
                k = next;
                continue;
            }
            Sample s;
            if constexpr (MODE == 0)
                s = eval_nearest(Pl, bg, min_w, b, cslot[0]);
            else
                s = eval_trilinear(Pl, inv, bg, min_w, b, cslot);
            if (s.valid && prev_valid && prev_s > 0.0f && s.s <= 0.0f) {
                const float t0 = t_min + (float)(k - 1) * step;
                depth = t0 + (t - t0) * (prev_s / (prev_s - s.s));
                hit = true;
                break;
            }
            prev_valid = s.valid;
            prev_s = s.s;
            k++;
        }
#if TSDF_RAYCAST_COUNT
        out_depth[i] = (float)n_march;
        out_hit[i] = hit ? 1 : 0;
        if (out_normal) {
            out_normal[3 * i] = (float)n_jump;
            out_normal[3 * i + 1] = (float)C.probes;
            out_normal[3 * i + 2] = (float)(hit ? k + 1 : k);
        }
        continue;
#endif
        out_depth[i] = depth;
        out_hit[i] = hit ? 1 : 0;
        if (out_normal) {
            float nx = 0.0f, ny = 0.0f, nz = 0.0f;
            if (hit) {
                // the trilinear sample at the hit point, whatever the march's mode
                const Base b = base_trilinear(inv, true, r.ox + depth * r.dx, r.oy + depth * r.dy,
                                              r.oz + depth * r.dz);
                uint32_t cslot[8];
                if (resolve_lane<8>(T, b.inside, b.x >> 3, b.y >> 3, b.z >> 3, straddle_mask(b),
                                    cslot)) {
                    const Sample g = eval_trilinear(Pl, inv, bg, min_w, b, cslot);
                    const float n2 = (g.gx * g.gx + g.gy * g.gy) + g.gz * g.gz;
                    if (g.valid && n2 > 0.0f) {
                        const float l = sqrtf(n2);
                        nx = g.gx / l;
                        ny = g.gy / l;
                        nz = g.gz / l;
                    }
                }
            }
            out_normal[3 * i] = nx;
            out_normal[3 * i + 1] = ny;
            out_normal[3 * i + 2] = nz;
        }
    }
}

}  // namespace

hipError_t launch_raycast(const Table& T, const Pool& Pl, const RayConst& R, const float* d_org,
                          const float* d_dir, uint64_t n, const OsPose* P, float t_min, float step,
                          uint32_t n_k, int mode, float min_w, float* d_depth, float* d_normal,
                          uint8_t* d_hit, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint64_t g = (n + RC_THREADS - 1) / RC_THREADS;
    const uint32_t grid = (uint32_t)(g > 8192 ? 8192 : g);
    OsPose Q{};
    if (P) Q = *P;
    if (mode == 0)
        k_raycast<0><<<grid, RC_THREADS, 0, st>>>(T, Pl, R.inv_vs, R.vs, R.bg, d_org, d_dir, n, Q,
                                                  P ? 1 : 0, t_min, step, n_k, min_w, d_depth,
                                                  d_normal, d_hit);
    else
        k_raycast<1><<<grid, RC_THREADS, 0, st>>>(T, Pl, R.inv_vs, R.vs, R.bg, d_org, d_dir, n, Q,
                                                  P ? 1 : 0, t_min, step, n_k, min_w, d_depth,
                                                  d_normal, d_hit);
    return hipGetLastError();
}

}  // namespace tsdf

// tsdf_sample.hip — sparse map queries (include/tsdf_hip_sample.h): the field
// sampled at arbitrary world points, one lane per point.
//   k_sample<MODE>  nearest voxel, or the trilinear interpolant of the 8 surrounding voxel centres
//                   with its analytic gradient
//   k_align         the trilinear sample of a cloud under a candidate pose, reduced to the
//                   Gauss-Newton terms of the point-to-TSDF error (21 + 6 + 1 doubles and a count)
//                   per workgroup by a fixed tree; k_align_sum adds the workgroups' partials in
//                   workgroup order (no floating-point atomics: the same bits on every call)
//
// Lookup scheme.  A point's 8 corners lie in 1, 2, 4 or 8 bricks: the base voxel's brick, plus one
// more per axis on which the cube crosses a brick face (b & 7 == 7) -- a lane probes the hash table
// for the bricks of its straddling axes only (about two thirds of the points need one probe), never
// 8 times.  A lane whose cube has an unallocated brick is invalid whatever its other bricks hold,
// and drops its remaining lookups.  The corner weights are read first; the 8 distances only where
// all 8 weights pass.
// TSDF_SAMPLE_SHARED=1 (A/B builds, `make variants`): each DISTINCT brick a wave needs is probed
// once, wave-uniformly (the leader loop of resolve_shared), and every lane that needs it takes the
// pool slot from that probe.  It issues far fewer requests and measured 1.8-2.7x SLOWER (DESIGN.md
// §11): a scan's wave touches tens of distinct bricks, the leader loop walks them one dependent
// round trip after the other, while the per-lane probes are all in flight at once.  Not shipped.
#include "tsdf_device.h"
#include "tsdf_ray.h"

#ifndef TSDF_SAMPLE_SHARED
#define TSDF_SAMPLE_SHARED 0
#endif

namespace tsdf {

namespace {

constexpr int SMP_THREADS = 256;
constexpr int SMP_WAVES = SMP_THREADS / 64;
constexpr int ALIGN_ACC = 28;  // H's upper triangle (21, row-major), b (6), sum r^2

// pool slot of a brick, INVALID_SLOT when the map does not hold it
__device__ __forceinline__ uint32_t brick_slot(const Table& T, int bx, int by, int bz) {
    const int64_t h = table_find(T, pack_brick(bx, by, bz));
    if (h < 0) return INVALID_SLOT;
    const uint32_t s = T.slots[h];
    return s < T.max_bricks ? s : INVALID_SLOT;
}

// The pool slots of a lane's NC corners (corner c = dx | dy << 1 | dz << 2): corner c lies in brick
// (bx, by, bz) + the offset c & m, m the lane's mask of straddling axes.  Returns false when the
// lane is inactive or one of its bricks is not in the map.  Every lane of the wave calls it.
// (The A/B variant, TSDF_SAMPLE_SHARED.)
template <int NC>
__device__ __forceinline__ bool resolve_shared(const Table& T, bool active, int bx, int by, int bz,
                                               uint32_t m, uint32_t (&cslot)[NC]) {
    // pend: bit o set while the brick at offset o (a subset of m) is still to be looked up
    uint32_t pend = 0;
    if (active) {
#pragma unroll
        for (uint32_t o = 0; o < (uint32_t)NC; o++)
            if ((o & ~m) == 0) pend |= 1u << o;
    }
    bool ok = active;
#pragma unroll
    for (int c = 0; c < NC; c++) cslot[c] = INVALID_SLOT;
    for (;;) {
        const uint64_t bal = __ballot(pend != 0);
        if (!bal) break;
        // the first lane with a pending brick leads: its lowest pending brick is probed once for
        // the wave, and every lane waiting for that brick takes the result
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)bal) - 1);
        const uint32_t lp = (uint32_t)__builtin_amdgcn_readlane((int)pend, leader);
        const int o = __ffs(lp) - 1;
        const int kx = __builtin_amdgcn_readlane(bx, leader) + (o & 1);
        const int ky = __builtin_amdgcn_readlane(by, leader) + ((o >> 1) & 1);
        const int kz = __builtin_amdgcn_readlane(bz, leader) + (o >> 2);
        const uint32_t s = brick_slot(T, kx, ky, kz);
        const uint32_t dx = (uint32_t)(kx - bx), dy = (uint32_t)(ky - by), dz = (uint32_t)(kz - bz);
        const uint32_t om = (dx | (dy << 1) | (dz << 2)) & 7u;
        if ((dx | dy | dz) <= 1u && ((pend >> om) & 1u)) {
            if (s == INVALID_SLOT) {
                ok = false;
                pend = 0;
            } else {
                pend &= ~(1u << om);
#pragma unroll
                for (uint32_t c = 0; c < (uint32_t)NC; c++)
                    if ((c & m) == om) cslot[c] = s;
            }
        }
    }
    return ok;
}

// the shipped lookup: every lane probes its own 1, 2, 4 or 8 bricks
template <int NC>
__device__ __forceinline__ bool resolve_lane(const Table& T, bool active, int bx, int by, int bz,
                                              uint32_t m, uint32_t (&cslot)[NC]) {
    bool ok = active;
#pragma unroll
    for (int c = 0; c < NC; c++) cslot[c] = INVALID_SLOT;
#pragma unroll
    for (uint32_t o = 0; o < (uint32_t)NC; o++) {
        if (ok && (o & ~m) == 0) {
            const uint32_t s = brick_slot(T, bx + (int)(o & 1), by + (int)((o >> 1) & 1),
                                          bz + (int)(o >> 2));
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

template <int NC>
__device__ __forceinline__ bool resolve(const Table& T, bool active, int bx, int by, int bz,
                                        uint32_t m, uint32_t (&cslot)[NC]) {
#if TSDF_SAMPLE_SHARED
    return resolve_shared<NC>(T, active, bx, by, bz, m, cslot);
#else
    return resolve_lane<NC>(T, active, bx, by, bz, m, cslot);
#endif
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

struct Sample {
    float s, w, gx, gy, gz;
    bool valid;
};

// The voxel floorf(p * inv): its (S, W), (bg, 0) where unallocated or outside |i| < 2^23.
__device__ __forceinline__ Sample sample_nearest(const Table& T, const Pool& Pl, float inv, float bg,
                                                 float min_w, bool live, float px, float py,
                                                 float pz) {
    const float vx = floorf(px * inv), vy = floorf(py * inv), vz = floorf(pz * inv);
    const float lim = (float)VOX_LIMIT;
    // decided on the floats (a NaN fails every comparison); the conversions below are then exact
    const bool inside = live && vx > -lim && vx < lim && vy > -lim && vy < lim && vz > -lim &&
                        vz < lim;
    const int x = inside ? (int)vx : 0, y = inside ? (int)vy : 0, z = inside ? (int)vz : 0;
    uint32_t cslot[1];
    const bool ok = resolve<1>(T, inside, x >> 3, y >> 3, z >> 3, 0u, cslot);
    Sample r{bg, 0.0f, 0.0f, 0.0f, 0.0f, false};
    if (ok) {
        const size_t i = (size_t)cslot[0] * BRICK_VOX + (((z & 7) << 6) | ((y & 7) << 3) | (x & 7));
        r.s = Pl.sdf[i];
        r.w = Pl.weight[i];
        r.valid = r.w > 0.0f && r.w >= min_w;
    }
    return r;
}

// The trilinear interpolant of the 8 voxel centres around p and its gradient (tsdf_hip_sample.h).
__device__ __forceinline__ Sample sample_trilinear(const Table& T, const Pool& Pl, float inv,
                                                   float bg, float min_w, bool live, float px,
                                                   float py, float pz) {
    const float ux = px * inv - 0.5f, uy = py * inv - 0.5f, uz = pz * inv - 0.5f;
    const float bfx = floorf(ux), bfy = floorf(uy), bfz = floorf(uz);
    const float fx = ux - bfx, fy = uy - bfy, fz = uz - bfz;
    // every corner b + {0, 1} inside |i| < 2^23, decided on the floats
    const float lo = -(float)(VOX_LIMIT - 1), hi = (float)(VOX_LIMIT - 2);
    const bool inside = live && isfinite(px) && isfinite(py) && isfinite(pz) && bfx >= lo &&
                        bfx <= hi && bfy >= lo && bfy <= hi && bfz >= lo && bfz <= hi;
    const int x = inside ? (int)bfx : 0, y = inside ? (int)bfy : 0, z = inside ? (int)bfz : 0;
    const int lx = x & 7, ly = y & 7, lz = z & 7;
    const uint32_t m = (lx == 7 ? 1u : 0u) | (ly == 7 ? 2u : 0u) | (lz == 7 ? 4u : 0u);
    uint32_t cslot[8];
    const bool ok = resolve<8>(T, inside, x >> 3, y >> 3, z >> 3, m, cslot);
    Sample r{bg, 0.0f, 0.0f, 0.0f, 0.0f, false};
    if (ok) {
        size_t idx[8];
        float w[8];
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int l = (((lz + (c >> 2)) & 7) << 6) | (((ly + ((c >> 1) & 1)) & 7) << 3) |
                          ((lx + (c & 1)) & 7);
            idx[c] = (size_t)cslot[c] * BRICK_VOX + l;
            w[c] = Pl.weight[idx[c]];
        }
        bool all = true;
        float wmin = w[0];
#pragma unroll
        for (int c = 0; c < 8; c++) {
            all = all && w[c] > 0.0f && w[c] >= min_w;
            wmin = fminf(wmin, w[c]);
        }
        if (all) {
            float s[8];
#pragma unroll
            for (int c = 0; c < 8; c++) s[c] = Pl.sdf[idx[c]];
            // s[dx | dy << 1 | dz << 2]; S: x, then y, then z
            const float c00 = lerp(s[0], s[1], fx), c10 = lerp(s[2], s[3], fx);
            const float c01 = lerp(s[4], s[5], fx), c11 = lerp(s[6], s[7], fx);
            r.s = lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz);
            r.w = wmin;
            // d/dx: the x differences over (y, z); d/dy: the y differences over (x, z); d/dz: the z
            // differences over (x, y)
            r.gx = lerp(lerp(s[1] - s[0], s[3] - s[2], fy), lerp(s[5] - s[4], s[7] - s[6], fy), fz) *
                   inv;
            r.gy = lerp(lerp(s[2] - s[0], s[3] - s[1], fx), lerp(s[6] - s[4], s[7] - s[5], fx), fz) *
                   inv;
            r.gz = lerp(lerp(s[4] - s[0], s[5] - s[1], fx), lerp(s[6] - s[2], s[7] - s[3], fx), fy) *
                   inv;
            r.valid = true;
        }
    }
    return r;
}

// One lane per point; the workgroup's loop bounds are uniform, so whole waves stay in the loop (the
// shared-lookup variant is a wave-wide operation) and lanes past n merely sample nothing.
template <int MODE>
__global__ __launch_bounds__(SMP_THREADS) void k_sample(Table T, Pool Pl, float inv, float bg,
                                                        const float* __restrict__ xyz, uint64_t n,
                                                        float min_w, float* __restrict__ out_s,
                                                        float* __restrict__ out_w,
                                                        float* __restrict__ out_g,
                                                        uint8_t* __restrict__ out_v) {
    const uint64_t stride = (uint64_t)gridDim.x * SMP_THREADS;
    for (uint64_t base = (uint64_t)blockIdx.x * SMP_THREADS; base < n; base += stride) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < n;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        if (live) {
            px = xyz[3 * i];
            py = xyz[3 * i + 1];
            pz = xyz[3 * i + 2];
        }
        const Sample r = MODE == 0 ? sample_nearest(T, Pl, inv, bg, min_w, live, px, py, pz)
                                   : sample_trilinear(T, Pl, inv, bg, min_w, live, px, py, pz);
        if (live) {
            out_s[i] = r.s;
            out_w[i] = r.w;
            out_v[i] = r.valid ? 1 : 0;
            if (out_g) {
                out_g[3 * i] = r.gx;
                out_g[3 * i + 1] = r.gy;
                out_g[3 * i + 2] = r.gz;
            }
        }
    }
}

// part[blockIdx.x * ALIGN_PART + k]: the workgroup's sums (k < ALIGN_ACC) and its valid count (as a
// double, k = ALIGN_ACC).  Shape of the sum: per lane over its points in index order, a xor
// butterfly over the wave's 64 lanes, then the workgroup's waves in order.
__global__ __launch_bounds__(SMP_THREADS) void k_align(Table T, Pool Pl, float inv, float bg,
                                                       const float* __restrict__ xyz, uint64_t n,
                                                       OsPose P, float min_w,
                                                       double* __restrict__ part) {
    double acc[ALIGN_ACC];
#pragma unroll
    for (int k = 0; k < ALIGN_ACC; k++) acc[k] = 0.0;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * SMP_THREADS;
    for (uint64_t base = (uint64_t)blockIdx.x * SMP_THREADS; base < n; base += stride) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < n;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (live) {
            x = xyz[3 * i];
            y = xyz[3 * i + 1];
            z = xyz[3 * i + 2];
        }
        const float qx = ((P.m[0] * x + P.m[1] * y) + P.m[2] * z) + P.m[3];
        const float qy = ((P.m[4] * x + P.m[5] * y) + P.m[6] * z) + P.m[7];
        const float qz = ((P.m[8] * x + P.m[9] * y) + P.m[10] * z) + P.m[11];
        const Sample r = sample_trilinear(T, Pl, inv, bg, min_w, live, qx, qy, qz);
        if (r.valid) {
            const double gx = r.gx, gy = r.gy, gz = r.gz, res = r.s;
            const double dx = qx, dy = qy, dz = qz;
            const double J[6] = {gx, gy, gz, dy * gz - dz * gy, dz * gx - dx * gz, dx * gy - dy * gx};
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++) acc[k++] += J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; a++) acc[21 + a] += J[a] * res;
            acc[27] += res * res;
            cnt++;
        }
    }
#pragma unroll
    for (int k = 0; k < ALIGN_ACC; k++)
        for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d, 64);
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    __shared__ double sh[SMP_WAVES][ALIGN_ACC + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < ALIGN_ACC; k++) sh[wave][k] = acc[k];
        sh[wave][ALIGN_ACC] = (double)cnt;
    }
    __syncthreads();
    if (threadIdx.x <= ALIGN_ACC) {
        double v = sh[0][threadIdx.x];
        for (int wv = 1; wv < SMP_WAVES; wv++) v += sh[wv][threadIdx.x];
        part[(size_t)blockIdx.x * ALIGN_PART + threadIdx.x] = v;
    }
}

// out[k] = the workgroups' partials added in workgroup order
__global__ __launch_bounds__(64) void k_align_sum(const double* __restrict__ part, uint32_t n_wg,
                                                  double* __restrict__ out) {
    if (threadIdx.x > ALIGN_ACC) return;
    double v = 0.0;
#pragma unroll 8
    for (uint32_t g = 0; g < n_wg; g++) v += part[(size_t)g * ALIGN_PART + threadIdx.x];
    out[threadIdx.x] = v;
}

// workgroups of a launch over n points: capped like k_query_dense's grid, the kernels stride
uint32_t sample_grid(uint64_t n, uint32_t cap) {
    const uint64_t g = (n + SMP_THREADS - 1) / SMP_THREADS;
    return (uint32_t)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

hipError_t launch_sample(const Table& T, const Pool& Pl, const RayConst& R, const float* d_xyz,
                         uint64_t n, int mode, float min_w, float* d_sdf, float* d_w, float* d_grad,
                         uint8_t* d_valid, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint32_t grid = sample_grid(n, 8192);
    if (mode == 0)
        k_sample<0><<<grid, SMP_THREADS, 0, st>>>(T, Pl, R.inv_vs, R.bg, d_xyz, n, min_w, d_sdf, d_w,
                                                  d_grad, d_valid);
    else
        k_sample<1><<<grid, SMP_THREADS, 0, st>>>(T, Pl, R.inv_vs, R.bg, d_xyz, n, min_w, d_sdf, d_w,
                                                  d_grad, d_valid);
    return hipGetLastError();
}

hipError_t launch_align(const Table& T, const Pool& Pl, const RayConst& R, const float* d_xyz,
                        uint64_t n, const OsPose& P, float min_w, double* d_part, hipStream_t st) {
    const uint32_t grid = sample_grid(n, ALIGN_MAX_WG);
    k_align<<<grid, SMP_THREADS, 0, st>>>(T, Pl, R.inv_vs, R.bg, d_xyz, n, P, min_w, d_part);
    k_align_sum<<<1, 64, 0, st>>>(d_part, grid, d_part + (size_t)ALIGN_MAX_WG * ALIGN_PART);
    return hipGetLastError();
}

}  // namespace tsdf

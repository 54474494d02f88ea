// tsdf_esdf.hip — the Euclidean distance field of a map box (include/tsdf_hip_esdf.h, DESIGN.md
// §14): the exact distance transform of the box's surface voxels, truncated at R voxels.
//   k_esdf_classify   reads (S, W) of every voxel of the box as k_query_dense does and writes its
//                     class byte (observed, site, S < 0) and g = site ? 0 : INF
//   k_esdf_x          g'(i) = min over |d| <= R inside the box of g(i + d) + d^2 along x
//   k_esdf_axis<0>    the same along y
//   k_esdf_axis<1>    the same along z, and the epilogue: the cap at R^2, one sqrtf, the scale by
//                     the voxel size, the sign and the flags
// The squared distances are integers in 16-bit planes (3 * 128^2 < INF = 0xFFFF; the sums are taken
// in 32 bits, so nothing saturates).  A pass stages a tile of its input in LDS with a halo of R
// voxels on either side of the pass axis (INF beyond the box: the box is the world) and each lane
// scans outward from d = 0; it stops once d^2 is no smaller than its running minimum, which is
// exact because g >= 0.  A tile that stages no finite value skips its scans (a workgroup vote): its
// results are INF whatever the scan does, and on a lidar map most tiles of the x pass are such.
// Tile shapes and their LDS bytes: esdf_plan.h.
//
// Flat launches on the context's stream, no workgroup waits on another, no atomics: every voxel's
// result is a pure function of the box, so the bits do not depend on scheduling.
#include "esdf_plan.h"
#include "tsdf_device.h"
#include "tsdf_ray.h"

// Offsets per round of a voxel's scan in the y and z passes; -DESDF_UNROLL=1 is the plain loop (an
// A/B build; DESIGN.md §14 has both times).  Both give the same bits.
#ifndef ESDF_UNROLL
#define ESDF_UNROLL 4
#endif

namespace tsdf {

namespace {

constexpr uint32_t CLS_OBSERVED = 1u, CLS_SITE = 2u, CLS_NEGATIVE = 8u;
constexpr uint32_t WAVES = ESDF_THREADS / ESDF_LANES;

__global__ __launch_bounds__(ESDF_THREADS) void k_esdf_classify(
    Table T, Pool Pl, int64_t lo0, int64_t lo1, int64_t lo2, uint32_t nx, uint32_t ny,
    uint64_t total, float bg, float band, float min_w, uint16_t* __restrict__ g,
    uint8_t* __restrict__ cls) {
    const uint64_t stride = (uint64_t)gridDim.x * ESDF_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * ESDF_THREADS + threadIdx.x; i < total; i += stride) {
        const int64_t xl = lo0 + (int64_t)(i % nx);
        const int64_t yl = lo1 + (int64_t)((i / nx) % ny);
        const int64_t zl = lo2 + (int64_t)(i / ((uint64_t)nx * ny));
        float s = bg, w = 0.0f;
        if (xl > -VOX_LIMIT && xl < VOX_LIMIT && yl > -VOX_LIMIT && yl < VOX_LIMIT &&
            zl > -VOX_LIMIT && zl < VOX_LIMIT) {
            const int x = (int)xl, y = (int)yl, z = (int)zl;
            const int64_t h = table_find(T, brick_key_of(x, y, z));
            if (h >= 0) {
                const uint32_t slot = T.slots[h];
                if (slot < T.max_bricks) {
                    const int l = ((z & 7) << 6) | ((y & 7) << 3) | (x & 7);
                    s = Pl.sdf[(size_t)slot * BRICK_VOX + l];
                    w = Pl.weight[(size_t)slot * BRICK_VOX + l];
                }
            }
        }
        const bool observed = w > 0.0f && w >= min_w;
        const bool site = observed && fabsf(s) <= band;
        cls[i] = (uint8_t)((observed ? CLS_OBSERVED : 0u) | (site ? CLS_SITE : 0u) |
                           (observed && s < 0.0f ? CLS_NEGATIVE : 0u));
        g[i] = (uint16_t)(site ? 0u : ESDF_INF);
    }
}

// The scan of one voxel: p points at its own cell of the tile, the cells at +-d lie `step` apart.
// The sums are 32-bit, so INF + d^2 cannot wrap and never beats a running minimum <= INF: no test
// for INF is needed.  U offsets are taken per round, their reads in flight together (one LDS round
// trip a round instead of one per offset: the scan is bound by that latency), and the exit is
// tested once a round: the offsets looked at beyond the exact exit have d^2 >= best and change
// nothing.  The x pass takes U = 1: its offsets are neighbouring 16-bit cells, which the compiler
// merges into wide reads off their natural alignment (measured: twice the plain loop's time).
template <uint32_t U>
__device__ __forceinline__ uint32_t scan_out(const uint16_t* p, uint32_t h, uint32_t step) {
    uint32_t best = p[0];
    uint32_t d = 1;
    if constexpr (U > 1) {
        for (; d + (U - 1) <= h; d += U) {
            if (d * d >= best) return best;
            uint32_t a[U], b[U];
#pragma unroll
            for (uint32_t k = 0; k < U; k++) {
                a[k] = p[-(int)((d + k) * step)];
                b[k] = p[(d + k) * step];
            }
#pragma unroll
            for (uint32_t k = 0; k < U; k++) {
                const uint32_t m = (a[k] < b[k] ? a[k] : b[k]) + (d + k) * (d + k);
                if (m < best) best = m;
            }
        }
    }
    for (; d <= h; d++) {
        const uint32_t dd = d * d;
        if (dd >= best) break;
        const uint32_t a = p[-(int)(d * step)], b = p[d * step];
        const uint32_t m = (a < b ? a : b) + dd;
        if (m < best) best = m;
    }
    return best;
}

// The x pass over `lines` = ny * nz lines of nx voxels: a tile is ESDF_X_LINES lines by ESDF_LANES
// voxels, each row staged with h voxels on either side.
__global__ __launch_bounds__(ESDF_THREADS) void k_esdf_x(const uint16_t* __restrict__ in,
                                                          uint16_t* __restrict__ out, uint32_t nx,
                                                          uint64_t lines, uint32_t h,
                                                          uint64_t tiles) {
    extern __shared__ __attribute__((aligned(16))) uint16_t esdf_tile[];
    const uint32_t lane = threadIdx.x % ESDF_LANES, wave = threadIdx.x / ESDF_LANES;
    const uint32_t W = ESDF_LANES + 2 * h;
    const uint64_t xt = (nx + ESDF_LANES - 1) / ESDF_LANES;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t x0 = (uint32_t)(t % xt) * ESDF_LANES;
        const uint64_t l0 = (t / xt) * ESDF_X_LINES;
        uint32_t seen = ESDF_INF;  // the smallest value this lane staged
        for (uint32_t r = wave; r < ESDF_X_LINES; r += WAVES) {
            const uint64_t line = l0 + r;
            for (uint32_t c = lane; c < W; c += ESDF_LANES) {
                const int64_t x = (int64_t)x0 + c - h;
                uint32_t v = ESDF_INF;
                if (line < lines && x >= 0 && x < (int64_t)nx) v = in[line * nx + (uint64_t)x];
                esdf_tile[r * W + c] = (uint16_t)v;
                seen = v < seen ? v : seen;
            }
        }
        // a tile without a finite value gives INF everywhere: no scan (most tiles of a sparse map)
        const bool live = __syncthreads_or(seen != ESDF_INF);
        for (uint32_t r = wave; r < ESDF_X_LINES; r += WAVES) {
            const uint64_t line = l0 + r;
            const uint32_t x = x0 + lane;
            if (line < lines && x < nx)
                out[line * nx + x] = (uint16_t)(
                    live ? scan_out<1>(esdf_tile + r * W + h + lane, h, 1) : ESDF_INF);
        }
        __syncthreads();
    }
}

// A pass along an axis of n voxels with `inner` contiguous voxels below it and `outer` slabs above
// it (y: inner = nx, outer = nz; z: inner = nx ny, outer = 1).  Lanes run along the inner index, so
// the global loads and stores are contiguous; a tile is ESDF_LANES of them by seg voxels of the
// axis, staged with h rows on either side.  LAST: the epilogue instead of the plane.
template <bool LAST>
__global__ __launch_bounds__(ESDF_THREADS) void k_esdf_axis(
    const uint16_t* __restrict__ in, uint16_t* __restrict__ out, uint64_t inner, uint32_t n,
    uint32_t h, uint32_t seg, uint64_t tiles, uint32_t r2, float vs,
    const uint8_t* __restrict__ cls, float* __restrict__ dist, uint8_t* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) uint16_t esdf_tile[];
    const uint32_t lane = threadIdx.x % ESDF_LANES, wave = threadIdx.x / ESDF_LANES;
    const uint64_t it = (inner + ESDF_LANES - 1) / ESDF_LANES;
    const uint64_t st = (n + seg - 1) / seg;
    const uint32_t rows = seg + 2 * h;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i = (t % it) * ESDF_LANES + lane;
        const uint64_t rest = t / it;
        const uint32_t j0 = (uint32_t)(rest % st) * seg;
        const uint64_t base = (rest / st) * n * inner;
        uint32_t seen = ESDF_INF;
        for (uint32_t r = wave; r < rows; r += WAVES) {
            const int64_t j = (int64_t)j0 + r - h;
            uint32_t v = ESDF_INF;
            if (i < inner && j >= 0 && j < (int64_t)n) v = in[base + (uint64_t)j * inner + i];
            esdf_tile[r * ESDF_LANES + lane] = (uint16_t)v;
            seen = v < seen ? v : seen;
        }
        const bool live = __syncthreads_or(seen != ESDF_INF);  // (as in k_esdf_x)
        for (uint32_t r = wave; r < seg; r += WAVES) {
            const uint32_t j = j0 + r;
            if (i < inner && j < n) {
                const uint32_t best =
                    live ? scan_out<ESDF_UNROLL>(esdf_tile + (h + r) * ESDF_LANES + lane, h,
                                                 ESDF_LANES)
                         : ESDF_INF;
                const uint64_t idx = base + (uint64_t)j * inner + i;
                if constexpr (LAST) {
                    const uint32_t c = cls[idx];
                    const bool capped = best > r2;  // (INF > R^2: no site counts as capped)
                    float f = sqrtf((float)(capped ? r2 : best)) * vs;
                    if (c & CLS_NEGATIVE) f = -f;  // a site behind the surface: -0.0f
                    dist[idx] = f;
                    if (flags)
                        flags[idx] = (uint8_t)((c & (CLS_OBSERVED | CLS_SITE)) | (capped ? 4u : 0u));
                } else {
                    out[idx] = (uint16_t)best;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_esdf(const Table& T, const Pool& Pl, const int64_t lo[3], const uint32_t n[3],
                       uint32_t radius, float band, float min_w, float bg, float vs, uint16_t* d_g0,
                       uint16_t* d_g1, uint8_t* d_cls, float* d_dist, uint8_t* d_flags,
                       hipStream_t st) {
    EsdfBox B{{n[0], n[1], n[2]}, (uint64_t)n[0] * n[1] * n[2]};
    if (!B.total) return hipSuccess;
    const uint64_t g = esdf_ceil_div(B.total, ESDF_THREADS);
    k_esdf_classify<<<esdf_grid(g), ESDF_THREADS, 0, st>>>(T, Pl, lo[0], lo[1], lo[2], n[0], n[1],
                                                           B.total, bg, band, min_w, d_g0, d_cls);
    const uint32_t hx = esdf_halo(radius, n[0]), hy = esdf_halo(radius, n[1]),
                   hz = esdf_halo(radius, n[2]);
    const uint32_t seg = esdf_seg(radius);
    const uint64_t tx = esdf_tiles_x(B);
    k_esdf_x<<<esdf_grid(tx), ESDF_THREADS, esdf_lds_x(hx), st>>>(d_g0, d_g1, n[0],
                                                                  (uint64_t)n[1] * n[2], hx, tx);
    const uint64_t ty = esdf_tiles_axis(radius, n[0], n[1], n[2]);
    k_esdf_axis<false><<<esdf_grid(ty), ESDF_THREADS, esdf_lds_axis(radius, hy), st>>>(
        d_g1, d_g0, n[0], n[1], hy, seg, ty, 0u, 0.0f, nullptr, nullptr, nullptr);
    const uint64_t plane = (uint64_t)n[0] * n[1];
    const uint64_t tz = esdf_tiles_axis(radius, plane, n[2], 1);
    k_esdf_axis<true><<<esdf_grid(tz), ESDF_THREADS, esdf_lds_axis(radius, hz), st>>>(
        d_g0, nullptr, plane, n[2], hz, seg, tz, radius * radius, vs, d_cls, d_dist, d_flags);
    return hipGetLastError();
}

}  // namespace tsdf

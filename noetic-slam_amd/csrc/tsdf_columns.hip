// tsdf_columns.hip — the column maps of a map box (include/tsdf_hip_columns.h): per
// (x, y) cell of the box the elevation, the ceiling, the occupied and free voxel counts and the
// flags, reduced over z on the GPU.
//   k_column_map   one wave per brick column (the 8 x 8 voxels in x, y of a brick, over all z);
//                  lane = (y & 7) << 3 | (x & 7), so a z-slice of a held brick is 64 consecutive
//                  floats of Pl.sdf and of Pl.weight.  The wave walks the z-bricks of the box bottom
//                  to top with one table_find each (the key is the same in every lane: a scalar
//                  probe); an absent brick, or one outside the key's range, costs that lookup and
//                  sets the lane's previous voxel to unobserved.  A held brick issues the loads of
//                  its (up to 8) slices of S and W before the first is used, then each lane steps
//                  through its voxels carrying (previous S, previous obs) across the bricks.
// Lanes whose column lies outside the box (brick columns cut by the box's x or y faces) or outside
// |i| < 2^23 load nothing; the former store nothing.  The kernel uses no wave-wide operation, no
// LDS, no atomics: every cell is a pure function of the box, so the bits do not depend on
// scheduling.  A workgroup takes COL_WAVES brick columns that are consecutive in x (columns_plan.h):
// a wave's stores are 32-byte runs, the workgroup's join into 128 bytes.  Flat launch on the
// context's stream, the grid capped at COL_GRID_CAP with a stride loop whose trips recompute
// everything from the index.
#include "columns_plan.h"
#include "tsdf_device.h"
#include "tsdf_ray.h"

namespace tsdf {

namespace {

struct ColState {
    uint32_t n_occ = 0, n_free = 0;
    float elev, ceil;
    bool has_elev = false, has_ceil = false;
    float ps = 0.0f;    // S of the voxel below
    bool pobs = false;  // ... and whether it is observed (false below the box)
};

// Rules 1 to 5 of the header for voxel z of the lane's column, read as (s, w).
__device__ __forceinline__ void col_voxel(ColState& C, int64_t z, float s, float w, float band,
                                          float min_w, float vs) {
    const bool obs = w > 0.0f && w >= min_w;
    const bool occ = obs && s <= band;
    C.n_occ += occ ? 1u : 0u;
    C.n_free += (obs && !occ) ? 1u : 0u;
    if (obs && C.pobs) {
        if (s > 0.0f && C.ps <= 0.0f) {  // up: the largest z wins
            const float t = s / (s - C.ps);
            C.elev = (((float)z + 0.5f) - t) * vs;
            C.has_elev = true;
        }
        if (C.ps > 0.0f && s <= 0.0f && !C.has_ceil) {  // down: the smallest z wins
            const float t = C.ps / (C.ps - s);
            C.ceil = (((float)(z - 1) + 0.5f) + t) * vs;
            C.has_ceil = true;
        }
    }
    C.ps = s;
    C.pobs = obs;
}

struct ColArgs {
    int64_t lo[3];
    uint32_t n[3];
    int64_t b0[3];
    uint32_t nbx, nbz;
    uint64_t cols;
    float bg, vs, band, min_w;
    uint32_t min_occ, min_free;
    float* elev;
    float* ceil;
    uint16_t* n_occ;
    uint16_t* n_free;
    uint8_t* flags;
};

__global__ __launch_bounds__(COL_THREADS) void k_column_map(Table T, Pool Pl, ColArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t groups = col_groups(A.cols);
    const int64_t hi2 = A.lo[2] + (int64_t)A.n[2];
    for (uint64_t trip = 0; trip * gridDim.x + blockIdx.x < groups; trip++) {
        const uint64_t c = col_index(trip, blockIdx.x, wave, gridDim.x);
        if (c >= A.cols) continue;  // (the last group's spare waves)
        const int64_t bx = col_bx(A.b0[0], A.nbx, c), by = col_by(A.b0[1], A.nbx, c);
        const int64_t x = bx * 8 + (int64_t)(lane & 7u), y = by * 8 + (int64_t)(lane >> 3);
        // (unsigned differences: a lane below lo wraps to a large value and fails the compare)
        const uint64_t dx = (uint64_t)x - (uint64_t)A.lo[0], dy = (uint64_t)y - (uint64_t)A.lo[1];
        const bool in_box = dx < A.n[0] && dy < A.n[1];
        const bool live = in_box && x > -VOX_LIMIT && x < VOX_LIMIT && y > -VOX_LIMIT && y < VOX_LIMIT;
        ColState C;
        C.elev = C.ceil = __uint_as_float(0x7FC00000u);
        if (col_brick_ok(bx) && col_brick_ok(by)) {
            for (uint32_t k = 0; k < A.nbz; k++) {
                const int64_t bz = A.b0[2] + (int64_t)k;
                uint32_t slot = T.max_bricks;
                if (col_brick_ok(bz)) {
                    const int64_t h = table_find(T, pack_brick((int)bx, (int)by, (int)bz));
                    if (h >= 0) slot = T.slots[h];
                }
                if (slot >= T.max_bricks) {  // absent: its voxels read (background, 0)
                    C.pobs = false;
                    continue;
                }
                // the brick's slices in the box, [z_lo, z_hi) of 0..8; voxel -2^23 is outside the
                // index domain and reads (background, 0) like a voxel of an absent brick
                const int64_t z0 = bz * 8;
                const int z_lo = A.lo[2] > z0 ? (int)(A.lo[2] - z0) : 0;
                const int z_hi = hi2 < z0 + 8 ? (int)(hi2 - z0) : 8;
                const int z_dom = z0 > -VOX_LIMIT ? 0 : (int)(-VOX_LIMIT + 1 - z0);
                const float* __restrict__ ps = Pl.sdf + (size_t)slot * BRICK_VOX + lane;
                const float* __restrict__ pw = Pl.weight + (size_t)slot * BRICK_VOX + lane;
                float s[8], w[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    s[i] = A.bg;
                    w[i] = 0.0f;
                }
                if (live) {
                    if (z_lo == 0 && z_hi == 8 && z_dom == 0) {  // a whole brick: 16 loads in flight
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            s[i] = ps[i * 64];
                            w[i] = pw[i * 64];
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            if (i >= z_lo && i < z_hi && i >= z_dom) {
                                s[i] = ps[i * 64];
                                w[i] = pw[i * 64];
                            }
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if (i >= z_lo && i < z_hi) col_voxel(C, z0 + i, s[i], w[i], A.band, A.min_w, A.vs);
            }
        }
        if (in_box) {
            const size_t idx = (size_t)dx + (size_t)A.n[0] * (size_t)dy;
            const bool occupied = C.n_occ >= A.min_occ;
            const bool free_ = !occupied && C.n_free >= A.min_free;
            if (A.elev) A.elev[idx] = C.elev;
            if (A.ceil) A.ceil[idx] = C.ceil;
            if (A.n_occ) A.n_occ[idx] = (uint16_t)C.n_occ;
            if (A.n_free) A.n_free[idx] = (uint16_t)C.n_free;
            if (A.flags)
                A.flags[idx] = (uint8_t)((C.n_occ + C.n_free > 0 ? 1u : 0u) | (occupied ? 2u : 0u) |
                                         (free_ ? 4u : 0u) | (C.has_elev ? 8u : 0u) |
                                         (C.has_ceil ? 16u : 0u));
        }
    }
}

}  // namespace

hipError_t launch_column_map(const Table& T, const Pool& Pl, const int64_t lo[3], const ColBox& B,
                             float band, float min_w, uint32_t min_occ, uint32_t min_free, float bg,
                             float vs, float* d_elev, float* d_ceil, uint16_t* d_n_occ,
                             uint16_t* d_n_free, uint8_t* d_flags, hipStream_t st) {
    if (!B.cells) return hipSuccess;
    ColArgs A;
    for (int a = 0; a < 3; a++) {
        A.lo[a] = lo[a];
        A.n[a] = B.n[a];
        A.b0[a] = B.b0[a];
    }
    A.nbx = B.nb[0];
    A.nbz = B.nb[2];
    A.cols = B.cols;
    A.bg = bg;
    A.vs = vs;
    A.band = band;
    A.min_w = min_w;
    A.min_occ = min_occ;
    A.min_free = min_free;
    A.elev = d_elev;
    A.ceil = d_ceil;
    A.n_occ = d_n_occ;
    A.n_free = d_n_free;
    A.flags = d_flags;
    k_column_map<<<col_grid(B.cols), COL_THREADS, 0, st>>>(T, Pl, A);
    return hipGetLastError();
}

}  // namespace tsdf

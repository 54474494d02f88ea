// columns_plan.h -- the host arithmetic of include/tsdf_hip_columns.h (tsdf_capi.cpp,
// tsdf_columns.hip): the argument rules of a column-map call, the brick columns that cover the box
// and the mapping from (trip, workgroup, wave) to a brick column that k_column_map uses.  Plain C++
// like esdf_plan.h, checked and sanitized on the CPU (tests/test_columns_plan.py).
//
// A brick column is the 8 x 8 voxels in x, y of one brick, over all z: one wave of k_column_map.
// The brick columns of a box are numbered x fastest, c = (bx - bx0) + nbx (by - by0), and a
// workgroup takes COL_WAVES consecutive numbers: brick columns that are neighbours in x (but where a
// row of them ends), so that its waves' 32-byte output runs join into 128 bytes.  The grid is
// capped at COL_GRID_CAP workgroups; workgroup w takes group w + trip * grid on its trip-th pass.
#pragma once
#include <cmath>
#include <cstdint>

#include "brick_key.h"

namespace tsdf {

constexpr uint32_t COL_WAVES = 4;             // brick columns (waves) per workgroup
constexpr uint32_t COL_THREADS = 64 * COL_WAVES;
constexpr uint32_t COL_GRID_CAP = 8192;       // workgroups per launch; the rest by stride
constexpr uint32_t COL_MAX_NZ = 65535;        // the counts are 16 bits
constexpr uint64_t COL_MAX_CELLS = 1ull << 26;  // nx * ny

// The argument rules in the order they are reported; COL_ARG_OK passes.
enum ColArg : int {
    COL_ARG_OK = 0,
    COL_ARG_BAND,    // occ_band not finite
    COL_ARG_WEIGHT,  // min_weight negative or NaN
    COL_ARG_COUNT,   // min_occ or min_free outside 1..65535
    COL_ARG_ORDER,   // hi < lo on an axis
    COL_ARG_EXTENT,  // an extent >= 2^31
    COL_ARG_HEIGHT,  // nz > 65535
    COL_ARG_CELLS,   // nx * ny > 2^26
};

inline const char* columns_arg_text(int a) {
    switch (a) {
    case COL_ARG_BAND: return "occ_band is not finite";
    case COL_ARG_WEIGHT: return "min_weight is negative or NaN";
    case COL_ARG_COUNT: return "min_occ and min_free must be in 1..65535";
    case COL_ARG_ORDER: return "hi < lo";
    case COL_ARG_EXTENT: return "box extent >= 2^31 voxels";
    case COL_ARG_HEIGHT: return "box above 65535 voxels in z";
    case COL_ARG_CELLS: return "box above 2^26 columns";
    default: return nullptr;
    }
}

struct ColBox {
    uint32_t n[3];      // extents (x, y, z)
    uint64_t cells;     // nx * ny output cells; 0 for an empty box (any extent 0)
    int64_t b0[3];      // the first brick per axis: floor(lo / 8)
    uint32_t nb[3];     // bricks per axis: floor((hi - 1) / 8) - b0 + 1
    uint64_t cols;      // brick columns: nb[0] * nb[1]
};

// floor(v / 8) for any int64
constexpr int64_t col_floor8(int64_t v) { return v >= 0 ? v / 8 : -((-(v + 1)) / 8) - 1; }

// The first rule the arguments break, and the box with its tiling when none is broken.  An empty
// box breaks neither size rule, whatever its other extents.
inline int columns_check(const int64_t lo[3], const int64_t hi[3], float occ_band, float min_weight,
                         uint32_t min_occ, uint32_t min_free, ColBox* box) {
    *box = ColBox{};
    if (!std::isfinite(occ_band)) return COL_ARG_BAND;
    if (!(min_weight >= 0.0f)) return COL_ARG_WEIGHT;
    if (min_occ < 1 || min_occ > 65535 || min_free < 1 || min_free > 65535) return COL_ARG_COUNT;
    uint64_t ext[3];
    for (int a = 0; a < 3; a++) {
        if (hi[a] < lo[a]) return COL_ARG_ORDER;
        // (the extent as unsigned: hi - lo of int64 bounds may exceed the int64 range)
        ext[a] = (uint64_t)hi[a] - (uint64_t)lo[a];
    }
    for (int a = 0; a < 3; a++)
        if (ext[a] >= (1ull << 31)) return COL_ARG_EXTENT;
    if (ext[0] == 0 || ext[1] == 0 || ext[2] == 0) {
        for (int a = 0; a < 3; a++) box->n[a] = (uint32_t)ext[a];
        return COL_ARG_OK;
    }
    if (ext[2] > COL_MAX_NZ) return COL_ARG_HEIGHT;
    if (ext[0] * ext[1] > COL_MAX_CELLS) return COL_ARG_CELLS;
    for (int a = 0; a < 3; a++) {
        box->n[a] = (uint32_t)ext[a];
        box->b0[a] = col_floor8(lo[a]);
        // (hi > lo here, so hi - 1 does not wrap)
        box->nb[a] = (uint32_t)(col_floor8(hi[a] - 1) - box->b0[a] + 1);
    }
    box->cells = ext[0] * ext[1];
    box->cols = (uint64_t)box->nb[0] * box->nb[1];
    return COL_ARG_OK;
}

// Groups of COL_WAVES brick columns, the launch's workgroups and the trips of its stride loop.
constexpr uint64_t col_groups(uint64_t cols) { return (cols + COL_WAVES - 1) / COL_WAVES; }
constexpr uint32_t col_grid(uint64_t cols) {
    return (uint32_t)(col_groups(cols) < 1
                          ? 1
                          : (col_groups(cols) > COL_GRID_CAP ? COL_GRID_CAP : col_groups(cols)));
}
constexpr uint64_t col_trips(uint64_t cols) {
    return (col_groups(cols) + col_grid(cols) - 1) / col_grid(cols);
}
// The brick column of wave `wave` of workgroup `wg` on its trip-th pass; >= cols: none.
constexpr uint64_t col_index(uint64_t trip, uint32_t wg, uint32_t wave, uint32_t grid) {
    return (trip * grid + wg) * COL_WAVES + wave;
}
// Its brick coordinates in x and y.
constexpr int64_t col_bx(int64_t bx0, uint32_t nbx, uint64_t c) { return bx0 + (int64_t)(c % nbx); }
constexpr int64_t col_by(int64_t by0, uint32_t nbx, uint64_t c) { return by0 + (int64_t)(c / nbx); }
// A brick coordinate a key can hold (brick_coord_ok of brick_key.h, for an int64); the bricks
// outside hold no voxel of |i| < 2^23.
constexpr bool col_brick_ok(int64_t b) { return b >= -BRICK_KEY_BIAS && b < BRICK_KEY_BIAS; }

}  // namespace tsdf

// frontier_plan.h -- the host arithmetic of include/tsdf_hip_frontier.h (tsdf_capi.cpp,
// tsdf_frontier.hip): the argument rules of a frontier call in the order they are reported, the
// table of neighbour offsets, the grid cap of the kernels' stride loop and the prefix that places
// every brick's frontier voxels.  Plain C++ like columns_plan.h and mesh_plan.h, checked and
// sanitized on the CPU (tests/test_frontier_plan.py).
//
// The box is the indexed mesh's (mesh_box_check) and the listed bricks are the map's sorted keys
// that pass mesh_brick_in_box(key, B, 0): only voxels of the box are emitted, and a neighbour
// outside it is read through the table, so the list needs no grow.
#pragma once
#include <cmath>
#include <cstdint>

#include "mesh_plan.h"

namespace tsdf {

constexpr uint32_t FRONTIER_THREADS = 512;    // one lane per voxel of a brick
constexpr uint32_t FRONTIER_GRID_CAP = 2048;  // workgroups per launch; the rest by stride
constexpr int FRONTIER_TILE = 10;             // in-brick coordinates -1 .. 8
constexpr int FRONTIER_OFFSETS = 26;

// The neighbour offsets (dx, dy, dz): the 6 faces, then the 12 edges, then the 8 corners, so that a
// connectivity of 6, 18 or 26 is a prefix of the table.
// (a struct, so that the kernels' __constant__ copy is initialised from it)
struct FrontierOffsets {
    int8_t d[FRONTIER_OFFSETS][3];
};
constexpr FrontierOffsets FRONTIER_OFFSET = {{
    {-1, 0, 0},  {1, 0, 0},   {0, -1, 0},  {0, 1, 0},  {0, 0, -1}, {0, 0, 1},
    {-1, -1, 0}, {1, -1, 0},  {-1, 1, 0},  {1, 1, 0},  {-1, 0, -1}, {1, 0, -1},
    {-1, 0, 1},  {1, 0, 1},   {0, -1, -1}, {0, 1, -1}, {0, -1, 1},  {0, 1, 1},
    {-1, -1, -1}, {1, -1, -1}, {-1, 1, -1}, {1, 1, -1}, {-1, -1, 1}, {1, -1, 1},
    {-1, 1, 1},  {1, 1, 1},
}};

// The argument rules in the order they are reported; FRONTIER_ARG_OK passes.
enum FrontierArg : int {
    FRONTIER_ARG_OK = 0,
    FRONTIER_ARG_HALF,     // exactly one of lo / hi NULL
    FRONTIER_ARG_BAND,     // free_band not finite
    FRONTIER_ARG_WEIGHT,   // min_weight negative or NaN
    FRONTIER_ARG_CONN,     // connectivity not 6, 18 or 26
    FRONTIER_ARG_UNKNOWN,  // min_unknown outside 1..connectivity
    FRONTIER_ARG_ORDER,    // hi < lo on an axis
    FRONTIER_ARG_EXTENT,   // an extent >= 2^31
};

inline const char* frontier_arg_text(int a) {
    switch (a) {
    case FRONTIER_ARG_HALF: return mesh_arg_text(MESH_ARG_HALF);
    case FRONTIER_ARG_BAND: return "free_band is not finite";
    case FRONTIER_ARG_WEIGHT: return "min_weight is negative or NaN";
    case FRONTIER_ARG_CONN: return "connectivity must be 6, 18 or 26";
    case FRONTIER_ARG_UNKNOWN: return "min_unknown must be in 1..connectivity";
    case FRONTIER_ARG_ORDER: return mesh_arg_text(MESH_ARG_ORDER);
    case FRONTIER_ARG_EXTENT: return mesh_arg_text(MESH_ARG_EXTENT);
    default: return nullptr;
    }
}

// The first rule the arguments break; *B the clamped box and *empty whether it holds no voxel when
// none is broken.
inline int frontier_check(const int64_t* lo, const int64_t* hi, float free_band, float min_weight,
                          int32_t connectivity, int32_t min_unknown, MeshBox* B, bool* empty) {
    const int box = mesh_box_check(lo, hi, B, empty);
    if (box == MESH_ARG_HALF) return FRONTIER_ARG_HALF;
    if (!std::isfinite(free_band)) return FRONTIER_ARG_BAND;
    if (!(min_weight >= 0.0f)) return FRONTIER_ARG_WEIGHT;
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return FRONTIER_ARG_CONN;
    if (min_unknown < 1 || min_unknown > connectivity) return FRONTIER_ARG_UNKNOWN;
    if (box == MESH_ARG_ORDER) return FRONTIER_ARG_ORDER;
    if (box == MESH_ARG_EXTENT) return FRONTIER_ARG_EXTENT;
    return FRONTIER_ARG_OK;
}

// The launch's workgroups for nb listed bricks: one per brick up to the cap.
constexpr uint32_t frontier_grid(uint64_t nb) {
    return (uint32_t)(nb < 1 ? 1 : (nb > FRONTIER_GRID_CAP ? FRONTIER_GRID_CAP : nb));
}

// Exclusive prefix of the bricks' frontier counts; the total in *n_voxels, the bricks with a
// count in *n_frontier_bricks.
inline void frontier_prefix(const uint32_t* cnt, uint64_t n, uint64_t* off, uint64_t* n_voxels,
                            uint64_t* n_frontier_bricks) {
    uint64_t v = 0, fb = 0;
    for (uint64_t i = 0; i < n; i++) {
        off[i] = v;
        v += cnt[i];
        if (cnt[i]) fb++;
    }
    *n_voxels = v;
    *n_frontier_bricks = fb;
}

// The sum of the bricks' free counts.
inline uint64_t frontier_sum(const uint32_t* cnt, uint64_t n) {
    uint64_t s = 0;
    for (uint64_t i = 0; i < n; i++) s += cnt[i];
    return s;
}

}  // namespace tsdf

// prune_plan.h -- the host arithmetic of include/tsdf_hip_prune.h (tsdf_capi.cpp): the pieces of an
// eviction's copy-out and the brick box of a world-frame cube.  Plain C++ like ctx_plan.h, checked
// and sanitized on the CPU (tests/test_prune_plan.py).
//
// Scratch bound: the evicted bricks leave the pool through a device scratch of at most
// EVICT_SCRATCH_BYTES = 64 MiB (sdf and weight together), gathered and copied to the caller piece
// by piece -- 16384 bricks a piece when both arrays are wanted, 32768 with one.  A map of many GiB
// therefore never needs a second copy of itself on the device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "brick_key.h"

namespace tsdf {

constexpr uint64_t EVICT_SCRATCH_BYTES = 64ull << 20;
constexpr uint64_t EVICT_BRICK_BYTES = 512 * sizeof(float);  // one array of one brick

// Bricks per copy-out piece for `arrays` wanted voxel arrays (sdf, weight: 0..2); 0 arrays copy
// nothing and need no piece.
inline uint64_t evict_piece_bricks(int arrays) {
    return arrays <= 0 ? 0 : EVICT_SCRATCH_BYTES / (EVICT_BRICK_BYTES * (uint64_t)arrays);
}

// One axis of the brick box of the world-frame cube of centre c and half-side r (metres) at voxel
// size vs: bricks lo <= b < hi with lo = floor((c - r) / (8 vs)), hi = floor((c + r) / (8 vs)) + 1,
// in double, clamped to the packable brick range [-2^20, 2^20] (hi is exclusive, so it may equal
// 2^20).  The cube's far face lying exactly on a brick face includes the brick beyond it: a brick
// is kept when the closed cube touches it.  Non-finite input (NaN included) clamps like +-inf.
inline int32_t box_clamp(double b) {
    if (!(b > (double)-BRICK_KEY_BIAS)) return b != b ? 0 : -BRICK_KEY_BIAS;
    if (b > (double)BRICK_KEY_BIAS) return BRICK_KEY_BIAS;
    return (int32_t)b;
}
inline void cube_box_axis(double c, double r, double vs, int32_t* lo, int32_t* hi) {
    const double side = 8.0 * vs;
    *lo = box_clamp(std::floor((c - r) / side));
    *hi = box_clamp(std::floor((c + r) / side) + 1.0);
    if (*hi < *lo) *hi = *lo;  // (NaN or r < 0: an empty box, never lo > hi)
}
inline void cube_box(const double c[3], double r, double vs, int32_t lo[3], int32_t hi[3]) {
    for (int a = 0; a < 3; a++) cube_box_axis(c[a], r, vs, &lo[a], &hi[a]);
}

}  // namespace tsdf

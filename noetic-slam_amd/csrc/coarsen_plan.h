// coarsen_plan.h -- the host arithmetic of include/tsdf_hip_coarsen.h (tsdf_capi.cpp,
// tsdf_coarsen.hip): the argument rules and the compatibility rules of the two contexts, the
// selection predicate, the parent of a brick, the child index arithmetic of a destination voxel,
// and the scratch sizes.  Plain C++ like merge_plan.h, checked and sanitized on the CPU
// (tests/test_coarsen_plan.py); the kernels evaluate the COARSEN_FN functions per brick and lane.
//
// The index arithmetic.  Destination brick D holds the coarse voxels V = 8 D + (x, y, z), lane
// l = x + 8 y + 64 z of its workgroup.  The children of V are the fine voxels
// 2 V + (a, b, c) = 16 D + (2 x + a, 2 y + b, 2 z + c): their brick is
// 2 D + (x >> 2, y >> 2, z >> 2) whatever (a, b, c) is -- one source brick per coarse voxel, child
// brick j = (x >> 2) + 2 (y >> 2) + 4 (z >> 2) of the eight bricks 2 D + (j & 1, j >> 1 & 1, j >> 2)
// -- and their local voxel in it is (2 (x & 3) + a, 2 (y & 3) + b, 2 (z & 3) + c).  The children
// a = 0, 1 are adjacent in x and start at an even index: one aligned 8-byte pair.
//
// The parent.  D = B >> 1 per axis, the floor of B / 2 for negative and odd B alike.  B ranges
// over the packable coordinates -2^20 <= B < 2^20, so D lies in -2^19 <= D < 2^19 and the child
// bricks 2 D + {0, 1} are packable again: no key of either map can overflow its field.
//
// The scratch.  A source brick has exactly one parent, so the distinct parents are at most the
// source's bricks n: a set of 2^k >= 2 n keys (at least COARSEN_SET_MIN), a list of n keys and
// per list entry a flag and a pool slot.  Beyond the minimum the set has fewer than 4 n slots:
// at most 32 n + 8 n + 8 n = 48 n bytes, plus the counters and the minimum set, under 32 KiB.
#pragma once
#include <cstdint>

#ifndef COARSEN_FN
#define COARSEN_FN inline
#endif

namespace tsdf {

constexpr int32_t COARSEN_BRICK_LIMIT = 1 << 20;  // packable brick coordinates: -2^20 <= b < 2^20
constexpr uint64_t COARSEN_SET_MIN = 1024;        // slots of the smallest parent set
constexpr uint64_t COARSEN_SCRATCH_FIXED = 32ull << 10;
constexpr uint64_t COARSEN_SCRATCH_PER_BRICK = 48;
// two words (selected bricks, parents) in a head of 16 and the flag kernel's 64 shards of a
// 128-byte line each
constexpr uint64_t COARSEN_COUNTER_BYTES = (16 + 64 * 16) * 8;

// The argument rules in the order they are reported; COARSEN_ARG_OK passes.
enum CoarsenArg : int {
    COARSEN_ARG_OK = 0,
    COARSEN_ARG_SIDE,      // not TSDF_COARSEN_INSIDE / _OUTSIDE
    COARSEN_ARG_BOX,       // exactly one of lo / hi NULL
    COARSEN_ARG_CHILDREN,  // min_children outside 1..8
    COARSEN_ARG_WEIGHT,    // min_weight negative or NaN
};

inline const char* coarsen_arg_text(int a) {
    switch (a) {
    case COARSEN_ARG_SIDE: return "side must be TSDF_COARSEN_INSIDE or _OUTSIDE";
    case COARSEN_ARG_BOX: return "exactly one of lo and hi is NULL";
    case COARSEN_ARG_CHILDREN: return "min_children must be 1..8";
    case COARSEN_ARG_WEIGHT: return "min_weight is negative or NaN";
    default: return nullptr;
    }
}

inline int coarsen_args(int32_t side, bool has_lo, bool has_hi, uint32_t min_children,
                        float min_weight) {
    if (side != 0 && side != 1) return COARSEN_ARG_SIDE;
    if (has_lo != has_hi) return COARSEN_ARG_BOX;
    if (min_children < 1 || min_children > 8) return COARSEN_ARG_CHILDREN;
    if (!(min_weight >= 0.0f)) return COARSEN_ARG_WEIGHT;
    return COARSEN_ARG_OK;
}

// The compatibility rules of the two contexts, likewise.
enum CoarsenCompat : int {
    COARSEN_COMPAT_OK = 0,
    COARSEN_COMPAT_VOXEL,  // (float)dst voxel_size is not 2.0f * (float)src voxel_size in its bits
    COARSEN_COMPAT_TRUNC,  // (float)sdf_trunc differs in its bits
    COARSEN_COMPAT_BG,     // a Voxblox context (background 0) against a VDBFusion one (sdf_trunc)
};

inline const char* coarsen_compat_text(int a) {
    switch (a) {
    case COARSEN_COMPAT_VOXEL:
        return "the destination's voxel size is not twice the source's";
    case COARSEN_COMPAT_TRUNC: return "the contexts' truncation distances differ";
    case COARSEN_COMPAT_BG: return "the contexts' backgrounds differ (Voxblox against VDBFusion)";
    default: return nullptr;
    }
}

inline uint32_t coarsen_float_bits(float f) {
    union { float f; uint32_t u; } v;
    v.f = f;
    return v.u;
}

// semantics: TSDF_SEM_VDBFUSION 0, TSDF_SEM_VOXBLOX 1, TSDF_SEM_VDBFUSION_F64 2 (merge_compat's
// notion of the background)
inline int coarsen_compat(double vs_dst, double vs_src, double tau_dst, double tau_src, int sem_dst,
                          int sem_src) {
    const float twice = 2.0f * (float)vs_src;
    if (coarsen_float_bits((float)vs_dst) != coarsen_float_bits(twice)) return COARSEN_COMPAT_VOXEL;
    if (coarsen_float_bits((float)tau_dst) != coarsen_float_bits((float)tau_src))
        return COARSEN_COMPAT_TRUNC;
    if ((sem_dst == 1) != (sem_src == 1)) return COARSEN_COMPAT_BG;
    return COARSEN_COMPAT_OK;
}

// Rule 1.  has_box = 0: every brick.
struct CoarsenSel {
    int32_t has_box, side;
    int32_t lo[3], hi[3];
};

COARSEN_FN bool coarsen_selected(const CoarsenSel& s, int32_t bx, int32_t by, int32_t bz) {
    if (!s.has_box) return true;
    const bool in = bx >= s.lo[0] && bx < s.hi[0] && by >= s.lo[1] && by < s.hi[1] &&
                    bz >= s.lo[2] && bz < s.hi[2];
    return s.side == 0 ? in : !in;
}

// Rule 2: floor(b / 2), written without a shift of a negative number
COARSEN_FN int32_t coarsen_parent(int32_t b) { return (b - (b & 1)) / 2; }

// Lane l of a destination brick's workgroup (coarse voxel (l & 7, l >> 3 & 7, l >> 6)):
// which of the eight child bricks 2 D + (j & 1, j >> 1 & 1, j >> 2) holds its children ...
COARSEN_FN int coarsen_child_brick(int l) {
    return ((l >> 2) & 1) | (((l >> 5) & 1) << 1) | (((l >> 8) & 1) << 2);
}
// ... the local voxel of child k = 0 in that brick (even: children k, k + 1 are one 8-byte pair) ...
COARSEN_FN int coarsen_child_base(int l) {
    return 2 * (l & 3) + 8 * (2 * ((l >> 3) & 3)) + 64 * (2 * ((l >> 6) & 3));
}
// ... and the offset of child k = a + 2 b + 4 c from it
COARSEN_FN int coarsen_child_offset(int k) { return (k & 1) + 8 * ((k >> 1) & 1) + 64 * (k >> 2); }

// The parent set: an open-addressing table of 2^k >= 2 * src_bricks keys (never more than half
// full), at least COARSEN_SET_MIN slots.
inline uint64_t coarsen_set_slots(uint64_t src_bricks) {
    uint64_t n = COARSEN_SET_MIN;
    while (n < 2 * src_bricks) n <<= 1;
    return n;
}

// Device scratch of one call: the set (8 B a slot), the parent list (8 B an entry, src_bricks
// entries), per entry its flag and its pool slot (4 B each), and the counters.
inline uint64_t coarsen_scratch_bytes(uint64_t src_bricks) {
    return 8 * coarsen_set_slots(src_bricks) + 16 * src_bricks + COARSEN_COUNTER_BYTES;
}

}  // namespace tsdf

// mesh_plan.h -- the host side of the indexed mesh (include/tsdf_hip_mesh.h; tsdf_capi.cpp): the
// box rules, the list of bricks a box examines, and the prefixes that place every brick's vertices
// and triangles.  Plain C++ like esdf_plan.h and prune_plan.h, checked and sanitized on the CPU
// (tests/test_mesh_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "brick_key.h"

namespace tsdf {

// The box of the cubes' min voxels, clamped to +-2^24: every voxel of a packable brick lies within
// +-2^23, so clamping changes no answer and the kernels compare 32-bit coordinates.
constexpr int64_t MESH_BOX_LIMIT = 1ll << 24;
struct MeshBox {
    int32_t lo[3], hi[3];
};

enum MeshArg { MESH_ARG_OK = 0, MESH_ARG_HALF, MESH_ARG_ORDER, MESH_ARG_EXTENT };

inline const char* mesh_arg_text(int a) {
    switch (a) {
        case MESH_ARG_HALF: return "lo and hi must both be given or both be NULL";
        case MESH_ARG_ORDER: return "hi < lo";
        case MESH_ARG_EXTENT: return "box extent >= 2^31 voxels";
        default: return "";
    }
}

// The header's box rules, the first that fails; *B the clamped box and *empty whether it holds no
// voxel.  Both NULL: the whole map.
inline int mesh_box_check(const int64_t* lo, const int64_t* hi, MeshBox* B, bool* empty) {
    *empty = false;
    if (!lo != !hi) return MESH_ARG_HALF;
    for (int a = 0; a < 3; a++) {
        B->lo[a] = (int32_t)-MESH_BOX_LIMIT;
        B->hi[a] = (int32_t)MESH_BOX_LIMIT;
    }
    if (!lo) return MESH_ARG_OK;
    for (int a = 0; a < 3; a++)
        if (hi[a] < lo[a]) return MESH_ARG_ORDER;
    for (int a = 0; a < 3; a++)
        // (the extent as unsigned: hi - lo of int64 bounds may exceed the int64 range)
        if ((uint64_t)hi[a] - (uint64_t)lo[a] >= (1ull << 31)) return MESH_ARG_EXTENT;
    for (int a = 0; a < 3; a++) {
        const int64_t l = std::min(std::max(lo[a], -MESH_BOX_LIMIT), MESH_BOX_LIMIT);
        const int64_t h = std::min(std::max(hi[a], -MESH_BOX_LIMIT), MESH_BOX_LIMIT);
        B->lo[a] = (int32_t)l;
        B->hi[a] = (int32_t)h;
        if (h <= l) *empty = true;
    }
    return MESH_ARG_OK;
}

// Does brick `key` hold a voxel of [B.lo, B.hi + grow)?
inline bool mesh_brick_in_box(uint64_t key, const MeshBox& B, int grow) {
    for (int a = 0; a < 3; a++) {
        const int64_t v0 = 8 * (int64_t)brick_key_coord(key, a);
        if (v0 + 8 <= (int64_t)B.lo[a] || v0 >= (int64_t)B.hi[a] + grow) return false;
    }
    return true;
}

// The bricks the kernels list, from the map's keys in (z, y, x) order and in that order: those that
// intersect the box grown by one voxel on the high side -- the cubes' bricks and the owners of
// their vertices.  Returns the number that intersect the box itself (tsdf_mesh_counts::n_bricks).
inline uint64_t mesh_list_bricks(const std::vector<uint64_t>& sorted_keys, const MeshBox& B,
                                 std::vector<uint64_t>* listed) {
    uint64_t examined = 0;
    listed->clear();
    for (uint64_t k : sorted_keys) {
        if (!mesh_brick_in_box(k, B, 1)) continue;
        listed->push_back(k);
        if (mesh_brick_in_box(k, B, 0)) examined++;
    }
    return examined;
}

// Exclusive prefixes of the bricks' triangle and vertex counts; the totals in *n_tri and *n_vert.
// vbase is 32-bit: the caller refuses a mesh whose *n_vert reaches 2^32 before it uses vbase.
inline void mesh_prefix(const uint32_t* tcnt, const uint32_t* vcnt, uint64_t n, uint64_t* toff,
                        uint32_t* vbase, uint64_t* n_tri, uint64_t* n_vert) {
    uint64_t t = 0, v = 0;
    for (uint64_t i = 0; i < n; i++) {
        toff[i] = t;
        vbase[i] = (uint32_t)v;
        t += tcnt[i];
        v += vcnt[i];
    }
    *n_tri = t;
    *n_vert = v;
}

}  // namespace tsdf

// esdf_plan.h -- the host arithmetic of include/tsdf_hip_esdf.h (tsdf_capi.cpp, tsdf_esdf.hip): the
// argument rules of a distance-field call, the tiles of its three passes with their LDS bytes, and
// its device scratch.  Plain C++ like prune_plan.h, checked and sanitized on the CPU
// (tests/test_esdf_plan.py).
//
// The passes (tsdf_esdf.hip).  g is a plane of 16-bit squared distances, ESDF_INF where no site has
// been seen: 3 * 128^2 = 49152 < ESDF_INF.  A pass along one axis replaces g(i) by
// min over |d| <= R inside the box of g(i + d) + d^2.
//   x pass    a workgroup takes ESDF_X_LINES lines by ESDF_LANES voxels of x, and stages each
//             line's segment with a halo of R voxels on either side.
//   y, z pass lanes run along the contiguous inner index (x for y; the whole x-y plane for z), a
//             workgroup takes ESDF_LANES of them by esdf_seg(R) voxels of the pass axis plus the
//             halo of R rows on either side.
// At R = 128 the largest tile is (64 + 256) rows * 64 lanes * 2 B = 40 KiB; with the ESDF_LDS_STATIC
// bytes of the kernels' workgroup vote, three workgroups fit the 160 KiB of a CU there and four at
// every smaller radius.
#pragma once
#include <cmath>
#include <cstdint>

namespace tsdf {

constexpr uint32_t ESDF_MAX_RADIUS = 128;         // TSDF_ESDF_MAX_RADIUS
constexpr uint64_t ESDF_MAX_VOXELS = 1ull << 28;  // the box bound: keeps the scratch bounded
constexpr uint32_t ESDF_INF = 0xFFFFu;            // "no site" in a 16-bit plane
constexpr uint32_t ESDF_THREADS = 256;
constexpr uint32_t ESDF_LANES = 64;    // voxels of the contiguous index per tile
constexpr uint32_t ESDF_X_LINES = 16;  // lines per tile of the x pass
constexpr uint64_t ESDF_SCRATCH_PER_VOXEL = 5;  // two u16 planes and the class byte
constexpr uint32_t ESDF_GRID_CAP = 8192;
constexpr uint32_t ESDF_LDS_STATIC = 256;  // LDS of a pass beside its tile (__syncthreads_or)

// The argument rules in the order they are reported; ESDF_ARG_OK passes.
enum EsdfArg : int {
    ESDF_ARG_OK = 0,
    ESDF_ARG_RADIUS,  // radius_vox == 0 or > ESDF_MAX_RADIUS
    ESDF_ARG_BAND,    // site_band negative or not finite
    ESDF_ARG_WEIGHT,  // min_weight negative or NaN
    ESDF_ARG_ORDER,   // hi < lo on an axis
    ESDF_ARG_EXTENT,  // an extent >= 2^31
    ESDF_ARG_SIZE,    // more than ESDF_MAX_VOXELS voxels
};

inline const char* esdf_arg_text(int a) {
    switch (a) {
    case ESDF_ARG_RADIUS: return "radius_vox must be in 1..128";
    case ESDF_ARG_BAND: return "site_band is negative or not finite";
    case ESDF_ARG_WEIGHT: return "min_weight is negative or NaN";
    case ESDF_ARG_ORDER: return "hi < lo";
    case ESDF_ARG_EXTENT: return "box extent >= 2^31 voxels";
    case ESDF_ARG_SIZE: return "box above 2^28 voxels";
    default: return nullptr;
    }
}

struct EsdfBox {
    uint32_t n[3];   // extents (x, y, z)
    uint64_t total;  // voxels
};

// The first rule the arguments break, and the box's extents when none is broken.
inline int esdf_check(const int64_t lo[3], const int64_t hi[3], uint32_t radius, float site_band,
                      float min_weight, EsdfBox* box) {
    *box = EsdfBox{};
    if (radius == 0 || radius > ESDF_MAX_RADIUS) return ESDF_ARG_RADIUS;
    if (!(site_band >= 0.0f) || std::isinf(site_band)) return ESDF_ARG_BAND;
    if (!(min_weight >= 0.0f)) return ESDF_ARG_WEIGHT;
    uint64_t ext[3];
    for (int a = 0; a < 3; a++) {
        if (hi[a] < lo[a]) return ESDF_ARG_ORDER;
        // (the extent as unsigned: hi - lo of int64 bounds may exceed the int64 range)
        ext[a] = (uint64_t)hi[a] - (uint64_t)lo[a];
    }
    for (int a = 0; a < 3; a++)
        if (ext[a] >= (1ull << 31)) return ESDF_ARG_EXTENT;
    // (an empty box is no size error, whatever its other extents; ext[0] ext[1] < 2^62)
    if (ext[0] == 0 || ext[1] == 0 || ext[2] == 0) {
        for (int a = 0; a < 3; a++) box->n[a] = (uint32_t)ext[a];
        return ESDF_ARG_OK;
    }
    const uint64_t plane = ext[0] * ext[1];
    if (plane > ESDF_MAX_VOXELS || plane * ext[2] > ESDF_MAX_VOXELS) return ESDF_ARG_SIZE;
    for (int a = 0; a < 3; a++) box->n[a] = (uint32_t)ext[a];
    box->total = plane * ext[2];
    return ESDF_ARG_OK;
}

inline uint64_t esdf_ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Voxels of the pass axis per tile of the y and z passes: longer segments at large radii, where
// the halo would otherwise be read many times over.
inline uint32_t esdf_seg(uint32_t radius) { return radius <= 48 ? 32u : 64u; }

// The halo a pass needs: no offset beyond the line's end finds a voxel of the box.
inline uint32_t esdf_halo(uint32_t radius, uint32_t n) {
    return n == 0 ? 0 : (radius < n - 1 ? radius : n - 1);
}

// LDS bytes and tile counts, for a halo of h voxels (esdf_halo of the pass axis).
inline uint32_t esdf_lds_x(uint32_t h) { return ESDF_X_LINES * (ESDF_LANES + 2 * h) * 2; }
inline uint32_t esdf_lds_axis(uint32_t radius, uint32_t h) {
    return (esdf_seg(radius) + 2 * h) * ESDF_LANES * 2;
}
inline uint64_t esdf_tiles_x(const EsdfBox& b) {
    return esdf_ceil_div(b.n[0], ESDF_LANES) * esdf_ceil_div((uint64_t)b.n[1] * b.n[2], ESDF_X_LINES);
}
// n voxels along the pass axis, `inner` contiguous voxels below it, `outer` slabs above it
inline uint64_t esdf_tiles_axis(uint32_t radius, uint64_t inner, uint32_t n, uint32_t outer) {
    return esdf_ceil_div(inner, ESDF_LANES) * esdf_ceil_div(n, esdf_seg(radius)) * outer;
}
inline uint32_t esdf_grid(uint64_t tiles) {
    return (uint32_t)(tiles < 1 ? 1 : (tiles > ESDF_GRID_CAP ? ESDF_GRID_CAP : tiles));
}

inline uint64_t esdf_scratch_bytes(uint64_t total) { return ESDF_SCRATCH_PER_VOXEL * total; }

}  // namespace tsdf

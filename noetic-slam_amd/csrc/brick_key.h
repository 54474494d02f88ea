// brick_key.h -- the host side of the brick key (tsdf_capi.cpp): a brick's signed coordinates,
// biased by 2^20, in three 21-bit fields, x lowest.  Plain C++ like host_pack.h, checked and
// sanitized on the CPU (tests/test_brick_key.py).
// Device twins: pack_brick / brick_key_of in tsdf_ray.h and the key arithmetic in tsdf_mesh.hip.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace tsdf {

constexpr int32_t BRICK_KEY_BIAS = 1 << 20;
constexpr uint64_t BRICK_KEY_FIELD = 0x1FFFFF;  // one axis' biased coordinate, at bit 21 * axis

// The coordinates a key can hold (the import's range rule)
inline bool brick_coord_ok(int32_t b) { return b >= -BRICK_KEY_BIAS && b < BRICK_KEY_BIAS; }

inline uint64_t brick_key_pack(int32_t bx, int32_t by, int32_t bz) {
    return (uint64_t)(bx + BRICK_KEY_BIAS) | ((uint64_t)(by + BRICK_KEY_BIAS) << 21) |
           ((uint64_t)(bz + BRICK_KEY_BIAS) << 42);
}

inline int32_t brick_key_coord(uint64_t key, int axis) {
    return (int32_t)((key >> (21 * axis)) & BRICK_KEY_FIELD) - BRICK_KEY_BIAS;
}

// The (z, y, x) brick order of export and mesh (the oracle's): with z in the highest field and the
// bias keeping every field's order, it is the order of the keys as integers.
inline bool brick_key_less_zyx(uint64_t a, uint64_t b) { return a < b; }

// The mesh halo a set of bricks needs: the +x / +y / +z neighbours (7 per brick) that are not in
// the set, sorted and unique.  `have` is sorted; a neighbour past the top of an axis' range has no
// key and is skipped.
inline std::vector<uint64_t> brick_halo_needed(const std::vector<uint64_t>& have) {
    std::vector<uint64_t> need;
    for (uint64_t k : have) {
        const uint64_t b[3] = {k & BRICK_KEY_FIELD, (k >> 21) & BRICK_KEY_FIELD,
                               (k >> 42) & BRICK_KEY_FIELD};
        for (int d = 1; d < 8; d++) {
            const uint64_t nx = b[0] + (d & 1), ny = b[1] + ((d >> 1) & 1), nz = b[2] + (d >> 2);
            if (nx > BRICK_KEY_FIELD || ny > BRICK_KEY_FIELD || nz > BRICK_KEY_FIELD) continue;
            const uint64_t q = nx | (ny << 21) | (nz << 42);
            if (!std::binary_search(have.begin(), have.end(), q)) need.push_back(q);
        }
    }
    std::sort(need.begin(), need.end());
    need.erase(std::unique(need.begin(), need.end()), need.end());
    return need;
}

}  // namespace tsdf

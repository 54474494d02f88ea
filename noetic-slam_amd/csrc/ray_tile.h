// ray_tile.h — which rays a k_count / k_place workgroup takes ("ray tiles").
//
// A block is RPB = 1024 rays of one scan; k_count takes a block per workgroup, k_place one half
// (512 slots) of it.  The points of a spinning LiDAR arrive column-major: H beams of column 0,
// then column 1, ...  1024 CONSECUTIVE points are therefore a wedge 1024 / H columns wide and the
// sensor's whole elevation range high (8 x 128: ~3 x 45 degrees), which crosses bricks along its
// whole height.  With a column height H the blocks are compact tiles instead:
//
//   group   32 columns = 32 H points = H / 32 blocks (the same points the consecutive mapping
//           gives those blocks, so block counts, the host's block prefix and grids do not change)
//   block   bt of group g: the points g 32 H + c H + 32 bt + b, columns c and beams b in [0, 32)
//   half    hf of the block: beams [16 hf, 16 hf + 16) of its 32 columns
//   slot    s in [0, 1024): hf = s >> 9, c = (s >> 4) & 31, b = 16 hf + (s & 15) -- beams are the
//           fast index, so 16 consecutive slots are 16 consecutive points (192 B of xyz)
//
// Points past the last full group, and every scan with H = 0, keep the consecutive mapping
// (slot s of block b = point 1024 b + s).  Either way the map is a bijection between the scan's
// (block, slot) pairs below n and its points, which is all the walk kernels need: a scan's sums
// are exact and a (brick, scan) segment holds its samples in arbitrary run order.
//
// Plain C++: the kernels, the host and the CPU checks (tests/cpp/ray_tile_check.cpp) share it.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAY_TILE_HD __host__ __device__
#else
#define RAY_TILE_HD
#endif

namespace tsdf {

constexpr uint32_t TILE_RAYS = 1024;  // slots per block (= RPB, tsdf_device.h)
constexpr uint32_t TILE_COLS = 32;    // columns per group and per block
constexpr uint32_t TILE_BEAMS = 32;   // beams per block
#ifndef TSDF_TILE_HALF_BEAMS
#define TSDF_TILE_HALF_BEAMS 16       // 16: a half is 32 columns x 16 beams; 32: 16 columns x 32 beams
#endif
constexpr uint32_t TILE_HALF_BEAMS = TSDF_TILE_HALF_BEAMS;
static_assert(TILE_HALF_BEAMS == 16 || TILE_HALF_BEAMS == 32, "a half is half a block's tile");

// the column heights the map takes (0: no tiles)
RAY_TILE_HD inline bool tile_height_ok(uint32_t H) {
    return H == 0 || (H % TILE_BEAMS == 0 && H >= 64 && H <= 256);
}

// Block b of a scan of n points with column height H: the point of its slot 0 and, when the block
// is a tile, H (0: its slots are consecutive points).
struct TileBlock {
    uint32_t base, H;
};

RAY_TILE_HD inline TileBlock tile_block(uint32_t n, uint32_t H, uint32_t b) {
    if (H != 0) {
        const uint32_t bpg = H / TILE_BEAMS, g = b / bpg, G = TILE_COLS * H;
        if ((uint64_t)(g + 1) * G <= n) return TileBlock{g * G + TILE_BEAMS * (b - g * bpg), H};
    }
    return TileBlock{b * TILE_RAYS, 0u};
}

// The scan's point in slot s of the block (s < 1024; at or past n: the slot is empty).
RAY_TILE_HD inline uint32_t tile_point(const TileBlock& tb, uint32_t s) {
    if (tb.H == 0) return tb.base + s;
    const uint32_t hf = s >> 9, q = s & 511u;
    const uint32_t c = TILE_HALF_BEAMS == 16 ? q >> 4 : 16u * hf + (q >> 5);
    const uint32_t bm = TILE_HALF_BEAMS == 16 ? 16u * hf + (q & 15u) : q & 31u;
    return tb.base + c * tb.H + bm;
}

// ------------------------------------------------------------------------------------------------
// Is a scan column-regular?  Tiling by index only pays on intact columns (with 5 % of the points
// missing the tiles touch MORE bricks than the wedges), so a scan gets tiles only when its points
// show the structure: n is a multiple of H and, seen from the scan's origin, the elevation runs
// one way down every column and jumps back where the next column starts.
//
// The check reads the column BOUNDARIES only, 48 B + 24 B per column (~72 KB of a 1.5 MB scan):
// at every boundary c H (0 < c < n / H) the step into point c H must be a reset and the steps on
// either side of it must not be -- a point dropped or inserted anywhere before shifts every later
// boundary by one, which one of the three sees -- and the step into the column's middle point must
// not be a reset either, which tells a sensor of H / 2 beams from one of H.  It does not read the
// columns' interiors: a cloud that passes with scrambled interiors is tiled for nothing, which
// costs speed, never results.  Callers try H = 64, 128, 256 in this order (a scan of 64-beam
// columns also passes at 128 and 256).

// Elevation of p seen from o, as a tangent (correctly rounded fp32 division and square root on
// host and device: both take the same decision).  NaN for a point on the vertical through o.
RAY_TILE_HD inline float tile_elev(const float* p, float ox, float oy, float oz) {
    const float dx = p[0] - ox, dy = p[1] - oy, dz = p[2] - oz;
    return dz / sqrtf(dx * dx + dy * dy);
}

// Boundary c (1 <= c < n / H) of the scan at xyz: dir = the columns' direction (+1: the elevation
// rises along a column, -1: it falls).  Comparisons with a NaN fail, so a NaN rejects.
RAY_TILE_HD inline bool tile_boundary_ok(const float* xyz, uint32_t H, uint32_t c, float ox,
                                         float oy, float oz, float dir) {
    const float* p = xyz + 3 * (size_t)(c * H - 2);
    const float e0 = tile_elev(p, ox, oy, oz), e1 = tile_elev(p + 3, ox, oy, oz);
    const float e2 = tile_elev(p + 6, ox, oy, oz), e3 = tile_elev(p + 9, ox, oy, oz);
    const float* m = xyz + 3 * (size_t)(c * H + H / 2 - 1);
    const float m0 = tile_elev(m, ox, oy, oz), m1 = tile_elev(m + 3, ox, oy, oz);
    return dir * (e1 - e0) > 0.0f && dir * (e2 - e1) < 0.0f && dir * (e3 - e2) > 0.0f &&
           dir * (m1 - m0) > 0.0f;
}

// The columns' direction from the first column's first and middle steps (0: none, reject).
RAY_TILE_HD inline float tile_direction(const float* xyz, uint32_t H, float ox, float oy,
                                        float oz) {
    const float d0 = tile_elev(xyz + 3, ox, oy, oz) - tile_elev(xyz, ox, oy, oz);
    const float* m = xyz + 3 * (size_t)(H / 2 - 1);
    const float d1 = tile_elev(m + 3, ox, oy, oz) - tile_elev(m, ox, oy, oz);
    if (d0 > 0.0f && d1 > 0.0f) return 1.0f;
    if (d0 < 0.0f && d1 < 0.0f) return -1.0f;
    return 0.0f;
}

// n can be H-beam columns at all (at least two columns: one boundary to look at)
RAY_TILE_HD inline bool tile_shape_ok(uint32_t n, uint32_t H) {
    return H >= 64 && n % H == 0 && n / H >= 2;
}

// The whole decision, serially (the CPU twin of k_tile_detect): the scan's column height, or 0.
inline uint32_t tile_detect(const float* xyz, uint32_t n, float ox, float oy, float oz) {
    for (uint32_t H = 64; H <= 256; H *= 2) {
        if (!tile_shape_ok(n, H)) continue;
        const float dir = tile_direction(xyz, H, ox, oy, oz);
        bool ok = dir != 0.0f;
        for (uint32_t c = 1; ok && c < n / H; c++) ok = tile_boundary_ok(xyz, H, c, ox, oy, oz, dir);
        if (ok) return H;
    }
    return 0u;
}

}  // namespace tsdf

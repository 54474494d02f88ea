// tsdf_sample_dev.h — the device code the sparse map queries share: tsdf_sample.hip (points) and
// tsdf_raycast.hip (rays) sample the field through one definition, so a ray's march reads exactly
// what tsdf_sample_device returns at the same point (include/tsdf_hip_sample.h states the
// arithmetic; both translation units are built with -ffp-contract=off).
//
// Lookup scheme.  A point's 8 corners lie in 1, 2, 4 or 8 bricks: the base voxel's brick, plus one
// more per axis on which the cube crosses a brick face (b & 7 == 7) -- a lane probes the hash table
// for the bricks of its straddling axes only (about two thirds of the points need one probe), never
// 8 times.  A lane whose cube has an unallocated brick is invalid whatever its other bricks hold,
// and drops its remaining lookups.  The corner weights are read first; the 8 distances only where
// all 8 weights pass.
// TSDF_SAMPLE_SHARED=1 (A/B builds, `make variants`): each DISTINCT brick a wave needs is probed
// once, wave-uniformly (the leader loop of resolve_shared), and every lane that needs it takes the
// pool slot from that probe.  It issues far fewer requests and measured 1.8-2.7x SLOWER (DESIGN.md
// §11): a scan's wave touches tens of distinct bricks, the leader loop walks them one dependent
// round trip after the other, while the per-lane probes are all in flight at once.  Not shipped.
#pragma once
#include "tsdf_device.h"
#include "tsdf_ray.h"

#ifndef TSDF_SAMPLE_SHARED
#define TSDF_SAMPLE_SHARED 0
#endif

namespace tsdf {

namespace {

// pool slot of a brick, INVALID_SLOT when the map does not hold it
__device__ __forceinline__ uint32_t brick_slot(const Table& T, int bx, int by, int bz) {
    const int64_t h = table_find(T, pack_brick(bx, by, bz));
    if (h < 0) return INVALID_SLOT;
    const uint32_t s = T.slots[h];
    return s < T.max_bricks ? s : INVALID_SLOT;
}

// The pool slots of a lane's NC corners (corner c = dx | dy << 1 | dz << 2): corner c lies in brick
// (bx, by, bz) + the offset c & m, m the lane's mask of straddling axes.  Returns false when the
// lane is inactive or one of its bricks is not in the map.  Every lane of the wave calls it.
// (The A/B variant, TSDF_SAMPLE_SHARED.)
template <int NC>
__device__ __forceinline__ bool resolve_shared(const Table& T, bool active, int bx, int by, int bz,
                                               uint32_t m, uint32_t (&cslot)[NC]) {
    // pend: bit o set while the brick at offset o (a subset of m) is still to be looked up
    uint32_t pend = 0;
    if (active) {
#pragma unroll
        for (uint32_t o = 0; o < (uint32_t)NC; o++)
            if ((o & ~m) == 0) pend |= 1u << o;
    }
    bool ok = active;
#pragma unroll
    for (int c = 0; c < NC; c++) cslot[c] = INVALID_SLOT;
    for (;;) {
        const uint64_t bal = __ballot(pend != 0);
        if (!bal) break;
        // the first lane with a pending brick leads: its lowest pending brick is probed once for
        // the wave, and every lane waiting for that brick takes the result
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)bal) - 1);
        const uint32_t lp = (uint32_t)__builtin_amdgcn_readlane((int)pend, leader);
        const int o = __ffs(lp) - 1;
        const int kx = __builtin_amdgcn_readlane(bx, leader) + (o & 1);
        const int ky = __builtin_amdgcn_readlane(by, leader) + ((o >> 1) & 1);
        const int kz = __builtin_amdgcn_readlane(bz, leader) + (o >> 2);
        const uint32_t s = brick_slot(T, kx, ky, kz);
        const uint32_t dx = (uint32_t)(kx - bx), dy = (uint32_t)(ky - by), dz = (uint32_t)(kz - bz);
        const uint32_t om = (dx | (dy << 1) | (dz << 2)) & 7u;
        if ((dx | dy | dz) <= 1u && ((pend >> om) & 1u)) {
            if (s == INVALID_SLOT) {
                ok = false;
                pend = 0;
            } else {
                pend &= ~(1u << om);
#pragma unroll
                for (uint32_t c = 0; c < (uint32_t)NC; c++)
                    if ((c & m) == om) cslot[c] = s;
            }
        }
    }
    return ok;
}

// the shipped lookup: every lane probes its own 1, 2, 4 or 8 bricks
template <int NC>
__device__ __forceinline__ bool resolve_lane(const Table& T, bool active, int bx, int by, int bz,
                                              uint32_t m, uint32_t (&cslot)[NC]) {
    bool ok = active;
#pragma unroll
    for (int c = 0; c < NC; c++) cslot[c] = INVALID_SLOT;
#pragma unroll
    for (uint32_t o = 0; o < (uint32_t)NC; o++) {
        if (ok && (o & ~m) == 0) {
            const uint32_t s = brick_slot(T, bx + (int)(o & 1), by + (int)((o >> 1) & 1),
                                          bz + (int)(o >> 2));
            if (s == INVALID_SLOT) {
                ok = false;
            } else {
#pragma unroll
                for (uint32_t c = 0; c < (uint32_t)NC; c++)
                    if ((c & m) == o) cslot[c] = s;
            }
        }
    }
    return ok;
}

template <int NC>
__device__ __forceinline__ bool resolve(const Table& T, bool active, int bx, int by, int bz,
                                        uint32_t m, uint32_t (&cslot)[NC]) {
#if TSDF_SAMPLE_SHARED
    return resolve_shared<NC>(T, active, bx, by, bz, m, cslot);
#else
    return resolve_lane<NC>(T, active, bx, by, bz, m, cslot);
#endif
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

struct Sample {
    float s, w, gx, gy, gz;
    bool valid;
};

// Where a sample reads: its base voxel (x, y, z) -- the voxel itself (nearest) or corner 0 of the
// cube (trilinear) -- the position inside the cube (trilinear), and whether the sample lies in the
// index domain at all (0, 0, 0 where it does not).
struct Base {
    int x, y, z;
    float fx, fy, fz;
    bool inside;
};

// nearest: the voxel floorf(p * inv), inside |i| < 2^23
__device__ __forceinline__ Base base_nearest(float inv, bool live, float px, float py, float pz) {
    const float vx = floorf(px * inv), vy = floorf(py * inv), vz = floorf(pz * inv);
    const float lim = (float)VOX_LIMIT;
    // decided on the floats (a NaN fails every comparison); the conversions below are then exact
    const bool inside = live && vx > -lim && vx < lim && vy > -lim && vy < lim && vz > -lim &&
                        vz < lim;
    return Base{inside ? (int)vx : 0, inside ? (int)vy : 0, inside ? (int)vz : 0, 0.0f, 0.0f, 0.0f,
                inside};
}

// trilinear: b = floorf(p * inv - 0.5f), f = u - b, every corner b + {0, 1} inside |i| < 2^23
__device__ __forceinline__ Base base_trilinear(float inv, bool live, float px, float py, float pz) {
    const float ux = px * inv - 0.5f, uy = py * inv - 0.5f, uz = pz * inv - 0.5f;
    const float bfx = floorf(ux), bfy = floorf(uy), bfz = floorf(uz);
    const float fx = ux - bfx, fy = uy - bfy, fz = uz - bfz;
    // decided on the floats
    const float lo = -(float)(VOX_LIMIT - 1), hi = (float)(VOX_LIMIT - 2);
    const bool inside = live && isfinite(px) && isfinite(py) && isfinite(pz) && bfx >= lo &&
                        bfx <= hi && bfy >= lo && bfy <= hi && bfz >= lo && bfz <= hi;
    return Base{inside ? (int)bfx : 0, inside ? (int)bfy : 0, inside ? (int)bfz : 0, fx, fy, fz,
                inside};
}

// the mask of axes on which the cube at base voxel b crosses a brick face
__device__ __forceinline__ uint32_t straddle_mask(const Base& b) {
    return ((b.x & 7) == 7 ? 1u : 0u) | ((b.y & 7) == 7 ? 2u : 0u) | ((b.z & 7) == 7 ? 4u : 0u);
}

// VALUES = false (the map merge's validity pass, tsdf_merge.hip): the sample's weight and validity
// alone, decided exactly as below; no distance is read and s, gx, gy, gz are not meaningful.

// the nearest sample of base voxel b in the brick at pool slot `slot`
template <bool VALUES = true>
__device__ __forceinline__ Sample eval_nearest(const Pool& Pl, float bg, float min_w, const Base& b,
                                               uint32_t slot) {
    Sample r{bg, 0.0f, 0.0f, 0.0f, 0.0f, false};
    const size_t i = (size_t)slot * BRICK_VOX + (((b.z & 7) << 6) | ((b.y & 7) << 3) | (b.x & 7));
    if constexpr (VALUES) r.s = Pl.sdf[i];
    r.w = Pl.weight[i];
    r.valid = r.w > 0.0f && r.w >= min_w;
    return r;
}

// the trilinear sample of the cube at base voxel b, its corners' bricks at pool slots cslot
template <bool VALUES = true>
__device__ __forceinline__ Sample eval_trilinear(const Pool& Pl, float inv, float bg, float min_w,
                                                 const Base& b, const uint32_t (&cslot)[8]) {
    const int lx = b.x & 7, ly = b.y & 7, lz = b.z & 7;
    const float fx = b.fx, fy = b.fy, fz = b.fz;
    Sample r{bg, 0.0f, 0.0f, 0.0f, 0.0f, false};
    size_t idx[8];
    float w[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int l = (((lz + (c >> 2)) & 7) << 6) | (((ly + ((c >> 1) & 1)) & 7) << 3) |
                      ((lx + (c & 1)) & 7);
        idx[c] = (size_t)cslot[c] * BRICK_VOX + l;
        w[c] = Pl.weight[idx[c]];
    }
    bool all = true;
    float wmin = w[0];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        all = all && w[c] > 0.0f && w[c] >= min_w;
        wmin = fminf(wmin, w[c]);
    }
    if constexpr (!VALUES) {
        if (all) {
            r.w = wmin;
            r.valid = true;
        }
        return r;
    }
    if (all) {
        float s[8];
#pragma unroll
        for (int c = 0; c < 8; c++) s[c] = Pl.sdf[idx[c]];
        // s[dx | dy << 1 | dz << 2]; S: x, then y, then z
        const float c00 = lerp(s[0], s[1], fx), c10 = lerp(s[2], s[3], fx);
        const float c01 = lerp(s[4], s[5], fx), c11 = lerp(s[6], s[7], fx);
        r.s = lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz);
        r.w = wmin;
        // d/dx: the x differences over (y, z); d/dy: the y differences over (x, z); d/dz: the z
        // differences over (x, y)
        r.gx = lerp(lerp(s[1] - s[0], s[3] - s[2], fy), lerp(s[5] - s[4], s[7] - s[6], fy), fz) *
               inv;
        r.gy = lerp(lerp(s[2] - s[0], s[3] - s[1], fx), lerp(s[6] - s[4], s[7] - s[5], fx), fz) *
               inv;
        r.gz = lerp(lerp(s[4] - s[0], s[5] - s[1], fx), lerp(s[6] - s[2], s[7] - s[3], fx), fy) *
               inv;
        r.valid = true;
    }
    return r;
}

// The voxel floorf(p * inv): its (S, W), (bg, 0) where unallocated or outside |i| < 2^23.
template <bool VALUES = true>
__device__ __forceinline__ Sample sample_nearest(const Table& T, const Pool& Pl, float inv, float bg,
                                                 float min_w, bool live, float px, float py,
                                                 float pz) {
    const Base b = base_nearest(inv, live, px, py, pz);
    uint32_t cslot[1];
    const bool ok = resolve<1>(T, b.inside, b.x >> 3, b.y >> 3, b.z >> 3, 0u, cslot);
    if (ok) return eval_nearest<VALUES>(Pl, bg, min_w, b, cslot[0]);
    return Sample{bg, 0.0f, 0.0f, 0.0f, 0.0f, false};
}

// The trilinear interpolant of the 8 voxel centres around p and its gradient (tsdf_hip_sample.h).
template <bool VALUES = true>
__device__ __forceinline__ Sample sample_trilinear(const Table& T, const Pool& Pl, float inv,
                                                   float bg, float min_w, bool live, float px,
                                                   float py, float pz) {
    const Base b = base_trilinear(inv, live, px, py, pz);
    uint32_t cslot[8];
    const bool ok = resolve<8>(T, b.inside, b.x >> 3, b.y >> 3, b.z >> 3, straddle_mask(b), cslot);
    if (ok) return eval_trilinear<VALUES>(Pl, inv, bg, min_w, b, cslot);
    return Sample{bg, 0.0f, 0.0f, 0.0f, 0.0f, false};
}

}  // namespace

}  // namespace tsdf

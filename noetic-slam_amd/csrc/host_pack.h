// host_pack.h -- the host side of libtsdf_hip's point input (tsdf_capi.cpp): the record ->
// packed-xyz packer, the host split's sector rule and the scheduler over the contexts' staging
// pools.  Plain C++ like pack_pool.h, checked and sanitized on the CPU (tests/test_host_pack.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>

#include "pack_pool.h"

namespace tsdf {

// A caller's PointCloud2-style records: record i starts at base + i * point_step and holds x, y, z
// (fp32, or fp64 with is_f64) at xyz_offset, at any alignment.
struct RecordView {
    const char* base;
    uint32_t point_step, xyz_offset;
    bool is_f64;
    bool layout_ok() const {
        const uint32_t need = is_f64 ? 24u : 12u;
        return point_step >= need && xyz_offset <= point_step - need;
    }
    bool packed_f32() const { return !is_f64 && point_step == 12 && xyz_offset == 0; }
};

// Records [i0, i1) as packed fp32 xyz in dst[0 .. 3 (i1 - i0)): one memcpy when they are packed
// fp32 already; fp64 is rounded to fp32 by the cast.
inline void pack_xyz(const RecordView& v, uint64_t i0, uint64_t i1, float* dst) {
    if (i1 <= i0) return;
    if (v.packed_f32()) {
        std::memcpy(dst, v.base + 12 * i0, (i1 - i0) * 12);
        return;
    }
    const char* q = v.base + i0 * v.point_step + v.xyz_offset;
    for (uint64_t i = i0; i < i1; i++, q += v.point_step, dst += 3) {
        if (v.is_f64) {
            double d[3];
            std::memcpy(d, q, sizeof d);
            dst[0] = (float)d[0];
            dst[1] = (float)d[1];
            dst[2] = (float)d[2];
        } else {
            std::memcpy(dst, q, 12);
        }
    }
}

// Records [i0, i1) of a cloud cut into n_dst contiguous shares, share k = [lo[k], lo[k + 1]) with
// lo[n_dst] >= i1 (a share may be empty): each record to its share's buffer, lo[k] at dst[k][0].
inline void pack_shares(const RecordView& v, uint64_t i0, uint64_t i1, const uint64_t* lo,
                        uint32_t n_dst, float* const* dst) {
    uint32_t k = 0;
    while (k + 1 < n_dst && lo[k + 1] <= i0) k++;
    for (uint64_t i = i0; i < i1; k++) {
        const uint64_t e = std::min(i1, lo[k + 1]);  // share k's piece of [i0, i1)
        pack_xyz(v, i, e, dst[k] + 3 * (i - lo[k]));
        i = e;
    }
}

// The sector of pseudo-angle a (tsdf_device.h, in [0, 4)) among N: the sector starts, rotated to
// ascending order u_j = s_((r0 + j) mod N), give sector (r0 + #{j: a >= u_j} - 1) mod N -- the
// kernels' in_sector test on every sector's [lo, hi) bounds (the wrap sector holds a < u_0 and
// a >= u_(N-1)) in N compares.  NaN: -1, no sector (every kernel drops the ray).
inline int sector_of_angle(float a, const float* u, uint32_t r0, uint32_t N) {
    uint32_t c = 0;
    for (uint32_t j = 0; j < N; j++) c += a >= u[j] ? 1u : 0u;
    uint32_t m = r0 + c + N - 1u;  // (r0 + c - 1) mod N without a division: m < 3N
    m -= m >= N ? N : 0u;
    m -= m >= N ? N : 0u;
    return a != a ? -1 : (int)m;
}

// The parts a cloud is cut into: one for the calling thread and one per worker of the given pools
// (a null entry: a context without a pool); below min_points one part, not worth waking anybody.
constexpr uint64_t PARTS_MIN_POINTS = 1u << 15;
inline int part_count(PackPool* const* pools, uint32_t n_pools, uint64_t n_points,
                      uint64_t min_points = PARTS_MIN_POINTS) {
    int parts = 1;
    for (uint32_t k = 0; k < n_pools && n_points >= min_points; k++)
        if (pools[k]) parts += pools[k]->parts() - 1;
    return parts;
}

// f(q, i0, i1) once for every part q = [n q / parts, n (q + 1) / parts), side by side: pool 0
// runs the caller's part and its workers', the later pools' workers the parts after them.
// Returns part_count().
inline int run_parts(PackPool* const* pools, uint32_t n_pools, uint64_t n_points,
                     const std::function<void(int, uint64_t, uint64_t)>& f,
                     uint64_t min_points = PARTS_MIN_POINTS) {
    const int parts = part_count(pools, n_pools, n_points, min_points);
    const uint64_t n = n_points, np = (uint64_t)parts;
    if (parts == 1) {
        f(0, 0, n);
        return 1;
    }
    const std::function<void(int)> part = [&f, n, np](int q) {
        f(q, n * (uint64_t)q / np, n * (uint64_t)(q + 1) / np);
    };
    int base = pools[0] ? pools[0]->parts() : 1;  // the first part of the next pool's workers
    for (uint32_t k = 1; k < n_pools; k++)
        if (pools[k]) {
            pools[k]->start(part, base - 1);
            base += pools[k]->parts() - 1;
        }
    if (pools[0]) pools[0]->run(part);
    else part(0);
    for (uint32_t k = 1; k < n_pools; k++)
        if (pools[k]) pools[k]->wait();
    return parts;
}

}  // namespace tsdf

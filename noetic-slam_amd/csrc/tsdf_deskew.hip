// tsdf_deskew.hip — motion-compensated Ouster frames (include/tsdf_hip_deskew.h):
//   k_os_deskew  UDP lidar packets of one frame + the xyz LUT + one pose per column -> world
//                points, each under the pose of its own column, in one pass: RANGE is decoded as
//                k_os_decode decodes it (tsdf_ouster.hip), projected and posed with k_os_xyz's
//                expressions, and no range image is written or read back in between.
// One workgroup per (packet, column), lanes stride over the column's pixels.  Everything is
// column-major (index m_id * h + u), the packet's own order: a column's lanes read contiguous
// packet bytes and LUT rows and write h * 12 contiguous bytes.  The caller has filled d_xyz with
// 0xFF bytes (NaN) and d_range with zeros: a skipped column and an r = 0 pixel write nothing.
// Two different valid columns with the same measurement_id: k_os_decode's caveat holds here too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tsdf_device.h"

namespace tsdf {

namespace {
__device__ __forceinline__ uint32_t le_u32(const uint8_t* p, uint32_t n) {
    uint32_t v = 0;
    for (uint32_t k = 0; k < n; k++) v |= (uint32_t)p[k] << (8 * k);
    return v;
}
}  // namespace

__global__ void __launch_bounds__(128)
k_os_deskew(const uint8_t* __restrict__ pk, uint32_t n_packets, OsLayout L,
            const float* __restrict__ dir, const float* __restrict__ off,
            const float* __restrict__ col_pose, float* __restrict__ xyz,
            uint32_t* __restrict__ rng) {
    const uint32_t col = blockIdx.x % L.cols_per_packet, p = blockIdx.x / L.cols_per_packet;
    if (p >= n_packets) return;
    const uint8_t* cb = pk + (size_t)p * L.packet_bytes + L.packet_header + col * L.col_bytes;
    // every lane reads the same header bytes: keep the id in a scalar register, so the pose row
    // below is a scalar load
    const uint32_t m_id = __builtin_amdgcn_readfirstlane(le_u32(cb + 8, 2));
    const uint32_t status = __builtin_amdgcn_readfirstlane(
        L.legacy ? le_u32(cb + L.col_bytes - 4, 4) : le_u32(cb + 10, 2));
    if (m_id >= L.w || !(status & 1u)) return;
    const float* m = col_pose + (size_t)12 * m_id;
    const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6],
                m7 = m[7], m8 = m[8], m9 = m[9], m10 = m[10], m11 = m[11];
    const OsField F = L.f[0];
    const size_t j0 = (size_t)m_id * L.h;
    for (uint32_t px = threadIdx.x; px < L.h; px += blockDim.x) {
        uint32_t r = le_u32(cb + L.col_header + px * L.pixel_bytes + F.offset, F.nbytes);
        if (F.mask) r &= F.mask;
        if (F.shift > 0) r >>= F.shift;
        if (F.shift < 0) r <<= -F.shift;
        const size_t j = j0 + px;
        if (rng) rng[j] = r;
        if (r == 0u) continue;
        const float rf = (float)r;
        const float x = rf * dir[3 * j] + off[3 * j];
        const float y = rf * dir[3 * j + 1] + off[3 * j + 1];
        const float z = rf * dir[3 * j + 2] + off[3 * j + 2];
        xyz[3 * j] = m0 * x + m1 * y + m2 * z + m3;
        xyz[3 * j + 1] = m4 * x + m5 * y + m6 * z + m7;
        xyz[3 * j + 2] = m8 * x + m9 * y + m10 * z + m11;
    }
}

hipError_t launch_os_deskew(const uint8_t* d_packets, uint32_t n_packets, const OsLayout& L,
                            const float* d_dir, const float* d_off, const float* d_col_pose,
                            float* d_xyz, uint32_t* d_range, hipStream_t st) {
    if (n_packets == 0) return hipSuccess;
    const uint32_t threads = L.h >= 128 ? 128u : 64u;
    k_os_deskew<<<n_packets * L.cols_per_packet, threads, 0, st>>>(
        d_packets, n_packets, L, d_dir, d_off, d_col_pose, d_xyz, d_range);
    return hipGetLastError();
}

}  // namespace tsdf

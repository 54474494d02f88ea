// os_headers.h -- the host side of the Ouster packet path (tsdf_capi.cpp): the packet layout per
// UDP profile, shared with the kernels (tsdf_ouster.hip, tsdf_deskew.hip), and the column headers
// of one frame's packets (timestamp, status, measurement id) under the SDK's ScanBatcher rule
// (ouster_client/src/lidar_scan.cpp:586-631).  Plain C++ like host_pack.h and brick_key.h, checked
// and sanitized on the CPU (tests/test_deskew_headers.py).
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/tsdf_hip.h"

namespace tsdf {

struct OsField {
    uint32_t nbytes;  // little-endian source bytes (0: the profile has no such field)
    uint32_t offset;  // byte offset in the pixel
    uint32_t mask;    // 0: none
    int32_t shift;    // > 0: right, < 0: left
};
struct OsLayout {
    uint32_t h, w, cols_per_packet, packet_bytes, packet_header, col_header, col_bytes,
        pixel_bytes, legacy;
    OsField f[4];  // RANGE, SIGNAL, REFLECTIVITY, NEAR_IR
};

// Ouster packet layouts per UDP profile (ouster_client/src/parsing.cpp:42-175): header / column /
// footer sizes and, for RANGE, SIGNAL, REFLECTIVITY, NEAR_IR: (bytes, offset, mask, shift).
inline bool os_layout(const tsdf_os_format* f, OsLayout& L) {
    if (!f || f->pixels_per_column == 0 || f->columns_per_packet == 0 || f->columns_per_frame == 0 ||
        f->pixels_per_column > 4096)
        return false;
    L = OsLayout{};
    L.h = f->pixels_per_column;
    L.w = f->columns_per_frame;
    L.cols_per_packet = f->columns_per_packet;
    switch (f->profile) {
        case TSDF_OS_LEGACY:
            L.pixel_bytes = 12;
            L.f[0] = {4, 0, 0x000FFFFFu, 0};
            L.f[1] = {2, 6, 0, 0};
            L.f[2] = {2, 4, 0, 0};
            L.f[3] = {2, 8, 0, 0};
            break;
        case TSDF_OS_RNG19_RFL8_SIG16_NIR16:
            L.pixel_bytes = 12;
            L.f[0] = {4, 0, 0x0007FFFFu, 0};
            L.f[1] = {2, 6, 0, 0};
            L.f[2] = {1, 4, 0, 0};
            L.f[3] = {2, 8, 0, 0};
            break;
        case TSDF_OS_RNG19_RFL8_SIG16_NIR16_DUAL:
            L.pixel_bytes = 16;
            L.f[0] = {4, 0, 0x0007FFFFu, 0};
            L.f[1] = {2, 8, 0, 0};
            L.f[2] = {1, 3, 0, 0};
            L.f[3] = {2, 12, 0, 0};
            break;
        case TSDF_OS_RNG15_RFL8_NIR8:
            L.pixel_bytes = 4;
            L.f[0] = {2, 0, 0x7FFFu, -3};
            L.f[1] = {0, 0, 0, 0};
            L.f[2] = {1, 2, 0, 0};
            L.f[3] = {1, 3, 0, -4};
            break;
        default:
            return false;
    }
    L.legacy = f->profile == TSDF_OS_LEGACY ? 1u : 0u;
    L.packet_header = L.legacy ? 0u : 32u;
    L.col_header = L.legacy ? 16u : 12u;
    const uint32_t col_footer = L.legacy ? 4u : 0u, packet_footer = L.legacy ? 0u : 32u;
    L.col_bytes = L.col_header + L.h * L.pixel_bytes + col_footer;
    L.packet_bytes = L.packet_header + L.cols_per_packet * L.col_bytes + packet_footer;
    return true;
}

inline uint64_t os_le(const uint8_t* p, uint32_t n) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < n; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

// The column headers of n_packets packets of one frame (host bytes, back to back) into the w
// entries of timestamp, status and measurement_id: all zeroed first; then, packet by packet and
// column by column, a column with m_id < w and status bit 0 set writes its three values at m_id
// (a later column with the same id overwrites an earlier one, as the batcher does).
inline int os_headers(const tsdf_os_format* fmt, const uint8_t* packets, uint32_t n_packets,
                      uint64_t* timestamp, uint32_t* status, uint16_t* measurement_id) {
    OsLayout L;
    if (!os_layout(fmt, L) || !timestamp || !status || !measurement_id || (n_packets && !packets))
        return TSDF_EINVAL;
    std::memset(timestamp, 0, sizeof(uint64_t) * L.w);
    std::memset(status, 0, sizeof(uint32_t) * L.w);
    std::memset(measurement_id, 0, sizeof(uint16_t) * L.w);
    for (uint32_t p = 0; p < n_packets; p++) {
        const uint8_t* pb = packets + (size_t)p * L.packet_bytes + L.packet_header;
        for (uint32_t col = 0; col < L.cols_per_packet; col++) {
            const uint8_t* cb = pb + (size_t)col * L.col_bytes;
            const uint32_t m_id = (uint32_t)os_le(cb + 8, 2);
            const uint32_t st =
                (uint32_t)(L.legacy ? os_le(cb + L.col_bytes - 4, 4) : os_le(cb + 10, 2));
            if (m_id >= L.w || !(st & 1u)) continue;
            timestamp[m_id] = os_le(cb, 8);
            status[m_id] = st;
            measurement_id[m_id] = (uint16_t)m_id;
        }
    }
    return TSDF_OK;
}

}  // namespace tsdf

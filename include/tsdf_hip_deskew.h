/* tsdf_hip_deskew.h — motion-compensated Ouster frames for libtsdf_hip.so: one pose per column.
 *
 * tsdf_os_decode_device + tsdf_os_cartesian_device (tsdf_hip.h) give every pixel of a frame one
 * pose.  A sweep takes about 100 ms, so on a moving platform that skews the frame (the reference
 * removes the skew on the CPU, dlio::OdomNode::deskewPointcloud, odom.cc:588-706: one SE(3) per
 * column timestamp).  Here one frame's packets and one pose per column go in, and world points come
 * out, each under the pose of its own column, in column (time) order; cut into consecutive
 * segments, they go to tsdf_integrate_batch_device_pose as sub-scans with an origin each.
 *
 * Like sampling and raycasting, this is a GPU-library feature outside the tsdf_hip.h contract:
 * TSDF_ABI_VERSION stays as it is and a caller detects the feature by the presence of the symbols
 * (dlsym / TSDF_DESKEW_API at compile time).
 *
 * Column headers (tsdf_os_headers; host only, no context, no GPU).  The SDK's ScanBatcher rule
 * (ouster_client/src/lidar_scan.cpp:586-631): the three arrays (w = columns_per_frame entries each)
 * are zeroed; then for every column of every packet, in order, m_id is the 2 bytes at byte 8 of
 * the column, status the 4 bytes of the legacy column footer or the 2 bytes at byte 10 of the
 * column header, ts the 8 bytes at byte 0 (all little-endian); a column with m_id >= w or status
 * bit 0 clear is skipped, any other sets timestamp[m_id] = ts, status[m_id] = status,
 * measurement_id[m_id] = m_id.
 *
 * Points (tsdf_os_deskew_device; all fp32, evaluated in the stated order; the library is built
 * without FMA contraction, so a restatement in the same order reproduces the bits).  Everything is
 * COLUMN-major, the packet's own order: pixel u of column m_id has index j = m_id * h + u in
 * d_dir_cm, d_off_cm, d_xyz and d_range_cm (tsdf_os_cartesian_device's images and LUT are
 * row-major, u * w + m_id: transpose the LUT once).
 *   Fill     d_xyz is filled with 0xFF bytes (every float a NaN) and d_range_cm with zeros.
 *   Skip     a column with m_id >= w or status bit 0 clear writes nothing (the rule above).
 *   Decode   r = the pixel's RANGE exactly as tsdf_os_decode_device decodes it (mm, masked /
 *            shifted per profile); d_range_cm[j] = r.
 *   Zero     r == 0 writes no point.
 *   Project  rf = (float)r; x = rf * dir[3j] + off[3j], likewise y and z (one product, one sum).
 *   Pose     with m = column m_id's 12 floats, 3x4 row-major (rotation | translation), per row
 *            X = ((m0 * x + m1 * y) + m2 * z) + m3 -- tsdf_os_cartesian_device's expression, so
 *            equal inputs give equal bits.  No test of the pose: a NaN row gives NaN by IEEE
 *            arithmetic.
 * So a point is a NaN triple when its column is missing or invalid, its pixel has zero range, or
 * its column's pose row is NaN.  The far-ray rule (tsdf_hip.h, "Index domain") drops such a ray
 * under every fusion rule and whatever min_range is, so d_xyz goes to the integrate as it is,
 * without compaction or read-back.  Two different valid columns with the same m_id in one frame:
 * which of them d_xyz keeps is not defined (identical repeats are harmless).
 *
 * Segments (the caller's side; tsdf_map.ouster.frame_segments).  K sub-scans, 1 <= K <= w:
 * b_k = floor(k * w / K), scan_offsets[k] = h * b_k (TSDF_SECTOR_RULE_INDEX's index rule); segment
 * k takes the pose of its column with a finite pose nearest (b_k + b_{k+1}) / 2 (integer
 * division; ties to the lower column); a segment without one takes position 0 and the identity
 * quaternion -- all of its points are NaN.
 */
#ifndef TSDF_HIP_DESKEW_H
#define TSDF_HIP_DESKEW_H

#include "tsdf_hip.h"

#define TSDF_DESKEW_API 1

#ifdef __cplusplus
extern "C" {
#endif

/* Column headers of n_packets packets of ONE frame (host memory, packed back to back) into host
 * arrays of columns_per_frame entries each.  TSDF_EINVAL for a bad format or a NULL pointer
 * (packets may be NULL only with n_packets == 0). */
int tsdf_os_headers(const tsdf_os_format* fmt, const uint8_t* packets, uint32_t n_packets,
                    uint64_t* timestamp, uint32_t* status, uint16_t* measurement_id);

/* n_packets packets of ONE frame into d_xyz (w * h x 3 float32) and, unless NULL, d_range_cm
 * (w * h uint32), by the rules above.  d_dir_cm, d_off_cm: the xyz LUT, w * h x 3 float32 each,
 * column-major; d_col_pose: w x 12 float32.  All pointers are device memory of the context's GPU.
 * The work is ordered on the context's stream and the call does not wait, like the other
 * tsdf_os_* calls: the inputs must be complete before the call and stay valid until the next
 * tsdf_sync.  n_packets == 0 still fills the outputs.  TSDF_EINVAL, with a message, for a bad
 * format, a NULL required buffer, or n_packets * columns_per_packet > 2^20. */
int tsdf_os_deskew_device(tsdf_ctx* ctx, const tsdf_os_format* fmt, const uint8_t* d_packets,
                          uint32_t n_packets, const float* d_dir_cm, const float* d_off_cm,
                          const float* d_col_pose, float* d_xyz, uint32_t* d_range_cm);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_DESKEW_H */

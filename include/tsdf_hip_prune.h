/* tsdf_hip_prune.h — removing bricks from the map of libtsdf_hip.so: prune and evict.
 *
 * tsdf_hip.h grows the map; these entry points shrink it, in place and on the GPU.  tsdf_prune is
 * VDBFusion's VDBVolume::Prune(min_weight); tsdf_evict_outside drops every brick outside a box of
 * brick coordinates and hands the dropped bricks to the caller in tsdf_export_bricks' format, so a
 * live node keeps a local map around the sensor and archives the rest (tsdf_import_bricks merges
 * an archived brick back with the border-merge rule).
 *
 * Like sampling and the raycast, this is a GPU-library feature outside the tsdf_hip.h contract:
 * TSDF_ABI_VERSION stays as it is and a caller detects the feature by the presence of the symbols
 * (dlsym / TSDF_PRUNE_API at compile time).
 *
 * VDBFusion is not among the sources this library was restated from, so the rules written here
 * ARE the contract; nothing else defines what these calls do.
 *
 * Common rules (those of tsdf_import_bricks).  Each call first flushes the pending batch and
 * waits for the field, so capacity growth and batch replay are settled before anything is
 * removed.  TSDF_EINVAL for a NULL context, for a context with an open border reduce (commit or
 * abort it first), for a NULL box, for lo[a] > hi[a] on any axis, and for a negative or NaN
 * min_weight.  A box with lo[a] == hi[a] on some axis is empty: every brick is outside it.
 *
 * What stays.  A removed brick reads as unobserved afterwards, everywhere: tsdf_query_dense gives
 * (background, 0), the sampling calls give invalid, the mesh has no cube with it, and the next
 * scan that reaches it allocates it afresh from the background.  The bricks that stay keep every
 * bit of their voxels.  The order of bricks inside the pool changes (the holes are filled from
 * the pool's tail), which no entry point shows: exports, meshes and halo lists are ordered by
 * brick coordinate.  When nothing is removed, nothing is touched.
 *
 * Capacity is not shrunk: the pool and the table keep their size (tsdf_stats.max_bricks), and no
 * device memory goes back to the driver.  The freed bricks are reused by later scans and imports
 * before the pool grows again.
 */
#ifndef TSDF_HIP_PRUNE_H
#define TSDF_HIP_PRUNE_H

#include "tsdf_hip.h"

#define TSDF_PRUNE_API 1

#ifdef __cplusplus
extern "C" {
#endif

/* After VDBFusion's VDBVolume::Prune: every voxel with W < min_weight is reset to the background
 * (bg, 0), bg being sdf_trunc for the VDBFusion semantics and 0 for Voxblox; every brick left
 * without an observed voxel (W > 0) is removed.  In place.  min_weight == 0 resets no voxel and
 * removes the bricks that hold no observed voxel.  *n_removed = bricks removed (may be NULL). */
int tsdf_prune(tsdf_ctx* ctx, float min_weight, uint64_t* n_removed);

/* Bricks whose brick coordinate b (voxel = 8 * b + local) is NOT in lo[a] <= b[a] < hi[a] on
 * every axis.  The map is not changed. */
int tsdf_count_outside(tsdf_ctx* ctx, const int32_t lo[3], const int32_t hi[3], uint64_t* n);

/* Remove those bricks and copy them out in tsdf_export_bricks' format and order (z, y, x):
 * coords 3 int32, sdf and weight 512 float32 (voxel z * 64 + y * 8 + x) per brick.  coords / sdf /
 * weight may each be NULL (not written); with all three NULL, cap is not looked at.  If any is
 * non-NULL and cap < the count: TSDF_EOVERFLOW, *n_out = the count, and the map is unchanged.
 * *n_out = bricks removed (may be NULL).  The copy-out needs device scratch of at most 64 MiB,
 * whatever the size of the map. */
int tsdf_evict_outside(tsdf_ctx* ctx, const int32_t lo[3], const int32_t hi[3], int32_t* coords,
                       float* sdf, float* weight, uint64_t cap, uint64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_PRUNE_H */

/* tsdf_hip_esdf.h — the Euclidean distance field of a map box of libtsdf_hip.so: how far the
 * nearest surface is from every voxel of the box.
 *
 * A TSDF knows the distance to the surface only inside its band, +-sdf_trunc.  Planners, collision
 * checkers and exploration code need clearance out to a metre or two: the ESDF layer that Voxblox
 * builds on top of its TSDF.  These entry points compute it for a box of voxels on the GPU: the
 * exact Euclidean distance transform of the box's surface voxels (its "sites"), truncated at a
 * radius, signed by the TSDF where the voxel is observed.
 *
 * Like sampling, raycasting and pruning, this is a GPU-library feature outside the tsdf_hip.h
 * contract: TSDF_ABI_VERSION stays as it is and a caller detects the feature by the presence of
 * the symbols (dlsym / TSDF_ESDF_API at compile time).
 *
 * The box and the output layout are tsdf_query_dense's: voxels lo..hi-1 per axis, x fastest
 * (index = x + nx (y + ny z), n = hi - lo).
 *
 * Semantics.  These rules ARE the contract; vs = (float)voxel_size, R = radius_vox.  Squared
 * distances are integers, the result takes one correctly rounded square root and one product, so a
 * restatement reproduces the bits.
 *
 *   1. Each voxel of the box reads (S, W) exactly as tsdf_query_dense does: a voxel of a brick the
 *      map does not hold, and a voxel outside |i| < 2^23, reads (background, 0).
 *        observed = W > 0 && W >= min_weight
 *        site     = observed && fabsf(S) <= site_band          (an fp32 compare)
 *   2. The box is the world: only sites inside the box count.  A caller who wants clearances that
 *      are exact up to R vs at the rim of a box pads the box by R and crops.
 *   3. d2(v) = min over the sites u of the box with |u - v|_inf <= R of |u - v|^2 (integer voxel
 *      offsets, an integer).  capped = no such site, or d2 > R^2; if capped, d2 = R^2.  This is the
 *      exact Euclidean transform truncated at R: a site within Euclidean distance R has every axis
 *      offset at most R.
 *   4. dist = sqrtf((float)d2) * vs, negated when observed && S < 0.  A site behind the surface
 *      therefore reads -0.0f: the bit keeps the sign and is part of the contract.  An unobserved
 *      voxel gets its distance to the nearest site with a positive sign and flags 0: what
 *      "unknown" means is the caller's business.
 *   5. flags = observed | site << 1 | capped << 2  (TSDF_ESDF_OBSERVED, _SITE, _CAPPED).
 *
 * Entry rules.  Each call flushes the pending batch and waits for the field, as the raycast does,
 * and its outputs are complete when it returns.  A context with an open border reduce is refused,
 * and so is a context created with n_sectors > 1.  TSDF_EINVAL, with a message, for: a NULL lo or
 * hi; radius_vox == 0 or radius_vox > TSDF_ESDF_MAX_RADIUS; a negative or non-finite site_band; a
 * negative or NaN min_weight; hi < lo on an axis; an extent of 2^31 voxels or more; a box above
 * 2^28 voxels; a NULL dist for a box that is not empty.  flags may be NULL.  An empty box (an
 * extent of 0) returns TSDF_OK and launches nothing.  The call never modifies the map.
 *
 * Scratch.  The call holds 5 bytes of device scratch per voxel of the box while it runs (two
 * planes of 16-bit squared distances and one byte of voxel class), at most 1.25 GiB at the 2^28
 * voxel bound; tsdf_esdf_dense adds the 5 bytes per voxel of the device copy of its outputs.  If
 * the scratch cannot be allocated the call returns TSDF_ENOMEM and leaves dist and flags
 * untouched.
 */
#ifndef TSDF_HIP_ESDF_H
#define TSDF_HIP_ESDF_H

#include "tsdf_hip.h"

#define TSDF_ESDF_API 1

#define TSDF_ESDF_OBSERVED 1u   /* W > 0 && W >= min_weight                      */
#define TSDF_ESDF_SITE     2u   /* observed && fabsf(S) <= site_band             */
#define TSDF_ESDF_CAPPED   4u   /* no site of the box within radius_vox (Euclid) */
#define TSDF_ESDF_MAX_RADIUS 128u

#ifdef __cplusplus
extern "C" {
#endif

/* The field of the box into host buffers: dist (n float32) and flags (n bytes; may be NULL). */
int tsdf_esdf_dense(tsdf_ctx* ctx, const int64_t lo[3], const int64_t hi[3], uint32_t radius_vox,
                    float site_band, float min_weight, float* dist, uint8_t* flags);

/* The same into device buffers on the context's device; d_flags may be NULL. */
int tsdf_esdf_dense_device(tsdf_ctx* ctx, const int64_t lo[3], const int64_t hi[3],
                           uint32_t radius_vox, float site_band, float min_weight, float* d_dist,
                           uint8_t* d_flags);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_ESDF_H */

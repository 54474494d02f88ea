/* tsdf_hip_merge.h — merging one map of libtsdf_hip.so into another under a rigid transform.
 *
 * tsdf_import_bricks merges bricks where they already sit.  These entry points move a field first:
 * the source map is resampled at the destination's voxel centres and fused by weight, on the GPU,
 * with no copy of either map over PCIe (Voxblox's mergeLayerAintoLayerB).  Uses: re-anchoring a
 * stretch of map after a pose-graph correction, fusing submaps at their optimised poses, fusing the
 * maps of two sessions or robots with a known relative pose.
 *
 * Like sampling, the raycast, prune and the distance field, this is a GPU-library feature outside
 * the tsdf_hip.h contract: TSDF_ABI_VERSION stays as it is and a caller detects the feature by the
 * presence of the symbols (dlsym / TSDF_MERGE_API at compile time).  No other source defines these
 * calls, so the rules written here ARE the contract.
 *
 * Semantics.  vs = (float)voxel_size.  All arithmetic is fp32 in the stated order unless marked
 * double; the library is built without FMA contraction, so a restatement in the same order
 * reproduces the bits.
 *
 *  1. Inverse pose.  pose is T_dst_src, 3x4 row-major (R | t): x_dst = R x_src + t.  The inverse
 *     is formed on the host in double: Ri = R^T (the entries copied) and
 *     ti[r] = -((Ri[r][0] t0 + Ri[r][1] t1) + Ri[r][2] t2); its twelve numbers are then rounded
 *     to fp32 (m, 3x4 row-major), as tsdf_align_terms_device rounds its pose.
 *  2. Centre and preimage.  Every destination voxel v with |v[a]| < 2^23 on every axis has the
 *     centre c[a] = ((float)v[a] + 0.5f) * vs and the preimage
 *     q[r] = ((m[r][0] c.x + m[r][1] c.y) + m[r][2] c.z) + m[r][3]  (the q of the align terms).
 *  3. Sample.  (s, w, valid) is exactly what tsdf_sample_device(src, q, mode, min_weight) returns
 *     (tsdf_hip_sample.h): TSDF_SAMPLE_NEAREST gives the voxel's (S, W); TSDF_SAMPLE_TRILINEAR the
 *     interpolant and the minimum corner weight, valid only in a fully observed cube.
 *  4. Fuse.  Where valid, (s, w) is merged into dst's voxel by the rule of tsdf_import_bricks, bit
 *     for bit: a copy where W == 0; else S <- (S W + s w) / (W + w), W <- W + w, capped at
 *     max_weight for TSDF_SEM_VOXBLOX.
 *  5. Allocation.  A destination brick is allocated if and only if it holds at least one voxel
 *     with a valid sample, or was there before: no empty brick is left behind.  Voxels outside the
 *     index domain are never written.
 *  6. Order independence.  The result is a pure function of the two fields and the arguments: it
 *     does not depend on thread order or on the order of bricks inside either pool.  The counts are
 *     integer sums; there are no floating-point atomics.
 *  7. Resampling is not copying.  In trilinear mode even the identity pose shrinks the observed
 *     set to the fully observed cubes (the sample point must lie in a cube whose eight corners are
 *     all observed), which on a single LiDAR scan is a small share of the voxels; the interpolant
 *     also smooths.  In nearest mode the identity pose is an exact copy, and so is any translation
 *     by whole voxels whose q does not round across a voxel face.
 *
 * Entry rules.  Both contexts are flushed and drained first.  TSDF_EINVAL, with a message in
 * tsdf_last_error(dst), for: a NULL context or src == dst; a bad mode; a negative or NaN
 * min_weight; a NULL pose, a non-finite pose entry or an inverse translation beyond the fp32
 * range; a rotation with max |R R^T - I| > 1e-5 or
 * det <= 0; contexts on different devices; (float)voxel_size or (float)sdf_trunc that differ in
 * their bits; different backgrounds (a TSDF_SEM_VOXBLOX context against a VDBFusion one;
 * TSDF_SEM_VDBFUSION and TSDF_SEM_VDBFUSION_F64 share field format and background and may be
 * mixed); either context with n_sectors > 1 or an open border reduce.  An empty source is TSDF_OK
 * with all-zero counts and nothing launched.
 *
 * Failure leaves both maps as they were, bit for bit.  The call learns new_bricks before it writes
 * anything to dst, and grows dst first, as tsdf_import_bricks does; if the bricks cannot fit
 * (max_bricks_hard reached, or device memory) it returns TSDF_ENOMEM with *out filled and dst
 * untouched.  src is never modified by either call.
 *
 * Scratch.  Device scratch on dst's device, freed on return: 48 bytes per candidate pair (a source
 * brick and a destination brick its image may reach) plus a fixed 32 KiB.  A source brick has
 * at most 27 candidate pairs while the coordinates of both maps and the translation stay
 * below 2^17 voxels (13 km at 10 cm), i.e. at most 1296 bytes per source brick against the 4096
 * bytes of the brick itself; beyond that the fp32 rounding of step 2 widens the search
 * (noetic-slam_amd/csrc/merge_plan.h).  No voxel tile is staged.
 */
#ifndef TSDF_HIP_MERGE_H
#define TSDF_HIP_MERGE_H

#include "tsdf_hip.h"
#include "tsdf_hip_sample.h"

#define TSDF_MERGE_API 1

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsdf_merge_stats {
    uint64_t src_bricks;       /* bricks the source holds */
    uint64_t candidate_bricks; /* destination bricks examined (implementation-defined, >= touched) */
    uint64_t touched_bricks;   /* destination bricks with at least one valid sample */
    uint64_t new_bricks;       /* of those, bricks dst did not hold before */
    uint64_t merged_voxels;    /* destination voxels that took a valid sample */
    uint64_t overlap_voxels;   /* of those, voxels dst had already observed (W > 0) */
} tsdf_merge_stats;

/* What the merge would do; neither map is changed.  out must not be NULL. */
int tsdf_merge_count(tsdf_ctx* dst, tsdf_ctx* src, const double pose[12], int32_t mode,
                     float min_weight, tsdf_merge_stats* out);

/* Do it; out may be NULL. */
int tsdf_merge_transformed(tsdf_ctx* dst, tsdf_ctx* src, const double pose[12], int32_t mode,
                           float min_weight, tsdf_merge_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_MERGE_H */

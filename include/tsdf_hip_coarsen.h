/* tsdf_hip_coarsen.h — coarsening a map of libtsdf_hip.so 2:1 into a map of twice the voxel size.
 *
 * Every other entry point works at one voxel size; tsdf_merge_transformed refuses contexts whose
 * voxel sizes differ.  These entry points take a source map at voxel size vs and fuse its 2:1
 * reduction into a destination map at 2 vs, on the GPU, with no copy of either map over PCIe.
 * Uses: a coarse global map beside a bounded live one (a sliding window coarsens what it evicts),
 * levels of detail for meshes, distance fields and column maps over large boxes, and submaps that
 * travel at less than sensor resolution.
 *
 * Like sampling, the raycast, prune, the distance field and the merge, this is a GPU-library
 * feature outside the tsdf_hip.h contract: TSDF_ABI_VERSION stays as it is and a caller detects
 * the feature by the presence of the symbols (dlsym / TSDF_COARSEN_API at compile time).  No other
 * source defines these calls, so the rules written here ARE the contract.
 *
 * Geometry.  A voxel v spans [v vs, (v + 1) vs) and has its centre at (v + 0.5) vs.  The coarse
 * voxel V at 2 vs is therefore exactly the union of the eight fine voxels 2 V + (a, b, c),
 * a, b, c in {0, 1}, and its centre is their centroid.  A brick has an even side (8), so all eight
 * children of a coarse voxel lie in ONE source brick, and the eight source bricks 2 D + (a, b, c)
 * map onto one destination brick D.
 *
 * Semantics.  All arithmetic is fp32 in the stated order; the library is built without FMA
 * contraction, so a restatement in the same order reproduces the bits.
 *
 *  1. Selection.  With lo == hi == NULL every source brick is selected.  Otherwise a source brick
 *     B is selected when lo[a] <= B[a] < hi[a] holds on every axis (TSDF_COARSEN_INSIDE), or when
 *     it does not (TSDF_COARSEN_OUTSIDE): the predicate of tsdf_count_outside
 *     (tsdf_hip_prune.h).  A box with lo[a] >= hi[a] on some axis holds no brick.
 *  2. Parent.  The destination brick of B is D[a] = B[a] >> 1 (arithmetic shift: floor).  The
 *     destination voxel V has the children 2 V + (a, b, c).  A child in a brick the source does
 *     not hold, or in a brick that is not selected, is unobserved.
 *  3. Valid child.  A child c is valid when W_c > 0 && W_c >= min_weight: the predicate of the
 *     nearest sample and of the mesh.
 *  4. Valid coarse voxel.  n = the number of valid children; V is valid iff n >= min_children.
 *     min_children is 1..8: 1 keeps everything seen, 8 keeps fully observed octets only.
 *  5. Value.  The children are visited in the order k = a + 2 b + 4 c, k = 0..7, the invalid ones
 *     skipped: sw = 0, ssw = 0; per valid child ssw = ssw + S_c * W_c and sw = sw + W_c; then
 *     s = ssw / sw and w = sw / (float)n.  The weight-weighted mean distance with the mean weight
 *     of what was seen: the coarse map's weights stay comparable with those of scans integrated
 *     into it directly.
 *  6. Fuse.  (s, w) is merged into dst's voxel by the rule of tsdf_import_bricks, bit for bit, as
 *     tsdf_merge_transformed does it: a copy where W == 0; else S <- (S W + s w) / (W + w),
 *     W <- W + w, capped at max_weight for TSDF_SEM_VOXBLOX.
 *  7. Allocation.  A destination brick is allocated if and only if it holds at least one valid
 *     coarse voxel, or was there before: no empty brick is left behind.
 *  8. Determinism.  The result is a pure function of the two fields and the arguments: it does
 *     not depend on thread order or on the order of bricks inside either pool.  The counts are
 *     integer sums; there are no floating-point atomics.
 *  9. Partition.  A coarse voxel reads one source brick only.  Coarsening two disjoint selections
 *     one after the other therefore gives the same dst as coarsening their union in one call,
 *     bit for bit, the set of bricks included, and into any starting dst -- as long as no
 *     destination voxel takes a value in both calls, which disjoint selections guarantee.  A
 *     sliding window relies on this: coarsening what leaves the window, eviction by eviction,
 *     adds up to the coarsening of everything that has left.
 *
 * Entry rules.  Both contexts are flushed and drained first.  TSDF_EINVAL, with a message in
 * tsdf_last_error(dst), for: a NULL context or src == dst; out == NULL for tsdf_coarsen_count;
 * side not TSDF_COARSEN_INSIDE / _OUTSIDE; exactly one of lo / hi NULL; min_children outside
 * 1..8; a negative or NaN min_weight; contexts on different devices; (float)dst.voxel_size not
 * equal in its bits to 2.0f * (float)src.voxel_size; (float)sdf_trunc that differ in their bits;
 * different backgrounds (a TSDF_SEM_VOXBLOX context against a VDBFusion one; TSDF_SEM_VDBFUSION
 * and TSDF_SEM_VDBFUSION_F64 share field format and background and may be mixed); either context
 * with n_sectors > 1 or an open border reduce.  An empty source or an empty selection is TSDF_OK
 * with all-zero counts (src_bricks = 0), and no kernel beyond the selection runs.
 *
 * Failure leaves both maps as they were, bit for bit.  The call learns new_bricks before it writes
 * anything to dst, and grows dst first, as tsdf_merge_transformed does; if the bricks cannot fit
 * (max_bricks_hard reached, or device memory) it returns TSDF_ENOMEM with *out filled and dst
 * untouched.  src is never modified by either call.
 *
 * Scratch.  Device scratch on dst's device, freed on return: at most 48 bytes per source brick
 * plus a fixed 32 KiB (noetic-slam_amd/csrc/coarsen_plan.h).  A source brick has exactly one
 * parent, so the sizes follow from the source's brick count and no counting pass runs.  No voxel
 * tile is staged.
 */
#ifndef TSDF_HIP_COARSEN_H
#define TSDF_HIP_COARSEN_H

#include "tsdf_hip.h"

#define TSDF_COARSEN_API 1

#define TSDF_COARSEN_INSIDE 0
#define TSDF_COARSEN_OUTSIDE 1

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsdf_coarsen_stats {
    uint64_t src_bricks;     /* source bricks selected (all of them without a box) */
    uint64_t parent_bricks;  /* distinct destination bricks floor(B / 2) of those: exact */
    uint64_t touched_bricks; /* of those, bricks with at least one valid coarse voxel */
    uint64_t new_bricks;     /* of those, bricks dst did not hold before */
    uint64_t coarse_voxels;  /* destination voxels that took a value */
    uint64_t overlap_voxels; /* of those, voxels dst had already observed (W > 0) */
    uint64_t child_voxels;   /* valid children of the valid coarse voxels (the sum of n) */
} tsdf_coarsen_stats;

/* What the call would do; neither map is changed.  out must not be NULL.
 * lo / hi: both NULL (the whole source) or a box of source brick coordinates (rule 1). */
int tsdf_coarsen_count(tsdf_ctx* dst, tsdf_ctx* src, const int32_t lo[3], const int32_t hi[3],
                       int32_t side, uint32_t min_children, float min_weight,
                       tsdf_coarsen_stats* out);

/* Do it; out may be NULL. */
int tsdf_coarsen_into(tsdf_ctx* dst, tsdf_ctx* src, const int32_t lo[3], const int32_t hi[3],
                      int32_t side, uint32_t min_children, float min_weight,
                      tsdf_coarsen_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_COARSEN_H */

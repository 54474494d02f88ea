/* tsdf_hip_frontier.h — the frontier voxels of libtsdf_hip.so: the observed free voxels that border
 * the unknown, of a voxel box or of the whole map, as a short deterministic list.
 *
 * This is what an exploring robot asks first: where does known free space end?  The list is the
 * input of a frontier-based or next-best-view planner, and its counts are the cheapest coverage
 * measure of a mapping session (n_free: the explored free volume in voxels).  The kernels visit
 * the bricks the map holds only, each with a one-voxel halo: a free voxel always lies in a held
 * brick and a brick the map does not hold is unknown as a whole.  16 bytes per frontier voxel come
 * back instead of tsdf_query_dense's 8 bytes per voxel of the box.
 *
 * Frontiers are meaningful on maps integrated with space carving: without it the observed band
 * around the surfaces is all the map holds, and the rule returns the rim of that band.
 *
 * Like sampling, the raycast, the column maps and the indexed mesh, this is a GPU-library feature
 * outside the tsdf_hip.h contract: TSDF_ABI_VERSION stays as it is and a caller detects the
 * feature by the presence of the symbols (dlsym / TSDF_FRONTIER_API at compile time).  No other
 * source defines these calls, so the rules written here ARE the contract.
 *
 * Semantics.  Comparisons are fp32, in the order written.
 *
 *  1. Voxel classes.  Every voxel reads (S, W) exactly as tsdf_query_dense does: a voxel of a
 *     brick the map does not hold, and a voxel outside |i| < 2^23, reads (background, 0).
 *       obs     = W > 0 && W >= min_weight
 *       free    = obs && S >= free_band
 *       unknown = !obs
 *  2. Neighbourhood.  connectivity is 6, 18 or 26: the 6 face offsets, plus the 12 edge offsets,
 *     plus the 8 corner offsets.
 *  3. Frontier rule.  Voxel v is a frontier voxel when it lies in the box, is free, and
 *     n_unknown(v), the number of unknown voxels among its neighbourhood, is at least min_unknown.
 *     The box restricts v only: neighbours are read outside it, as the mesh's normals are.
 *     lo / hi are voxel bounds [lo, hi); both NULL is the whole map, and the box rules are the
 *     indexed mesh's (tsdf_hip_mesh.h).
 *  4. Outputs per frontier voxel.  coords: int32 x 3, the voxel index.  n_unknown: uint8.  dir:
 *     int8 x 3, the integer sum of the offsets to its unknown neighbours: the direction in which
 *     the unknown lies (no floating point is involved; (0, 0, 0) where they cancel).  n_unknown
 *     and dir may be NULL.
 *  5. Order.  Bricks in (z, y, x) order (the order of the keys as integers, as export and the mesh
 *     use); within a brick the in-brick voxel order l = z*64 + y*8 + x.
 *  6. Determinism.  The result is a pure function of the field and the arguments: it does not
 *     depend on thread order or on the order of bricks inside the pool.  Ranks come from integer
 *     prefix sums; no atomic decides an output position.
 *  7. Counts (tsdf_frontier_counts).  n_bricks: held bricks that intersect the box.
 *     n_frontier_bricks: those with at least one frontier voxel.  n_voxels: frontier voxels.
 *     n_free: free voxels in the box.
 *
 * Capacity protocol (the indexed mesh's).  tsdf_frontier_count only counts.  tsdf_frontier_voxels
 * and tsdf_frontier_voxels_device always fill *out; if n_voxels > cap they return TSDF_EOVERFLOW
 * and write nothing to the buffers.  The device variant's buffers are device memory of the
 * context's GPU; it is complete on return and allocates no output staging.
 *
 * Entry rules.  The context is flushed and drained first.  The map is never modified.  An empty
 * map or an empty box (hi == lo on an axis) returns TSDF_OK with zero counts and launches nothing.
 * TSDF_EINVAL, with a message in tsdf_last_error prefixed "frontier: ", in this order, for:
 *    1. a NULL ctx (no message); a NULL out;
 *    2. exactly one of lo / hi NULL;
 *    3. a free_band that is not finite;
 *    4. a negative or NaN min_weight;
 *    5. a connectivity that is not 6, 18 or 26;
 *    6. a min_unknown outside 1..connectivity;
 *    7. hi < lo on an axis;
 *    8. an extent of 2^31 voxels or more;
 *    9. a NULL coords where n_voxels > 0 and cap suffices;
 *   10. a context with n_sectors > 1 or an open border reduce.
 * (Rule 9 needs the counts, so it is reported after rule 10's refusal, which needs no launch.)
 * TSDF_ENOMEM when scratch cannot be allocated; the buffers are left untouched.
 *
 * Scratch.  Device scratch on the context's device, freed on return: 24 bytes per listed brick
 * (its key, two counts and an offset), where the listed bricks are those that intersect the box
 * (every brick without a box).  tsdf_frontier_voxels stages its outputs on the device as well: 12
 * bytes per frontier voxel, plus 1 with n_unknown and 3 with dir.  The host holds the map's brick
 * keys, 8 bytes each.
 */
#ifndef TSDF_HIP_FRONTIER_H
#define TSDF_HIP_FRONTIER_H

#include "tsdf_hip.h"

#define TSDF_FRONTIER_API 1

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsdf_frontier_counts {
    uint64_t n_bricks;          /* held bricks that intersect the box */
    uint64_t n_frontier_bricks; /* bricks with at least one frontier voxel */
    uint64_t n_voxels;          /* frontier voxels */
    uint64_t n_free;            /* free voxels in the box */
} tsdf_frontier_counts;

/* lo / hi: the voxel-index box [lo, hi) of the frontier voxels; both NULL = the whole map.
 * out must not be NULL. */
int tsdf_frontier_count(tsdf_ctx* ctx, const int64_t lo[3], const int64_t hi[3], float free_band,
                        float min_weight, int32_t connectivity, int32_t min_unknown,
                        tsdf_frontier_counts* out);

/* Host outputs: coords 3 int32, n_unknown 1 uint8 and dir 3 int8 per frontier voxel, cap voxels
 * each; n_unknown and dir may be NULL. */
int tsdf_frontier_voxels(tsdf_ctx* ctx, const int64_t lo[3], const int64_t hi[3], float free_band,
                         float min_weight, int32_t connectivity, int32_t min_unknown,
                         int32_t* coords, uint8_t* n_unknown, int8_t* dir, uint64_t cap,
                         tsdf_frontier_counts* out);

/* The same; coords, n_unknown and dir are device memory of the context's GPU, complete when the
 * call returns. */
int tsdf_frontier_voxels_device(tsdf_ctx* ctx, const int64_t lo[3], const int64_t hi[3],
                                float free_band, float min_weight, int32_t connectivity,
                                int32_t min_unknown, int32_t* coords, uint8_t* n_unknown,
                                int8_t* dir, uint64_t cap, tsdf_frontier_counts* out);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_FRONTIER_H */

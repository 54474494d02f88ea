/* tsdf_hip_columns.h — the column maps of a map box of libtsdf_hip.so: per (x, y) cell of the box,
 * how high the ground is, how low the ceiling is, and whether the box's height slab is occupied,
 * free or unknown.
 *
 * This is the 2.5-D product a ground robot's navigation stack consumes first: an elevation map
 * plus what a nav_msgs/OccupancyGrid holds.  The reduction over z runs on the GPU, brick column by
 * brick column, and skips the bricks the map does not hold; 15 bytes per column come back instead
 * of tsdf_query_dense's 8 bytes per voxel.
 *
 * Like sampling, raycasting, pruning and the distance field, this is a GPU-library feature outside
 * the tsdf_hip.h contract: TSDF_ABI_VERSION stays as it is and a caller detects the feature by the
 * presence of the symbols (dlsym / TSDF_COLUMNS_API at compile time).
 *
 * The box is tsdf_query_dense's: voxels lo..hi-1 per axis, n = hi - lo.  There is one output cell
 * per column of the box, x fastest: index = (x - lo[0]) + nx (y - lo[1]).  Each output is an array
 * of nx ny cells, and any of the five may be NULL; for a box that is not empty at least one must be
 * given.
 *
 * Semantics.  These rules ARE the contract.  They are evaluated in fp32 in the order written, with
 * vs = (float)voxel_size, so a restatement reproduces the bits.
 *
 *   1. Every voxel of the column reads (S, W) exactly as tsdf_query_dense does: a voxel of a brick
 *      the map does not hold, and a voxel outside |i| < 2^23, reads (background, 0).
 *        obs  = W > 0 && W >= min_weight
 *        occ  = obs && S <= occ_band
 *        free = obs && !occ
 *   2. n_occ and n_free count the column's occ and free voxels over z in [lo[2], hi[2]).
 *   3. A pair (z-1, z) with both voxels in the box and both obs is
 *        an up crossing    when S_z > 0 && S_{z-1} <= 0: the surface faces +z, as a floor or the top
 *                          of an object does;
 *        a down crossing   when S_{z-1} > 0 && S_z <= 0: a ceiling or an underside.
 *      An unobserved voxel between two observed ones hides the crossing.
 *   4. elev comes from the up crossing of largest z:
 *        t = S_z / (S_z - S_{z-1}),  elev = (((float)z + 0.5f) - t) * vs
 *   5. ceil comes from the down crossing of smallest z:
 *        t = S_{z-1} / (S_{z-1} - S_z),  ceil = (((float)(z-1) + 0.5f) + t) * vs
 *   6. Where there is no crossing the value is the quiet NaN 0x7FC00000.  The two values are
 *      independent of each other, so a shelf gives ceil < elev.
 *   7. flags = OBSERVED | OCCUPIED | FREE | HAS_ELEV | HAS_CEIL (TSDF_COLUMN_*):
 *        OBSERVED = n_occ + n_free > 0
 *        OCCUPIED = n_occ >= min_occ
 *        FREE     = !OCCUPIED && n_free >= min_free
 *      A column that is neither OCCUPIED nor FREE is unknown.
 *
 * Entry rules.  Each call flushes the pending batch and waits for it, as the raycast does, and its
 * outputs are complete when it returns.  A context with an open border reduce is refused, and so is
 * a context created with n_sectors > 1.  The call never modifies the map.  An empty box (an extent
 * of 0) returns TSDF_OK, launches nothing and leaves the buffers untouched, whatever its other
 * extents.  TSDF_EINVAL, with a message prefixed "columns: ", in this order, for: a NULL lo or hi;
 * an occ_band that is not finite (a negative one is allowed); a negative or NaN min_weight; min_occ
 * or min_free outside 1..65535; hi < lo on an axis; an extent of 2^31 voxels or more; nz > 65535
 * (the counts are 16 bits); nx ny > 2^26; all five outputs NULL for a box that is not empty.
 *
 * Scratch.  tsdf_column_map holds the device copy of the outputs it was asked for while it runs (at
 * most 15 bytes per column).  If that cannot be allocated the call returns TSDF_ENOMEM and leaves
 * the buffers untouched.  tsdf_column_map_device allocates nothing.
 */
#ifndef TSDF_HIP_COLUMNS_H
#define TSDF_HIP_COLUMNS_H

#include "tsdf_hip.h"

#define TSDF_COLUMNS_API 1

#define TSDF_COLUMN_OBSERVED 1u   /* n_occ + n_free > 0                  */
#define TSDF_COLUMN_OCCUPIED 2u   /* n_occ >= min_occ                    */
#define TSDF_COLUMN_FREE     4u   /* !OCCUPIED && n_free >= min_free     */
#define TSDF_COLUMN_HAS_ELEV 8u   /* the column has an up crossing       */
#define TSDF_COLUMN_HAS_CEIL 16u  /* the column has a down crossing      */

#ifdef __cplusplus
extern "C" {
#endif

/* The column maps of the box into host buffers of nx ny cells each; any may be NULL. */
int tsdf_column_map(tsdf_ctx* ctx, const int64_t lo[3], const int64_t hi[3], float occ_band,
                    float min_weight, uint32_t min_occ, uint32_t min_free, float* elev, float* ceil,
                    uint16_t* n_occ, uint16_t* n_free, uint8_t* flags);

/* The same into device buffers on the context's device; any may be NULL. */
int tsdf_column_map_device(tsdf_ctx* ctx, const int64_t lo[3], const int64_t hi[3], float occ_band,
                           float min_weight, uint32_t min_occ, uint32_t min_free, float* d_elev,
                           float* d_ceil, uint16_t* d_n_occ, uint16_t* d_n_free, uint8_t* d_flags);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_COLUMNS_H */

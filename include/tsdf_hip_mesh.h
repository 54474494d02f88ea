/* tsdf_hip_mesh.h — the indexed triangle mesh of libtsdf_hip.so: shared vertices, per-vertex
 * normals, optionally of a voxel box only, into host or device memory.
 *
 * tsdf_extract_mesh* (tsdf_hip.h) writes a triangle soup: 9 floats per triangle, every vertex once
 * per triangle that uses it.  These entry points write the same triangles as (vertices, indices):
 * one vertex per grid edge the surface crosses, as VDBFusion's extract_triangle_mesh, Open3D, a
 * mesh message or a PLY file hold a mesh.  The soup entry points and their output do not change.
 *
 * Like sampling, the raycast, prune, the distance field and the merge, this is a GPU-library
 * feature outside the tsdf_hip.h contract: TSDF_ABI_VERSION stays as it is and a caller detects
 * the feature by the presence of the symbols (dlsym / TSDF_MESH_API at compile time).  No other
 * source defines these calls, so the rules written here ARE the contract.
 *
 * Semantics.  vs = (float)voxel_size.  All arithmetic is fp32 in the stated order; the library is
 * built without FMA contraction, so a restatement in the same order reproduces the bits.
 *
 *  1. Cubes and triangles.  The rule is exactly the soup's: the cube with min voxel m is meshed
 *     when all 8 voxels m + {0,1}^3 are observed (W > 0 and W >= min_weight); corner c is inside
 *     when S < 0; the case's triangles come from table `table` (TSDF_MC_*, tsdf_mc_table_of).  A
 *     box adds one condition: m lies in [lo, hi) on every axis.  Triangles come in the soup's
 *     order: the brick of m in (z, y, x) order, then the cube by its in-brick voxel
 *     l = z*64 + y*8 + x, then the table's order.  vertices[triangles], flattened, equals the soup
 *     of tsdf_extract_mesh_table bit for bit; with a box it equals the soup's triangles whose cube
 *     lies in the box, in the same order.
 *  2. Vertices.  One vertex per grid edge (min voxel a, axis k; the other end is b = a + e_k) that
 *     at least one emitted triangle references: there are no unreferenced vertices.  Two edges are
 *     two vertices even where their positions coincide (S_a == 0 gives t = 0 on up to three edges
 *     of a).  The position uses the soup's arithmetic in the soup's order:
 *     p[j] = ((float)a[j] + 0.5f) * vs, and on axis k p[k] = p[k] + t * vs with
 *     t = S_a / (S_a - S_b).  Vertices are ordered by the brick of a in (z, y, x) order, then the
 *     in-brick voxel l of a, then the axis.
 *  3. Normals.  "Observed" is rule 1's.  inv = 1.0f / vs, the reciprocal of tsdf_hip_sample.h.  For
 *     a voxel v and an axis j, with p = v + e_j and m = v - e_j:
 *       both observed:   g_j(v) = (S(p) - S(m)) * (0.5f * inv)
 *       only p observed: g_j(v) = (S(p) - S(v)) * inv
 *       only m observed: g_j(v) = (S(v) - S(m)) * inv
 *       neither:         g_j(v) = 0
 *     The vertex gradient is g = g(a) + t * (g(b) - g(a)) per component, normalised by the
 *     raycast's rule: n2 = (gx gx + gy gy) + gz gz; if n2 > 0 the normal is g / sqrtf(n2) per
 *     component, else (0, 0, 0).  It points towards increasing S: out of the surface, towards
 *     where the sensor was.  Gradients read voxels outside the box: the box restricts cubes only.
 *  4. Indices are uint32, three per triangle.  A mesh with 2^32 vertices or more is refused with
 *     TSDF_EINVAL before anything is written.
 *  5. Determinism.  The result is a pure function of the field and the arguments: it does not
 *     depend on thread order or on the order of bricks inside the pool.  The vertex set is built
 *     with integer ORs and ranked with integer prefix sums; there are no floating-point atomics.
 *
 * Capacity protocol.  tsdf_mesh_indexed_count only counts.  tsdf_mesh_indexed and
 * tsdf_mesh_indexed_device always fill *out; if n_vertices > cap_vertices or
 * n_triangles > cap_triangles they return TSDF_EOVERFLOW and write nothing to the outputs.
 * vertices and normals hold 3 floats per vertex, triangles 3 indices per triangle; normals may be
 * NULL (no normals are computed).  The map is never modified by any of the three calls.
 *
 * Entry rules.  The context is flushed and drained first.  TSDF_EINVAL, with a message in
 * tsdf_last_error, for: a NULL context (no message) or a NULL out; a bad table; a negative or NaN
 * min_weight; exactly one of lo / hi NULL; hi < lo on an axis; an extent of 2^31 voxels or more; a
 * NULL vertices or triangles where the mesh is not empty and the capacities suffice; a context
 * with n_sectors > 1 or an open border reduce.  The sharded mesh keeps tsdf_extract_mesh_local: an
 * indexed mesh across ranks (shared vertices on cubes that straddle two owners) is out of scope.
 * An empty map or an empty box (hi == lo on an axis) returns TSDF_OK with zero counts and launches
 * nothing.
 *
 * Scratch.  Device scratch on the context's device, freed on return: 224 bytes per listed brick
 * (its key, a 1536-bit vertex mask of 192 bytes, two counts and two offsets), where the listed
 * bricks are those that intersect the box grown by one voxel on the high side (the whole map
 * without a box), plus 4 bytes per brick of the map.  tsdf_mesh_indexed stages its outputs on the
 * device as well: 12 bytes per triangle and 12 (24 with normals) per vertex.  The host holds the
 * map's brick keys, 8 bytes each.
 */
#ifndef TSDF_HIP_MESH_H
#define TSDF_HIP_MESH_H

#include "tsdf_hip.h"

#define TSDF_MESH_API 1

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsdf_mesh_counts {
    uint64_t n_bricks;    /* bricks examined (those that intersect the box) */
    uint64_t n_vertices;
    uint64_t n_triangles;
} tsdf_mesh_counts;

/* lo / hi: the voxel-index box [lo, hi) of the cubes' MIN voxels; both NULL = the whole map.
 * out must not be NULL. */
int tsdf_mesh_indexed_count(tsdf_ctx* ctx, float min_weight, int32_t table, const int64_t lo[3],
                            const int64_t hi[3], tsdf_mesh_counts* out);

/* Host outputs. */
int tsdf_mesh_indexed(tsdf_ctx* ctx, float min_weight, int32_t table, const int64_t lo[3],
                      const int64_t hi[3], float* vertices, float* normals, uint32_t* triangles,
                      uint64_t cap_vertices, uint64_t cap_triangles, tsdf_mesh_counts* out);

/* The same; vertices, normals and triangles are device memory of the context's GPU, complete when
 * the call returns. */
int tsdf_mesh_indexed_device(tsdf_ctx* ctx, float min_weight, int32_t table, const int64_t lo[3],
                             const int64_t hi[3], float* vertices, float* normals,
                             uint32_t* triangles, uint64_t cap_vertices, uint64_t cap_triangles,
                             tsdf_mesh_counts* out);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_MESH_H */

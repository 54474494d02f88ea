/* tsdf_hip_sample.h — sparse map queries of libtsdf_hip.so: the read side of the TSDF map.
 *
 * tsdf_hip.h writes the map and reads it back wholesale (dense boxes, bricks, the mesh).  These
 * entry points answer a question about a cloud instead: the signed distance, its weight and its
 * gradient at arbitrary world points, and the Gauss-Newton normal equations of the point-to-TSDF
 * error of a cloud under a candidate pose (scan-to-map refinement, consistency checks before a
 * fuse, loop-closure verification, free-space tests).
 *
 * Why a header of its own: tsdf_hip.h is the contract every library of this project exports,
 * the CPU oracle included, and TSDF_ABI_VERSION numbers that contract.  Sampling is a GPU-library
 * feature the oracle does not restate, so it extends the library without changing the contract:
 * TSDF_ABI_VERSION stays as it is and a caller detects the feature by the presence of the symbols
 * (dlsym / TSDF_SAMPLE_API at compile time).
 *
 * Common rules.  Each call flushes the pending batch and waits for the field, as tsdf_query_dense
 * does, and its outputs are complete when it returns.  A context with an open border reduce is
 * refused, and so is a context created with n_sectors > 1: its field is one shard of the map, and
 * sampling across shard borders needs a halo exchange like the mesh's (tsdf_extract_mesh_halo),
 * which these entry points do not implement.  TSDF_EINVAL, with a message, for a bad mode, a NULL
 * required buffer, or a negative or NaN min_weight.  n == 0 returns TSDF_OK and launches nothing.
 *
 * Semantics (all fp32, evaluated in the stated order; the library is built without FMA
 * contraction, so a restatement in the same order reproduces the bits).  inv = 1.0f / (float)
 * voxel_size, bg = the background distance ((float)sdf_trunc, or 0 for TSDF_SEM_VOXBLOX),
 * lerp(a, b, t) = a + t * (b - a).
 *
 *   TSDF_SAMPLE_NEAREST    the voxel floorf(p * inv) per axis: its (sdf, weight), or (bg, 0) where
 *                          the voxel is unallocated or outside the index domain, as
 *                          tsdf_query_dense reads it.  grad = 0.  valid = W > 0 && W >= min_weight.
 *   TSDF_SAMPLE_TRILINEAR  u = p * inv - 0.5f (voxel centres at (i + 0.5) voxel_size, where the
 *                          mesh places them), b = floorf(u), f = u - b; the corners are the voxels
 *                          b + (dx, dy, dz).  Valid iff p is finite, every corner lies inside
 *                          |i| < 2^23 and every corner has W > 0 && W >= min_weight (the observed
 *                          cube rule of tsdf_extract_mesh).  Then sdf is the corners' sdf lerped
 *                          along x, then y, then z; weight the minimum corner weight; grad the
 *                          analytic derivative of that interpolant in metres per metre: per axis,
 *                          the four corner differences along it lerped over the other two axes in
 *                          x, y, z order, times inv.  Invalid: sdf = bg, weight = 0, grad = 0.
 */
#ifndef TSDF_HIP_SAMPLE_H
#define TSDF_HIP_SAMPLE_H

#include "tsdf_hip.h"

#define TSDF_SAMPLE_API 1

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_SAMPLE_NEAREST 0
#define TSDF_SAMPLE_TRILINEAR 1

/* Samples at n device points d_xyz (n x 3 float32) into device buffers: d_sdf, d_weight (n
 * float32), d_grad (3 n float32; may be NULL) and d_valid (n bytes, 0 / 1).  d_xyz must be
 * complete before the call (the library runs on its own stream). */
int tsdf_sample_device(tsdf_ctx* ctx, const float* d_xyz, uint64_t n, int32_t mode,
                       float min_weight, float* d_sdf, float* d_weight, float* d_grad,
                       uint8_t* d_valid);

/* The same for host points in PointCloud2-style records (the layout arguments of tsdf_integrate;
 * float64 coordinates are rounded to float32) into host buffers; grad may be NULL.  Any n: clouds
 * beyond the context's max_points are sampled in pieces. */
int tsdf_sample(tsdf_ctx* ctx, const void* pts, uint64_t n, uint32_t point_step,
                uint32_t xyz_offset, int32_t xyz_is_f64, int32_t mode, float min_weight,
                float* sdf, float* weight, float* grad, uint8_t* valid);

/* Gauss-Newton terms of the point-to-TSDF error of a cloud under a pose.  pose: 3x4 row-major
 * (rotation | translation), rounded to float32 as tsdf_os_cartesian_device rounds its pose;
 * q = ((r0 x + r1 y) + r2 z) + t per row; (S, g) the trilinear sample at q.  Over the valid
 * points, everything converted to double: residual r = S, Jacobian J = [g, q x g] (a left
 * perturbation (dt, dtheta) of the world pose), and
 *   out[0..35] = H = sum J^T J (row-major), out[36..41] = b = sum J^T r, out[42] = sum r^2,
 *   out[43] = the number of valid points.
 * out is a host buffer.  The sums have a fixed shape (a fixed tree per workgroup, the workgroups'
 * partials added in workgroup order, no floating-point atomics): the same inputs give the same 44
 * doubles bit for bit on every call.  One 6x6 solve H d = -b then refines the pose. */
#define TSDF_ALIGN_WORDS 44
int tsdf_align_terms_device(tsdf_ctx* ctx, const float* d_xyz, uint64_t n, const double pose[12],
                            float min_weight, double out[TSDF_ALIGN_WORDS]);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_SAMPLE_H */

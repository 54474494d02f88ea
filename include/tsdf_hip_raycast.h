/* tsdf_hip_raycast.h — raycasting the map of libtsdf_hip.so: what the sensor would see.
 *
 * tsdf_hip_sample.h answers what the field is at given points.  These entry points answer what
 * lies along given rays: the depth of the first surface, its normal and a hit flag per ray -- the
 * model scan of scan-to-model registration, a predicted range image to hold a pose or a
 * loop-closure candidate against a live scan, free-space and visibility tests, a depth / normal
 * image without extracting the mesh.
 *
 * Like sampling, raycasting is a GPU-library feature outside the tsdf_hip.h contract:
 * TSDF_ABI_VERSION stays as it is and a caller detects the feature by the presence of the symbols
 * (dlsym / TSDF_RAYCAST_API at compile time).
 *
 * Common rules (those of tsdf_hip_sample.h).  Each call flushes the pending batch and waits for
 * the field, and its outputs are complete when it returns.  A context with an open border reduce
 * is refused, and so is a context created with n_sectors > 1.  n == 0 returns TSDF_OK and
 * launches nothing.  TSDF_EINVAL, with a message, for a NULL required buffer; a bad mode; a
 * negative or NaN min_weight; a non-finite t_min, t_max or step; step <= 0, t_min < 0 or
 * t_max < t_min; and (t_max - t_min) / step >= 2^20, computed in double (the bound on any walk of
 * this library).
 *
 * Semantics (all fp32, evaluated in the stated order; the library is built without FMA
 * contraction and with correctly rounded division and square root, so a restatement in the same
 * order reproduces the bits).  mode and min_weight are those of tsdf_sample_device.
 *
 *   Ray      pose == NULL: origin o and direction d as given.  Otherwise the pose, 3x4 row-major
 *            (rotation | translation), is rounded to float32 as tsdf_align_terms_device rounds
 *            its pose, and per row o = ((r0 x + r1 y) + r2 z) + t of the given origin and
 *            d = (r0 x + r1 y) + r2 z of the given direction.  d is not normalised: t counts in
 *            units of |d|, so unit directions give metres.
 *   Lattice  t_k = t_min + (float)k * step (one product and one sum, not accumulated) for
 *            k = 0, 1, ... while t_k <= t_max and k < 2^20 (the argument rule keeps k below 2^20
 *            in exact arithmetic; the cap only ends a lattice that fp32 rounding would stall).
 *            p_k = o + t_k * d per axis.  (S_k, valid_k) is exactly what tsdf_sample_device
 *            returns at p_k for mode and min_weight.
 *   Hit      the smallest k >= 1 with valid_{k-1} && valid_k && S_{k-1} > 0 && S_k <= 0: a
 *            front-facing zero crossing between two observed samples.  Back-facing crossings and
 *            unobserved gaps are marched through.  Then hit = 1 and
 *              depth = t_{k-1} + (t_k - t_{k-1}) * (S_{k-1} / (S_{k-1} - S_k)).
 *            No such k: depth = 0, hit = 0, normal = (0, 0, 0).  Non-finite rays and zero
 *            directions have no rule of their own: a non-finite p_k is invalid by the sampling
 *            rules, and a zero direction samples one point over and over, which never crosses.
 *   Normal   (when requested; the same for both modes) the TSDF_SAMPLE_TRILINEAR sample at
 *            p* = o + depth * d per axis with the same min_weight.  If it is valid and
 *            n2 = (gx gx + gy gy) + gz gz > 0, normal = g / sqrtf(n2) per component (one square
 *            root, three divisions); otherwise (0, 0, 0).  It points against the ray on a
 *            front-facing hit: the direction in which the distance grows.
 */
#ifndef TSDF_HIP_RAYCAST_H
#define TSDF_HIP_RAYCAST_H

#include "tsdf_hip_sample.h"

#define TSDF_RAYCAST_API 1

#ifdef __cplusplus
extern "C" {
#endif

/* n rays in device buffers d_org and d_dir (n x 3 float32 each) into device buffers d_depth (n
 * float32), d_normal (3 n float32; may be NULL) and d_hit (n bytes, 0 / 1).  pose may be NULL.
 * The rays must be complete before the call (the library runs on its own stream). */
int tsdf_raycast_device(tsdf_ctx* ctx, const float* d_org, const float* d_dir, uint64_t n,
                        const double pose[12], float t_min, float t_max, float step, int32_t mode,
                        float min_weight, float* d_depth, float* d_normal, uint8_t* d_hit);

/* The same for host buffers; normal may be NULL.  Any n: beyond the context's max_points the rays
 * are cast in pieces. */
int tsdf_raycast(tsdf_ctx* ctx, const float* org, const float* dir, uint64_t n,
                 const double pose[12], float t_min, float t_max, float step, int32_t mode,
                 float min_weight, float* depth, float* normal, uint8_t* hit);

#ifdef __cplusplus
}
#endif
#endif /* TSDF_HIP_RAYCAST_H */

// tsdf_sample.hip — sparse map queries (include/tsdf_hip_sample.h): the field
// sampled at arbitrary world points, one lane per point.
//   k_sample<MODE>  nearest voxel, or the trilinear interpolant of the 8 surrounding voxel centres
//                   with its analytic gradient
//   k_align         the trilinear sample of a cloud under a candidate pose, reduced to the
//                   Gauss-Newton terms of the point-to-TSDF error (21 + 6 + 1 doubles and a count)
//                   per workgroup by a fixed tree; k_align_sum adds the workgroups' partials in
//                   workgroup order (no floating-point atomics: the same bits on every call)
//
// The lookup and the sampling arithmetic live in tsdf_sample_dev.h, shared with tsdf_raycast.hip.
#include "tsdf_sample_dev.h"

namespace tsdf {

namespace {

constexpr int SMP_THREADS = 256;
constexpr int SMP_WAVES = SMP_THREADS / 64;
constexpr int ALIGN_ACC = 28;  // H's upper triangle (21, row-major), b (6), sum r^2

// One lane per point; the workgroup's loop bounds are uniform, so whole waves stay in the loop (the
// shared-lookup variant is a wave-wide operation) and lanes past n merely sample nothing.
template <int MODE>
__global__ __launch_bounds__(SMP_THREADS) void k_sample(Table T, Pool Pl, float inv, float bg,
                                                        const float* __restrict__ xyz, uint64_t n,
                                                        float min_w, float* __restrict__ out_s,
                                                        float* __restrict__ out_w,
                                                        float* __restrict__ out_g,
                                                        uint8_t* __restrict__ out_v) {
    const uint64_t stride = (uint64_t)gridDim.x * SMP_THREADS;
    for (uint64_t base = (uint64_t)blockIdx.x * SMP_THREADS; base < n; base += stride) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < n;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        if (live) {
            px = xyz[3 * i];
            py = xyz[3 * i + 1];
            pz = xyz[3 * i + 2];
        }
        const Sample r = MODE == 0 ? sample_nearest(T, Pl, inv, bg, min_w, live, px, py, pz)
                                   : sample_trilinear(T, Pl, inv, bg, min_w, live, px, py, pz);
        if (live) {
            out_s[i] = r.s;
            out_w[i] = r.w;
            out_v[i] = r.valid ? 1 : 0;
            if (out_g) {
                out_g[3 * i] = r.gx;
                out_g[3 * i + 1] = r.gy;
                out_g[3 * i + 2] = r.gz;
            }
        }
    }
}

// part[blockIdx.x * ALIGN_PART + k]: the workgroup's sums (k < ALIGN_ACC) and its valid count (as a
// double, k = ALIGN_ACC).  Shape of the sum: per lane over its points in index order, a xor
// butterfly over the wave's 64 lanes, then the workgroup's waves in order.
__global__ __launch_bounds__(SMP_THREADS) void k_align(Table T, Pool Pl, float inv, float bg,
                                                       const float* __restrict__ xyz, uint64_t n,
                                                       OsPose P, float min_w,
                                                       double* __restrict__ part) {
    double acc[ALIGN_ACC];
#pragma unroll
    for (int k = 0; k < ALIGN_ACC; k++) acc[k] = 0.0;
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * SMP_THREADS;
    for (uint64_t base = (uint64_t)blockIdx.x * SMP_THREADS; base < n; base += stride) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < n;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (live) {
            x = xyz[3 * i];
            y = xyz[3 * i + 1];
            z = xyz[3 * i + 2];
        }
        const float qx = ((P.m[0] * x + P.m[1] * y) + P.m[2] * z) + P.m[3];
        const float qy = ((P.m[4] * x + P.m[5] * y) + P.m[6] * z) + P.m[7];
        const float qz = ((P.m[8] * x + P.m[9] * y) + P.m[10] * z) + P.m[11];
        const Sample r = sample_trilinear(T, Pl, inv, bg, min_w, live, qx, qy, qz);
        if (r.valid) {
            const double gx = r.gx, gy = r.gy, gz = r.gz, res = r.s;
            const double dx = qx, dy = qy, dz = qz;
            const double J[6] = {gx, gy, gz, dy * gz - dz * gy, dz * gx - dx * gz, dx * gy - dy * gx};
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = a; b < 6; b++) acc[k++] += J[a] * J[b];
#pragma unroll
            for (int a = 0; a < 6; a++) acc[21 + a] += J[a] * res;
            acc[27] += res * res;
            cnt++;
        }
    }
#pragma unroll
    for (int k = 0; k < ALIGN_ACC; k++)
        for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d, 64);
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    __shared__ double sh[SMP_WAVES][ALIGN_ACC + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < ALIGN_ACC; k++) sh[wave][k] = acc[k];
        sh[wave][ALIGN_ACC] = (double)cnt;
    }
    __syncthreads();
    if (threadIdx.x <= ALIGN_ACC) {
        double v = sh[0][threadIdx.x];
        for (int wv = 1; wv < SMP_WAVES; wv++) v += sh[wv][threadIdx.x];
        part[(size_t)blockIdx.x * ALIGN_PART + threadIdx.x] = v;
    }
}

// out[k] = the workgroups' partials added in workgroup order
__global__ __launch_bounds__(64) void k_align_sum(const double* __restrict__ part, uint32_t n_wg,
                                                  double* __restrict__ out) {
    if (threadIdx.x > ALIGN_ACC) return;
    double v = 0.0;
#pragma unroll 8
    for (uint32_t g = 0; g < n_wg; g++) v += part[(size_t)g * ALIGN_PART + threadIdx.x];
    out[threadIdx.x] = v;
}

// workgroups of a launch over n points: capped like k_query_dense's grid, the kernels stride
uint32_t sample_grid(uint64_t n, uint32_t cap) {
    const uint64_t g = (n + SMP_THREADS - 1) / SMP_THREADS;
    return (uint32_t)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

hipError_t launch_sample(const Table& T, const Pool& Pl, const RayConst& R, const float* d_xyz,
                         uint64_t n, int mode, float min_w, float* d_sdf, float* d_w, float* d_grad,
                         uint8_t* d_valid, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint32_t grid = sample_grid(n, 8192);
    if (mode == 0)
        k_sample<0><<<grid, SMP_THREADS, 0, st>>>(T, Pl, R.inv_vs, R.bg, d_xyz, n, min_w, d_sdf, d_w,
                                                  d_grad, d_valid);
    else
        k_sample<1><<<grid, SMP_THREADS, 0, st>>>(T, Pl, R.inv_vs, R.bg, d_xyz, n, min_w, d_sdf, d_w,
                                                  d_grad, d_valid);
    return hipGetLastError();
}

hipError_t launch_align(const Table& T, const Pool& Pl, const RayConst& R, const float* d_xyz,
                        uint64_t n, const OsPose& P, float min_w, double* d_part, hipStream_t st) {
    const uint32_t grid = sample_grid(n, ALIGN_MAX_WG);
    k_align<<<grid, SMP_THREADS, 0, st>>>(T, Pl, R.inv_vs, R.bg, d_xyz, n, P, min_w, d_part);
    k_align_sum<<<1, 64, 0, st>>>(d_part, grid, d_part + (size_t)ALIGN_MAX_WG * ALIGN_PART);
    return hipGetLastError();
}

}  // namespace tsdf

// orbx_lm.h — what the two single-vertex Levenberg kernels share (k_pose_opt of orbx_pose.hip, k_sim3_opt of orbx_sim3opt.hip): the
// fixed-order workgroup sum that hands every thread of a 256-thread workgroup the same bits, g2o's Huber kernel and Eigen's
// Quaternion(Matrix3).  Device code only; every function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>

// robust_kernel_impl.cpp:78-91 (rho[2] is never used: base_edge.h:96-102)
static __device__ __forceinline__ void huber(double e, double delta, double &rho0, double &rho1)
{
    const double dsqr = delta * delta;
    if (e <= dsqr) { rho0 = e; rho1 = 1.0; return; }
    const double sqrte = sqrt(e);
    rho0 = 2.0 * sqrte * delta - dsqr;
    rho1 = delta / sqrte;
}

static __device__ __forceinline__ double wave_sum(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// a[k] summed over the workgroup's 256 threads, for every thread: the xor butterfly across the wave (both partners add the same two
// numbers, so all 64 lanes hold the same bits), then ((w0 + w1) + (w2 + w3)) over the four waves through red[4 * K]
template <int K>
static __device__ __forceinline__ void block_sum(double (&a)[K], double *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) a[k] = wave_sum(a[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[wave * K + k] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) a[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
    __syncthreads();
}

// Eigen's Quaternion(Matrix3): m row-major
static __device__ __forceinline__ void quat_from_matrix(const double m[9], double &qx, double &qy, double &qz, double &qw)
{
    double t = (m[0] + m[4]) + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        qw = 0.5 * t;
        t = 0.5 / t;
        qx = (m[7] - m[5]) * t; qy = (m[2] - m[6]) * t; qz = (m[3] - m[1]) * t;
        return;
    }
    // i = the largest diagonal entry, j = i + 1, k = i + 2 (mod 3); the three cases written out (no indexed register arrays)
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i ? m[4] : m[0])) i = 2;
    if (i == 0) {
        t = sqrt(((m[0] - m[4]) - m[8]) + 1.0);
        qx = 0.5 * t; t = 0.5 / t;
        qw = (m[7] - m[5]) * t; qy = (m[3] + m[1]) * t; qz = (m[6] + m[2]) * t;
    } else if (i == 1) {
        t = sqrt(((m[4] - m[8]) - m[0]) + 1.0);
        qy = 0.5 * t; t = 0.5 / t;
        qw = (m[2] - m[6]) * t; qz = (m[7] + m[5]) * t; qx = (m[1] + m[3]) * t;
    } else {
        t = sqrt(((m[8] - m[0]) - m[4]) + 1.0);
        qz = 0.5 * t; t = 0.5 / t;
        qw = (m[3] - m[1]) * t; qx = (m[2] + m[6]) * t; qy = (m[5] + m[7]) * t;
    }
}

// orbx_lm.h — what the Levenberg kernels share (k_pose_opt of orbx_pose.hip, k_sim3_opt of orbx_sim3opt.hip, the k_lba_* of orbx_lba.hip): the
// fixed-order workgroup sum that hands every thread of a 256-thread workgroup the same bits, g2o's Huber kernel and Eigen's
// Quaternion(Matrix3), and g2o's SE3Quat with its exponential update (k_pose_opt, k_lba_*).  Device code only; every function is inlined into its kernel.
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

// g2o's SE3Quat: a unit quaternion and a translation
struct Pose { double qx, qy, qz, qw, tx, ty, tz; };

// SE3Quat::normalizeRotation
static __device__ __forceinline__ void quat_normalize(double &qx, double &qy, double &qz, double &qw)
{
    if (qw < 0.0) { qx = -qx; qy = -qy; qz = -qz; qw = -qw; }
    const double n = sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw);
    qx /= n; qy /= n; qz /= n; qw /= n;
}

static __device__ __forceinline__ void quat_to_matrix(const Pose &P, double R[9])
{
    const double tx = 2.0 * P.qx, ty = 2.0 * P.qy, tz = 2.0 * P.qz;
    const double twx = tx * P.qw, twy = ty * P.qw, twz = tz * P.qw, txx = tx * P.qx, txy = ty * P.qx, txz = tz * P.qx;
    const double tyy = ty * P.qy, tyz = tz * P.qy, tzz = tz * P.qz;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// VertexSE3Expmap::oplusImpl: SE3Quat::exp(x) * P (se3quat.h:223-257, :104-110); x[0..2] rotation, x[3..5] translation
static __device__ __forceinline__ Pose pose_update(const Pose &P, const double x[6])
{
    const double o0 = x[0], o1 = x[1], o2 = x[2];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double O[9] = { 0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0 };
    double O2[9], R[9], V[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
    if (theta < 0.00001) {
#pragma unroll
        for (int k = 0; k < 9; k++) { R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + O[k]) + O2[k]; V[k] = R[k]; }
    } else {
        const double s = sin(theta), c = cos(theta);
        const double a = s / theta, b = (1.0 - c) / (theta * theta), cc = (theta - s) / ((theta * theta) * theta);
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const double id = k % 4 == 0 ? 1.0 : 0.0;
            R[k] = (id + a * O[k]) + b * O2[k];
            V[k] = (id + b * O[k]) + cc * O2[k];
        }
    }
    Pose E;
    quat_from_matrix(R, E.qx, E.qy, E.qz, E.qw);
    quat_normalize(E.qx, E.qy, E.qz, E.qw);
    E.tx = (V[0] * x[3] + V[1] * x[4]) + V[2] * x[5];
    E.ty = (V[3] * x[3] + V[4] * x[4]) + V[5] * x[5];
    E.tz = (V[6] * x[3] + V[7] * x[4]) + V[8] * x[5];
    // E * P: t = E.t + E.q * P.t ; q = E.q * P.q, normalised
    Pose N;
    {
        const double ux = 2.0 * (E.qy * P.tz - E.qz * P.ty), uy = 2.0 * (E.qz * P.tx - E.qx * P.tz), uz = 2.0 * (E.qx * P.ty - E.qy * P.tx);
        N.tx = E.tx + ((P.tx + E.qw * ux) + (E.qy * uz - E.qz * uy));
        N.ty = E.ty + ((P.ty + E.qw * uy) + (E.qz * ux - E.qx * uz));
        N.tz = E.tz + ((P.tz + E.qw * uz) + (E.qx * uy - E.qy * ux));
    }
    N.qw = ((E.qw * P.qw - E.qx * P.qx) - E.qy * P.qy) - E.qz * P.qz;
    N.qx = ((E.qw * P.qx + E.qx * P.qw) + E.qy * P.qz) - E.qz * P.qy;
    N.qy = ((E.qw * P.qy + E.qy * P.qw) + E.qz * P.qx) - E.qx * P.qz;
    N.qz = ((E.qw * P.qz + E.qz * P.qw) + E.qx * P.qy) - E.qy * P.qx;
    quat_normalize(N.qx, N.qy, N.qz, N.qw);
    return N;
}

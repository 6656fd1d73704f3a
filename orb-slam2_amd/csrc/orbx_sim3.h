// orbx_sim3.h — g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) restated once for the two files that optimise over it: k_sim3_opt of
// orbx_sim3opt.hip (OptimizeSim3) and the k_eg_* of orbx_essential.hip (OptimizeEssentialGraph).  The value type keeps an UNNORMALISED
// quaternion, a translation and a scale, as g2o does.  map, inverse, operator* and the exponential are the functions k_sim3_opt was
// measured with, moved here unchanged; sim3_log is the logarithm only the essential graph's EdgeSim3 needs.
// Device code; every function is inlined into its kernel.
#pragma once
#include "orbx_lm.h"

namespace {

struct Sim3 { double qx, qy, qz, qw, tx, ty, tz, s; };

// sim3.h:144-146: s * (r * xyz) + t (r is NOT a unit quaternion here)
__device__ __forceinline__ void sim3_map(const Sim3 &S, double X, double Y, double Z, double &x, double &y, double &z)
{
    quat_rot(S.qx, S.qy, S.qz, S.qw, X, Y, Z, x, y, z);
    x = S.s * x + S.tx; y = S.s * y + S.ty; z = S.s * z + S.tz;
}

// sim3.h:233-236: Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
__device__ __forceinline__ Sim3 sim3_inverse(const Sim3 &S)
{
    Sim3 I;
    I.qx = -S.qx; I.qy = -S.qy; I.qz = -S.qz; I.qw = S.qw;
    const double k = -1.0 / S.s;
    quat_rot(I.qx, I.qy, I.qz, I.qw, k * S.tx, k * S.ty, k * S.tz, I.tx, I.ty, I.tz);
    I.s = 1.0 / S.s;
    return I;
}

// sim3.h:266-272: r = a.r * b.r (no normalisation, unlike SE3Quat), t = a.s * (a.r * b.t) + a.t, s = a.s * b.s
__device__ __forceinline__ Sim3 sim3_mul(const Sim3 &a, const Sim3 &b)
{
    Sim3 N;
    quat_mul(a.qx, a.qy, a.qz, a.qw, b.qx, b.qy, b.qz, b.qw, N.qx, N.qy, N.qz, N.qw);
    double x, y, z;
    quat_rot(a.qx, a.qy, a.qz, a.qw, b.tx, b.ty, b.tz, x, y, z);
    N.tx = a.s * x + a.tx; N.ty = a.s * y + a.ty; N.tz = a.s * z + a.tz;
    N.s = a.s * b.s;
    return N;
}

// sim3.h:70-142: Sim3(Vector7d), u[0..2] rotation, u[3..5] translation, u[6] log scale; r = Quaterniond(R) is not normalised
__device__ __forceinline__ Sim3 sim3_exp(const double u[7])
{
    const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double O[9] = { 0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0 };
    double O2[9], R[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
    Sim3 E;
    E.s = exp(sigma);
    const double eps = 0.00001;
    const bool small_theta = theta < eps;
    double A, B, C, ra = 1.0, rb = 1.0;   // R = (I + ra Omega) + rb Omega2; ra = rb = 1 written without the products when theta < eps
    if (!small_theta) {
        ra = sin(theta) / theta;
        rb = (1.0 - cos(theta)) / (theta * theta);
    }
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small_theta) {
            A = 1.0 / 2.0; B = 1.0 / 6.0;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (E.s - 1.0) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * E.s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * E.s) / (sigma2 * sigma);
        } else {
            const double a = E.s * sin(theta), b = E.s * cos(theta);
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double id = k % 4 == 0 ? 1.0 : 0.0;
        R[k] = small_theta ? (id + O[k]) + O2[k] : (id + ra * O[k]) + rb * O2[k];
    }
    quat_from_matrix(R, E.qx, E.qy, E.qz, E.qw);
    double W[9];   // W = A Omega + B Omega2 + C I
#pragma unroll
    for (int k = 0; k < 9; k++) W[k] = (A * O[k] + B * O2[k]) + (k % 4 == 0 ? C : 0.0);
    E.tx = (W[0] * u[3] + W[1] * u[4]) + W[2] * u[5];
    E.ty = (W[3] * u[3] + W[4] * u[4]) + W[5] * u[5];
    E.tz = (W[6] * u[3] + W[7] * u[4]) + W[8] * u[5];
    return E;
}

__device__ __forceinline__ Sim3 xf_load(const double *xf)
{
    Sim3 T;
    T.qx = xf[0]; T.qy = xf[1]; T.qz = xf[2]; T.qw = xf[3]; T.tx = xf[4]; T.ty = xf[5]; T.tz = xf[6]; T.s = xf[7];
    return T;
}

__device__ __forceinline__ void xf_store(double *xf, const Sim3 &T)
{
    xf[0] = T.qx; xf[1] = T.qy; xf[2] = T.qz; xf[3] = T.qw; xf[4] = T.tx; xf[5] = T.ty; xf[6] = T.tz; xf[7] = T.s;
}

// Eigen's PartialPivLU of a 3 x 3 matrix and its solve (W.lu().solve(t), sim3.h:217), W row major.  Column k = 0, 1: the pivot is the
// FIRST row i >= k with the largest |W[i][k]| (maxCoeff's visitor replaces on >), rows k and pivot are exchanged in W and t, the entries
// below the pivot are divided by it, then the trailing block has (multiplier * pivot row) subtracted entry by entry.  Solve: the unit lower
// triangle forward, y1 = t1 - l10 y0, y2 = t2 - (l20 y0 + l21 y1); the upper triangle backward, x2 = y2 / u22, x1 = (y1 - u12 x2) / u11,
// x0 = (y0 - (u01 x1 + u02 x2)) / u00.  The exchanges are selects on named scalars: no indexed register array.
__device__ __forceinline__ void lu3_solve(const double W[9], double t0, double t1, double t2, double &x0, double &x1, double &x2)
{
    double a00 = W[0], a01 = W[1], a02 = W[2], a10 = W[3], a11 = W[4], a12 = W[5], a20 = W[6], a21 = W[7], a22 = W[8];
#define EG_SWAP(c, p, q) do { const double _p = (c) ? (q) : (p), _q = (c) ? (p) : (q); (p) = _p; (q) = _q; } while (0)
    {
        int piv = 0;
        double big = fabs(a00);
        if (fabs(a10) > big) { big = fabs(a10); piv = 1; }
        if (fabs(a20) > big) { big = fabs(a20); piv = 2; }
        const bool s1 = piv == 1, s2 = piv == 2;
        EG_SWAP(s1, a00, a10); EG_SWAP(s1, a01, a11); EG_SWAP(s1, a02, a12); EG_SWAP(s1, t0, t1);
        EG_SWAP(s2, a00, a20); EG_SWAP(s2, a01, a21); EG_SWAP(s2, a02, a22); EG_SWAP(s2, t0, t2);
        if (big != 0.0) { a10 = a10 / a00; a20 = a20 / a00; }
        a11 = a11 - a10 * a01; a12 = a12 - a10 * a02;
        a21 = a21 - a20 * a01; a22 = a22 - a20 * a02;
    }
    {
        const bool s = fabs(a21) > fabs(a11);
        EG_SWAP(s, a10, a20); EG_SWAP(s, a11, a21); EG_SWAP(s, a12, a22); EG_SWAP(s, t1, t2);
        if (a11 != 0.0) a21 = a21 / a11;
        a22 = a22 - a21 * a12;
    }
#undef EG_SWAP
    const double y0 = t0, y1 = t1 - a10 * y0, y2 = t2 - (a20 * y0 + a21 * y1);
    x2 = y2 / a22;
    x1 = (y1 - a12 * x2) / a11;
    x0 = (y0 - (a01 * x1 + a02 * x2)) / a00;
}

// sim3.h:148-230: Sim3::log() -> res[0..2] omega, res[3..5] upsilon, res[6] sigma.  R = r.toRotationMatrix() of the quaternion AS IT
// STANDS (Eigen does not normalise), d = 0.5 * (((R00 + R11) + R22) - 1); the four branches on fabs(sigma) < eps and d > 1 - eps;
// omega = 0.5 deltaR(R) or theta / (2 sqrt(1 - d d)) deltaR(R); W = (A Omega + (B Omega) Omega) + C I, the product (B Omega) Omega with
// the scaled factor rounded first and each entry summed (p0 + p1) + p2; upsilon = W.lu().solve(t) (lu3_solve).  branch: 0 .. 3 =
// 2 * (fabs(sigma) >= eps) + (d <= 1 - eps), for the tests that count them.
__device__ __forceinline__ void sim3_log(const Sim3 &S, double res[7], int *branch = nullptr)
{
    const double sigma = log(S.s);
    const Pose Q = { S.qx, S.qy, S.qz, S.qw, 0.0, 0.0, 0.0 };
    double R[9];
    quat_to_matrix(Q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dx = R[7] - R[5], dy = R[2] - R[6], dz = R[3] - R[1];   // deltaR
    const double eps = 0.00001;
    const bool small_sigma = fabs(sigma) < eps, small_rot = d > 1.0 - eps;
    double A, B, C, k;
    if (small_rot) {
        k = 0.5;
        if (small_sigma) {
            C = 1.0; A = 1.0 / 2.0; B = 1.0 / 6.0;
        } else {
            C = (S.s - 1.0) / sigma;
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * S.s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * S.s) / (sigma2 * sigma);
        }
    } else {
        const double theta = acos(d);
        const double theta2 = theta * theta;
        k = theta / (2.0 * sqrt(1.0 - d * d));
        if (small_sigma) {
            C = 1.0;
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        } else {
            C = (S.s - 1.0) / sigma;
            const double a = S.s * sin(theta), b = S.s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
        }
    }
    if (branch) *branch = (small_sigma ? 0 : 2) + (small_rot ? 0 : 1);
    const double o0 = k * dx, o1 = k * dy, o2 = k * dz;
    const double O[9] = { 0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0 };
    double BO[9], W[9];
#pragma unroll
    for (int q = 0; q < 9; q++) BO[q] = B * O[q];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double bo2 = (BO[3 * r] * O[c] + BO[3 * r + 1] * O[3 + c]) + BO[3 * r + 2] * O[6 + c];
            W[3 * r + c] = (A * O[3 * r + c] + bo2) + (r == c ? C : 0.0);
        }
    res[0] = o0; res[1] = o1; res[2] = o2;
    lu3_solve(W, S.tx, S.ty, S.tz, res[3], res[4], res[5]);
    res[6] = sigma;
}

}   // namespace

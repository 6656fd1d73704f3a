// orbx_lm.h — g2o's small pieces, one copy each, for the Levenberg kernels (k_pose_opt of orbx_pose.hip, k_sim3_opt of orbx_sim3opt.hip,
// the k_lba_* of orbx_lba.hip, the k_eg_* of orbx_essential.hip) and the one host loop of the bundle adjustments and the essential graph
// (lm_host_loop):
//   sums      block_sum: the fixed-order workgroup sum that hands every thread of a 4- or 16-wave workgroup the same bits
//   solver    ldlt_small<N>: the dense (H + lambda I) x = b of the one-vertex problems; hu_max_diag<N>
//   damping   lm_*: the rule of optimization_algorithm_levenberg.cpp (rho, lambda, ni, the two stops), host and device
//   robust    huber
//   geometry  Eigen's Quaternion(Matrix3), quaternion * vector and quaternion product; g2o's SE3Quat (Pose) with map and the exponential
//             update; Cam, Obs and computeError of the mono / stereo reprojection edges
// Two things are NOT here.  The pose Jacobians: k_pose_opt's (EdgeSE3ProjectXYZOnlyPose, products with invz) and jac_pose of orbx_lba.hip
// (EdgeSE3ProjectXYZ, divisions) are different reference expressions with different bits.  And the Omega, Omega^2, R = (I + a Omega) + b
// Omega^2 of the exponentials: pose_update below and sim3_exp of orbx_sim3.h each keep their own.  Each fuses R with its own
// theta < 1e-5 branch (pose_update fills V there, sim3_exp selects per entry next to its A, B, C), and a helper for Omega and Omega^2
// alone lets the compiler take -(o o) from the o o of theta: the same bits, one multiplication fewer, and so not the instructions these
// kernels were measured with.
// Everything but lm_* is device code; every device function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include "orbx_wave.h"

// robust_kernel_impl.cpp:78-91 (rho[2] is never used: base_edge.h:96-102)
static __device__ __forceinline__ void huber(double e, double delta, double &rho0, double &rho1)
{
    const double dsqr = delta * delta;
    if (e <= dsqr) { rho0 = e; rho1 = 1.0; return; }
    const double sqrte = sqrt(e);
    rho0 = 2.0 * sqrte * delta - dsqr;
    rho1 = delta / sqrte;
}

// a[k] summed over the workgroup's WAVES x 64 threads, for every thread: the xor butterfly across the wave (all 64 lanes hold the same
// bits), then through red[WAVES * K] ((w0 + w1) + (w2 + w3)) over each four waves and, of 16 waves, the same tree over the four fours
template <int WAVES = 4, int K>
static __device__ __forceinline__ void block_sum(double (&a)[K], double *red)
{
    static_assert(WAVES == 4 || WAVES == 16, "a tree of fours");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) a[k] = wave_sum(a[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[wave * K + k] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double q[WAVES / 4];
#pragma unroll
        for (int g = 0; g < WAVES / 4; g++) q[g] = (red[(4 * g) * K + k] + red[(4 * g + 1) * K + k]) + (red[(4 * g + 2) * K + k] + red[(4 * g + 3) * K + k]);
        if constexpr (WAVES == 4) a[k] = q[0];
        else a[k] = (q[0] + q[1]) + (q[2] + q[3]);
    }
    __syncthreads();
}

// (H + lambda I) x = b by LDL^T without pivoting; H's upper triangle in row order (00 01 .. 0(N-1) 11 12 ..).  false (x untouched) unless
// every pivot is > 0 (linear_solver_dense.h:104-112)
template <int N>
static __device__ __forceinline__ bool ldlt_small(const double *Hu, const double *b, double lambda, double *x)
{
    double A[N][N], L[N][N], d[N];
    int k = 0;
#pragma unroll
    for (int r = 0; r < N; r++)
#pragma unroll
        for (int c = r; c < N; c++) { A[r][c] = A[c][r] = Hu[k++]; }
#pragma unroll
    for (int r = 0; r < N; r++) A[r][r] += lambda;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double dj = A[j][j];
#pragma unroll
        for (int m = 0; m < j; m++) dj -= (L[j][m] * L[j][m]) * d[m];
        if (!(dj > 0.0)) return false;
        d[j] = dj;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double v = A[i][j];
#pragma unroll
            for (int m = 0; m < j; m++) v -= (L[i][m] * L[j][m]) * d[m];
            L[i][j] = v / dj;
        }
    }
    double y[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        double v = b[i];
#pragma unroll
        for (int m = 0; m < i; m++) v -= L[i][m] * y[m];
        y[i] = v;
    }
#pragma unroll
    for (int i = 0; i < N; i++) y[i] = y[i] / d[i];
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double v = y[i];
#pragma unroll
        for (int m = i + 1; m < N; m++) v -= L[m][i] * x[m];
        x[i] = v;
    }
    return true;
}

// the largest |diagonal entry| of H, its upper triangle in row order (optimization_algorithm_levenberg.cpp:166-180)
template <int N>
static __device__ __forceinline__ double hu_max_diag(const double *Hu)
{
    double md = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) md = fmax(fabs(Hu[k * N - k * (k - 1) / 2]), md);
    return md;
}

// The damping of optimization_algorithm_levenberg.cpp:66-164, on the host and in a kernel, over the caller's own lambda, ni (2 at the
// start) and stop_bad.  One outer iteration of its callers:
//   linearise -> ini_chi = cur_chi; the first time lm_start(max |diagonal|, ..)
//   do { solve with lambda, evaluate the trial; rho = lm_gain(..); where lm_accepts(rho, temp_chi): lm_accept(..), cur_chi = temp_chi, the
//        trial is the estimate; else lm_reject(..), the estimate goes back; qmax++ } while (rho < 0 && qmax < 10 [&& not stopped])
//   if (lm_done(qmax, rho, ini_chi, cur_chi, stop_bad)) break
// (The accept branch stays with the caller: its two sides are where the estimate is kept or restored.)
// user_lambda_init: setUserLambdaInit's value; computeLambdaInit (:166-180) returns it where it is > 0, else tau * the largest diagonal
static __host__ __device__ __forceinline__ void lm_start(double max_diag, double &lambda, double &ni, int &stop_bad, double user_lambda_init = 0.0)   // :93-97
{
    lambda = user_lambda_init > 0.0 ? user_lambda_init : 1e-5 * max_diag; ni = 2.0; stop_bad = 0;
}

// scale: computeScale's sum of x_j (lambda x_j + b_j)
static __host__ __device__ __forceinline__ double lm_gain(double cur_chi, double temp_chi, double scale)
{
    scale += 1e-3;
    return (cur_chi - temp_chi) / scale;
}

static __host__ __device__ __forceinline__ bool lm_accepts(double rho, double temp_chi) { return rho > 0.0 && std::isfinite(temp_chi); }

static __host__ __device__ __forceinline__ void lm_accept(double rho, double &lambda, double &ni)
{
    const double t = 2.0 * rho - 1.0;
    double alpha = 1.0 - (t * t) * t;
    alpha = fmin(alpha, 2.0 / 3.0);
    lambda *= fmax(1.0 / 3.0, alpha);
    ni = 2.0;
}

static __host__ __device__ __forceinline__ void lm_reject(double &lambda, double &ni) { lambda *= ni; ni *= 2.0; }

// the end of an outer iteration: the trials ran out or the step was exactly useless, or three iterations in a row gained under 1e-3
static __host__ __device__ __forceinline__ bool lm_done(int qmax, double rho, double ini_chi, double cur_chi, int &stop_bad)
{
    if (qmax == 10 || rho == 0.0) return true;
    if ((ini_chi - cur_chi) * 1e3 < ini_chi) stop_bad++; else stop_bad = 0;
    return stop_bad >= 3;
}

// ---- host only: SparseOptimizer::optimize(max_it) for the solvers whose kernels run one step per launch (LbaRun::optimize of orbx_lba.hip,
// orbx_optimize_essential_graph): the sequence above driven over a fetched status record of doubles, [0] chi2, [1] computeScale's sum,
// [2] the largest diagonal entry (behind linearise), [3] != 0 where the solve succeeded (behind a trial; a failed one counts as chi2 DBL_MAX).
struct LmRun {
    int rc;                                            // the first failure of linearise() / trial(); the rest is then not to be read
    int iterations, trials, n_solve_failed;
    bool evaluated;                                    // linearise() ran at least once
    double chi2, lambda, lambda_init, chi2_start;      // at the end (0 if no iteration ran); lm_start's lambda, the first linearisation's chi2
};

// linearise() and trial(lambda) launch their kernels and fetch the record (ORBX_OK or the failure); status() is where it was fetched to.  A
// trial evaluates into the copy that is not the estimate: swap() makes that copy the estimate (discardTop()), a rejected trial leaves it
// (pop()).  stop_up(): the caller's stop flag, asked before every iteration and behind every trial (sparse_optimizer.cpp:356, :376).
template <class Linearise, class Trial, class Status, class StopUp, class Swap>
static inline LmRun lm_host_loop(int max_it, double user_lambda_init, Linearise linearise, Trial trial, Status status, StopUp stop_up, Swap swap)
{
    LmRun r = {};
    double lambda = 0.0, ni = 2.0, cur_chi = 0.0;
    int stop_bad = 0;
    for (int it = 0; it < max_it && !stop_up(); it++) {
        if ((r.rc = linearise())) return r;
        const double *hs = status();
        r.evaluated = true;
        cur_chi = hs[0];
        const double ini_chi = cur_chi;
        if (it == 0) {
            r.chi2_start = cur_chi;
            lm_start(hs[2], lambda, ni, stop_bad, user_lambda_init);
            r.lambda_init = lambda;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            if ((r.rc = trial(lambda))) return r;
            r.trials++;
            const bool ok = hs[3] != 0.0;
            r.n_solve_failed += !ok;
            const double temp_chi = ok ? hs[0] : DBL_MAX;
            rho = lm_gain(cur_chi, temp_chi, hs[1]);
            if (lm_accepts(rho, temp_chi)) {
                lm_accept(rho, lambda, ni);
                cur_chi = temp_chi;
                swap();
            } else lm_reject(lambda, ni);   // the edges keep the errors of the rejected state
            qmax++;
        } while (rho < 0.0 && qmax < 10 && !stop_up());
        r.iterations++;
        if (lm_done(qmax, rho, ini_chi, cur_chi, stop_bad)) break;
    }
    r.chi2 = cur_chi; r.lambda = lambda;
    return r;
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

// Eigen's Quaternion * vector: uv = 2 (q.vec x v); v + w uv + q.vec x uv (the quaternion need not be a unit one)
static __device__ __forceinline__ void quat_rot(double qx, double qy, double qz, double qw, double X, double Y, double Z, double &x, double &y, double &z)
{
    const double ux = 2.0 * (qy * Z - qz * Y), uy = 2.0 * (qz * X - qx * Z), uz = 2.0 * (qx * Y - qy * X);
    x = (X + qw * ux) + (qy * uz - qz * uy);
    y = (Y + qw * uy) + (qz * ux - qx * uz);
    z = (Z + qw * uz) + (qx * uy - qy * ux);
}

// Eigen's quaternion product a * b, not normalised
static __device__ __forceinline__ void quat_mul(double ax, double ay, double az, double aw, double bx, double by, double bz, double bw,
                                                double &qx, double &qy, double &qz, double &qw)
{
    qw = ((aw * bw - ax * bx) - ay * by) - az * bz;
    qx = ((aw * bx + ax * bw) + ay * bz) - az * by;
    qy = ((aw * by + ay * bw) + az * bx) - ax * bz;
    qz = ((aw * bz + az * bw) + ax * by) - ay * bx;
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

// SE3Quat::map
static __device__ __forceinline__ void se3_map(const Pose &P, double X, double Y, double Z, double &x, double &y, double &z)
{
    quat_rot(P.qx, P.qy, P.qz, P.qw, X, Y, Z, x, y, z);
    x = x + P.tx; y = y + P.ty; z = z + P.tz;
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
    double rx, ry, rz;
    quat_rot(E.qx, E.qy, E.qz, E.qw, P.tx, P.ty, P.tz, rx, ry, rz);
    N.tx = E.tx + rx; N.ty = E.ty + ry; N.tz = E.tz + rz;
    quat_mul(E.qx, E.qy, E.qz, E.qw, P.qx, P.qy, P.qz, P.qw, N.qx, N.qy, N.qz, N.qw);
    quat_normalize(N.qx, N.qy, N.qz, N.qw);
    return N;
}

// a camera (fx fy cx cy mbf) and one observation of the mono / stereo reprojection edges: stereo where u_right is not negative
struct Cam { double fx, fy, cx, cy, bf; };
struct Obs { double mx, my, mr, w; bool stereo; };

static __device__ __forceinline__ Cam cam_load(const float *c) { return Cam{ (double)c[0], (double)c[1], (double)c[2], (double)c[3], (double)c[4] }; }

// computeError of EdgeSE3ProjectXYZ[OnlyPose] / EdgeStereoSE3ProjectXYZ[OnlyPose] at the mapped point (types_six_dof_expmap.h, cam_project
// :141-157): error = measurement - projection; returns chi2 = e . (w e)
static __device__ __forceinline__ double edge_error(const Obs &o, const Cam &C, double x, double y, double z, double err[3])
{
    if (o.stereo) {
        const double invz = (double)(float)(1.0 / z);   // types_six_dof_expmap.cpp:300: `const float invz = 1.0f/trans_xyz[2]`
        const double u = (x * invz) * C.fx + C.cx, v = (y * invz) * C.fy + C.cy;
        err[0] = o.mx - u; err[1] = o.my - v; err[2] = o.mr - (u - C.bf * invz);
        return (err[0] * (o.w * err[0]) + err[1] * (o.w * err[1])) + err[2] * (o.w * err[2]);
    }
    err[0] = o.mx - ((x / z) * C.fx + C.cx); err[1] = o.my - ((y / z) * C.fy + C.cy); err[2] = 0.0;
    return err[0] * (o.w * err[0]) + err[1] * (o.w * err[1]);
}

// orbx_lba.hip — Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:528-862) as a host-driven Levenberg loop over short chains of
// launches on the calling thread's stream.  Everything is fp64 on wave64, plain VALU, no atomics; every sum is taken in an order that is a
// fixed function of the problem's shape, so a call is byte-reproducible.  The contract is include/orbx.h (orbx_local_bundle_adjustment),
// its numpy restatement tests/lba_model.py.
//
// State on the device: two copies of the estimates (poses as g2o's SE3Quat, points), `cur` and `trial`; accepting a trial swaps them
// (g2o's push / discardTop / pop).  Per edge: the chi2 of its last evaluation (what OptimizableGraph::Edge::chi2() returns at the two
// classifications), W = Jp^T (rho1 Omega) Jl, and its flag byte.  Per point: Hll, bl, Dinv, Dinv bl, x_l.  Per active free keyframe (a
// "row" of the reduced system): Hpp, bp.  The reduced system S (n = 6 rows <= 1536) is dense.
//
// One linearisation:   k_lba_points<true> (a thread per point walks its edges in order: errors, rho, both Jacobians, Hll, bl, W)
//                      k_lba_kf           (a workgroup per row: Hpp, bp by the butterfly + fixed LDS order of k_pose_opt)
//                      k_lba_reduce       (one workgroup: the robust chi2 over the points, the largest diagonal entry)
// One damping trial:   k_lba_prep         (Dinv = (Hll + lambda I)^-1 by cofactors, Dinv bl)
//                      k_lba_schur        (a workgroup per block (i, j >= i) of S; the diagonal ones also b_S)
//                      k_lba_solve        (one workgroup: LDL^T of S without pivoting, a column of L staged in LDS per step, both triangular solves)
//                      k_lba_update       (x_l, the pose and point updates into the trial copy)
//                      k_lba_points<false> (errors and robust chi2 at the trial state)
//                      k_lba_reduce       (chi2 and the scale sum)
// Between the rounds:  k_lba_classify, k_lba_active (the level-0 edges of every keyframe compacted in point order, the rows, the active points).
// The host reads one small status record back per linearisation and per trial and computes rho, lambda and ni in double.
//
// Optimizer::BundleAdjustment (src/Optimizer.cc:48-281, orbx_bundle_adjustment, model tests/gba_model.py) is the same staging, the same
// linearisation and the same trial in ONE round over every edge: k_gba_active / k_gba_rows in place of k_lba_active (no edge ever leaves
// level 0, the keyframes outnumber a workgroup), no k_lba_classify, and the solve in panels over many workgroups (orbx_ldlt.hip, the same
// bytes as k_lba_solve), so n = 6 rows goes to 12 288.  orbx_debug_set_lba_solver puts the panels under the local call as well.
#include "orbx_resident.h"
#include "orbx_lm.h"
#include "orbx_ldlt.h"
#include <float.h>
#include <algorithm>
#include <cmath>

namespace {

struct Lba {
    int K, P, E;
    int nx;                            // the length of x: 6 x the free keyframes the entry point admits
    double delta_mono;                 // Huber's delta of a monocular edge: the entry point's own thHuberMono / thHuber2D, a float widened
    // inputs (the uploaded blob)
    const float *Tcw, *cam, *Xw, *mx, *my, *mr, *isig;
    const uint8_t *fixed;
    const int32_t *edge_kf, *edge_point, *point_off, *kf_off, *kf_edges;
    // state
    double *pose[2], *pts[2];          // [K][7], [P][3]
    double *echi, *W;                  // [E], [E][18]
    uint8_t *flags, *pactive;          // [E], [P]
    double *Hll, *bl, *Dinv, *db, *xl, *chi_pt;   // [P][6] [P][3] [P][6] [P][3] [P][3] [P]
    int32_t *kf_act, *kf_cnt, *row, *rowkf;       // [E] [K] [K] [K]
    double *Hpp, *bp;                  // [rows][21], [rows][6]
    double *S, *bS, *x;                // [n][n], [n], [n]
    double *status;                    // chi2, scale, max diagonal, solve ok
    int32_t *counts;                   // rows, active points
    // outputs
    double *pose_out, *point_out;
    float *Tcw_out, *Xw_out;
};

__device__ __forceinline__ Pose pose_load(const double *p) { return Pose{ p[0], p[1], p[2], p[3], p[4], p[5], p[6] }; }
__device__ __forceinline__ void pose_store(double *p, const Pose &P) { p[0] = P.qx; p[1] = P.qy; p[2] = P.qz; p[3] = P.qw; p[4] = P.tx; p[5] = P.ty; p[6] = P.tz; }

__device__ __forceinline__ Obs obs_load(const Lba &L, int e)
{
    Obs o;
    const float ur = L.mr[e];
    o.mx = (double)L.mx[e]; o.my = (double)L.my[e]; o.mr = (double)ur; o.w = (double)L.isig[e];
    o.stereo = !(ur < 0.f);   // src/Optimizer.cc:675
    return o;
}

// _jacobianOplusXj, the 2/3 x 6 pose block (types_six_dof_expmap.cpp:126-138, :214-233); the third row only for a stereo edge
__device__ __forceinline__ void jac_pose(const Cam &C, bool stereo, double x, double y, double z, double B[3][6])
{
    const double z_2 = z * z;
    B[0][0] = x * y / z_2 * C.fx; B[0][1] = -(1.0 + (x * x / z_2)) * C.fx; B[0][2] = y / z * C.fx;
    B[0][3] = -1.0 / z * C.fx; B[0][4] = 0.0; B[0][5] = x / z_2 * C.fx;
    B[1][0] = (1.0 + y * y / z_2) * C.fy; B[1][1] = -x * y / z_2 * C.fy; B[1][2] = -x / z * C.fy;
    B[1][3] = 0.0; B[1][4] = -1.0 / z * C.fy; B[1][5] = y / z_2 * C.fy;
    if (stereo) {
        B[2][0] = B[0][0] - C.bf * y / z_2; B[2][1] = B[0][1] + C.bf * x / z_2; B[2][2] = B[0][2];
        B[2][3] = B[0][3]; B[2][4] = 0.0; B[2][5] = B[0][5] - C.bf / z_2;
    } else {
#pragma unroll
        for (int c = 0; c < 6; c++) B[2][c] = 0.0;
    }
}

// _jacobianOplusXi, the 2/3 x 3 point block (:115-124 monocular: (-1./z * tmp) * R with the zero entries of tmp in the sums; :202-212 stereo)
__device__ __forceinline__ void jac_point(const Cam &C, bool stereo, const double R[9], double x, double y, double z, double A[3][3])
{
    if (stereo) {
        const double z_2 = z * z;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            A[0][c] = -C.fx * R[c] / z + C.fx * x * R[6 + c] / z_2;
            A[1][c] = -C.fy * R[3 + c] / z + C.fy * y * R[6 + c] / z_2;
            A[2][c] = A[0][c] - C.bf * R[6 + c] / z_2;
        }
        return;
    }
    const double s = -1.0 / z;
    const double t00 = s * C.fx, t01 = s * 0.0, t02 = s * (-x / z * C.fx), t10 = s * 0.0, t11 = s * C.fy, t12 = s * (-y / z * C.fy);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        A[0][c] = (t00 * R[c] + t01 * R[3 + c]) + t02 * R[6 + c];
        A[1][c] = (t10 * R[c] + t11 * R[3 + c]) + t12 * R[6 + c];
        A[2][c] = 0.0;
    }
}

// ---------------------------------------------------------------- start and finish

__global__ __launch_bounds__(256) void k_lba_init(Lba L)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < L.K) {   // Converter::toSE3Quat: the float matrix widened, SE3Quat(R, t)
        const float *T = L.Tcw + 16 * (size_t)t;
        double m[9];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) m[3 * r + c] = (double)T[4 * r + c];
        Pose S;
        quat_from_matrix(m, S.qx, S.qy, S.qz, S.qw);
        quat_normalize(S.qx, S.qy, S.qz, S.qw);
        S.tx = (double)T[3]; S.ty = (double)T[7]; S.tz = (double)T[11];
        pose_store(L.pose[0] + 7 * (size_t)t, S); pose_store(L.pose[1] + 7 * (size_t)t, S);
    }
    if (t < L.P) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double v = (double)L.Xw[3 * (size_t)t + c];
            L.pts[0][3 * (size_t)t + c] = v; L.pts[1][3 * (size_t)t + c] = v; L.xl[3 * (size_t)t + c] = 0.0;
        }
    }
    if (t < L.E) { L.flags[t] = 0; L.echi[t] = 0.0; }
    if (t < L.nx) L.x[t] = 0.0;
}

__global__ __launch_bounds__(256) void k_lba_finish(Lba L, int cur)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < L.K) {   // Converter::toCvMat(SE3Quat)
        const Pose P = pose_load(L.pose[cur] + 7 * (size_t)t);
        double R[9];
        quat_to_matrix(P, R);
        const double tt[3] = { P.tx, P.ty, P.tz };
        double *po = L.pose_out + 12 * (size_t)t;
        float *To = L.Tcw_out + 16 * (size_t)t;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) { po[4 * r + c] = R[3 * r + c]; To[4 * r + c] = (float)R[3 * r + c]; }
            po[4 * r + 3] = tt[r]; To[4 * r + 3] = (float)tt[r];
        }
        To[12] = 0.f; To[13] = 0.f; To[14] = 0.f; To[15] = 1.f;
    }
    if (t < L.P) {
        for (int c = 0; c < 3; c++) {
            const double v = L.pts[cur][3 * (size_t)t + c];
            L.point_out[3 * (size_t)t + c] = v; L.Xw_out[3 * (size_t)t + c] = (float)v;
        }
    }
}

// ---------------------------------------------------------------- the active set of a round (initializeOptimization, sparse_optimizer.cpp:206-266)

// one workgroup.  Thread k compacts keyframe k's level-0 edges, in point order, into kf_act / kf_cnt; the free keyframes that have one get the
// rows 0, 1, .. in keyframe order; a point is active when it has a level-0 edge
__global__ __launch_bounds__(1024) void k_lba_active(Lba L)
{
    __shared__ int sc[1024];
    __shared__ int wsum[16];
    const int t = threadIdx.x;
    int act = 0;
    if (t < L.K) {
        int m = 0;
        const int b = L.kf_off[t], e1 = L.kf_off[t + 1];
        for (int q = b; q < e1; q++) {
            const int e = L.kf_edges[q];
            if (!(L.flags[e] & 1)) L.kf_act[b + m++] = e;
        }
        L.kf_cnt[t] = m;
        act = (!L.fixed[t] && m > 0) ? 1 : 0;
    }
    sc[t] = act;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    if (t < L.K) {
        L.row[t] = act ? sc[t] - 1 : -1;
        if (act) L.rowkf[sc[t] - 1] = t;
    }
    int np = 0;
    for (int p = t; p < L.P; p += 1024) {
        int a = 0;
        for (int e = L.point_off[p]; e < L.point_off[p + 1]; e++) a |= !(L.flags[e] & 1);
        L.pactive[p] = (uint8_t)a;
        np += a;
    }
    np = wave_sum(np);
    if ((t & 63) == 0) wsum[t >> 6] = np;
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int w = 0; w < 16; w++) s += wsum[w];
        L.counts[0] = sc[1023];
        L.counts[1] = s;
        L.status[3] = 1.0;   // without a row there is no solve to fail
    }
}

// The active set of orbx_bundle_adjustment, whose edges are all at level 0 for the whole call (kf_act is kf_edges itself) and whose
// keyframes outnumber a workgroup.  k_gba_active, a thread per keyframe and per point: the edge count, whether the keyframe gets a row
// (row = 0, else -1), whether the point is a vertex.  k_gba_rows, one workgroup, four consecutive keyframes per thread (n_kf <= 4096): the
// rows 0, 1, .. in keyframe order, the counts.
__global__ __launch_bounds__(256) void k_gba_active(Lba L)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < L.K) {
        const int m = L.kf_off[t + 1] - L.kf_off[t];
        L.kf_cnt[t] = m;
        L.row[t] = (!L.fixed[t] && m > 0) ? 0 : -1;
    }
    if (t < L.P) L.pactive[t] = (uint8_t)(L.point_off[t + 1] > L.point_off[t]);
}

__global__ __launch_bounds__(1024) void k_gba_rows(Lba L)
{
    __shared__ int sc[1024];
    __shared__ int wsum[16];
    const int t = threadIdx.x;
    int act[4], mine = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int k = 4 * t + q;
        act[q] = (k < L.K && L.row[k] == 0) ? 1 : 0;
        mine += act[q];
    }
    sc[t] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    int r = sc[t] - mine;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (act[q]) { L.row[4 * t + q] = r; L.rowkf[r] = 4 * t + q; r++; }
    int np = 0;
    for (int p = t; p < L.P; p += 1024) np += L.pactive[p];
    np = wave_sum(np);
    if ((t & 63) == 0) wsum[t >> 6] = np;
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int w = 0; w < 16; w++) s += wsum[w];
        L.counts[0] = sc[1023];
        L.counts[1] = s;
        L.status[3] = 1.0;
    }
}

// ---------------------------------------------------------------- errors and linearisation

// a thread per point, its level-0 edges one after the other in edge order.  LIN = false: computeActiveErrors (the edge's chi2, the point's
// share of the robust chi2).  LIN = true: also linearizeOplus and constructQuadraticForm (base_binary_edge.hpp) for the point vertex and the
// mixed block: Hll, bl, W = Jp^T (rho1 Omega) Jl
template <bool LIN>
__global__ __launch_bounds__(256) void k_lba_points(Lba L, int st, int robust)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L.P) return;
    if (!L.pactive[p]) { L.chi_pt[p] = 0.0; return; }
    const double delta_mono = L.delta_mono, delta_stereo = (double)(float)sqrt(7.815);   // src/Optimizer.cc:650-651, :101-102
    const double X[3] = { L.pts[st][3 * (size_t)p], L.pts[st][3 * (size_t)p + 1], L.pts[st][3 * (size_t)p + 2] };
    double H[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, b[3] = { 0.0, 0.0, 0.0 }, chi_sum = 0.0;
    for (int e = L.point_off[p]; e < L.point_off[p + 1]; e++) {
        if (L.flags[e] & 1) continue;
        const int k = L.edge_kf[e];
        const Pose T = pose_load(L.pose[st] + 7 * (size_t)k);
        const Cam C = cam_load(L.cam + 5 * (size_t)k);
        const Obs o = obs_load(L, e);
        double x, y, z, err[3];
        se3_map(T, X[0], X[1], X[2], x, y, z);
        const double chi = edge_error(o, C, x, y, z, err);
        L.echi[e] = chi;
        double rho0 = chi, rho1 = 1.0;
        if (robust) huber(chi, o.stereo ? delta_stereo : delta_mono, rho0, rho1);
        chi_sum += rho0;
        if (!LIN) continue;
        double R[9], A[3][3];
        quat_to_matrix(T, R);
        jac_point(C, o.stereo, R, x, y, z, A);
        const double rw = rho1 * o.w;
        const double omr[3] = { -(o.w * err[0]) * rho1, -(o.w * err[1]) * rho1, -(o.w * err[2]) * rho1 };
        int q = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = r; c < 3; c++, q++) H[q] += ((A[0][r] * rw) * A[0][c] + (A[1][r] * rw) * A[1][c]) + (A[2][r] * rw) * A[2][c];
            b[r] += (A[0][r] * omr[0] + A[1][r] * omr[1]) + A[2][r] * omr[2];
        }
        if (L.row[k] >= 0) {
            double B[3][6];
            jac_pose(C, o.stereo, x, y, z, B);
            double *W = L.W + 18 * (size_t)e;
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) W[3 * r + c] = ((B[0][r] * rw) * A[0][c] + (B[1][r] * rw) * A[1][c]) + (B[2][r] * rw) * A[2][c];
        }
    }
    L.chi_pt[p] = chi_sum;
    if (LIN) {
#pragma unroll
        for (int q = 0; q < 6; q++) L.Hll[6 * (size_t)p + q] = H[q];
#pragma unroll
        for (int r = 0; r < 3; r++) L.bl[3 * (size_t)p + r] = b[r];
    }
}

// a workgroup per row: Hpp (upper triangle in row order) and bp over the keyframe's level-0 edges, strided over the threads in the
// keyframe's point order; the order of the sum is a function of the count alone
__global__ __launch_bounds__(256) void k_lba_kf(Lba L, int st, int robust)
{
    __shared__ double red[4 * 27];
    const int r0 = blockIdx.x, k = L.rowkf[r0], tid = threadIdx.x;
    const double delta_mono = L.delta_mono, delta_stereo = (double)(float)sqrt(7.815);
    const Pose T = pose_load(L.pose[st] + 7 * (size_t)k);
    const Cam C = cam_load(L.cam + 5 * (size_t)k);
    const int32_t *list = L.kf_act + L.kf_off[k];
    const int cnt = L.kf_cnt[k];
    double acc[27];
#pragma unroll
    for (int q = 0; q < 27; q++) acc[q] = 0.0;
    for (int m = tid; m < cnt; m += 256) {
        const int e = list[m], p = L.edge_point[e];
        const double X[3] = { L.pts[st][3 * (size_t)p], L.pts[st][3 * (size_t)p + 1], L.pts[st][3 * (size_t)p + 2] };
        const Obs o = obs_load(L, e);
        double x, y, z, err[3], B[3][6];
        se3_map(T, X[0], X[1], X[2], x, y, z);
        const double chi = edge_error(o, C, x, y, z, err);
        double rho0 = chi, rho1 = 1.0;
        if (robust) huber(chi, o.stereo ? delta_stereo : delta_mono, rho0, rho1);
        jac_pose(C, o.stereo, x, y, z, B);
        const double rw = rho1 * o.w;
        const double omr[3] = { -(o.w * err[0]) * rho1, -(o.w * err[1]) * rho1, -(o.w * err[2]) * rho1 };
        int q = 0;
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
            for (int c = r; c < 6; c++, q++) acc[q] += ((B[0][r] * rw) * B[0][c] + (B[1][r] * rw) * B[1][c]) + (B[2][r] * rw) * B[2][c];
            acc[21 + r] += (B[0][r] * omr[0] + B[1][r] * omr[1]) + B[2][r] * omr[2];
        }
    }
    block_sum(acc, red);
    if (tid == 0) {   // one thread, constant indices: an index that depends on the thread would put acc[] into scratch
#pragma unroll
        for (int q = 0; q < 21; q++) L.Hpp[21 * (size_t)r0 + q] = acc[q];
#pragma unroll
        for (int q = 0; q < 6; q++) L.bp[6 * (size_t)r0 + q] = acc[21 + q];
    }
}

// one workgroup: what = 0 after a linearisation (chi2, the largest |diagonal entry| of the active vertices' Hessian blocks), 1 after a
// trial (chi2, computeScale: sum over x of x_j (lambda x_j + b_j), poses first).  Each thread takes its indices ascending, stride 1024.
__global__ __launch_bounds__(1024) void k_lba_reduce(Lba L, int what, double lambda)
{
    __shared__ double red[16 * 2];
    __shared__ double mx[16];
    const int t = threadIdx.x, rows = L.counts[0];
    double a[2] = { 0.0, 0.0 };
    double md = 0.0;
    if (what == 1)
        for (int j = t; j < 6 * rows; j += 1024) a[1] += L.x[j] * (lambda * L.x[j] + L.bp[j]);
    else
        for (int j = t; j < 6 * rows; j += 1024) {
            const int r = j / 6, c = j - 6 * r;
            const int diag[6] = { 0, 6, 11, 15, 18, 20 };
            md = fmax(fabs(L.Hpp[21 * (size_t)r + diag[c]]), md);
        }
    for (int p = t; p < L.P; p += 1024) {
        if (!L.pactive[p]) continue;
        a[0] += L.chi_pt[p];
        if (what == 1) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double xv = L.xl[3 * (size_t)p + c];
                a[1] += xv * (lambda * xv + L.bl[3 * (size_t)p + c]);
            }
        } else {
            md = fmax(fabs(L.Hll[6 * (size_t)p]), md); md = fmax(fabs(L.Hll[6 * (size_t)p + 3]), md); md = fmax(fabs(L.Hll[6 * (size_t)p + 5]), md);
        }
    }
    block_sum<16>(a, red);
    md = wave_max(md);
    if ((t & 63) == 0) mx[t >> 6] = md;
    __syncthreads();
    if (t == 0) {
        for (int w = 0; w < 16; w++) md = fmax(md, mx[w]);
        L.status[0] = a[0]; L.status[1] = a[1]; L.status[2] = md;
    }
}

// ---------------------------------------------------------------- a damping trial

// setLambda on Hll, then Eigen's fixed-size inverse(): cofactors, the determinant along the first column, no singularity test
__global__ __launch_bounds__(256) void k_lba_prep(Lba L, double lambda)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L.P || !L.pactive[p]) return;
    const double *H = L.Hll + 6 * (size_t)p;
    const double m00 = H[0] + lambda, m01 = H[1], m02 = H[2], m11 = H[3] + lambda, m12 = H[4], m22 = H[5] + lambda;
    const double c00 = m11 * m22 - m12 * m12, c01 = m12 * m02 - m01 * m22, c02 = m01 * m12 - m11 * m02;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = (c00 * m00 + c01 * m01) + c02 * m02, inv = 1.0 / det;
    const double D[6] = { c00 * inv, c01 * inv, c02 * inv, c11 * inv, c12 * inv, c22 * inv };
    const double *b = L.bl + 3 * (size_t)p;
    double *Do = L.Dinv + 6 * (size_t)p, *d = L.db + 3 * (size_t)p;
#pragma unroll
    for (int q = 0; q < 6; q++) Do[q] = D[q];
    d[0] = (D[0] * b[0] + D[1] * b[1]) + D[2] * b[2];
    d[1] = (D[1] * b[0] + D[3] * b[1]) + D[4] * b[2];
    d[2] = (D[2] * b[0] + D[4] * b[1]) + D[5] * b[2];
}

// a workgroup per block (i = blockIdx.y, j = blockIdx.x >= i) of S = Hpp + lambda I - sum over the points (W_i Dinv) W_j^T
// (block_solver.hpp:372-439).  The threads stride over row i's level-0 edges; the edge of the same point in row j's list, which is sorted by
// edge and so by point, is found by binary search.  The diagonal workgroups also give b_S = bp - sum W_i (Dinv bl).  Block (i, j) is
// written with its mirror image; of a diagonal block the upper triangle is what both halves get.
__global__ __launch_bounds__(256) void k_lba_schur(Lba L, double lambda)
{
    __shared__ double red[4 * 36];
    const int i = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    if (j < i) return;
    const int n = 6 * L.counts[0];
    const int ki = L.rowkf[i], kj = L.rowkf[j];
    const int32_t *li = L.kf_act + L.kf_off[ki], *lj = L.kf_act + L.kf_off[kj];
    const int ci = L.kf_cnt[ki], cj = L.kf_cnt[kj];
    double acc[36], ab[6];
#pragma unroll
    for (int q = 0; q < 36; q++) acc[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 6; q++) ab[q] = 0.0;
    for (int m = tid; m < ci; m += 256) {
        const int e = li[m], p = L.edge_point[e];
        int e2 = e;
        if (i != j) {
            const int lo_e = L.point_off[p], hi_e = L.point_off[p + 1];
            int lo = 0, hi = cj;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (lj[mid] < lo_e) lo = mid + 1; else hi = mid;
            }
            if (lo >= cj || lj[lo] >= hi_e) continue;
            e2 = lj[lo];
        }
        const double *Wi = L.W + 18 * (size_t)e, *Wj = L.W + 18 * (size_t)e2, *Dp = L.Dinv + 6 * (size_t)p;
        const double D[3][3] = { { Dp[0], Dp[1], Dp[2] }, { Dp[1], Dp[3], Dp[4] }, { Dp[2], Dp[4], Dp[5] } };
        double wj[18];
#pragma unroll
        for (int q = 0; q < 18; q++) wj[q] = Wj[q];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const double w0 = Wi[3 * r], w1 = Wi[3 * r + 1], w2 = Wi[3 * r + 2];
            const double b0 = (w0 * D[0][0] + w1 * D[1][0]) + w2 * D[2][0];
            const double b1 = (w0 * D[0][1] + w1 * D[1][1]) + w2 * D[2][1];
            const double b2 = (w0 * D[0][2] + w1 * D[1][2]) + w2 * D[2][2];
#pragma unroll
            for (int c = 0; c < 6; c++) acc[6 * r + c] += (b0 * wj[3 * c] + b1 * wj[3 * c + 1]) + b2 * wj[3 * c + 2];
            if (i == j) {
                const double *d = L.db + 3 * (size_t)p;
                ab[r] += (w0 * d[0] + w1 * d[1]) + w2 * d[2];
            }
        }
    }
    block_sum(acc, red);
    if (i == j) block_sum(ab, red);
    if (tid != 0) return;   // one thread writes, with constant indices: an index that depends on the thread would put acc[] into scratch
    if (i == j) {
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const int a = r < c ? r : c, b = r < c ? c : r;   // the upper triangle's entry (a, b)
                double h = L.Hpp[21 * (size_t)i + (a * 6 - a * (a - 1) / 2 + (b - a))];
                if (r == c) h += lambda;
                L.S[(size_t)(6 * i + r) * n + 6 * i + c] = h - acc[6 * a + b];
            }
            L.bS[6 * i + r] = L.bp[6 * (size_t)i + r] - ab[r];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const double v = 0.0 - acc[6 * r + c];
                L.S[(size_t)(6 * i + r) * n + 6 * j + c] = v;
                L.S[(size_t)(6 * j + c) * n + 6 * i + r] = v;
            }
    }
}

// one workgroup: S = L D L^T without pivoting on the lower triangle, column by column (right-looking: the column of L is staged in LDS, then
// every entry (i, k), i >= k > j, loses (l_i l_k) d_j), the forward substitution carried along, then the division by D and the backward
// substitution by columns.  Every entry sees its subtractions in ascending (backward: descending) column order, a function of n alone.
// A pivot <= 0 (or NaN) ends it: status[3] = 0, x keeps the previous solution (the reference's solver leaves _x alone when it fails).
__global__ __launch_bounds__(1024) void k_lba_solve(Lba L)
{
    __shared__ double l[1536];
    const int n = 6 * L.counts[0], tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    double *S = L.S, *y = L.bS;
    for (int j = 0; j < n; j++) {
        const double d = S[(size_t)j * n + j], yj = y[j];
        if (!(d > 0.0)) {
            if (tid == 0) L.status[3] = 0.0;
            return;
        }
        for (int i = j + 1 + tid; i < n; i += 1024) {
            const double li = S[(size_t)i * n + j] / d;
            S[(size_t)i * n + j] = li; l[i] = li;
            y[i] -= li * yj;
        }
        __syncthreads();
        for (int i = j + 1 + ty; i < n; i += 32) {
            const double li = l[i];
            for (int k = j + 1 + tx; k <= i; k += 32) S[(size_t)i * n + k] -= (li * l[k]) * d;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += 1024) y[i] = y[i] / S[(size_t)i * n + i];
    __syncthreads();
    for (int j = n - 1; j >= 0; j--) {
        const double xj = y[j];
        for (int i = tid; i < j; i += 1024) y[i] -= S[(size_t)j * n + i] * xj;
        __syncthreads();
    }
    for (int i = tid; i < n; i += 1024) L.x[i] = y[i];
    if (tid == 0) L.status[3] = 1.0;
}

// thread t: keyframe t's trial pose (SE3Quat::exp(x) * pose for a row, a copy otherwise) and point t's x_l = Dinv (bl - W^T x_p) over its
// level-0 edges in order, trial point = point + x_l.  After a failed solve x and x_l are the previous ones (optimizer.update(_solver->x())).
__global__ __launch_bounds__(256) void k_lba_update(Lba L, int cur)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const bool ok = L.status[3] != 0.0;
    if (t < L.K) {
        Pose P = pose_load(L.pose[cur] + 7 * (size_t)t);
        const int r = L.row[t];
        if (r >= 0) {
            double x[6];
#pragma unroll
            for (int c = 0; c < 6; c++) x[c] = L.x[6 * r + c];
            P = pose_update(P, x);
        }
        pose_store(L.pose[1 - cur] + 7 * (size_t)t, P);
    }
    if (t < L.P) {
        const size_t p = (size_t)t;
        double X[3] = { L.pts[cur][3 * p], L.pts[cur][3 * p + 1], L.pts[cur][3 * p + 2] };
        if (L.pactive[t]) {
            if (ok) {
                double c[3] = { L.bl[3 * p], L.bl[3 * p + 1], L.bl[3 * p + 2] };
                for (int e = L.point_off[t]; e < L.point_off[t + 1]; e++) {
                    if (L.flags[e] & 1) continue;
                    const int r = L.row[L.edge_kf[e]];
                    if (r < 0) continue;
                    const double *W = L.W + 18 * (size_t)e, *x = L.x + 6 * r;
#pragma unroll
                    for (int q = 0; q < 3; q++)
                        c[q] -= ((((W[q] * x[0] + W[3 + q] * x[1]) + W[6 + q] * x[2]) + W[9 + q] * x[3]) + W[12 + q] * x[4]) + W[15 + q] * x[5];
                }
                const double *D = L.Dinv + 6 * p;
                L.xl[3 * p] = (D[0] * c[0] + D[1] * c[1]) + D[2] * c[2];
                L.xl[3 * p + 1] = (D[1] * c[0] + D[3] * c[1]) + D[4] * c[2];
                L.xl[3 * p + 2] = (D[2] * c[0] + D[4] * c[1]) + D[5] * c[2];
            }
#pragma unroll
            for (int q = 0; q < 3; q++) X[q] += L.xl[3 * p + q];
        }
#pragma unroll
        for (int q = 0; q < 3; q++) L.pts[1 - cur][3 * p + q] = X[q];
    }
}

// bit = 1: the classification after round 1 (:753-783), bit = 2: the final check (:797-825).  chi2() is the edge's last evaluation, a
// level-1 edge's that of round 1; isDepthPositive() is taken at the current estimates; the thresholds compare in double.
__global__ __launch_bounds__(256) void k_lba_classify(Lba L, int cur, int bit)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= L.E) return;
    const int k = L.edge_kf[e], p = L.edge_point[e];
    const Pose T = pose_load(L.pose[cur] + 7 * (size_t)k);
    const double X[3] = { L.pts[cur][3 * (size_t)p], L.pts[cur][3 * (size_t)p + 1], L.pts[cur][3 * (size_t)p + 2] };
    double x, y, z;
    se3_map(T, X[0], X[1], X[2], x, y, z);
    const bool stereo = !(L.mr[e] < 0.f);
    const bool bad = L.echi[e] > (stereo ? 7.815 : 5.991) || !(z > 0.0);
    if (bad) L.flags[e] = (uint8_t)(L.flags[e] | bit);
}

}   // namespace

// ---------------------------------------------------------------- host side (include/orbx.h: orbx_local_bundle_adjustment)

// orbx_debug_lba_profile: the LaunchProfile (orbx_resident.h) of the calling thread's bundle adjustments (tools/bench_lba.py: the per-kernel
// time per trial).  Slots: LBA_K_*.
enum { LBA_K_INIT, LBA_K_ACTIVE, LBA_K_LINEARIZE, LBA_K_KF, LBA_K_REDUCE, LBA_K_PREP, LBA_K_SCHUR, LBA_K_SOLVE, LBA_K_UPDATE, LBA_K_ERRORS,
       LBA_K_CLASSIFY, LBA_K_FINISH, LBA_K_COUNT };
static thread_local LaunchProfile<LBA_K_COUNT> g_prof;

extern "C" int orbx_debug_lba_profile(int enable, double *ms, int32_t *launches) { return g_prof.entry(enable, ms, launches); }

// has_edge_out / has_point_out: the entry point's own per-edge (edge_flags) or per-point (point_included) output is there, or it has none
static int lba_check(const char *who, const orbx_lba_problem *p, const float *Tcw_out, const float *Xw_out, bool has_edge_out,
                     bool has_point_out, int max_kf, int max_free, int *n_free)
{
    if (!p || !Tcw_out) { orbx_set_error("%s: NULL problem or Tcw_out", who); return ORBX_E_INVALID; }
    if (p->n_kf < 1 || p->n_points < 0 || p->n_edges < 0) { orbx_set_error("%s: n_kf = %d, n_points = %d, n_edges = %d", who, p->n_kf, p->n_points, p->n_edges); return ORBX_E_INVALID; }
    if (p->n_kf > max_kf || p->n_points > (1 << 20) || p->n_edges > (1 << 22)) {
        orbx_set_error("%s: n_kf = %d, n_points = %d, n_edges = %d beyond %d, 2^20, 2^22", who, p->n_kf, p->n_points, p->n_edges, max_kf);
        return ORBX_E_CAPACITY;
    }
    if (!p->Tcw || !p->cam || !p->fixed || (p->n_points && (!p->Xw || !Xw_out || !has_point_out)) ||
        (p->n_edges && (!p->edge_kf || !p->edge_point || !p->x || !p->y || !p->u_right || !p->inv_sigma2 || !has_edge_out))) {
        orbx_set_error("%s: a NULL array", who);
        return ORBX_E_INVALID;
    }
    int nf = 0;
    for (int k = 0; k < p->n_kf; k++) nf += p->fixed[k] == 0;
    std::vector<int32_t> seen((size_t)p->n_kf, -1);
    for (int e = 0; e < p->n_edges; e++) {
        const int k = p->edge_kf[e], q = p->edge_point[e];
        if (k < 0 || k >= p->n_kf || q < 0 || q >= p->n_points) { orbx_set_error("%s: edge %d: keyframe %d or point %d out of range", who, e, k, q); return ORBX_E_INVALID; }
        if (e && q < p->edge_point[e - 1]) { orbx_set_error("%s: edge %d: the edges of a point are not contiguous, or the points not ascending", who, e); return ORBX_E_INVALID; }
        if (seen[k] == q) { orbx_set_error("%s: edge %d: a second edge between point %d and keyframe %d", who, e, q, k); return ORBX_E_INVALID; }
        seen[k] = q;
    }
    if (nf > max_free) { orbx_set_error("%s: %d keyframes with fixed == 0, more than %d", who, nf, max_free); return ORBX_E_CAPACITY; }
    *n_free = nf;
    return ORBX_OK;
}

// orbx_debug_set_lba_solver: the form of the dense solve in the calling thread's orbx_local_bundle_adjustment calls, 0 = k_lba_solve (one
// workgroup), 1 = the panels of orbx_ldlt.hip.  Both give the same bytes.  orbx_bundle_adjustment always takes the panels.
static thread_local int g_lba_solver = 0;

extern "C" int orbx_debug_set_lba_solver(int form)
{
    if (form != 0 && form != 1) { orbx_set_error("orbx_debug_set_lba_solver: form = %d", form); return ORBX_E_INVALID; }
    g_lba_solver = form;
    return ORBX_OK;
}

extern "C" int orbx_debug_ldlt_panel_width(void) { return LDLT_W; }

// what one call has staged: the kernels' argument block and where the download block of the work area holds what
struct LbaStage {
    Lba L;
    size_t w_counts, w_pose, w_point, w_Tcw, w_Xw, w_flags, out;
    const int32_t *point_off;   // the points' edge ranges, in the host blob
};

// the blob (the problem's arrays, the points' edge ranges, the keyframes' edge lists in point order) uploaded, the work area laid out:
// [status | counts | pose_out point_out Tcw_out Xw_out flags] is what comes down, the state follows.  max_rows: the most rows the reduced
// system can have, x_len: the entries of x, delta_mono: Lba::delta_mono.  own_lists: the keyframes' edge lists are compacted between rounds
// (k_lba_active) and need an area of their own; without it kf_act is kf_edges itself, never written.
static int lba_stage(CallCtx *c, const orbx_lba_problem *p, int max_rows, int x_len, double delta_mono, bool own_lists, LbaStage *st)
{
    int rc;
    const size_t K = (size_t)p->n_kf, P = (size_t)p->n_points, E = (size_t)p->n_edges, F = (size_t)max_rows, N = 6 * F;
    BlobCursor b = { nullptr, nullptr, 0 };
    const size_t o_T = b.take(64 * K), o_cam = b.take(20 * K), o_fix = b.take(K), o_X = b.take(12 * P), o_ek = b.take(4 * E), o_ep = b.take(4 * E),
                 o_x = b.take(4 * E), o_y = b.take(4 * E), o_r = b.take(4 * E), o_w = b.take(4 * E), o_po = b.take(4 * (P + 1)), o_ko = b.take(4 * (K + 1)),
                 o_ke = b.take(4 * E);
    const size_t blob = b.o;
    BlobCursor w = { nullptr, nullptr, 0 };
    const size_t w_status = w.take(64), w_counts = w.take(16), w_pose = w.take(96 * K), w_point = w.take(24 * P), w_Tcw = w.take(64 * K),
                 w_Xw = w.take(12 * P), w_flags = w.take(E);
    const size_t out = w.o;
    const size_t w_p0 = w.take(56 * K), w_p1 = w.take(56 * K), w_q0 = w.take(24 * P), w_q1 = w.take(24 * P), w_echi = w.take(8 * E), w_W = w.take(144 * E),
                 w_pact = w.take(P), w_Hll = w.take(48 * P), w_bl = w.take(24 * P), w_Dinv = w.take(48 * P), w_db = w.take(24 * P), w_xl = w.take(24 * P),
                 w_chi = w.take(8 * P), w_kact = w.take(own_lists ? 4 * E : 0), w_kcnt = w.take(4 * K), w_row = w.take(4 * K), w_rowkf = w.take(4 * K),
                 w_Hpp = w.take(168 * F), w_bp = w.take(48 * F), w_S = w.take(8 * N * N), w_bS = w.take(8 * N), w_xv = w.take(8 * (size_t)x_len);
    if ((rc = call_reserve(c, blob, w.o, out))) return rc;
    uint8_t *h = c->h_blob;
    memcpy(h + o_T, p->Tcw, 64 * K); memcpy(h + o_cam, p->cam, 20 * K); memcpy(h + o_fix, p->fixed, K);
    if (P) memcpy(h + o_X, p->Xw, 12 * P);
    if (E) {
        memcpy(h + o_ek, p->edge_kf, 4 * E); memcpy(h + o_ep, p->edge_point, 4 * E); memcpy(h + o_x, p->x, 4 * E); memcpy(h + o_y, p->y, 4 * E);
        memcpy(h + o_r, p->u_right, 4 * E); memcpy(h + o_w, p->inv_sigma2, 4 * E);
    }
    int32_t *po = (int32_t *)(h + o_po), *ko = (int32_t *)(h + o_ko), *ke = (int32_t *)(h + o_ke);
    memset(po, 0, 4 * (P + 1)); memset(ko, 0, 4 * (K + 1));
    for (size_t e = 0; e < E; e++) { po[p->edge_point[e] + 1]++; ko[p->edge_kf[e] + 1]++; }
    for (size_t q = 0; q < P; q++) po[q + 1] += po[q];
    for (size_t k = 0; k < K; k++) ko[k + 1] += ko[k];
    {
        std::vector<int32_t> fill(ko, ko + K);
        for (size_t e = 0; e < E; e++) ke[fill[p->edge_kf[e]]++] = (int32_t)e;
    }
    if ((rc = call_upload(c, blob))) return rc;

    Lba &L = st->L;
    memset(&L, 0, sizeof L);
    L.K = p->n_kf; L.P = p->n_points; L.E = p->n_edges; L.nx = x_len; L.delta_mono = delta_mono;
    uint8_t *d = c->d_blob, *wk = c->d_work;
    L.Tcw = (const float *)(d + o_T); L.cam = (const float *)(d + o_cam); L.fixed = d + o_fix; L.Xw = (const float *)(d + o_X);
    L.edge_kf = (const int32_t *)(d + o_ek); L.edge_point = (const int32_t *)(d + o_ep);
    L.mx = (const float *)(d + o_x); L.my = (const float *)(d + o_y); L.mr = (const float *)(d + o_r); L.isig = (const float *)(d + o_w);
    L.point_off = (const int32_t *)(d + o_po); L.kf_off = (const int32_t *)(d + o_ko); L.kf_edges = (const int32_t *)(d + o_ke);
    L.status = (double *)(wk + w_status); L.counts = (int32_t *)(wk + w_counts);
    L.pose_out = (double *)(wk + w_pose); L.point_out = (double *)(wk + w_point); L.Tcw_out = (float *)(wk + w_Tcw); L.Xw_out = (float *)(wk + w_Xw);
    L.flags = wk + w_flags;
    L.pose[0] = (double *)(wk + w_p0); L.pose[1] = (double *)(wk + w_p1); L.pts[0] = (double *)(wk + w_q0); L.pts[1] = (double *)(wk + w_q1);
    L.echi = (double *)(wk + w_echi); L.W = (double *)(wk + w_W); L.pactive = wk + w_pact;
    L.Hll = (double *)(wk + w_Hll); L.bl = (double *)(wk + w_bl); L.Dinv = (double *)(wk + w_Dinv); L.db = (double *)(wk + w_db);
    L.xl = (double *)(wk + w_xl); L.chi_pt = (double *)(wk + w_chi);
    L.kf_act = own_lists ? (int32_t *)(wk + w_kact) : const_cast<int32_t *>(L.kf_edges); L.kf_cnt = (int32_t *)(wk + w_kcnt); L.row = (int32_t *)(wk + w_row); L.rowkf = (int32_t *)(wk + w_rowkf);
    L.Hpp = (double *)(wk + w_Hpp); L.bp = (double *)(wk + w_bp); L.S = (double *)(wk + w_S); L.bS = (double *)(wk + w_bS); L.x = (double *)(wk + w_xv);
    st->w_counts = w_counts; st->w_pose = w_pose; st->w_point = w_point; st->w_Tcw = w_Tcw; st->w_Xw = w_Xw; st->w_flags = w_flags; st->out = out;
    st->point_off = po;
    return ORBX_OK;
}

// the Levenberg loop of one call: the state that outlives a round, and optimize() = SparseOptimizer::optimize(max_it) on the active set
struct LbaRun {
    CallCtx *c, *pc;       // pc: the context while orbx_debug_lba_profile is on, else nullptr
    const Lba &L;
    size_t w_counts;
    const volatile unsigned char *stop;
    int dbg, solver;
    int cur = 0, trials_total = 0;
    bool evaluated = false;

    // a thread per keyframe and point, per point, per edge, per anything k_lba_init clears
    unsigned g_vert() const { return grid256(std::max(L.K, L.P)); }
    unsigned g_pts() const { return grid256(L.P); }
    unsigned g_edges() const { return grid256(L.E); }
    unsigned g_all() const { return grid256(std::max(std::max(L.K, L.P), std::max(L.E, L.nx))); }

    bool stop_up() const { return (stop && *stop) || (dbg >= 0 && trials_total >= dbg); }
    int fetch_status() { return call_fetch(c, w_counts + 16); }
    const int32_t *counts() const { return (const int32_t *)((const uint8_t *)c->h_out + w_counts); }   // rows, active points, behind fetch_status

    void init() { g_prof.launch(LBA_K_INIT, pc, [&] { hipLaunchKernelGGL(k_lba_init, dim3(g_all()), dim3(256), 0, c->stream, L); }); }
    void finish() { g_prof.launch(LBA_K_FINISH, pc, [&] { hipLaunchKernelGGL(k_lba_finish, dim3(g_vert()), dim3(256), 0, c->stream, L, cur); }); }

    // the launches of one linearisation and of one trial under lm_host_loop (orbx_lm.h); without an active point no iteration runs
    LmRun optimize(int rows, int npts, int max_it, int robust)
    {
        hipStream_t s = c->stream;
        const LmRun r = lm_host_loop(
            npts > 0 ? max_it : 0, 0.0,
            [&] {
                g_prof.launch(LBA_K_LINEARIZE, pc, [&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lba_points<true>), dim3(g_pts()), dim3(256), 0, s, L, cur, robust); });
                if (rows) g_prof.launch(LBA_K_KF, pc, [&] { hipLaunchKernelGGL(k_lba_kf, dim3(rows), dim3(256), 0, s, L, cur, robust); });
                g_prof.launch(LBA_K_REDUCE, pc, [&] { hipLaunchKernelGGL(k_lba_reduce, dim3(1), dim3(1024), 0, s, L, 0, 0.0); });
                return fetch_status();
            },
            [&](double lambda) {
                g_prof.launch(LBA_K_PREP, pc, [&] { hipLaunchKernelGGL(k_lba_prep, dim3(g_pts()), dim3(256), 0, s, L, lambda); });
                if (rows) {
                    g_prof.launch(LBA_K_SCHUR, pc, [&] { hipLaunchKernelGGL(k_lba_schur, dim3(rows, rows), dim3(256), 0, s, L, lambda); });
                    g_prof.launch(LBA_K_SOLVE, pc, [&] {
                        if (solver == 0) hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(1024), 0, s, L);
                        else orbx_ldlt_panel_launch(L.S, L.bS, L.x, L.status + 3, 6 * rows, s);
                    });
                }
                g_prof.launch(LBA_K_UPDATE, pc, [&] { hipLaunchKernelGGL(k_lba_update, dim3(g_vert()), dim3(256), 0, s, L, cur); });
                g_prof.launch(LBA_K_ERRORS, pc, [&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lba_points<false>), dim3(g_pts()), dim3(256), 0, s, L, 1 - cur, robust); });
                g_prof.launch(LBA_K_REDUCE, pc, [&] { hipLaunchKernelGGL(k_lba_reduce, dim3(1), dim3(1024), 0, s, L, 1, lambda); });
                const int rc = fetch_status();
                if (!rc) trials_total++;
                return rc;
            },
            [&] { return (const double *)c->h_out; }, [&] { return stop_up(); }, [&] { cur = 1 - cur; });   // discardTop(): the trial copy is the estimate
        evaluated = evaluated || r.evaluated;
        return r;
    }
};

// the download block fetched, and what both entry points hand back from it
static int lba_deliver(CallCtx *c, const LbaStage &st, float *Tcw_out, float *Xw_out, double *pose_out, double *point_out)
{
    const int rc = call_fetch(c, st.out);
    if (rc) return rc;
    const size_t K = (size_t)st.L.K, P = (size_t)st.L.P;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    memcpy(Tcw_out, ho + st.w_Tcw, 64 * K);
    if (P) memcpy(Xw_out, ho + st.w_Xw, 12 * P);
    if (pose_out) memcpy(pose_out, ho + st.w_pose, 96 * K);
    if (point_out && P) memcpy(point_out, ho + st.w_point, 24 * P);
    return ORBX_OK;
}

extern "C" int orbx_local_bundle_adjustment(int device, const orbx_lba_problem *p, const orbx_lba_options *opt, float *Tcw_out, float *Xw_out,
                                            uint8_t *edge_flags, double *pose_out, double *point_out, orbx_lba_report *report)
{
    const char *who = "orbx_local_bundle_adjustment";
    int n_free = 0;
    int rc = lba_check(who, p, Tcw_out, Xw_out, edge_flags != nullptr, true, 1024, 256, &n_free);
    if (rc) return rc;
    orbx_lba_report rep;
    memset(&rep, 0, sizeof rep);
    const volatile unsigned char *stop = opt ? opt->stop : nullptr;
    if (stop && *stop) {   // :736-738
        rep.stopped = 1;
        if (report) *report = rep;
        return ORBX_OK;
    }
    CallCtx *c, *pc;
    if ((rc = orbx_call_ctx(device, &c))) return rc;
    LbaStage st;
    if ((rc = lba_stage(c, p, n_free, 1536, (double)(float)sqrt(5.991), true, &st))) return rc;   // thHuberMono, :650
    if ((rc = g_prof.ctx(c, &pc))) return rc;
    const Lba &L = st.L;
    const size_t E = (size_t)p->n_edges;
    hipStream_t s = c->stream;
    LbaRun run = { c, pc, L, st.w_counts, stop, opt ? opt->debug_stop_at_trial : -1, g_lba_solver };
    const unsigned g_pts = run.g_pts(), g_edges = run.g_edges();

    run.init();
    for (int round = 0; round < 2; round++) {
        g_prof.launch(LBA_K_ACTIVE, pc, [&] { hipLaunchKernelGGL(k_lba_active, dim3(1), dim3(1024), 0, s, L); });
        if ((rc = run.fetch_status())) return rc;
        const int rows = run.counts()[0], npts = run.counts()[1];
        rep.n_active_kf[round] = rows; rep.n_active_points[round] = npts;
        const LmRun r = run.optimize(rows, npts, round == 0 ? 5 : 10, round == 0);
        if (r.rc) return r.rc;
        rep.iterations[round] = r.iterations; rep.trials[round] = r.trials; rep.chi2[round] = r.chi2; rep.lambda[round] = r.lambda;
        if (round == 0) {
            if (run.stop_up()) rep.stopped = 2;   // :745-747
            if (!run.evaluated && E) {   // stopped before any evaluation: the errors at the start estimates (the reference reads uninitialised memory)
                g_prof.launch(LBA_K_ERRORS, pc, [&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lba_points<false>), dim3(g_pts), dim3(256), 0, s, L, run.cur, 1); });
                run.evaluated = true;
            }
            if (E) g_prof.launch(LBA_K_CLASSIFY, pc, [&] { hipLaunchKernelGGL(k_lba_classify, dim3(g_edges), dim3(256), 0, s, L, run.cur, 1); });
            if (rep.stopped) break;
        } else if (run.stop_up()) rep.stopped = 3;
    }
    if (E) g_prof.launch(LBA_K_CLASSIFY, pc, [&] { hipLaunchKernelGGL(k_lba_classify, dim3(g_edges), dim3(256), 0, s, L, run.cur, 2); });
    run.finish();
    if ((rc = lba_deliver(c, st, Tcw_out, Xw_out, pose_out, point_out))) return rc;
    const uint8_t *flags = (const uint8_t *)c->h_out + st.w_flags;
    for (size_t e = 0; e < E; e++) {
        const uint8_t f = flags[e];
        edge_flags[e] = f; rep.n_level1 += f & 1; rep.n_erase += (f >> 1) & 1;
    }
    if (report) *report = rep;
    return ORBX_OK;
}

// ---------------------------------------------------------------- include/orbx.h: orbx_bundle_adjustment
// Optimizer::BundleAdjustment (reference src/Optimizer.cc:48-281) between :67 and :232: the same staging, linearisation and trial as above,
// ONE round on every edge, the reduced system solved in panels (orbx_ldlt.hip).  k_lba_schur runs on all row pairs: a pair of keyframes
// without a common point costs a workgroup that walks row i's edges through a binary search each and writes 36 zeros twice.

extern "C" int orbx_bundle_adjustment(int device, const orbx_lba_problem *p, const orbx_ba_options *opt, float *Tcw_out, float *Xw_out,
                                      uint8_t *point_included, double *pose_out, double *point_out, orbx_ba_report *report)
{
    const char *who = "orbx_bundle_adjustment";
    int n_free = 0;
    int rc = lba_check(who, p, Tcw_out, Xw_out, true, point_included != nullptr, 4096, 2048, &n_free);
    if (rc) return rc;
    const int iterations = opt ? opt->iterations : 10, robust = opt ? opt->robust != 0 : 1;
    if (iterations < 0) { orbx_set_error("%s: iterations = %d", who, iterations); return ORBX_E_INVALID; }
    orbx_ba_report rep;
    memset(&rep, 0, sizeof rep);
    const volatile unsigned char *stop = opt ? opt->stop : nullptr;
    const bool up_on_entry = stop && *stop;   // setForceStopFlag (:64-65): optimize() then runs no iteration, the recovery still does
    CallCtx *c, *pc;
    if ((rc = orbx_call_ctx(device, &c))) return rc;
    int max_rows = 0;   // the free keyframes with an edge: S is dense and sized by the keyframes that get a row
    {
        std::vector<uint8_t> seen((size_t)p->n_kf, 0);
        for (int e = 0; e < p->n_edges; e++) seen[p->edge_kf[e]] = 1;
        for (int k = 0; k < p->n_kf; k++) max_rows += seen[k] && !p->fixed[k];
    }
    LbaStage st;
    // thHuber2D is sqrt(5.99) here (:101), not LocalBundleAdjustment's 5.991; every edge stays at level 0, so the edge lists are the uploaded ones
    if ((rc = lba_stage(c, p, max_rows, std::max(6 * max_rows, 1), (double)(float)sqrt(5.99), false, &st))) return rc;
    if ((rc = g_prof.ctx(c, &pc))) return rc;
    const Lba &L = st.L;
    hipStream_t s = c->stream;
    LbaRun run = { c, pc, L, st.w_counts, stop, opt ? opt->debug_stop_at_trial : -1, 1 };

    run.init();
    g_prof.launch(LBA_K_ACTIVE, pc, [&] {
        hipLaunchKernelGGL(k_gba_active, dim3(run.g_vert()), dim3(256), 0, s, L);
        hipLaunchKernelGGL(k_gba_rows, dim3(1), dim3(1024), 0, s, L);
    });
    if ((rc = run.fetch_status())) return rc;
    rep.n_active_kf = run.counts()[0]; rep.n_active_points = run.counts()[1];
    if (up_on_entry) rep.stopped = 1;
    else {
        const LmRun r = run.optimize(rep.n_active_kf, rep.n_active_points, iterations, robust);
        if (r.rc) return r.rc;
        rep.iterations = r.iterations; rep.trials = r.trials; rep.chi2 = r.chi2; rep.lambda = r.lambda; rep.lambda_init = r.lambda_init;
        if (run.stop_up()) rep.stopped = 2;
    }
    run.finish();
    if ((rc = lba_deliver(c, st, Tcw_out, Xw_out, pose_out, point_out))) return rc;
    for (size_t q = 0; q < (size_t)p->n_points; q++) point_included[q] = st.point_off[q + 1] > st.point_off[q];
    if (report) *report = rep;
    return ORBX_OK;
}

// ---------------------------------------------------------------- include/orbx.h: orbx_debug_ldlt_solve

extern "C" int orbx_debug_ldlt_solve(int device, int n, const double *S, const double *b, double *x, int form, int *ok)
{
    const char *who = "orbx_debug_ldlt_solve";
    if (!S || !b || !x || !ok) { orbx_set_error("%s: a NULL argument", who); return ORBX_E_INVALID; }
    if (n < 1 || (form != 0 && form != 1)) { orbx_set_error("%s: n = %d, form = %d", who, n, form); return ORBX_E_INVALID; }
    if (n > (form == 0 ? 1536 : 6 * 2048)) { orbx_set_error("%s: n = %d beyond %d", who, n, form == 0 ? 1536 : 6 * 2048); return ORBX_E_CAPACITY; }
    int rc;
    CallCtx *c;
    if ((rc = orbx_call_ctx(device, &c))) return rc;
    // k_lba_solve takes its size as 6 x a row count: form 0 solves diag(S, I) of the next multiple of 6.  The added rows of L are exact
    // zeros and the added unknowns +0, so every operation on the first n rows has the operands it has without them.
    const size_t N = (size_t)n, M = form == 0 ? (N + 5) / 6 * 6 : N;
    BlobCursor bl = { nullptr, nullptr, 0 };
    const size_t o_S = bl.take(8 * M * M), o_b = bl.take(8 * M), o_x = bl.take(8 * M), o_cnt = bl.take(16);
    BlobCursor w = { nullptr, nullptr, 0 };
    const size_t w_status = w.take(64), w_x = w.take(8 * M);
    if ((rc = call_reserve(c, bl.o, w.o, w.o))) return rc;
    uint8_t *h = c->h_blob;
    double *hS = (double *)(h + o_S), *hb = (double *)(h + o_b), *hx = (double *)(h + o_x);
    memset(hS, 0, 8 * M * M); memset(hb, 0, 8 * M); memset(hx, 0, 8 * M);
    for (size_t i = 0; i < N; i++) memcpy(hS + i * M, S + i * N, 8 * N);
    for (size_t i = N; i < M; i++) hS[i * M + i] = 1.0;
    memcpy(hb, b, 8 * N); memcpy(hx, x, 8 * N);
    ((int32_t *)(h + o_cnt))[0] = (int32_t)(M / 6);
    if ((rc = call_upload(c, bl.o))) return rc;
    Lba L;
    memset(&L, 0, sizeof L);
    L.S = (double *)(c->d_blob + o_S); L.bS = (double *)(c->d_blob + o_b); L.counts = (int32_t *)(c->d_blob + o_cnt);
    L.status = (double *)(c->d_work + w_status); L.x = (double *)(c->d_work + w_x);
    ORBX_HIP(hipMemcpyAsync(L.x, c->d_blob + o_x, 8 * M, hipMemcpyDeviceToDevice, c->stream));
    if (form == 0) hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(1024), 0, c->stream, L);
    else orbx_ldlt_panel_launch(L.S, L.bS, L.x, L.status + 3, n, c->stream);
    if ((rc = call_fetch(c, w.o))) return rc;
    *ok = ((const double *)c->h_out)[3] != 0.0;
    memcpy(x, (const uint8_t *)c->h_out + w_x, 8 * N);
    return ORBX_OK;
}

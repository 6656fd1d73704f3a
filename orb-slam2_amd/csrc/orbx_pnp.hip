// orbx_pnp.hip — k_pnp: every hypothesis of PnPsolver's EPnP RANSAC (reference src/PnPsolver.cc:193-249, 271-350, 386-961) for every job
// of one call.  One wave64 per (job, hypothesis), four waves per workgroup.  A wave finds its job by bisecting the jobs' first-wave
// numbers (at most 64) and runs compute_pose twice at most: on the four sampled correspondences, every lane summing the four serially,
// and -- when the row reaches min_inliers -- on the row's own inliers (Refine), lane l summing the members i = l (mod 64) and a xor
// butterfly closing every sum.  Everything of EPnP that is not a sum over correspondences is lane-uniform fp64 in registers, except the
// matrices of the one Jacobi SVD routine that restates every OpenCV call: they live in LDS (A stacked on V, 24 x 12 doubles per wave), the
// disjoint pivots of a round-robin round go side by side on groups of eight lanes, and a rotation's rows are spread over the eight.
// CheckInliers is one lane per correspondence, 64 at a time; __ballot of the predicate IS the mask word.  No atomics, no scratch.
// The arithmetic is restated in include/orbx.h (orbx_pnp_hypotheses) and, in numpy, in tests/pnp_model.py.  Behind the kernel: the
// refusals, the staging (one blob up, one block down) and the delivery of the two calls (pnp_check, pnp_run and the entry points).
#include "orbx_resident.h"
#include "orbx_wave.h"

// One job of k_pnp.  Every pointer is a device address.  first = the number of this job's first wave, as in k_sim3.
struct PnpJob {
    int n, n_hyp, min_inliers, first;
    const float *P3Dw, *P2D, *max_err;
    const int32_t *samples;
    int32_t *n_inliers; double *Rt; uint64_t *bits;
    int32_t *n_refined; double *Rt_refined; uint64_t *refined_bits;
    double K[4];
};

namespace {

#define PNP_LD 12                  // row stride of B
#define PNP_EPS 0x1p-49            // the skip test of a pivot
#define PNP_CUT 0x1p-51            // the zero cut of a solve, times the sum of the singular values

// what one wave keeps in LDS: B = A (m rows) stacked on V (n rows), the four vectors compute_L_6x10 and compute_ccs read, l_6x10, the
// singular values and their order
struct PnpLds {
    double B[24 * PNP_LD];
    double vt[4][12];
    double L[60];
    double w[12];
    int order[12];
    int pad[4];
};

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// The one-sided cyclic Jacobi of the contract on the m x n matrix in rows 0 .. m-1 of B; rows m .. m+n-1 become V.  Afterwards the
// columns of A are orthogonal, w[j] = their norms.
__device__ __forceinline__ void svd(PnpLds &S, const int m, const int n, const int lane)
{
    double *B = S.B;
    for (int e = lane; e < n * n; e += 64) B[(m + e / n) * PNP_LD + e % n] = (e / n == e % n) ? 1.0 : 0.0;
    wsync();
    const int N = (n + 1) & ~1, half = N >> 1, slot = lane >> 3, sub = lane & 7, rows = m + n;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        for (int r = 0; r < N - 1; r++) {
            bool rotate = false;
            int p = 0, q = 0;
            double c = 0.0, s = 0.0;
            if (slot < half) {
                const int a = slot == 0 ? N - 1 : (r + slot) % (N - 1);
                const int b = slot == 0 ? r : (r + (N - 1) - slot) % (N - 1);
                p = a < b ? a : b;
                q = a < b ? b : a;
                if (q < n) {
                    double al = 0.0, be = 0.0, g = 0.0;
                    for (int i = 0; i < m; i++) {
                        const double x = B[i * PNP_LD + p], y = B[i * PNP_LD + q];
                        al = al + x * x;
                        be = be + y * y;
                        g = g + x * y;
                    }
                    if (!(fabs(g) <= PNP_EPS * sqrt(al * be))) {
                        rotate = true;
                        const double g2 = g * 2.0, beta = al - be, gamma = sqrt(g2 * g2 + beta * beta);
                        if (beta < 0.0) {
                            const double delta = (gamma - beta) * 0.5;
                            s = sqrt(delta / gamma);
                            c = g2 / ((gamma * s) * 2.0);
                        } else {
                            c = sqrt((gamma + beta) / (gamma * 2.0));
                            s = g2 / ((gamma * c) * 2.0);
                        }
                    }
                }
            }
            wsync();
            if (rotate) {
                for (int rr = sub; rr < rows; rr += 8) {
                    const double x = B[rr * PNP_LD + p], y = B[rr * PNP_LD + q];
                    B[rr * PNP_LD + p] = c * x + s * y;
                    B[rr * PNP_LD + q] = c * y - s * x;
                }
            }
            changed |= __ballot(rotate) != 0;
            wsync();
        }
        if (!changed) break;
    }
    if (lane < n) {
        double s2 = 0.0;
        for (int i = 0; i < m; i++) { const double x = B[i * PNP_LD + lane]; s2 = s2 + x * x; }
        S.w[lane] = sqrt(s2);
    }
    wsync();
}

// order[r] = the column of the r-th largest w, of equal ones the earlier index first; the same in every lane
__device__ __forceinline__ void sort_desc(PnpLds &S, const int n)
{
    unsigned used = 0;
    for (int r = 0; r < n; r++) {
        int best = -1;
        double wb = 0.0;
        for (int j = 0; j < n; j++) {
            if ((used >> j) & 1) continue;
            const double wj = S.w[j];
            if (best < 0 || wj > wb) { best = j; wb = wj; }
        }
        S.order[r] = best;
        used |= 1u << best;
    }
    wsync();
}

// x = V diag(1 / w) U^T b behind svd(S, M, n), n <= NMAX; the same in every lane
template <int M, int NMAX>
__device__ __forceinline__ void solve(const PnpLds &S, const int n, const double (&b)[M], double (&x)[NMAX])
{
    double sum = 0.0;
    for (int k = 0; k < n; k++) sum = sum + S.w[k];
    const double thr = sum * PNP_CUT;
#pragma unroll
    for (int j = 0; j < NMAX; j++) x[j] = 0.0;
    for (int k = 0; k < n; k++) {
        const double wk = S.w[k];
        if (!(wk > thr)) continue;
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < M; i++) t = t + S.B[i * PNP_LD + k] * b[i];
        t = (t / wk) / wk;
#pragma unroll
        for (int j = 0; j < NMAX; j++) if (j < n) x[j] = x[j] + S.B[(M + j) * PNP_LD + k] * t;
    }
}

// qr_solve (:871-961) on the 6 x 4 system of gauss_newton; x keeps its value when a pivot column is zero
__device__ __forceinline__ void qr_solve(double (&A)[6][4], double (&b)[6], double (&x)[4])
{
    double A1[4], A2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double eta = fabs(A[k][k]);
#pragma unroll
        for (int i = k; i < 5; i++) { const double elt = fabs(A[i][k]); if (eta < elt) eta = elt; }   // never the last row
        if (eta == 0.0) return;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
#pragma unroll
        for (int i = k; i < 6; i++) { A[i][k] = A[i][k] * inv_eta; sum = sum + A[i][k] * A[i][k]; }
        double sigma = sqrt(sum);
        if (A[k][k] < 0.0) sigma = -sigma;
        A[k][k] = A[k][k] + sigma;
        A1[k] = sigma * A[k][k];
        A2[k] = (-eta) * sigma;
#pragma unroll
        for (int j = k + 1; j < 4; j++) {
            double sm = 0.0;
#pragma unroll
            for (int i = k; i < 6; i++) sm = sm + A[i][k] * A[i][j];
            const double tau = sm / A1[k];
#pragma unroll
            for (int i = k; i < 6; i++) A[i][j] = A[i][j] - tau * A[i][k];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double tau = 0.0;
#pragma unroll
        for (int i = j; i < 6; i++) tau = tau + A[i][j] * b[i];
        tau = tau / A1[j];
#pragma unroll
        for (int i = j; i < 6; i++) b[i] = b[i] - tau * A[i][j];
    }
    x[3] = b[3] / A2[3];
#pragma unroll
    for (int i = 2; i >= 0; i--) {
        double sum = 0.0;
#pragma unroll
        for (int j = i + 1; j < 4; j++) sum = sum + A[i][j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
}

// the correspondences compute_pose runs on: the four of a sample row, in its order and summed serially by every lane, or the set bits of
// a mask, lane l taking i = l (mod 64) in rising order
struct Members {
    bool serial;
    int cnt, iters, first;
    const int32_t *sm;
    const volatile uint64_t *bits;   // stored by lane 0 of this wave, read back behind a fence
};

template <class F>
__device__ __forceinline__ void for_members(const Members &M, const int lane, F f)
{
    for (int it = 0; it < M.iters; it++) {
        int idx;
        bool act;
        if (M.serial) { idx = M.sm[it]; act = true; }
        else { idx = it * 64 + lane; act = (M.bits[it] >> lane) & 1; }
        if (act) f(idx);
    }
}

struct Corr { double p0, p1, p2, u, v; };

__device__ __forceinline__ Corr corr_load(const PnpJob &J, const int i)
{
    Corr c;
    c.p0 = (double)J.P3Dw[3 * i]; c.p1 = (double)J.P3Dw[3 * i + 1]; c.p2 = (double)J.P3Dw[3 * i + 2];
    c.u = (double)J.P2D[2 * i]; c.v = (double)J.P2D[2 * i + 1];
    return c;
}

// compute_barycentric_coordinates (:434-444) of one correspondence
__device__ __forceinline__ void alphas_of(const Corr &c, const double (&c0)[3], const double (&ci)[9], double (&a)[4])
{
    const double d0 = c.p0 - c0[0], d1 = c.p1 - c0[1], d2 = c.p2 - c0[2];
#pragma unroll
    for (int j = 0; j < 3; j++) a[1 + j] = (ci[3 * j] * d0 + ci[3 * j + 1] * d1) + ci[3 * j + 2] * d2;
    a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

// compute_pose (:488-536) on the members M -> R, t
__device__ __forceinline__ void compute_pose(const PnpJob &J, const Members &M, PnpLds &S, const int lane, double (&Rb)[3][3], double (&tb)[3])
{
    const double fu = J.K[0], fv = J.K[1], uc = J.K[2], vc = J.K[3];
    const double nc = (double)M.cnt;
    double *B = S.B;

    // ---- choose_control_points (:386-420)
    double c0[3] = { 0.0, 0.0, 0.0 };
    for_members(M, lane, [&](int i) {
        const Corr c = corr_load(J, i);
        c0[0] = c0[0] + c.p0; c0[1] = c0[1] + c.p1; c0[2] = c0[2] + c.p2;
    });
#pragma unroll
    for (int j = 0; j < 3; j++) { if (!M.serial) c0[j] = wave_sum(c0[j]); c0[j] = c0[j] / nc; }
    double ptp[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };   // 00 01 02 11 12 22
    for_members(M, lane, [&](int i) {
        const Corr c = corr_load(J, i);
        const double d0 = c.p0 - c0[0], d1 = c.p1 - c0[1], d2 = c.p2 - c0[2];
        ptp[0] = ptp[0] + d0 * d0; ptp[1] = ptp[1] + d0 * d1; ptp[2] = ptp[2] + d0 * d2;
        ptp[3] = ptp[3] + d1 * d1; ptp[4] = ptp[4] + d1 * d2; ptp[5] = ptp[5] + d2 * d2;
    });
    if (!M.serial) {
#pragma unroll
        for (int j = 0; j < 6; j++) ptp[j] = wave_sum(ptp[j]);
    }
    wsync();
    if (lane == 0) {
        B[0] = ptp[0]; B[1] = ptp[1]; B[2] = ptp[2];
        B[PNP_LD] = ptp[1]; B[PNP_LD + 1] = ptp[3]; B[PNP_LD + 2] = ptp[4];
        B[2 * PNP_LD] = ptp[2]; B[2 * PNP_LD + 1] = ptp[4]; B[2 * PNP_LD + 2] = ptp[5];
    }
    wsync();
    svd(S, 3, 3, lane);
    sort_desc(S, 3);
    double cws[4][3];
#pragma unroll
    for (int j = 0; j < 3; j++) cws[0][j] = c0[j];
#pragma unroll
    for (int i = 1; i < 4; i++) {
        const int o = S.order[i - 1];
        const double k = sqrt(S.w[o] / nc);
#pragma unroll
        for (int j = 0; j < 3; j++) cws[i][j] = c0[j] + k * B[(3 + j) * PNP_LD + o];
    }

    // ---- compute_barycentric_coordinates (:422-433): CC_inv, column by column
    wsync();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 1; j < 4; j++) B[i * PNP_LD + j - 1] = cws[j][i] - cws[0][i];
    }
    wsync();
    svd(S, 3, 3, lane);
    double ci[9];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double e[3] = { j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0 };
        double x[3];
        solve<3, 3>(S, 3, e, x);
#pragma unroll
        for (int i = 0; i < 3; i++) ci[3 * i + j] = x[i];
    }

    // ---- fill_M and MtM (:447-462, :503): the rows of one control point per pass
    wsync();
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
        double acc[3][12];
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int k = 0; k < 12; k++) acc[j][k] = 0.0;
        for_members(M, lane, [&](int i) {
            const Corr c = corr_load(J, i);
            double a[4], M1[12], M2[12];
            alphas_of(c, c0, ci, a);
            const double du = uc - c.u, dv = vc - c.v;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                M1[3 * q] = a[q] * fu; M1[3 * q + 1] = 0.0; M1[3 * q + 2] = a[q] * du;
                M2[3 * q] = 0.0; M2[3 * q + 1] = a[q] * fv; M2[3 * q + 2] = a[q] * dv;
            }
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int k = 3 * blk + j; k < 12; k++) acc[j][k] = (acc[j][k] + M1[3 * blk + j] * M1[k]) + M2[3 * blk + j] * M2[k];
        });
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int k = 3 * blk + j; k < 12; k++) {
                const double v = M.serial ? acc[j][k] : wave_sum(acc[j][k]);
                if (lane == 0) { B[(3 * blk + j) * PNP_LD + k] = v; B[k * PNP_LD + 3 * blk + j] = v; }
            }
    }
    wsync();
    svd(S, 12, 12, lane);
    sort_desc(S, 12);
    if (lane < 48) S.vt[lane / 12][lane % 12] = B[(12 + lane % 12) * PNP_LD + S.order[11 - lane / 12]];
    wsync();

    // ---- compute_L_6x10 (:771-811), one row per lane, and compute_rho (:813-821)
    if (lane < 6) {
        const int a = lane < 3 ? 0 : lane < 5 ? 1 : 2, b = lane < 3 ? lane + 1 : lane < 5 ? lane - 1 : 3;
        double dv[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) dv[i][k] = S.vt[i][3 * a + k] - S.vt[i][3 * b + k];
        double *row = S.L + 10 * lane;
#define PNP_DD(i, j) dot3(dv[i][0], dv[i][1], dv[i][2], dv[j][0], dv[j][1], dv[j][2])
        row[0] = PNP_DD(0, 0);
        row[1] = 2.0 * PNP_DD(0, 1);
        row[2] = PNP_DD(1, 1);
        row[3] = 2.0 * PNP_DD(0, 2);
        row[4] = 2.0 * PNP_DD(1, 2);
        row[5] = PNP_DD(2, 2);
        row[6] = 2.0 * PNP_DD(0, 3);
        row[7] = 2.0 * PNP_DD(1, 3);
        row[8] = 2.0 * PNP_DD(2, 3);
        row[9] = PNP_DD(3, 3);
#undef PNP_DD
    }
    wsync();
    double rho[6];
    {
        int e = 0;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a + 1; b < 4; b++) {
                const double d0 = cws[a][0] - cws[b][0], d1 = cws[a][1] - cws[b][1], d2 = cws[a][2] - cws[b][2];
                rho[e++] = (d0 * d0 + d1 * d1) + d2 * d2;
            }
    }

    // the first correspondence, the only one solve_for_sign looks at
    double a_first[4];
    alphas_of(corr_load(J, M.first), c0, ci, a_first);

    double err_best = 0.0;
    for (int ap = 0; ap < 3; ap++) {
        // ---- find_betas_approx_1 / _2 / _3 (:678-769)
        const int ncol = ap == 0 ? 4 : ap == 1 ? 3 : 5;
        if (lane < 6 * ncol) {
            const int r = lane / ncol, c = lane % ncol;
            const int src = ap == 0 ? (c == 2 ? 3 : c == 3 ? 6 : c) : c;
            B[r * PNP_LD + c] = S.L[10 * r + src];
        }
        wsync();
        svd(S, 6, ncol, lane);
        double bs[5], betas[4];
        solve<6, 5>(S, ncol, rho, bs);
        if (ap == 0) {
            if (bs[0] < 0.0) {
                betas[0] = sqrt(-bs[0]);
                betas[1] = (-bs[1]) / betas[0]; betas[2] = (-bs[2]) / betas[0]; betas[3] = (-bs[3]) / betas[0];
            } else {
                betas[0] = sqrt(bs[0]);
                betas[1] = bs[1] / betas[0]; betas[2] = bs[2] / betas[0]; betas[3] = bs[3] / betas[0];
            }
        } else {
            if (bs[0] < 0.0) {
                betas[0] = sqrt(-bs[0]);
                betas[1] = (bs[2] < 0.0) ? sqrt(-bs[2]) : 0.0;
            } else {
                betas[0] = sqrt(bs[0]);
                betas[1] = (bs[2] > 0.0) ? sqrt(bs[2]) : 0.0;
            }
            if (bs[1] < 0.0) betas[0] = -betas[0];
            betas[2] = ap == 2 ? bs[3] / betas[0] : 0.0;
            betas[3] = 0.0;
        }

        // ---- gauss_newton (:823-869)
        double x[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int it = 0; it < 5; it++) {
            double A[6][4], bb[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double *l = S.L + 10 * i;
                const double l0 = l[0], l1 = l[1], l2 = l[2], l3 = l[3], l4 = l[4], l5 = l[5], l6 = l[6], l7 = l[7], l8 = l[8], l9 = l[9];
                const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
                A[i][0] = (((2.0 * l0) * b0 + l1 * b1) + l3 * b2) + l6 * b3;
                A[i][1] = ((l1 * b0 + (2.0 * l2) * b1) + l4 * b2) + l7 * b3;
                A[i][2] = ((l3 * b0 + l4 * b1) + (2.0 * l5) * b2) + l8 * b3;
                A[i][3] = ((l6 * b0 + l7 * b1) + l8 * b2) + (2.0 * l9) * b3;
                bb[i] = rho[i] - ((((((((((l0 * b0) * b0 + (l1 * b0) * b1) + (l2 * b1) * b1) + (l3 * b0) * b2) + (l4 * b1) * b2) + (l5 * b2) * b2)
                                     + (l6 * b0) * b3) + (l7 * b1) * b3) + (l8 * b2) * b3) + (l9 * b3) * b3);
            }
            qr_solve(A, bb, x);
#pragma unroll
            for (int i = 0; i < 4; i++) betas[i] = betas[i] + x[i];
        }

        // ---- compute_R_and_t (:662-673): compute_ccs, compute_pcs with solve_for_sign, estimate_R_and_t, reprojection_error
        double ccs[4][3];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < 4; i++) v = v + betas[i] * S.vt[i][3 * j + k];
                ccs[j][k] = v;
            }
        const double pcz = ((a_first[0] * ccs[0][2] + a_first[1] * ccs[1][2]) + a_first[2] * ccs[2][2]) + a_first[3] * ccs[3][2];
        if (pcz < 0.0) {
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 3; k++) ccs[j][k] = -ccs[j][k];
        }
        double pc0[3] = { 0.0, 0.0, 0.0 };
        for_members(M, lane, [&](int i) {
            const Corr c = corr_load(J, i);
            double a[4];
            alphas_of(c, c0, ci, a);
#pragma unroll
            for (int j = 0; j < 3; j++) pc0[j] = pc0[j] + (((a[0] * ccs[0][j] + a[1] * ccs[1][j]) + a[2] * ccs[2][j]) + a[3] * ccs[3][j]);
        });
#pragma unroll
        for (int j = 0; j < 3; j++) { if (!M.serial) pc0[j] = wave_sum(pc0[j]); pc0[j] = pc0[j] / nc; }
        double abt[9];
#pragma unroll
        for (int j = 0; j < 9; j++) abt[j] = 0.0;
        for_members(M, lane, [&](int i) {
            const Corr c = corr_load(J, i);
            double a[4];
            alphas_of(c, c0, ci, a);
            const double w0 = c.p0 - c0[0], w1 = c.p1 - c0[1], w2 = c.p2 - c0[2];   // pw0 is cws[0]: the same sum, the same division
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double pj = (((a[0] * ccs[0][j] + a[1] * ccs[1][j]) + a[2] * ccs[2][j]) + a[3] * ccs[3][j]) - pc0[j];
                abt[3 * j] = abt[3 * j] + pj * w0; abt[3 * j + 1] = abt[3 * j + 1] + pj * w1; abt[3 * j + 2] = abt[3 * j + 2] + pj * w2;
            }
        });
        if (!M.serial) {
#pragma unroll
            for (int j = 0; j < 9; j++) abt[j] = wave_sum(abt[j]);
        }
        wsync();
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 9; j++) B[(j / 3) * PNP_LD + j % 3] = abt[j];
        }
        wsync();
        svd(S, 3, 3, lane);
        double U[3][3], V[3][3], R[3][3], t[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) { U[i][k] = B[i * PNP_LD + k] / S.w[k]; V[i][k] = B[(3 + i) * PNP_LD + k]; }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[i][j] = dot3(U[i][0], U[i][1], U[i][2], V[j][0], V[j][1], V[j][2]);
        const double det = (((((R[0][0] * R[1][1]) * R[2][2] + (R[0][1] * R[1][2]) * R[2][0]) + (R[0][2] * R[1][0]) * R[2][1])
                             - (R[0][2] * R[1][1]) * R[2][0]) - (R[0][1] * R[1][0]) * R[2][2]) - (R[0][0] * R[1][2]) * R[2][1];
        if (det < 0.0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = pc0[i] - dot3(R[i][0], R[i][1], R[i][2], c0[0], c0[1], c0[2]);
        double sum2 = 0.0;
        for_members(M, lane, [&](int i) {
            const Corr c = corr_load(J, i);
            const double Xc = dot3(R[0][0], R[0][1], R[0][2], c.p0, c.p1, c.p2) + t[0];
            const double Yc = dot3(R[1][0], R[1][1], R[1][2], c.p0, c.p1, c.p2) + t[1];
            const double inv_Zc = 1.0 / (dot3(R[2][0], R[2][1], R[2][2], c.p0, c.p1, c.p2) + t[2]);
            const double ue = uc + (fu * Xc) * inv_Zc, ve = vc + (fv * Yc) * inv_Zc;
            const double eu = c.u - ue, ev = c.v - ve;
            sum2 = sum2 + sqrt(eu * eu + ev * ev);
        });
        if (!M.serial) sum2 = wave_sum(sum2);
        const double err = sum2 / nc;
        if (ap == 0 || err < err_best) {
            err_best = err;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                tb[i] = t[i];
#pragma unroll
                for (int j = 0; j < 3; j++) Rb[i][j] = R[i][j];
            }
        }
        wsync();
    }
}

// CheckInliers (:319-350) of the pose R, t over all n correspondences -> the count; the mask words and the twelve doubles are stored
__device__ __forceinline__ int check_inliers(const PnpJob &J, const double (&R)[3][3], const double (&t)[3], const int lane, uint64_t *bits,
                                             double *Rt)
{
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        finite = finite && isfinite(t[i]);
#pragma unroll
        for (int j = 0; j < 3; j++) finite = finite && isfinite(R[i][j]);
    }
    const double fu = J.K[0], fv = J.K[1], uc = J.K[2], vc = J.K[3];
    const int n = J.n, words = (n + 63) >> 6;
    int count = 0;
    for (int wd = 0; wd < words; wd++) {
        const int i = wd * 64 + lane;
        bool in = false;
        if (i < n && finite) {
            const double x = (double)J.P3Dw[3 * i], y = (double)J.P3Dw[3 * i + 1], z = (double)J.P3Dw[3 * i + 2];
            const float Xc = (float)((dot3(R[0][0], R[0][1], R[0][2], x, y, z)) + t[0]);
            const float Yc = (float)((dot3(R[1][0], R[1][1], R[1][2], x, y, z)) + t[1]);
            const float invZc = (float)(1.0 / ((dot3(R[2][0], R[2][1], R[2][2], x, y, z)) + t[2]));
            const double ue = uc + (fu * (double)Xc) * (double)invZc;
            const double ve = vc + (fv * (double)Yc) * (double)invZc;
            const float distX = (float)((double)J.P2D[2 * i] - ue), distY = (float)((double)J.P2D[2 * i + 1] - ve);
            const float error2 = distX * distX + distY * distY;
            in = error2 < J.max_err[i];
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) bits[wd] = m;
        count += __popcll(m);
    }
    if (lane == 0) {   // constant indices only: a select chain over the lanes becomes an indexed table in scratch
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int k = 0; k < 9; k++) Rt[k] = finite ? R[k / 3][k % 3] : qnan;
#pragma unroll
        for (int k = 0; k < 3; k++) Rt[9 + k] = finite ? t[k] : qnan;
    }
    return count;
}

__global__ __launch_bounds__(256) void k_pnp(const PnpJob *__restrict__ jobs, int njobs, int total)
{
    __shared__ PnpLds lds[4];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = blockIdx.x * 4 + wv;
    if (g >= total) return;
    const int lane = threadIdx.x & 63;
    PnpLds &S = lds[wv];
    int lo = 0, hi = njobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g >= jobs[mid].first) lo = mid; else hi = mid;
    }
    const PnpJob &J = jobs[lo];
    const int h = g - J.first, n = J.n, words = (n + 63) >> 6;
    uint64_t *bits = J.bits + (long long)h * words, *rbits = J.refined_bits + (long long)h * words;

    double R[3][3], t[3];
    Members M;
    M.serial = true; M.cnt = 4; M.iters = 4; M.sm = J.samples + 4 * (long long)h; M.bits = nullptr; M.first = M.sm[0];
    compute_pose(J, M, S, lane, R, t);
    const int count = check_inliers(J, R, t, lane, bits, J.Rt + 12 * (long long)h);
    if (lane == 0) J.n_inliers[h] = count;

    if (count < J.min_inliers) {   // no Refine for this row
        for (int wd = lane; wd < words; wd += 64) rbits[wd] = 0;
        if (lane < 12) J.Rt_refined[12 * (long long)h + lane] = __longlong_as_double(0x7ff8000000000000LL);
        if (lane == 0) J.n_refined[h] = -1;
        return;
    }
    // ---- Refine (:271-316) from this row's own mask; the words lane 0 stored are read back by every lane
    __threadfence();
    const volatile uint64_t *vb = bits;
    int first = 0;
    for (int wd = 0; wd < words; wd++) {
        const uint64_t m = vb[wd];
        if (m) { first = wd * 64 + __builtin_ctzll(m); break; }
    }
    M.serial = false; M.cnt = count; M.iters = words; M.sm = nullptr; M.bits = bits; M.first = first;
    compute_pose(J, M, S, lane, R, t);
    const int count2 = check_inliers(J, R, t, lane, rbits, J.Rt_refined + 12 * (long long)h);
    if (lane == 0) J.n_refined[h] = count2;
}

}   // namespace

// ---------------------------------------------------------------- host side (include/orbx.h: orbx_pnp_hypotheses)

static int pnp_check(const char *who, int j, const orbx_pnp_job &J)
{
    if (!J.P3Dw || !J.P2D || !J.max_err || !J.samples || !J.n_inliers || !J.Rt || !J.inlier_bits || !J.n_refined || !J.Rt_refined || !J.refined_bits) {
        orbx_set_error("%s: job %d: a NULL array", who, j);
        return ORBX_E_INVALID;
    }
    if (J.n < 4 || J.n > 65535) { orbx_set_error("%s: job %d: n = %d outside [4, 65535]", who, j, J.n); return ORBX_E_INVALID; }
    if (J.n_hyp < 1 || J.n_hyp > 1024) { orbx_set_error("%s: job %d: n_hyp = %d outside [1, 1024]", who, j, J.n_hyp); return ORBX_E_INVALID; }
    if (J.min_inliers < 4) { orbx_set_error("%s: job %d: min_inliers = %d below 4", who, j, J.min_inliers); return ORBX_E_INVALID; }
    for (int h = 0; h < J.n_hyp; h++) {
        const int32_t *s = J.samples + 4 * (size_t)h;
        for (int a = 0; a < 4; a++) {
            if (s[a] < 0 || s[a] >= J.n) {
                orbx_set_error("%s: job %d: hypothesis %d: a sample index outside [0, %d)", who, j, h, J.n);
                return ORBX_E_INVALID;
            }
            for (int b = 0; b < a; b++)
                if (s[a] == s[b]) { orbx_set_error("%s: job %d: hypothesis %d: two equal sample indices", who, j, h); return ORBX_E_INVALID; }
        }
    }
    return ORBX_OK;
}

// a job's arrays, stated once (JobArrays, orbx_resident.h): what goes up, and the results, which lie in the work area
static void pnp_arrays(JobArrays &w, const orbx_pnp_job &in, PnpJob &J)
{
    const size_t n = (size_t)in.n, nh = (size_t)in.n_hyp, wb = 8 * nh * ((n + 63) / 64);
    w.in(J.P3Dw, in.P3Dw, 12 * n); w.in(J.P2D, in.P2D, 8 * n); w.in(J.max_err, in.max_err, 4 * n); w.in(J.samples, in.samples, 16 * nh);
    w.out(J.n_inliers, in.n_inliers, 4 * nh); w.out(J.Rt, in.Rt, 96 * nh); w.out(J.bits, in.inlier_bits, wb);
    w.out(J.n_refined, in.n_refined, 4 * nh); w.out(J.Rt_refined, in.Rt_refined, 96 * nh); w.out(J.refined_bits, in.refined_bits, wb);
}

static int pnp_run(const char *who, int device, orbx_pnp_job *jobs, int njobs)
{
    if (!jobs || njobs < 1 || njobs > 64) { orbx_set_error("%s: invalid argument (jobs, 1 <= njobs <= 64)", who); return ORBX_E_INVALID; }
    size_t words = 0, total = 0;
    for (int j = 0; j < njobs; j++) {
        const int rc = pnp_check(who, j, jobs[j]);
        if (rc) return rc;
        words += 2 * (size_t)jobs[j].n_hyp * (((size_t)jobs[j].n + 63) / 64);
        total += (size_t)jobs[j].n_hyp;
    }
    if (words > ((size_t)1 << 22)) { orbx_set_error("%s: %zu mask words in all, more than 2^22", who, words); return ORBX_E_CAPACITY; }
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    const size_t jobs_b = a16(sizeof(PnpJob) * (size_t)njobs);
    PnpJob none = {};
    JobArrays size(JobArrays::MEASURE, c, jobs_b, 0);
    for (int j = 0; j < njobs; j++) pnp_arrays(size, jobs[j], none);
    const size_t blob = size.up.o, out = size.down.o;
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    JobArrays stage(JobArrays::STAGE, c, jobs_b, 0);
    int first = 0;
    for (int j = 0; j < njobs; j++) {
        const orbx_pnp_job &in = jobs[j];
        PnpJob &J = ((PnpJob *)c->h_blob)[j];
        memset(&J, 0, sizeof J);
        J.n = in.n; J.n_hyp = in.n_hyp; J.min_inliers = in.min_inliers; J.first = first;
        first += in.n_hyp;
        pnp_arrays(stage, in, J);
        memcpy(J.K, in.K, sizeof J.K);
    }
    if ((rc = call_upload(c, blob))) return rc;
    hipLaunchKernelGGL(k_pnp, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, c->stream, (const PnpJob *)c->d_blob, njobs, (int)total);   // one wave per hypothesis
    if ((rc = call_fetch(c, out))) return rc;
    JobArrays deliver(JobArrays::DELIVER, c, jobs_b, 0);
    for (int j = 0; j < njobs; j++) pnp_arrays(deliver, jobs[j], none);
    return ORBX_OK;
}

extern "C" int orbx_pnp_hypotheses(int device, orbx_pnp_job *job)
{
    if (!job) { orbx_set_error("orbx_pnp_hypotheses: a NULL job"); return ORBX_E_INVALID; }
    return pnp_run("orbx_pnp_hypotheses", device, job, 1);
}

extern "C" int orbx_pnp_hypotheses_batch(int device, orbx_pnp_job *jobs, int njobs)
{
    return pnp_run("orbx_pnp_hypotheses_batch", device, jobs, njobs);
}

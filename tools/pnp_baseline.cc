// tools/pnp_baseline.cc -- the hypothesis loop of PnPsolver (reference src/PnPsolver.cc:193-249, 271-350, 386-961) restated in plain C++
// WITHOUT cv::Mat and CvMat: the arithmetic of include/orbx.h (orbx_pnp_hypotheses) on a host core, hypothesis by hypothesis, the sums
// over a refinement's members in the contract's order (64 partial sums and the xor butterfly), so that its results are the device's bit for
// bit.  tools/bench_pnp.py compiles it (g++ -O2 -ffp-contract=off -shared) and times it beside the device calls.  It evaluates and refines
// EVERY row, as the device does; the reference stops at the first refinement that succeeds.  It is not the reference and says nothing
// about OpenCV's speed.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include <orbx.h>

namespace {

const int LD = 12;
const double EPS = 1.0 / 562949953421312.0;      // 2^-49
const double CUT = 1.0 / 2251799813685248.0;     // 2^-51

struct Sv { double B[24 * LD], w[12]; int order[12]; };

inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

void svd(Sv &S, int m, int n)
{
    double *B = S.B;
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) B[(m + r) * LD + c] = r == c ? 1.0 : 0.0;
    const int N = (n + 1) & ~1, half = N >> 1, rows = m + n;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        for (int r = 0; r < N - 1; r++)
            for (int slot = 0; slot < half; slot++) {       // the pivots of a round are disjoint: any order
                const int a = slot == 0 ? N - 1 : (r + slot) % (N - 1), b = slot == 0 ? r : (r + (N - 1) - slot) % (N - 1);
                const int p = a < b ? a : b, q = a < b ? b : a;
                if (q >= n) continue;
                double al = 0.0, be = 0.0, g = 0.0;
                for (int i = 0; i < m; i++) {
                    const double x = B[i * LD + p], y = B[i * LD + q];
                    al = al + x * x; be = be + y * y; g = g + x * y;
                }
                if (fabs(g) <= EPS * sqrt(al * be)) continue;
                changed = true;
                const double g2 = g * 2.0, beta = al - be, gamma = sqrt(g2 * g2 + beta * beta);
                double c, s;
                if (beta < 0.0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = g2 / ((gamma * s) * 2.0);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2.0));
                    s = g2 / ((gamma * c) * 2.0);
                }
                for (int rr = 0; rr < rows; rr++) {
                    const double x = B[rr * LD + p], y = B[rr * LD + q];
                    B[rr * LD + p] = c * x + s * y;
                    B[rr * LD + q] = c * y - s * x;
                }
            }
        if (!changed) break;
    }
    for (int j = 0; j < n; j++) {
        double s2 = 0.0;
        for (int i = 0; i < m; i++) { const double x = B[i * LD + j]; s2 = s2 + x * x; }
        S.w[j] = sqrt(s2);
    }
}

void sort_desc(Sv &S, int n)
{
    unsigned used = 0;
    for (int r = 0; r < n; r++) {
        int best = -1;
        for (int j = 0; j < n; j++) {
            if ((used >> j) & 1) continue;
            if (best < 0 || S.w[j] > S.w[best]) best = j;
        }
        S.order[r] = best;
        used |= 1u << best;
    }
}

void solve(const Sv &S, int m, int n, const double *b, double *x)
{
    double sum = 0.0;
    for (int k = 0; k < n; k++) sum = sum + S.w[k];
    const double thr = sum * CUT;
    for (int j = 0; j < n; j++) x[j] = 0.0;
    for (int k = 0; k < n; k++) {
        const double wk = S.w[k];
        if (!(wk > thr)) continue;
        double t = 0.0;
        for (int i = 0; i < m; i++) t = t + S.B[i * LD + k] * b[i];
        t = (t / wk) / wk;
        for (int j = 0; j < n; j++) x[j] = x[j] + S.B[(m + j) * LD + k] * t;
    }
}

void qr_solve(double A[6][4], double b[6], double x[4])
{
    double A1[4], A2[4];
    for (int k = 0; k < 4; k++) {
        double eta = fabs(A[k][k]);
        for (int i = k; i < 5; i++) { const double elt = fabs(A[i][k]); if (eta < elt) eta = elt; }
        if (eta == 0.0) return;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
        for (int i = k; i < 6; i++) { A[i][k] = A[i][k] * inv_eta; sum = sum + A[i][k] * A[i][k]; }
        double sigma = sqrt(sum);
        if (A[k][k] < 0.0) sigma = -sigma;
        A[k][k] = A[k][k] + sigma;
        A1[k] = sigma * A[k][k];
        A2[k] = (-eta) * sigma;
        for (int j = k + 1; j < 4; j++) {
            double sm = 0.0;
            for (int i = k; i < 6; i++) sm = sm + A[i][k] * A[i][j];
            const double tau = sm / A1[k];
            for (int i = k; i < 6; i++) A[i][j] = A[i][j] - tau * A[i][k];
        }
    }
    for (int j = 0; j < 4; j++) {
        double tau = 0.0;
        for (int i = j; i < 6; i++) tau = tau + A[i][j] * b[i];
        tau = tau / A1[j];
        for (int i = j; i < 6; i++) b[i] = b[i] - tau * A[i][j];
    }
    x[3] = b[3] / A2[3];
    for (int i = 2; i >= 0; i--) {
        double sum = 0.0;
        for (int j = i + 1; j < 4; j++) sum = sum + A[i][j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
}

struct Members { bool serial; int cnt, words, first; const int32_t *sm; const uint64_t *bits; };

// SUM of the contract over K running values: f(i, acc) adds member i's terms to acc[K]
template <int K, class F>
void msum(const Members &M, double (&out)[K], F f)
{
    if (M.serial) {
        for (int k = 0; k < K; k++) out[k] = 0.0;
        for (int k = 0; k < 4; k++) f(M.sm[k], out);
        return;
    }
    static thread_local double acc[64][K], tmp[64][K];
    memset(acc, 0, sizeof acc);
    for (int wd = 0; wd < M.words; wd++)
        for (int lane = 0; lane < 64; lane++)
            if ((M.bits[wd] >> lane) & 1) f(wd * 64 + lane, acc[lane]);
    for (int s = 32; s >= 1; s >>= 1) {
        for (int l = 0; l < 64; l++)
            for (int k = 0; k < K; k++) tmp[l][k] = acc[l][k] + acc[l ^ s][k];
        memcpy(acc, tmp, sizeof acc);
    }
    for (int k = 0; k < K; k++) out[k] = acc[0][k];
}

struct Corr { double p0, p1, p2, u, v; };

inline Corr corr_load(const orbx_pnp_job &J, int i)
{
    Corr c;
    c.p0 = J.P3Dw[3 * i]; c.p1 = J.P3Dw[3 * i + 1]; c.p2 = J.P3Dw[3 * i + 2];
    c.u = J.P2D[2 * i]; c.v = J.P2D[2 * i + 1];
    return c;
}

inline void alphas_of(const Corr &c, const double c0[3], const double ci[9], double a[4])
{
    const double d0 = c.p0 - c0[0], d1 = c.p1 - c0[1], d2 = c.p2 - c0[2];
    for (int j = 0; j < 3; j++) a[1 + j] = (ci[3 * j] * d0 + ci[3 * j + 1] * d1) + ci[3 * j + 2] * d2;
    a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

void compute_pose(const orbx_pnp_job &J, const Members &M, Sv &S, double Rb[3][3], double tb[3])
{
    const double fu = J.K[0], fv = J.K[1], uc = J.K[2], vc = J.K[3], nc = (double)M.cnt;
    double *B = S.B;
    double c0[3];
    msum<3>(M, c0, [&](int i, double *acc) { const Corr c = corr_load(J, i); acc[0] = acc[0] + c.p0; acc[1] = acc[1] + c.p1; acc[2] = acc[2] + c.p2; });
    for (int j = 0; j < 3; j++) c0[j] = c0[j] / nc;
    double ptp[6];
    msum<6>(M, ptp, [&](int i, double *acc) {
        const Corr c = corr_load(J, i);
        const double d0 = c.p0 - c0[0], d1 = c.p1 - c0[1], d2 = c.p2 - c0[2];
        acc[0] = acc[0] + d0 * d0; acc[1] = acc[1] + d0 * d1; acc[2] = acc[2] + d0 * d2;
        acc[3] = acc[3] + d1 * d1; acc[4] = acc[4] + d1 * d2; acc[5] = acc[5] + d2 * d2;
    });
    B[0] = ptp[0]; B[1] = ptp[1]; B[2] = ptp[2];
    B[LD] = ptp[1]; B[LD + 1] = ptp[3]; B[LD + 2] = ptp[4];
    B[2 * LD] = ptp[2]; B[2 * LD + 1] = ptp[4]; B[2 * LD + 2] = ptp[5];
    svd(S, 3, 3);
    sort_desc(S, 3);
    double cws[4][3];
    for (int j = 0; j < 3; j++) cws[0][j] = c0[j];
    for (int i = 1; i < 4; i++) {
        const int o = S.order[i - 1];
        const double k = sqrt(S.w[o] / nc);
        for (int j = 0; j < 3; j++) cws[i][j] = c0[j] + k * B[(3 + j) * LD + o];
    }
    for (int i = 0; i < 3; i++)
        for (int j = 1; j < 4; j++) B[i * LD + j - 1] = cws[j][i] - cws[0][i];
    svd(S, 3, 3);
    double ci[9];
    for (int j = 0; j < 3; j++) {
        const double e[3] = { j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0 };
        double x[3];
        solve(S, 3, 3, e, x);
        for (int i = 0; i < 3; i++) ci[3 * i + j] = x[i];
    }
    double up[78];
    msum<78>(M, up, [&](int i, double *acc) {
        const Corr c = corr_load(J, i);
        double a[4], M1[12], M2[12];
        alphas_of(c, c0, ci, a);
        const double du = uc - c.u, dv = vc - c.v;
        for (int q = 0; q < 4; q++) {
            M1[3 * q] = a[q] * fu; M1[3 * q + 1] = 0.0; M1[3 * q + 2] = a[q] * du;
            M2[3 * q] = 0.0; M2[3 * q + 1] = a[q] * fv; M2[3 * q + 2] = a[q] * dv;
        }
        int e = 0;
        for (int j = 0; j < 12; j++)
            for (int k = j; k < 12; k++, e++) acc[e] = (acc[e] + M1[j] * M1[k]) + M2[j] * M2[k];
    });
    for (int j = 0, e = 0; j < 12; j++)
        for (int k = j; k < 12; k++, e++) B[j * LD + k] = B[k * LD + j] = up[e];
    svd(S, 12, 12);
    sort_desc(S, 12);
    double vt[4][12];
    for (int i = 0; i < 4; i++)
        for (int c = 0; c < 12; c++) vt[i][c] = B[(12 + c) * LD + S.order[11 - i]];
    double L[6][10], rho[6];
    for (int row = 0, a = 0; a < 3; a++)
        for (int b = a + 1; b < 4; b++, row++) {
            double dv[4][3];
            for (int i = 0; i < 4; i++)
                for (int k = 0; k < 3; k++) dv[i][k] = vt[i][3 * a + k] - vt[i][3 * b + k];
#define DD(i, j) dot3(dv[i][0], dv[i][1], dv[i][2], dv[j][0], dv[j][1], dv[j][2])
            double *l = L[row];
            l[0] = DD(0, 0); l[1] = 2.0 * DD(0, 1); l[2] = DD(1, 1); l[3] = 2.0 * DD(0, 2); l[4] = 2.0 * DD(1, 2);
            l[5] = DD(2, 2); l[6] = 2.0 * DD(0, 3); l[7] = 2.0 * DD(1, 3); l[8] = 2.0 * DD(2, 3); l[9] = DD(3, 3);
#undef DD
            const double d0 = cws[a][0] - cws[b][0], d1 = cws[a][1] - cws[b][1], d2 = cws[a][2] - cws[b][2];
            rho[row] = (d0 * d0 + d1 * d1) + d2 * d2;
        }
    double a_first[4];
    alphas_of(corr_load(J, M.first), c0, ci, a_first);
    double err_best = 0.0;
    for (int ap = 0; ap < 3; ap++) {
        const int ncol = ap == 0 ? 4 : ap == 1 ? 3 : 5;
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < ncol; c++) B[r * LD + c] = L[r][ap == 0 ? (c == 2 ? 3 : c == 3 ? 6 : c) : c];
        svd(S, 6, ncol);
        double bs[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 }, betas[4];
        solve(S, 6, ncol, rho, bs);
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
        double x[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int it = 0; it < 5; it++) {
            double A[6][4], bb[6];
            for (int i = 0; i < 6; i++) {
                const double *l = L[i];
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
            for (int i = 0; i < 4; i++) betas[i] = betas[i] + x[i];
        }
        double ccs[4][3];
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) {
                double v = 0.0;
                for (int i = 0; i < 4; i++) v = v + betas[i] * vt[i][3 * j + k];
                ccs[j][k] = v;
            }
        const double pcz = ((a_first[0] * ccs[0][2] + a_first[1] * ccs[1][2]) + a_first[2] * ccs[2][2]) + a_first[3] * ccs[3][2];
        if (pcz < 0.0)
            for (int j = 0; j < 4; j++)
                for (int k = 0; k < 3; k++) ccs[j][k] = -ccs[j][k];
        double pc0[3];
        msum<3>(M, pc0, [&](int i, double *acc) {
            double a[4];
            alphas_of(corr_load(J, i), c0, ci, a);
            for (int j = 0; j < 3; j++) acc[j] = acc[j] + (((a[0] * ccs[0][j] + a[1] * ccs[1][j]) + a[2] * ccs[2][j]) + a[3] * ccs[3][j]);
        });
        for (int j = 0; j < 3; j++) pc0[j] = pc0[j] / nc;
        double abt[9];
        msum<9>(M, abt, [&](int i, double *acc) {
            const Corr c = corr_load(J, i);
            double a[4];
            alphas_of(c, c0, ci, a);
            const double w0 = c.p0 - c0[0], w1 = c.p1 - c0[1], w2 = c.p2 - c0[2];
            for (int j = 0; j < 3; j++) {
                const double pj = (((a[0] * ccs[0][j] + a[1] * ccs[1][j]) + a[2] * ccs[2][j]) + a[3] * ccs[3][j]) - pc0[j];
                acc[3 * j] = acc[3 * j] + pj * w0; acc[3 * j + 1] = acc[3 * j + 1] + pj * w1; acc[3 * j + 2] = acc[3 * j + 2] + pj * w2;
            }
        });
        for (int j = 0; j < 9; j++) B[(j / 3) * LD + j % 3] = abt[j];
        svd(S, 3, 3);
        double U[3][3], V[3][3], R[3][3], t[3];
        for (int i = 0; i < 3; i++)
            for (int k = 0; k < 3; k++) { U[i][k] = B[i * LD + k] / S.w[k]; V[i][k] = B[(3 + i) * LD + k]; }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = dot3(U[i][0], U[i][1], U[i][2], V[j][0], V[j][1], V[j][2]);
        const double det = (((((R[0][0] * R[1][1]) * R[2][2] + (R[0][1] * R[1][2]) * R[2][0]) + (R[0][2] * R[1][0]) * R[2][1])
                             - (R[0][2] * R[1][1]) * R[2][0]) - (R[0][1] * R[1][0]) * R[2][2]) - (R[0][0] * R[1][2]) * R[2][1];
        if (det < 0.0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
        for (int i = 0; i < 3; i++) t[i] = pc0[i] - dot3(R[i][0], R[i][1], R[i][2], c0[0], c0[1], c0[2]);
        double sum2[1];
        msum<1>(M, sum2, [&](int i, double *acc) {
            const Corr c = corr_load(J, i);
            const double Xc = dot3(R[0][0], R[0][1], R[0][2], c.p0, c.p1, c.p2) + t[0];
            const double Yc = dot3(R[1][0], R[1][1], R[1][2], c.p0, c.p1, c.p2) + t[1];
            const double inv_Zc = 1.0 / (dot3(R[2][0], R[2][1], R[2][2], c.p0, c.p1, c.p2) + t[2]);
            const double ue = uc + (fu * Xc) * inv_Zc, ve = vc + (fv * Yc) * inv_Zc;
            const double eu = c.u - ue, ev = c.v - ve;
            acc[0] = acc[0] + sqrt(eu * eu + ev * ev);
        });
        const double err = sum2[0] / nc;
        if (ap == 0 || err < err_best) {
            err_best = err;
            for (int i = 0; i < 3; i++) {
                tb[i] = t[i];
                for (int j = 0; j < 3; j++) Rb[i][j] = R[i][j];
            }
        }
    }
}

int check_inliers(const orbx_pnp_job &J, const double R[3][3], const double t[3], uint64_t *bits, double *Rt)
{
    bool finite = true;
    for (int i = 0; i < 3; i++) {
        finite = finite && std::isfinite(t[i]);
        for (int j = 0; j < 3; j++) finite = finite && std::isfinite(R[i][j]);
    }
    const double fu = J.K[0], fv = J.K[1], uc = J.K[2], vc = J.K[3];
    const int n = J.n, words = (n + 63) >> 6;
    int count = 0;
    for (int wd = 0; wd < words; wd++) {
        uint64_t m = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int i = wd * 64 + lane;
            if (i >= n || !finite) continue;
            const double x = J.P3Dw[3 * i], y = J.P3Dw[3 * i + 1], z = J.P3Dw[3 * i + 2];
            const float Xc = (float)(dot3(R[0][0], R[0][1], R[0][2], x, y, z) + t[0]);
            const float Yc = (float)(dot3(R[1][0], R[1][1], R[1][2], x, y, z) + t[1]);
            const float invZc = (float)(1.0 / (dot3(R[2][0], R[2][1], R[2][2], x, y, z) + t[2]));
            const double ue = uc + (fu * (double)Xc) * (double)invZc;
            const double ve = vc + (fv * (double)Yc) * (double)invZc;
            const float distX = (float)((double)J.P2D[2 * i] - ue), distY = (float)((double)J.P2D[2 * i + 1] - ve);
            const float error2 = distX * distX + distY * distY;
            if (error2 < J.max_err[i]) { m |= (uint64_t)1 << lane; count++; }
        }
        bits[wd] = m;
    }
    const uint64_t qnan = 0x7ff8000000000000ull;
    for (int k = 0; k < 12; k++) {
        const double v = k < 9 ? R[k / 3][k % 3] : t[k - 9];
        if (finite) Rt[k] = v; else memcpy(&Rt[k], &qnan, 8);
    }
    return count;
}

}   // namespace

// every row of every job, as orbx_pnp_hypotheses_batch delivers them
extern "C" int pnp_loop(orbx_pnp_job *jobs, int njobs)
{
    Sv S;
    for (int jn = 0; jn < njobs; jn++) {
        const orbx_pnp_job &J = jobs[jn];
        const int words = (J.n + 63) >> 6;
        for (int h = 0; h < J.n_hyp; h++) {
            uint64_t *bits = J.inlier_bits + (size_t)h * words, *rbits = J.refined_bits + (size_t)h * words;
            double R[3][3], t[3];
            Members M;
            M.serial = true; M.cnt = 4; M.words = 0; M.sm = J.samples + 4 * (size_t)h; M.bits = 0; M.first = M.sm[0];
            compute_pose(J, M, S, R, t);
            const int count = J.n_inliers[h] = check_inliers(J, R, t, bits, J.Rt + 12 * (size_t)h);
            if (count < J.min_inliers) {
                const uint64_t qnan = 0x7ff8000000000000ull;
                memset(rbits, 0, 8 * (size_t)words);
                for (int k = 0; k < 12; k++) memcpy(&J.Rt_refined[12 * (size_t)h + k], &qnan, 8);
                J.n_refined[h] = -1;
                continue;
            }
            int first = 0;
            for (int wd = 0; wd < words; wd++)
                if (bits[wd]) { first = wd * 64 + __builtin_ctzll(bits[wd]); break; }
            M.serial = false; M.cnt = count; M.words = words; M.sm = 0; M.bits = bits; M.first = first;
            compute_pose(J, M, S, R, t);
            J.n_refined[h] = check_inliers(J, R, t, rbits, J.Rt_refined + 12 * (size_t)h);
        }
    }
    return 0;
}

// orbx_initializer.hip — k_mono_hyp, k_mono_reconstruct, k_mono_decide: Initializer::Initialize (reference src/Initializer.cc:52-1026)
// behind the drawing of the sample rows.
// k_mono_hyp: one wave64 per (model, hypothesis), four waves per workgroup, 2 x n_hyp waves.  Solve phase: the eight sampled matches are
// normalised by eight lanes, the 16 x 9 (H) or 8 x 9 (F) system goes to LDS stacked on V (25 x 9 floats per wave) and the one Jacobi
// routine of the contract runs on it: the four disjoint pivots of a round-robin round side by side on the four 16-lane groups, one lane
// per matrix row: a lane squares its row in double, a xor butterfly over the group's 16 closes the pivot's three sums, then the lanes rotate.  Everything behind the null vector
// (the 3 x 3 products, inv, F's rank-2 projection through the same routine) is lane-uniform in registers.  Check phase: one lane per match,
// 64 at a time, from the pre-gathered (u1, v1, u2, v2); __ballot of the predicate IS the mask word; the score is each lane's serial float
// sum closed by a xor butterfly.
// k_mono_reconstruct: one workgroup of 256 per motion hypothesis (8).  Every wave repeats the arg-max over the two score columns (a
// butterfly of (score, index) pairs) and the 3 x 3 decomposition; nothing is broadcast through memory.  Then CheckRT: one thread per
// inlier match with the 4x4 routine of k_triangulate in registers, n_good an integer sum of ballots, the cosine of rank min(50, n_good - 1)
// by bisecting the 32 bits of an order-preserving key over the accepted cosines in LDS (exact, no sort).
// k_mono_decide: one workgroup: the 8- or 4-way decision of ReconstructH / ReconstructF and the winner's points scattered to P3D.
// No atomics, no scratch.  The arithmetic is restated in include/orbx.h (orbx_mono_init_hypotheses) and, in numpy, in tests/init_model.py.
// Behind the kernels: the refusals, Normalize and the acos thresholds (the host half), the staging and the three entry points.
#include "orbx_resident.h"
#include "orbx_wave.h"
#include <float.h>
#include <math.h>

#define MONO_MAX_N 8192

// what k_mono_decide leaves at the head of the work area; P3D[n1][3] and triangulated[n1] follow it
struct MonoDec {
    int ok, model, best_h, best_f, winner, pad;
    float SH, SF;
    float M[9];
    int32_t n_good[8];
    float cosp[8];
    float R[8][9], t[8][3];
};

// The arguments of the three kernels, by value.  Every pointer is a device address.
struct MonoArgs {
    int n, n1, n_hyp, words;
    const float4 *pts;        // [n] u1 v1 u2 v2 of match i
    const int32_t *first;     // [n] mvMatches12[i].first
    const int32_t *samples;   // [n_hyp][8]
    float norm1[4], norm2[4]; // meanX meanY sX sY of Normalize
    float T1[9], T2[9], T2inv[9];
    float inv_sigma2, th2, K[4];
    float c_gt, c_ge;         // the acos thresholds of min_parallax
    int min_tri;
    float *score, *mats; uint64_t *bits;   // the table: [2][n_hyp], [2][n_hyp][9], [2][n_hyp][words]; 0 = H, 1 = F
    int given_model; float given_M[9]; const uint64_t *given_mask;   // orbx_mono_init_reconstruct: 1 / 2, no table
    float *p3d; uint8_t *flag;             // [8][n][3], [8][n]: 0 not accepted, 1 accepted, 2 accepted with parallax
    MonoDec *dec; float *P3D; uint8_t *tri;
};

namespace {

#define MONO_LD 9                                              // row stride of B: odd, so the rows of a column fall on different banks
#define MONO_EPS2 ((double)(2.0f * 1.1920928955078125e-7f))    // the skip test of a pivot

#include "orbx_svd4.h"   // jacobi_pair, null_vector: the 4x4 routine of CheckRT's Triangulate

// what one wave keeps in LDS: B = A (m rows) stacked on V (n rows), and the squared norms of A's columns
struct MonoLds {
    float B[25 * MONO_LD];
    float pad;
    double w2[9];
};

// the correctly rounded float square root (through double: the second rounding is innocuous for a square root)
__device__ __forceinline__ float fsqrt(float x) { return (float)sqrt((double)x); }

// "NaN" of the contract: every NaN leaves the device as the quiet NaN 0x7fc00000
__device__ __forceinline__ float canon(float x) { return x != x ? __uint_as_float(0x7fc00000u) : x; }

// cv::Mat product of two 3 x 3: one cast from a double accumulation
__device__ __forceinline__ void mm3(const float (&X)[9], const float (&Y)[9], float (&Z)[9])
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Z[3 * r + c] = (float)dotd(X[3 * r], X[3 * r + 1], X[3 * r + 2], Y[c], Y[3 + c], Y[6 + c]);
}

__device__ __forceinline__ double det3(const float (&m)[9])
{
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
    return (m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6)) + m2 * (m3 * m7 - m4 * m6);
}

// cv::Mat::inv of a 3 x 3: zeros for a zero determinant
__device__ __forceinline__ void inv3(const float (&m)[9], float (&o)[9])
{
    double d = det3(m);
    if (d == 0.0) {
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = 0.0f;
        return;
    }
    d = 1.0 / d;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
    o[0] = (float)((m4 * m8 - m5 * m7) * d); o[1] = (float)((m2 * m7 - m1 * m8) * d); o[2] = (float)((m1 * m5 - m2 * m4) * d);
    o[3] = (float)((m5 * m6 - m3 * m8) * d); o[4] = (float)((m0 * m8 - m2 * m6) * d); o[5] = (float)((m2 * m3 - m0 * m5) * d);
    o[6] = (float)((m3 * m7 - m4 * m6) * d); o[7] = (float)((m1 * m6 - m0 * m7) * d); o[8] = (float)((m0 * m4 - m1 * m3) * d);
}

// The one-sided Jacobi of the contract on the m x n float matrix in rows 0 .. m-1 of B, n odd; rows m .. m+n-1 become V.  Afterwards the
// columns of A are orthogonal and w2[j] = their squared norms.  Group k - 1 of 16 lanes owns the k-th pivot of a round.
__device__ __forceinline__ void svd(MonoLds &S, const int m, const int n, const int lane)
{
    float *B = S.B;
    for (int e = lane; e < n * n; e += 64) B[(m + e / n) * MONO_LD + e % n] = (e / n == e % n) ? 1.0f : 0.0f;
    wsync();
    const int k = (lane >> 4) + 1, sub = lane & 15, rows = m + n, half = (n + 1) >> 1;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        for (int r = 0; r < n; r++) {
            bool rotate = false;
            int p = 0, q = 0;
            float c = 0.0f, s = 0.0f;
            if (k < half) {
                const int a = (r + k) % n, b = (r + n - k) % n;
                p = a < b ? a : b;
                q = a < b ? b : a;
                double al = 0.0, be = 0.0, g = 0.0;
                for (int i = sub; i < m; i += 16) {   // m <= 16: one row per lane, and a butterfly over the group's 16
                    const double x = (double)B[i * MONO_LD + p], y = (double)B[i * MONO_LD + q];
                    al = al + x * x;
                    be = be + y * y;
                    g = g + x * y;
                }
#pragma unroll
                for (int st = 8; st >= 1; st >>= 1) {
                    al = al + __shfl_xor(al, st, 64);
                    be = be + __shfl_xor(be, st, 64);
                    g = g + __shfl_xor(g, st, 64);
                }
                if (!(fabs(g) <= MONO_EPS2 * sqrt(al * be))) {
                    rotate = true;
                    const double g2 = g * 2.0, beta = al - be, gamma = sqrt(g2 * g2 + beta * beta);
                    if (beta < 0.0) {
                        const double delta = (gamma - beta) * 0.5;
                        s = (float)sqrt(delta / gamma);
                        c = (float)(g2 / ((gamma * (double)s) * 2.0));
                    } else {
                        c = (float)sqrt((gamma + beta) / (gamma * 2.0));
                        s = (float)(g2 / ((gamma * (double)c) * 2.0));
                    }
                }
            }
            wsync();
            if (rotate) {
                for (int rr = sub; rr < rows; rr += 16) {
                    const float x = B[rr * MONO_LD + p], y = B[rr * MONO_LD + q];
                    B[rr * MONO_LD + p] = c * x + s * y;
                    B[rr * MONO_LD + q] = (-s) * x + c * y;
                }
            }
            changed |= __ballot(rotate) != 0;
            wsync();
        }
        if (!changed) break;
    }
    if (lane < n) {
        double s2 = 0.0;
        for (int i = 0; i < m; i++) { const double x = (double)B[i * MONO_LD + lane]; s2 = s2 + x * x; }
        S.w2[lane] = s2;
    }
    wsync();
}

// U w Vt of the 3 x 3 matrix M ("U w Vt" of the contract); the same in every lane
__device__ __forceinline__ void svd3(MonoLds &S, const int lane, const float (&M)[9], float (&U)[9], float (&w)[3], float (&Vt)[9])
{
    wsync();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) S.B[(k / 3) * MONO_LD + k % 3] = M[k];
    }
    wsync();
    svd(S, 3, 3, lane);
    const double a0 = S.w2[0], a1 = S.w2[1], a2 = S.w2[2];
    // descending, of equal values the earlier first: the r-th is the first unused j that no later unused one exceeds
    int o0 = 0;
    if (a1 > a0) o0 = 1;
    if (a2 > (o0 == 0 ? a0 : a1)) o0 = 2;
    int o1, o2;
    if (o0 == 0) { o1 = a2 > a1 ? 2 : 1; o2 = 3 - o1; }
    else if (o0 == 1) { o1 = a2 > a0 ? 2 : 0; o2 = 2 - o1; }
    else { o1 = a1 > a0 ? 1 : 0; o2 = 1 - o1; }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int o = r == 0 ? o0 : r == 1 ? o1 : o2;
        const double wd = sqrt(S.w2[o]);
        const float sc = wd > (double)FLT_MIN ? (float)(1.0 / wd) : 0.0f;
        w[r] = (float)wd;
#pragma unroll
        for (int i = 0; i < 3; i++) { U[3 * i + r] = S.B[i * MONO_LD + o] * sc; Vt[3 * r + i] = S.B[(3 + i) * MONO_LD + o]; }
    }
}

__global__ __launch_bounds__(256) void k_mono_hyp(const MonoArgs A)
{
    __shared__ MonoLds lds[4];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = blockIdx.x * 4 + wv;
    if (g >= 2 * A.n_hyp) return;
    const int lane = threadIdx.x & 63;
    MonoLds &S = lds[wv];
    const int model = g >= A.n_hyp ? 1 : 0, h = g - model * A.n_hyp, m = model ? 8 : 16;
    const int n = A.n, words = A.words;

    // ---- the system of ComputeH21 (:274-301) / ComputeF21 (:329-345) on the eight normalised matches of the row
    if (lane < 8) {
        const float4 pt = A.pts[A.samples[8 * h + lane]];
        const float u1 = (pt.x - A.norm1[0]) * A.norm1[2], v1 = (pt.y - A.norm1[1]) * A.norm1[3];
        const float u2 = (pt.z - A.norm2[0]) * A.norm2[2], v2 = (pt.w - A.norm2[1]) * A.norm2[3];
        if (model == 0) {
            float *r0 = S.B + 2 * lane * MONO_LD, *r1 = r0 + MONO_LD;
            r0[0] = 0.0f; r0[1] = 0.0f; r0[2] = 0.0f; r0[3] = -u1; r0[4] = -v1; r0[5] = -1.0f; r0[6] = v2 * u1; r0[7] = v2 * v1; r0[8] = v2;
            r1[0] = u1; r1[1] = v1; r1[2] = 1.0f; r1[3] = 0.0f; r1[4] = 0.0f; r1[5] = 0.0f; r1[6] = (-u2) * u1; r1[7] = (-u2) * v1; r1[8] = -u2;
        } else {
            float *r0 = S.B + lane * MONO_LD;
            r0[0] = u2 * u1; r0[1] = u2 * v1; r0[2] = u2; r0[3] = v2 * u1; r0[4] = v2 * v1; r0[5] = v2; r0[6] = u1; r0[7] = v1; r0[8] = 1.0f;
        }
    }
    wsync();
    svd(S, m, 9, lane);
    int col = 0;
    double best = S.w2[0];
    for (int j = 1; j < 9; j++) { const double sd = S.w2[j]; if (sd <= best) { best = sd; col = j; } }   // a tie takes the later column
    float X[9];
#pragma unroll
    for (int k = 0; k < 9; k++) X[k] = S.B[(m + k) * MONO_LD + col];

    float M21[9], M12[9], tmp[9];
    if (model == 0) {
        mm3(A.T2inv, X, tmp);
        mm3(tmp, A.T1, M21);
        inv3(M21, M12);
    } else {
        float U[9], w[3], Vt[9], Dg[9], T2t[9];
        svd3(S, lane, X, U, w, Vt);
#pragma unroll
        for (int k = 0; k < 9; k++) { Dg[k] = 0.0f; T2t[k] = A.T2[(k % 3) * 3 + k / 3]; }
        Dg[0] = w[0]; Dg[4] = w[1];
        mm3(U, Dg, tmp);
        mm3(tmp, Vt, X);
        mm3(T2t, X, tmp);
        mm3(tmp, A.T1, M21);
#pragma unroll
        for (int k = 0; k < 9; k++) M12[k] = 0.0f;
    }

    // ---- CheckHomography (:360-448) / CheckFundamental (:450-528): one lane per match
    uint64_t *bits = A.bits + ((size_t)model * A.n_hyp + h) * words;
    const float inv_s2 = A.inv_sigma2, th = model ? 3.841f : 5.991f, thScore = 5.991f;
    float acc = 0.0f;
    for (int wd = 0; wd < words; wd++) {
        const int i = wd * 64 + lane;
        bool in = false;
        if (i < n) {
            const float4 pt = A.pts[i];
            const float u1 = pt.x, v1 = pt.y, u2 = pt.z, v2 = pt.w;
            in = true;
            float chi1, chi2;
            if (model == 0) {
                const float w2in1inv = (float)(1.0 / (double)(M12[6] * u2 + M12[7] * v2 + M12[8]));
                const float u2in1 = (M12[0] * u2 + M12[1] * v2 + M12[2]) * w2in1inv;
                const float v2in1 = (M12[3] * u2 + M12[4] * v2 + M12[5]) * w2in1inv;
                chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_s2;
                const float w1in2inv = (float)(1.0 / (double)(M21[6] * u1 + M21[7] * v1 + M21[8]));
                const float u1in2 = (M21[0] * u1 + M21[1] * v1 + M21[2]) * w1in2inv;
                const float v1in2 = (M21[3] * u1 + M21[4] * v1 + M21[5]) * w1in2inv;
                chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_s2;
            } else {
                const float a2 = M21[0] * u1 + M21[1] * v1 + M21[2];
                const float b2 = M21[3] * u1 + M21[4] * v1 + M21[5];
                const float c2 = M21[6] * u1 + M21[7] * v1 + M21[8];
                const float num2 = a2 * u2 + b2 * v2 + c2;
                chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2;
                const float a1 = M21[0] * u2 + M21[3] * v2 + M21[6];
                const float b1 = M21[1] * u2 + M21[4] * v2 + M21[7];
                const float c1 = M21[2] * u2 + M21[5] * v2 + M21[8];
                const float num1 = a1 * u1 + b1 * v1 + c1;
                chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2;
            }
            if (chi1 > th) in = false; else acc = acc + (thScore - chi1);   // a NaN takes the else
            if (chi2 > th) in = false; else acc = acc + (thScore - chi2);
        }
        const unsigned long long mk = __ballot(in);
        if (lane == 0) bits[wd] = mk;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc = acc + __shfl_xor(acc, s, 64);
    if (lane == 0) {   // constant indices only
        A.score[(size_t)model * A.n_hyp + h] = canon(acc);
        float *o = A.mats + 9 * ((size_t)model * A.n_hyp + h);
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = canon(M21[k]);
    }
}

// ---- the choice (:203, :257, :133-142): what every wave of k_mono_reconstruct and k_mono_decide works out for itself
struct MonoSel { int model, best_h, best_f; float SH, SF; const uint64_t *mask; };

// the earliest strictly greatest score above 0.0f of one column -> its index (-1 none) and value (0.0f)
__device__ __forceinline__ void col_best(const float *sc, const int nh, const int lane, int &bi, float &bv)
{
    bv = 0.0f;
    bi = 0x7fffffff;
    for (int i = lane; i < nh; i += 64) { const float v = sc[i]; if (v > bv) { bv = v; bi = i; } }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float ov = __shfl_xor(bv, s, 64);
        const int oi = __shfl_xor(bi, s, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (bi == 0x7fffffff) bi = -1;
}

__device__ __forceinline__ MonoSel mono_select(const MonoArgs &A, const int lane)
{
    MonoSel s;
    if (A.given_model) {
        s.model = A.given_model; s.best_h = -1; s.best_f = -1; s.SH = 0.0f; s.SF = 0.0f; s.mask = A.given_mask;
        return s;
    }
    col_best(A.score, A.n_hyp, lane, s.best_h, s.SH);
    col_best(A.score + A.n_hyp, A.n_hyp, lane, s.best_f, s.SF);
    const float RH = s.SH / (s.SH + s.SF);
    const bool takeH = (double)RH > 0.40;
    const int best = takeH ? s.best_h : s.best_f;
    s.model = best < 0 ? 0 : takeH ? 1 : 2;
    s.mask = best < 0 ? nullptr : A.bits + ((size_t)(takeH ? 0 : A.n_hyp) + best) * A.words;
    return s;
}

__device__ __forceinline__ void sel_matrix(const MonoArgs &A, const MonoSel &s, float (&M)[9])
{
    if (A.given_model) {
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = A.given_M[k];
    } else {
        const float *src = A.mats + 9 * ((size_t)(s.model == 1 ? 0 : A.n_hyp) + (s.model == 1 ? s.best_h : s.best_f));
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = src[k];
    }
}

// t = t / cv::norm(t)
__device__ __forceinline__ void normalise3(float (&t)[3])
{
    const double inv = 1.0 / sqrt(dotd(t[0], t[1], t[2], t[0], t[1], t[2]));
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (float)((double)t[k] * inv);
}

// motion hypothesis `hyp` of ReconstructH (:654-766) / ReconstructF (:548-557, :1006-1026) -> false: the row does not exist
__device__ __forceinline__ bool mono_motion(const MonoArgs &A, const int model, const float (&M)[9], MonoLds &S, const int lane, const int hyp,
                                            float (&R)[9], float (&t)[3])
{
    const float K[9] = { A.K[0], 0.0f, A.K[2], 0.0f, A.K[1], A.K[3], 0.0f, 0.0f, 1.0f };
    float tmp[9], X[9], U[9], w[3], Vt[9];
    if (model == 1) {
        float invK[9];
        inv3(K, invK);
        mm3(invK, M, tmp);
        mm3(tmp, K, X);
        svd3(S, lane, X, U, w, Vt);
        const float s = (float)(det3(U) * det3(Vt));
        const float d1 = w[0], d2 = w[1], d3 = w[2];
        if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
        const float aux1 = fsqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
        const float aux3 = fsqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
        const int i = hyp & 3;
        const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
        float Rp[9] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, tp[3];
        if (hyp < 4) {
            const float aux_st = fsqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
            const float ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
            const float st = (i == 0 || i == 3) ? aux_st : -aux_st;
            Rp[0] = ct; Rp[2] = -st; Rp[4] = 1.0f; Rp[6] = st; Rp[8] = ct;
            tp[0] = x1 * (d1 - d3); tp[1] = 0.0f * (d1 - d3); tp[2] = (-x3) * (d1 - d3);
        } else {
            const float aux_sp = fsqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
            const float cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
            const float sp = (i == 0 || i == 3) ? aux_sp : -aux_sp;
            Rp[0] = cp; Rp[2] = sp; Rp[4] = -1.0f; Rp[6] = sp; Rp[8] = -cp;
            tp[0] = x1 * (d1 + d3); tp[1] = 0.0f * (d1 + d3); tp[2] = x3 * (d1 + d3);
        }
        float sU[9];
#pragma unroll
        for (int k = 0; k < 9; k++) sU[k] = s * U[k];
        mm3(sU, Rp, tmp);
        mm3(tmp, Vt, R);
#pragma unroll
        for (int r = 0; r < 3; r++) t[r] = (float)dotd(U[3 * r], U[3 * r + 1], U[3 * r + 2], tp[0], tp[1], tp[2]);
        normalise3(t);
        return true;
    }
    if (hyp >= 4) return false;
    float Kt[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Kt[k] = K[(k % 3) * 3 + k / 3];
    mm3(Kt, M, tmp);
    mm3(tmp, K, X);
    svd3(S, lane, X, U, w, Vt);
    t[0] = U[2]; t[1] = U[5]; t[2] = U[8];
    normalise3(t);
    float W[9] = { 0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f };
    if (hyp & 1) { W[1] = 1.0f; W[3] = -1.0f; }   // W^T for R2
    mm3(U, W, tmp);
    mm3(tmp, Vt, R);
    if (det3(R) < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = -R[k];
    }
    if (hyp & 2) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
    return true;
}

// an unsigned key in the order of the floats, every NaN above every number
__device__ __forceinline__ uint32_t cos_key(float c)
{
    if (c != c) return 0xfffffffeu;
    const uint32_t b = __float_as_uint(c);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_cos(uint32_t k)
{
    if (k == 0xfffffffeu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the sum of v over the workgroup's 256 threads, the same in every thread
__device__ __forceinline__ int block_sum(int v, int *part, const int wv, const int lane)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
    __syncthreads();
    if (lane == 0) part[wv] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(256) void k_mono_reconstruct(const MonoArgs A)
{
    __shared__ MonoLds lds[4];
    __shared__ uint32_t keys[MONO_MAX_N];
    __shared__ int part[4];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, tid = threadIdx.x, hyp = blockIdx.x, n = A.n;
    MonoLds &S = lds[wv];

    const MonoSel sel = mono_select(A, lane);
    float M[9] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, R[9], t[3];
    bool exists = false;
    if (sel.model) {
        sel_matrix(A, sel, M);
        exists = mono_motion(A, sel.model, M, S, lane, hyp, R, t);
    }
    MonoDec *D = A.dec;
    if (hyp == 0 && tid == 0) {
        D->model = sel.model; D->best_h = sel.best_h; D->best_f = sel.best_f; D->SH = sel.SH; D->SF = sel.SF; D->pad = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) D->M[k] = M[k];
    }
    if (!exists) {   // the same decision in every thread of the workgroup
        if (tid == 0) {
            D->n_good[hyp] = 0; D->cosp[hyp] = 1.0f;
#pragma unroll
            for (int k = 0; k < 9; k++) D->R[hyp][k] = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) D->t[hyp][k] = 0.0f;
        }
        return;
    }

    // ---- CheckRT (:886-1004)
    const float fx = A.K[0], fy = A.K[1], cx = A.K[2], cy = A.K[3], th2 = A.th2;
    float P2[12];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
        P2[c] = (float)dotd(fx, 0.0f, cx, b0, b1, b2);
        P2[4 + c] = (float)dotd(0.0f, fy, cy, b0, b1, b2);
        P2[8 + c] = (float)dotd(0.0f, 0.0f, 1.0f, b0, b1, b2);
    }
    const float P1[12] = { fx, 0.0f, cx, 0.0f, 0.0f, fy, cy, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f };
    float O2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) O2[r] = (float)(-dotd(R[r], R[3 + r], R[6 + r], t[0], t[1], t[2]));

    float *p3d = A.p3d + 3 * (size_t)hyp * n;
    uint8_t *flag = A.flag + (size_t)hyp * n;
    int mine = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        if (i >= n) break;
        uint8_t fl = 0;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        uint32_t key = 0xffffffffu;
        if ((sel.mask[i >> 6] >> (i & 63)) & 1) {
            const float4 pt = A.pts[i];
            float At[4][4], v[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                At[c][0] = pt.x * P1[8 + c] - P1[c];
                At[c][1] = pt.y * P1[8 + c] - P1[4 + c];
                At[c][2] = pt.z * P2[8 + c] - P2[c];
                At[c][3] = pt.w * P2[8 + c] - P2[4 + c];
            }
            null_vector(At, v);
            px = v[0] / v[3]; py = v[1] / v[3]; pz = v[2] / v[3];
            bool ok = isfinite(px) && isfinite(py) && isfinite(pz);
            float cosp = 0.0f;
            if (ok) {
                const float dist1 = (float)sqrt(dotd(px, py, pz, px, py, pz));
                const float nx = px - O2[0], ny = py - O2[1], nz = pz - O2[2];
                const float dist2 = (float)sqrt(dotd(nx, ny, nz, nx, ny, nz));
                cosp = (float)(dotd(px, py, pz, nx, ny, nz) / (double)(dist1 * dist2));
                const bool low = (double)cosp < 0.99998;
                if (pz <= 0.0f && low) ok = false;
                const float qx = (float)(dotd(R[0], R[1], R[2], px, py, pz) + (double)t[0]);
                const float qy = (float)(dotd(R[3], R[4], R[5], px, py, pz) + (double)t[1]);
                const float qz = (float)(dotd(R[6], R[7], R[8], px, py, pz) + (double)t[2]);
                if (qz <= 0.0f && low) ok = false;
                const float invZ1 = (float)(1.0 / (double)pz);
                const float im1x = fx * px * invZ1 + cx, im1y = fy * py * invZ1 + cy;
                if ((im1x - pt.x) * (im1x - pt.x) + (im1y - pt.y) * (im1y - pt.y) > th2) ok = false;
                const float invZ2 = (float)(1.0 / (double)qz);
                const float im2x = fx * qx * invZ2 + cx, im2y = fy * qy * invZ2 + cy;
                if ((im2x - pt.z) * (im2x - pt.z) + (im2y - pt.w) * (im2y - pt.w) > th2) ok = false;
                if (ok) { fl = low ? 2 : 1; key = cos_key(cosp); mine++; }
            }
            if (!ok) { px = 0.0f; py = 0.0f; pz = 0.0f; }
        }
        flag[i] = fl;
        p3d[3 * (size_t)i] = px; p3d[3 * (size_t)i + 1] = py; p3d[3 * (size_t)i + 2] = pz;
        keys[i] = key;
    }
    const int n_good = block_sum(mine, part, wv, lane);   // its barriers also publish keys[]

    // ---- the cosine of rank min(50, n_good - 1): the smallest key with more than `rank` keys at or below it, bit by bit
    float cosp = 1.0f;
    if (n_good > 0) {
        const int rank = n_good - 1 < 50 ? n_good - 1 : 50;
        uint32_t kk = 0;
        for (int bit = 31; bit >= 0; bit--) {
            const uint32_t trial = kk | ((1u << bit) - 1u);
            int cnt = 0;
            for (int i = tid; i < n; i += 256) cnt += keys[i] <= trial ? 1 : 0;
            if (block_sum(cnt, part, wv, lane) <= rank) kk |= 1u << bit;
        }
        cosp = key_cos(kk);
    }
    if (tid == 0) {
        D->n_good[hyp] = n_good; D->cosp[hyp] = cosp;
#pragma unroll
        for (int k = 0; k < 9; k++) D->R[hyp][k] = canon(R[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) D->t[hyp][k] = canon(t[k]);
    }
}

__global__ __launch_bounds__(256) void k_mono_decide(const MonoArgs A)
{
    const int tid = threadIdx.x, lane = threadIdx.x & 63, n = A.n;
    MonoDec *D = A.dec;
    const MonoSel sel = mono_select(A, lane);
    int N = 0;
    if (sel.model) for (int wd = 0; wd < A.words; wd++) N += __popcll(sel.mask[wd]);

    bool ok = false;
    int winner = -1;
    if (sel.model == 1) {   // :769-811
        int bestGood = 0, second = 0;
        float bestCos = 1.0f;
        for (int i = 0; i < 8; i++) {
            const int nGood = D->n_good[i];
            if (nGood > bestGood) { second = bestGood; bestGood = nGood; winner = i; bestCos = D->cosp[i]; }
            else if (nGood > second) second = nGood;
        }
        const bool par = winner >= 0 && bestCos >= -1.0f && bestCos < A.c_ge;
        ok = (double)second < 0.75 * (double)bestGood && par && bestGood > A.min_tri && (double)bestGood > 0.9 * (double)N;
    } else if (sel.model == 2) {   // :569-639
        const int g0 = D->n_good[0], g1 = D->n_good[1], g2 = D->n_good[2], g3 = D->n_good[3];
        const int m23 = g2 > g3 ? g2 : g3, m123 = g1 > m23 ? g1 : m23, maxGood = g0 > m123 ? g0 : m123;
        const int n9 = (int)(0.9 * (double)N), nMinGood = n9 > A.min_tri ? n9 : A.min_tri;
        const double lim = 0.7 * (double)maxGood;
        const int nsimilar = ((double)g0 > lim) + ((double)g1 > lim) + ((double)g2 > lim) + ((double)g3 > lim);
        if (!(maxGood < nMinGood || nsimilar > 1)) {
            winner = maxGood == g0 ? 0 : maxGood == g1 ? 1 : maxGood == g2 ? 2 : 3;
            const float c = D->cosp[winner];
            ok = c >= -1.0f && c < A.c_gt;
        }
    }
    for (int i = tid; i < 3 * A.n1; i += 256) A.P3D[i] = 0.0f;
    for (int i = tid; i < A.n1; i += 256) A.tri[i] = 0;
    __syncthreads();
    if (ok) {
        const float *p3d = A.p3d + 3 * (size_t)winner * n;
        const uint8_t *flag = A.flag + (size_t)winner * n;
        for (int i = tid; i < n; i += 256) {
            const uint8_t fl = flag[i];
            if (!fl) continue;
            const int f = A.first[i];   // strictly rising: no two matches write one slot
            A.P3D[3 * (size_t)f] = p3d[3 * (size_t)i]; A.P3D[3 * (size_t)f + 1] = p3d[3 * (size_t)i + 1]; A.P3D[3 * (size_t)f + 2] = p3d[3 * (size_t)i + 2];
            A.tri[f] = fl == 2 ? 1 : 0;
        }
    }
    if (tid == 0) { D->ok = ok ? 1 : 0; D->winner = winner; }
}

}   // namespace

// ---------------------------------------------------------------- host side (include/orbx.h: orbx_mono_init_hypotheses)

// Normalize (:831-883) over all keypoints of one frame, in the reference's order -> meanX meanY sX sY and T
static void mono_normalize(const float *xy, int N, float nrm[4], float T[9])
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < N; i++) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
    meanX = meanX / N; meanY = meanY / N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; i++) { meanDevX += fabsf(xy[2 * i] - meanX); meanDevY += fabsf(xy[2 * i + 1] - meanY); }
    meanDevX = meanDevX / N; meanDevY = meanDevY / N;
    const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
    nrm[0] = meanX; nrm[1] = meanY; nrm[2] = sX; nrm[3] = sY;
    const float t[9] = { sX, 0.0f, -meanX * sX, 0.0f, sY, -meanY * sY, 0.0f, 0.0f, 1.0f };
    memcpy(T, t, sizeof t);
}

static void mono_inv3_host(const float m[9], float o[9])
{
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
    double d = (m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6)) + m2 * (m3 * m7 - m4 * m6);
    if (d == 0.0) { for (int k = 0; k < 9; k++) o[k] = 0.0f; return; }
    d = 1.0 / d;
    o[0] = (float)((m4 * m8 - m5 * m7) * d); o[1] = (float)((m2 * m7 - m1 * m8) * d); o[2] = (float)((m1 * m5 - m2 * m4) * d);
    o[3] = (float)((m5 * m6 - m3 * m8) * d); o[4] = (float)((m0 * m8 - m2 * m6) * d); o[5] = (float)((m2 * m3 - m0 * m5) * d);
    o[6] = (float)((m3 * m7 - m4 * m6) * d); o[7] = (float)((m1 * m6 - m0 * m7) * d); o[8] = (float)((m0 * m4 - m1 * m3) * d);
}

static float mono_degrees(float c)
{
    const float d = (float)(acos((double)c) * 180 / 3.1415926535897932384626433832795);   // CV_PI
    return d != d ? nanf("") : d;   // "NaN" of the contract
}

// the smallest float c of [-1, 1] whose parallax fails the test against min_parallax (`>=` or `>`); the float above 1 when none fails
static float mono_cos_threshold(float min_parallax, bool ge)
{
    auto key = [](float c) { uint32_t b; memcpy(&b, &c, 4); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); };
    auto unkey = [](uint32_t k) { const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float c; memcpy(&c, &b, 4); return c; };
    auto pass = [&](uint32_t k) { const float d = mono_degrees(unkey(k)); return ge ? d >= min_parallax : d > min_parallax; };
    uint32_t lo = key(-1.0f), hi = key(1.0f) + 1;   // the answer lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pass(mid)) lo = mid + 1; else hi = mid;
    }
    return unkey(lo);
}

// the refusals that do not concern the samples
static int mono_check_frames(const char *who, const orbx_mono_init_job &J)
{
    if (!J.xy1 || !J.xy2 || !J.matches) { orbx_set_error("%s: a NULL array", who); return ORBX_E_INVALID; }
    if (J.n < 8 || J.n > MONO_MAX_N) { orbx_set_error("%s: n = %d outside [8, %d]", who, J.n, MONO_MAX_N); return ORBX_E_INVALID; }
    if (J.n1 < J.n || J.n1 > 65535 || J.n2 < J.n || J.n2 > 65535) {
        orbx_set_error("%s: n1 = %d, n2 = %d outside [n, 65535]", who, J.n1, J.n2);
        return ORBX_E_INVALID;
    }
    for (int i = 0; i < J.n; i++) {
        const int a = J.matches[2 * i], b = J.matches[2 * i + 1];
        if (a < 0 || a >= J.n1 || b < 0 || b >= J.n2) { orbx_set_error("%s: match %d: an index outside its frame", who, i); return ORBX_E_INVALID; }
        if (i && a <= J.matches[2 * i - 2]) { orbx_set_error("%s: match %d: first is not strictly rising", who, i); return ORBX_E_INVALID; }
    }
    return ORBX_OK;
}

static int mono_check_samples(const char *who, const orbx_mono_init_job &J)
{
    if (J.n_hyp < 1 || J.n_hyp > 1024) { orbx_set_error("%s: n_hyp = %d outside [1, 1024]", who, J.n_hyp); return ORBX_E_INVALID; }
    if (!J.samples) { orbx_set_error("%s: a NULL array", who); return ORBX_E_INVALID; }
    for (int h = 0; h < J.n_hyp; h++) {
        const int32_t *s = J.samples + 8 * (size_t)h;
        for (int a = 0; a < 8; a++) {
            if (s[a] < 0 || s[a] >= J.n) { orbx_set_error("%s: hypothesis %d: a sample index outside [0, %d)", who, h, J.n); return ORBX_E_INVALID; }
            for (int b = 0; b < a; b++)
                if (s[a] == s[b]) { orbx_set_error("%s: hypothesis %d: two equal sample indices", who, h); return ORBX_E_INVALID; }
        }
    }
    return ORBX_OK;
}

// what a call downloads behind MonoDec
struct MonoPlan { size_t o_dec, o_p3d, o_tri, o_score, o_mats, o_bits, o_wp3d, o_wflag, head, work; };

// The staging of one call: the blob (matches gathered, firsts, samples, mask) up, the work area laid out, the arguments filled.  table:
// the call evaluates the table; recon: it reconstructs.  What the call downloads leads the work area: the table, or the decision and the points.
static int mono_stage(CallCtx *c, const orbx_mono_init_job &J, bool table, bool recon, const uint64_t *mask, MonoArgs &A, MonoPlan &P)
{
    const size_t n = (size_t)J.n, n1 = (size_t)J.n1, nh = table ? (size_t)J.n_hyp : 0, words = (n + 63) / 64;
    BlobCursor w = { nullptr, nullptr, 0 };
    memset(&P, 0, sizeof P);
    if (recon) { P.o_dec = w.take(sizeof(MonoDec)); P.o_p3d = w.take(12 * n1); P.o_tri = w.take(n1); P.head = w.o; }
    if (table) { P.o_score = w.take(8 * nh); P.o_mats = w.take(72 * nh); P.o_bits = w.take(16 * nh * words); if (!recon) P.head = w.o; }
    if (recon) { P.o_wp3d = w.take(96 * n); P.o_wflag = w.take(8 * n); }
    P.work = w.o;
    const size_t blob = a16(16 * n) + a16(4 * n) + a16(32 * nh) + a16(8 * words);
    int rc = call_reserve(c, blob, P.work, P.head);
    if (rc) return rc;

    memset(&A, 0, sizeof A);
    A.n = J.n; A.n1 = J.n1; A.n_hyp = (int)nh; A.words = (int)words;
    BlobCursor b = { c->h_blob, c->d_blob, 0 };
    {   // the packing copy: (u1, v1, u2, v2) and first per match
        const size_t at = b.take(16 * n), af = b.take(4 * n);
        float *pts = (float *)(b.h + at);
        int32_t *first = (int32_t *)(b.h + af);
        for (size_t i = 0; i < n; i++) {
            const int m1 = J.matches[2 * i], m2 = J.matches[2 * i + 1];
            pts[4 * i] = J.xy1[2 * m1]; pts[4 * i + 1] = J.xy1[2 * m1 + 1]; pts[4 * i + 2] = J.xy2[2 * m2]; pts[4 * i + 3] = J.xy2[2 * m2 + 1];
            first[i] = m1;
        }
        A.pts = (const float4 *)(b.d + at); A.first = (const int32_t *)(b.d + af);
    }
    if (table) {
        A.samples = (const int32_t *)b.put(J.samples, 32 * nh);
        mono_normalize(J.xy1, J.n1, A.norm1, A.T1);
        mono_normalize(J.xy2, J.n2, A.norm2, A.T2);
        mono_inv3_host(A.T2, A.T2inv);
        A.score = (float *)(c->d_work + P.o_score); A.mats = (float *)(c->d_work + P.o_mats); A.bits = (uint64_t *)(c->d_work + P.o_bits);
    }
    if (mask) A.given_mask = (const uint64_t *)b.put(mask, 8 * words);
    const float s2 = J.sigma * J.sigma;
    A.inv_sigma2 = (float)(1.0 / (double)s2);
    A.th2 = (float)(4.0 * (double)s2);
    memcpy(A.K, J.K, sizeof A.K);
    if (recon) {
        A.c_gt = mono_cos_threshold(J.min_parallax, false);
        A.c_ge = mono_cos_threshold(J.min_parallax, true);
        A.min_tri = J.min_triangulated;
        A.dec = (MonoDec *)(c->d_work + P.o_dec); A.P3D = (float *)(c->d_work + P.o_p3d); A.tri = c->d_work + P.o_tri;
        A.p3d = (float *)(c->d_work + P.o_wp3d); A.flag = c->d_work + P.o_wflag;
    }
    return call_upload(c, b.o);
}

extern "C" int orbx_mono_init_hypotheses(int device, orbx_mono_init_job *job)
{
    const char *who = "orbx_mono_init_hypotheses";
    if (!job) { orbx_set_error("%s: a NULL job", who); return ORBX_E_INVALID; }
    const orbx_mono_init_job &J = *job;
    int rc = mono_check_frames(who, J);
    if (!rc) rc = mono_check_samples(who, J);
    if (rc) return rc;
    if (!J.score_h || !J.score_f || !J.H21 || !J.F21 || !J.bits_h || !J.bits_f) { orbx_set_error("%s: a NULL array", who); return ORBX_E_INVALID; }
    CallCtx *c;
    if ((rc = orbx_call_ctx(device, &c))) return rc;
    MonoArgs A;
    MonoPlan P;
    if ((rc = mono_stage(c, J, true, false, nullptr, A, P))) return rc;
    hipLaunchKernelGGL(k_mono_hyp, dim3((unsigned)((2 * J.n_hyp + 3) / 4)), dim3(256), 0, c->stream, A);   // one wave per (model, hypothesis)
    if ((rc = call_fetch(c, P.head))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    const size_t nh = (size_t)J.n_hyp, wb = 8 * nh * (size_t)A.words;
    memcpy(J.score_h, ho + P.o_score, 4 * nh); memcpy(J.score_f, ho + P.o_score + 4 * nh, 4 * nh);
    memcpy(J.H21, ho + P.o_mats, 36 * nh); memcpy(J.F21, ho + P.o_mats + 36 * nh, 36 * nh);
    memcpy(J.bits_h, ho + P.o_bits, wb); memcpy(J.bits_f, ho + P.o_bits + wb, wb);
    return ORBX_OK;
}

extern "C" int orbx_mono_init_reconstruct(int device, const orbx_mono_init_job *job, int model, const float *M, const uint64_t *mask,
                                          orbx_mono_init_recon *out)
{
    const char *who = "orbx_mono_init_reconstruct";
    if (!job || !M || !mask || !out || !out->P3D || !out->triangulated) { orbx_set_error("%s: a NULL argument", who); return ORBX_E_INVALID; }
    const orbx_mono_init_job &J = *job;
    if (model != 1 && model != 2) { orbx_set_error("%s: model = %d outside {1, 2}", who, model); return ORBX_E_INVALID; }
    int rc = mono_check_frames(who, J);
    if (rc) return rc;
    if (J.n % 64 && (mask[J.n / 64] >> (J.n % 64))) { orbx_set_error("%s: a mask bit at or above n", who); return ORBX_E_INVALID; }
    CallCtx *c;
    if ((rc = orbx_call_ctx(device, &c))) return rc;
    MonoArgs A;
    MonoPlan P;
    if ((rc = mono_stage(c, J, false, true, mask, A, P))) return rc;
    A.given_model = model;
    memcpy(A.given_M, M, sizeof A.given_M);
    hipLaunchKernelGGL(k_mono_reconstruct, dim3(8), dim3(256), 0, c->stream, A);   // one workgroup per motion hypothesis
    hipLaunchKernelGGL(k_mono_decide, dim3(1), dim3(256), 0, c->stream, A);
    if ((rc = call_fetch(c, P.head))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    const MonoDec *D = (const MonoDec *)(ho + P.o_dec);
    out->ok = D->ok; out->winner = D->winner;
    memcpy(out->n_good, D->n_good, sizeof out->n_good); memcpy(out->cos_parallax, D->cosp, sizeof out->cos_parallax);
    memcpy(out->R, D->R, sizeof out->R); memcpy(out->t, D->t, sizeof out->t);
    memcpy(out->P3D, ho + P.o_p3d, 12 * (size_t)J.n1); memcpy(out->triangulated, ho + P.o_tri, (size_t)J.n1);
    return ORBX_OK;
}

extern "C" int orbx_mono_init_initialize(int device, orbx_mono_init_job *job, orbx_mono_init_result *res)
{
    const char *who = "orbx_mono_init_initialize";
    if (!job || !res || !res->P3D || !res->triangulated) { orbx_set_error("%s: a NULL argument", who); return ORBX_E_INVALID; }
    const orbx_mono_init_job &J = *job;
    int rc = mono_check_frames(who, J);
    if (!rc) rc = mono_check_samples(who, J);
    if (rc) return rc;
    CallCtx *c;
    if ((rc = orbx_call_ctx(device, &c))) return rc;
    MonoArgs A;
    MonoPlan P;
    if ((rc = mono_stage(c, J, true, true, nullptr, A, P))) return rc;
    hipLaunchKernelGGL(k_mono_hyp, dim3((unsigned)((2 * J.n_hyp + 3) / 4)), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(k_mono_reconstruct, dim3(8), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(k_mono_decide, dim3(1), dim3(256), 0, c->stream, A);
    if ((rc = call_fetch(c, P.head))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    const MonoDec *D = (const MonoDec *)(ho + P.o_dec);
    res->ok = D->ok; res->model = D->model; res->best_h = D->best_h; res->best_f = D->best_f; res->SH = D->SH; res->SF = D->SF;
    memcpy(res->M, D->M, sizeof res->M);
    res->winner = D->winner;
    memset(res->R21, 0, sizeof res->R21); memset(res->t21, 0, sizeof res->t21);
    if (D->ok) { memcpy(res->R21, D->R[D->winner], sizeof res->R21); memcpy(res->t21, D->t[D->winner], sizeof res->t21); }
    res->parallax = D->winner >= 0 ? mono_degrees(D->cosp[D->winner]) : 0.0f;   // the epilogue: the C library's acos, on the host
    memcpy(res->n_good, D->n_good, sizeof res->n_good); memcpy(res->cos_parallax, D->cosp, sizeof res->cos_parallax);
    memcpy(res->P3D, ho + P.o_p3d, 12 * (size_t)J.n1); memcpy(res->triangulated, ho + P.o_tri, (size_t)J.n1);
    return ORBX_OK;
}

// tools/init_baseline.cc -- the table of orbx_mono_init_hypotheses (include/orbx.h: Normalize, the one Jacobi routine, H21i / F21i,
// CheckHomography / CheckFundamental for every sample row) as a plain C++ loop on ONE host core, without cv::Mat: the same arithmetic in
// the same order, so its bits can be compared with the device's (the score keeps the contract's 64 partial sums and their butterfly).
// A LOWER BOUND for a host implementation, not the reference: the reference's Initializer needs OpenCV (cv::SVDecomp on cv::Mat, two
// threads), nothing in this repository has timed it, and no speed-up over it may be claimed from this figure.
//   g++ -O2 -ffp-contract=off -std=c++11 -shared -fPIC -I include tools/init_baseline.cc -o libinit_baseline.so   (tools/bench_init.py)
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <orbx.h>

namespace {

const double EPS2 = (double)(2.0f * 1.1920928955078125e-7f);

double dotd(float a0, float a1, float a2, float b0, float b1, float b2) { return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2; }

void mm3(const float *X, const float *Y, float *Z)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Z[3 * r + c] = (float)dotd(X[3 * r], X[3 * r + 1], X[3 * r + 2], Y[c], Y[3 + c], Y[6 + c]);
}

void inv3(const float *m, float *o)
{
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
    double d = (m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6)) + m2 * (m3 * m7 - m4 * m6);
    if (d == 0.0) { for (int k = 0; k < 9; k++) o[k] = 0.0f; return; }
    d = 1.0 / d;
    o[0] = (float)((m4 * m8 - m5 * m7) * d); o[1] = (float)((m2 * m7 - m1 * m8) * d); o[2] = (float)((m1 * m5 - m2 * m4) * d);
    o[3] = (float)((m5 * m6 - m3 * m8) * d); o[4] = (float)((m0 * m8 - m2 * m6) * d); o[5] = (float)((m2 * m3 - m0 * m5) * d);
    o[6] = (float)((m3 * m7 - m4 * m6) * d); o[7] = (float)((m1 * m6 - m0 * m7) * d); o[8] = (float)((m0 * m4 - m1 * m3) * d);
}

void normalize(const float *xy, int N, float nrm[4], float T[9])
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < N; i++) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
    meanX = meanX / N; meanY = meanY / N;
    float devX = 0, devY = 0;
    for (int i = 0; i < N; i++) { devX += fabsf(xy[2 * i] - meanX); devY += fabsf(xy[2 * i + 1] - meanY); }
    devX = devX / N; devY = devY / N;
    const float sX = (float)(1.0 / (double)devX), sY = (float)(1.0 / (double)devY);
    nrm[0] = meanX; nrm[1] = meanY; nrm[2] = sX; nrm[3] = sY;
    const float t[9] = { sX, 0.0f, -meanX * sX, 0.0f, sY, -meanY * sY, 0.0f, 0.0f, 1.0f };
    memcpy(T, t, sizeof t);
}

// "SVD" of the contract: B = A (m rows) stacked on V (n rows), row stride 9, n odd -> w2[n]
void svd(float *B, int m, int n, double *w2)
{
    for (int e = 0; e < n * n; e++) B[(m + e / n) * 9 + e % n] = (e / n == e % n) ? 1.0f : 0.0f;
    const int rows = m + n, half = (n + 1) >> 1;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        for (int r = 0; r < n; r++)
            for (int k = 1; k < half; k++) {
                const int a = (r + k) % n, b = (r + n - k) % n, p = a < b ? a : b, q = a < b ? b : a;
                double va[16], vb[16], vg[16];     // the stated butterfly over 16 slots, one row each
                for (int i = 0; i < 16; i++) {
                    const double x = i < m ? (double)B[i * 9 + p] : 0.0, y = i < m ? (double)B[i * 9 + q] : 0.0;
                    va[i] = 0.0 + x * x; vb[i] = 0.0 + y * y; vg[i] = i < m ? 0.0 + x * y : 0.0;
                }
                for (int st = 8; st >= 1; st >>= 1)     // slot 0 of the xor butterfly: i ^ st == i + st for i < st, and a + b == b + a
                    for (int i = 0; i < st; i++) { va[i] = va[i] + va[i + st]; vb[i] = vb[i] + vb[i + st]; vg[i] = vg[i] + vg[i + st]; }
                const double al = va[0], be = vb[0], g = vg[0];
                if (fabs(g) <= EPS2 * sqrt(al * be)) continue;
                changed = true;
                const double g2 = g * 2.0, beta = al - be, gamma = sqrt(g2 * g2 + beta * beta);
                float c, s;
                if (beta < 0.0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(g2 / ((gamma * (double)s) * 2.0));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2.0));
                    s = (float)(g2 / ((gamma * (double)c) * 2.0));
                }
                for (int rr = 0; rr < rows; rr++) {
                    const float x = B[rr * 9 + p], y = B[rr * 9 + q];
                    B[rr * 9 + p] = c * x + s * y;
                    B[rr * 9 + q] = (-s) * x + c * y;
                }
            }
        if (!changed) break;
    }
    for (int j = 0; j < n; j++) {
        double s2 = 0.0;
        for (int i = 0; i < m; i++) { const double x = (double)B[i * 9 + j]; s2 = s2 + x * x; }
        w2[j] = s2;
    }
}

void null9(float *B, int m, float *X)
{
    double w2[9];
    svd(B, m, 9, w2);
    int col = 0;
    double best = w2[0];
    for (int j = 1; j < 9; j++) if (w2[j] <= best) { best = w2[j]; col = j; }
    for (int k = 0; k < 9; k++) X[k] = B[(m + k) * 9 + col];
}

void usv3(const float *M, float *U, float *w, float *Vt)
{
    float B[6 * 9];
    double w2[3];
    for (int k = 0; k < 9; k++) B[(k / 3) * 9 + k % 3] = M[k];
    svd(B, 3, 3, w2);
    int order[3], used = 0;
    for (int r = 0; r < 3; r++) {
        int best = -1;
        for (int j = 0; j < 3; j++) {
            if ((used >> j) & 1) continue;
            if (best < 0 || w2[j] > w2[best]) best = j;
        }
        order[r] = best; used |= 1 << best;
    }
    for (int r = 0; r < 3; r++) {
        const int o = order[r];
        const double wd = sqrt(w2[o]);
        const float sc = wd > (double)FLT_MIN ? (float)(1.0 / wd) : 0.0f;
        w[r] = (float)wd;
        for (int i = 0; i < 3; i++) { U[3 * i + r] = B[i * 9 + o] * sc; Vt[3 * r + i] = B[(3 + i) * 9 + o]; }
    }
}

float canon(float x) { return x != x ? nanf("") : x; }

}   // namespace

// the whole table of one job into its output arrays, as orbx_mono_init_hypotheses returns it; 0, or -1 for a job the call would refuse for its sizes
extern "C" int mono_init_table_loop(const orbx_mono_init_job *J)
{
    const int n = J->n, nh = J->n_hyp, words = (n + 63) / 64;
    if (n < 8 || n > 8192 || nh < 1) return -1;
    float nrm1[4], nrm2[4], T1[9], T2[9], T2inv[9], T2t[9];
    normalize(J->xy1, J->n1, nrm1, T1);
    normalize(J->xy2, J->n2, nrm2, T2);
    inv3(T2, T2inv);
    for (int k = 0; k < 9; k++) T2t[k] = T2[(k % 3) * 3 + k / 3];
    static float pts[4 * 8192];
    for (int i = 0; i < n; i++) {
        const int m1 = J->matches[2 * i], m2 = J->matches[2 * i + 1];
        pts[4 * i] = J->xy1[2 * m1]; pts[4 * i + 1] = J->xy1[2 * m1 + 1]; pts[4 * i + 2] = J->xy2[2 * m2]; pts[4 * i + 3] = J->xy2[2 * m2 + 1];
    }
    const float s2 = J->sigma * J->sigma, inv_s2 = (float)(1.0 / (double)s2);
    for (int model = 0; model < 2; model++)
        for (int h = 0; h < nh; h++) {
            float B[25 * 9], X[9], M21[9], M12[9], tmp[9];
            const int m = model ? 8 : 16;
            for (int j = 0; j < 8; j++) {
                const float *pt = pts + 4 * J->samples[8 * h + j];
                const float u1 = (pt[0] - nrm1[0]) * nrm1[2], v1 = (pt[1] - nrm1[1]) * nrm1[3];
                const float u2 = (pt[2] - nrm2[0]) * nrm2[2], v2 = (pt[3] - nrm2[1]) * nrm2[3];
                if (!model) {
                    const float r0[9] = { 0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2 };
                    const float r1[9] = { u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, (-u2) * u1, (-u2) * v1, -u2 };
                    memcpy(B + 2 * j * 9, r0, sizeof r0); memcpy(B + (2 * j + 1) * 9, r1, sizeof r1);
                } else {
                    const float r0[9] = { u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0f };
                    memcpy(B + j * 9, r0, sizeof r0);
                }
            }
            null9(B, m, X);
            if (!model) {
                mm3(T2inv, X, tmp); mm3(tmp, T1, M21); inv3(M21, M12);
            } else {
                float U[9], w[3], Vt[9], Dg[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
                usv3(X, U, w, Vt);
                Dg[0] = w[0]; Dg[4] = w[1];
                mm3(U, Dg, tmp); mm3(tmp, Vt, X); mm3(T2t, X, tmp); mm3(tmp, T1, M21);
            }
            const float th = model ? 3.841f : 5.991f, thScore = 5.991f;
            float acc[64];
            for (int l = 0; l < 64; l++) acc[l] = 0.0f;
            uint64_t *bits = (model ? J->bits_f : J->bits_h) + (size_t)h * words;
            for (int wd = 0; wd < words; wd++) bits[wd] = 0;
            for (int i = 0; i < n; i++) {
                const float u1 = pts[4 * i], v1 = pts[4 * i + 1], u2 = pts[4 * i + 2], v2 = pts[4 * i + 3];
                float chi1, chi2;
                if (!model) {
                    const float w2in1inv = (float)(1.0 / (double)(M12[6] * u2 + M12[7] * v2 + M12[8]));
                    const float u2in1 = (M12[0] * u2 + M12[1] * v2 + M12[2]) * w2in1inv, v2in1 = (M12[3] * u2 + M12[4] * v2 + M12[5]) * w2in1inv;
                    chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_s2;
                    const float w1in2inv = (float)(1.0 / (double)(M21[6] * u1 + M21[7] * v1 + M21[8]));
                    const float u1in2 = (M21[0] * u1 + M21[1] * v1 + M21[2]) * w1in2inv, v1in2 = (M21[3] * u1 + M21[4] * v1 + M21[5]) * w1in2inv;
                    chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_s2;
                } else {
                    const float a2 = M21[0] * u1 + M21[1] * v1 + M21[2], b2 = M21[3] * u1 + M21[4] * v1 + M21[5], c2 = M21[6] * u1 + M21[7] * v1 + M21[8];
                    const float num2 = a2 * u2 + b2 * v2 + c2;
                    chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2;
                    const float a1 = M21[0] * u2 + M21[3] * v2 + M21[6], b1 = M21[1] * u2 + M21[4] * v2 + M21[7], c1 = M21[2] * u2 + M21[5] * v2 + M21[8];
                    const float num1 = a1 * u1 + b1 * v1 + c1;
                    chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2;
                }
                bool in = true;
                float &a = acc[i & 63];
                if (chi1 > th) in = false; else a = a + (thScore - chi1);
                if (chi2 > th) in = false; else a = a + (thScore - chi2);
                if (in) bits[i >> 6] |= (uint64_t)1 << (i & 63);
            }
            for (int s = 32; s >= 1; s >>= 1) {
                float nx[64];
                for (int l = 0; l < 64; l++) nx[l] = acc[l] + acc[l ^ s];
                memcpy(acc, nx, sizeof nx);
            }
            (model ? J->score_f : J->score_h)[h] = canon(acc[0]);
            float *o = (model ? J->F21 : J->H21) + 9 * (size_t)h;
            for (int k = 0; k < 9; k++) o[k] = canon(M21[k]);
        }
    return 0;
}

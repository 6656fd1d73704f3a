// tools/sim3_baseline.cc -- the hypothesis loop of Sim3Solver (reference src/Sim3Solver.cc:233-371) restated in plain C++ WITHOUT
// cv::Mat: the arithmetic of include/orbx.h (orbx_sim3_hypotheses) on a host core, hypothesis by hypothesis.  tools/bench_sim3.py compiles
// it (g++ -O2 -ffp-contract=off -shared) and times it beside the device calls: a LOWER BOUND on what the reference's loop costs, whose
// four cv::Mat per point and hypothesis, cv::eigen, cv::Rodrigues and allocations are all absent here.  It is a lower bound and not the
// reference, and says nothing about OpenCV's speed.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <orbx.h>

namespace {

inline double dotd(float a0, float a1, float a2, float b0, float b1, float b2) { return ((double)a0 * b0 + (double)a1 * b1) + (double)a2 * b2; }
inline float hyp(float a, float b) { return (float)sqrt((double)a * a + (double)b * b); }
inline void rot(float &a, float &b, float c, float s)
{
    const float a0 = a, b0 = b;
    a = a0 * c - b0 * s;
    b = a0 * s + b0 * c;
}

bool jacobi_rot(int K, int L, float A[4][4], float W[4], float V[4][4])
{
    const float p = A[K][L];
    if ((double)p * (double)p <= (1.0 / 70368744177664.0) /* 2^-46 */ * fabs((double)W[K] * (double)W[L])) return false;
    const float y = (W[L] - W[K]) * 0.5f;
    float t = fabsf(y) + hyp(p, y);
    float s = hyp(p, t);
    const float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0.f) { s = -s; t = -t; }
    A[K][L] = 0.f;
    W[K] -= t;
    W[L] += t;
    for (int i = 0; i < K; i++) rot(A[i][K], A[i][L], c, s);
    for (int i = K + 1; i < L; i++) rot(A[K][i], A[i][L], c, s);
    for (int i = L + 1; i < 4; i++) rot(A[K][i], A[L][i], c, s);
    for (int i = 0; i < 4; i++) rot(V[K][i], V[L][i], c, s);
    return true;
}

void top_eigenvector(float A[4][4], float q[4])
{
    float V[4][4], W[4];
    for (int i = 0; i < 4; i++) {
        W[i] = A[i][i];
        for (int k = 0; k < 4; k++) V[i][k] = i == k ? 1.0f : 0.0f;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        for (int k = 0; k < 3; k++)
            for (int l = k + 1; l < 4; l++) changed |= jacobi_rot(k, l, A, W, V);
        if (!changed) break;
    }
    int best = 0;
    for (int i = 1; i < 4; i++)
        if (W[i] > W[best]) best = i;
    for (int k = 0; k < 4; k++) q[k] = V[best][k];
}

inline float pix(float f, float c, float X, float invz)
{
    const float x = X * invz;
    return f * x + c;
}

inline float err2(float u0, float v0, float u1, float v1)
{
    const float d0 = u0 - u1, d1 = v0 - v1;
    return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}

void one_hypothesis(const orbx_sim3_job &J, int h)
{
    const int n = J.n, words = (n + 63) / 64;
    const int32_t *sm = J.samples + 3 * (size_t)h;
    uint64_t *bits = J.inlier_bits + (size_t)h * words;
    float P1[3][3], P2[3][3], O1[3], O2[3];
    for (int i = 0; i < 3; i++)
        for (int r = 0; r < 3; r++) { P1[r][i] = J.X1[3 * sm[i] + r]; P2[r][i] = J.X2[3 * sm[i] + r]; }
    for (int r = 0; r < 3; r++) {
        O1[r] = (float)((double)((P1[r][0] + P1[r][1]) + P1[r][2]) * (1.0 / 3.0));
        O2[r] = (float)((double)((P2[r][0] + P2[r][1]) + P2[r][2]) * (1.0 / 3.0));
        for (int i = 0; i < 3; i++) { P1[r][i] -= O1[r]; P2[r][i] -= O2[r]; }
    }
    float M[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) M[r][c] = (float)dotd(P2[r][0], P2[r][1], P2[r][2], P1[c][0], P1[c][1], P1[c][2]);
    float A[4][4];
    memset(A, 0, sizeof A);
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[0][1] = M[1][2] - M[2][1];
    A[0][2] = M[2][0] - M[0][2];
    A[0][3] = M[0][1] - M[1][0];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[1][2] = M[0][1] + M[1][0];
    A[1][3] = M[2][0] + M[0][2];
    A[2][2] = ((-M[0][0]) + M[1][1]) - M[2][2];
    A[2][3] = M[1][2] + M[2][1];
    A[3][3] = ((-M[0][0]) - M[1][1]) + M[2][2];
    float q[4];
    top_eigenvector(A, q);
    if (q[1] == 0.f && q[2] == 0.f && q[3] == 0.f) {
        const uint32_t qnan = 0x7fc00000u;
        for (int k = 0; k < 13; k++) memcpy(J.srt + 13 * (size_t)h + k, &qnan, 4);
        for (int wd = 0; wd < words; wd++) bits[wd] = 0;
        J.n_inliers[h] = 0;
        return;
    }
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const double n2 = ((ww + xx) + yy) + zz;
    float R[3][3];
    R[0][0] = (float)((((ww + xx) - yy) - zz) / n2);
    R[0][1] = (float)((2.0 * (xy - wz)) / n2);
    R[0][2] = (float)((2.0 * (xz + wy)) / n2);
    R[1][0] = (float)((2.0 * (xy + wz)) / n2);
    R[1][1] = (float)((((ww - xx) + yy) - zz) / n2);
    R[1][2] = (float)((2.0 * (yz - wx)) / n2);
    R[2][0] = (float)((2.0 * (xz - wy)) / n2);
    R[2][1] = (float)((2.0 * (yz + wx)) / n2);
    R[2][2] = (float)((((ww - xx) - yy) + zz) / n2);
    float s12 = 1.0f;
    if (!J.fix_scale) {
        double nom = 0.0, den = 0.0;
        for (int r = 0; r < 3; r++)
            for (int i = 0; i < 3; i++) {
                const float p3 = (float)dotd(R[r][0], R[r][1], R[r][2], P2[0][i], P2[1][i], P2[2][i]);
                nom += (double)P1[r][i] * (double)p3;
                den += (double)(p3 * p3);
            }
        s12 = (float)(nom / den);
    }
    const double sd = (double)s12, si = 1.0 / (double)s12;
    float t12[3], sR[3][3], sRi[3][3], t21[3];
    for (int r = 0; r < 3; r++) t12[r] = (float)((double)O1[r] - sd * dotd(R[r][0], R[r][1], R[r][2], O2[0], O2[1], O2[2]));
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { sR[r][c] = (float)(sd * (double)R[r][c]); sRi[r][c] = (float)(si * (double)R[c][r]); }
    for (int r = 0; r < 3; r++) t21[r] = (float)(-dotd(sRi[r][0], sRi[r][1], sRi[r][2], t12[0], t12[1], t12[2]));
    float *out = J.srt + 13 * (size_t)h;
    out[0] = s12;
    for (int k = 0; k < 9; k++) out[1 + k] = R[k / 3][k % 3];
    for (int k = 0; k < 3; k++) out[10 + k] = t12[k];

    const float fx1 = J.K1[0], fy1 = J.K1[1], cx1 = J.K1[2], cy1 = J.K1[3];
    const float fx2 = J.K2[0], fy2 = J.K2[1], cx2 = J.K2[2], cy2 = J.K2[3];
    int count = 0;
    for (int wd = 0; wd < words; wd++) bits[wd] = 0;
    for (int i = 0; i < n; i++) {
        const float a0 = J.X1[3 * i], a1 = J.X1[3 * i + 1], a2 = J.X1[3 * i + 2];
        const float b0 = J.X2[3 * i], b1 = J.X2[3 * i + 1], b2 = J.X2[3 * i + 2];
        const float ia = 1.0f / a2, ib = 1.0f / b2;
        const float u11 = pix(fx1, cx1, a0, ia), v11 = pix(fy1, cy1, a1, ia);
        const float u22 = pix(fx2, cx2, b0, ib), v22 = pix(fy2, cy2, b1, ib);
        const float c0 = (float)(dotd(sR[0][0], sR[0][1], sR[0][2], b0, b1, b2) + (double)t12[0]);
        const float c1 = (float)(dotd(sR[1][0], sR[1][1], sR[1][2], b0, b1, b2) + (double)t12[1]);
        const float c2 = (float)(dotd(sR[2][0], sR[2][1], sR[2][2], b0, b1, b2) + (double)t12[2]);
        const float ic = 1.0f / c2;
        const float e1 = err2(u11, v11, pix(fx1, cx1, c0, ic), pix(fy1, cy1, c1, ic));
        const float d0 = (float)(dotd(sRi[0][0], sRi[0][1], sRi[0][2], a0, a1, a2) + (double)t21[0]);
        const float d1 = (float)(dotd(sRi[1][0], sRi[1][1], sRi[1][2], a0, a1, a2) + (double)t21[1]);
        const float d2 = (float)(dotd(sRi[2][0], sRi[2][1], sRi[2][2], a0, a1, a2) + (double)t21[2]);
        const float id = 1.0f / d2;
        const float e2 = err2(pix(fx2, cx2, d0, id), pix(fy2, cy2, d1, id), u22, v22);
        if (e1 < J.max_err1[i] && e2 < J.max_err2[i]) { bits[i >> 6] |= (uint64_t)1 << (i & 63); count++; }
    }
    J.n_inliers[h] = count;
}

}   // namespace

// the arguments of orbx_sim3_hypotheses_batch without the device (and without its refusals: the caller passes valid jobs)
extern "C" int sim3_loop(orbx_sim3_job *jobs, int njobs)
{
    for (int j = 0; j < njobs; j++)
        for (int h = 0; h < jobs[j].n_hyp; h++) one_hypothesis(jobs[j], h);
    return 0;
}

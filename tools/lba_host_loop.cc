// tools/lba_host_loop.cc -- the local bundle adjustment of include/orbx.h (orbx_local_bundle_adjustment) restated in plain C++ for ONE host
// core: the same two rounds, Huber kernels, Levenberg rules and dense Schur complement, with rotation matrices instead of quaternions and
// no care for the order of sums.  tools/bench_lba.py builds it and times it next to the device call.  It is a LOWER BOUND for a host
// solver of this structure, not the reference: g2o (sparse Schur, SimplicialLDLT under an AMD ordering, virtual calls per edge) cannot
// be built here and nobody has timed it.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace {

struct P3 { double R[9], t[3]; };

void exp_update(P3 &T, const double *x)
{
    const double th = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    const double O[9] = { 0, -x[2], x[1], x[2], 0, -x[0], -x[1], x[0], 0 };
    double O2[9], dR[9], V[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) O2[3 * r + c] = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
    double a = 1, b = 0.5, cc = 1.0 / 6;
    if (th > 1e-5) { a = sin(th) / th; b = (1 - cos(th)) / (th * th); cc = (th - sin(th)) / (th * th * th); }
    for (int k = 0; k < 9; k++) { const double id = k % 4 == 0; dR[k] = id + a * O[k] + b * O2[k]; V[k] = id + b * O[k] + cc * O2[k]; }
    P3 N;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) N.R[3 * r + c] = dR[3 * r] * T.R[c] + dR[3 * r + 1] * T.R[3 + c] + dR[3 * r + 2] * T.R[6 + c];
        N.t[r] = V[3 * r] * x[3] + V[3 * r + 1] * x[4] + V[3 * r + 2] * x[5] + dR[3 * r] * T.t[0] + dR[3 * r + 1] * T.t[1] + dR[3 * r + 2] * T.t[2];
    }
    T = N;
}

struct Prob {
    int K, P, E;
    const float *cam; const uint8_t *fixed; const int32_t *ek, *ep; const float *mx, *my, *mr, *w;
};

// error of edge e at (T, X): chi2; err, Pc out
inline double edge_err(const Prob &p, int e, const P3 &T, const double *X, double *err, double *Pc)
{
    for (int r = 0; r < 3; r++) Pc[r] = T.R[3 * r] * X[0] + T.R[3 * r + 1] * X[1] + T.R[3 * r + 2] * X[2] + T.t[r];
    const float *c = p.cam + 5 * p.ek[e];
    const bool st = !(p.mr[e] < 0.f);
    const double iz = st ? (double)(float)(1.0 / Pc[2]) : 1.0 / Pc[2];
    const double u = Pc[0] * iz * c[0] + c[2], v = Pc[1] * iz * c[1] + c[3];
    err[0] = p.mx[e] - u; err[1] = p.my[e] - v; err[2] = st ? p.mr[e] - (u - c[4] * iz) : 0.0;
    return p.w[e] * (err[0] * err[0] + err[1] * err[1] + err[2] * err[2]);
}

inline void rho(double chi, double delta, bool robust, double &r0, double &r1)
{
    r0 = chi; r1 = 1;
    if (robust && chi > delta * delta) { const double s = sqrt(chi); r0 = 2 * s * delta - delta * delta; r1 = delta / s; }
}

}   // namespace

// Tcw [K][16], Xw [P][3] in and out (float); flags [E] out; report: trials[2], chi2[2].  Returns 0.
extern "C" int lba_host_loop(int K, const float *Tcw, const float *cam, const uint8_t *fixed, int P, const float *Xw, int E, const int32_t *ek,
                             const int32_t *ep, const float *mx, const float *my, const float *mr, const float *w, float *Tcw_out, float *Xw_out,
                             uint8_t *flags, int *trials, double *chi2_out)
{
    const Prob p = { K, P, E, cam, fixed, ek, ep, mx, my, mr, w };
    const double dm = (double)(float)sqrt(5.991), ds = (double)(float)sqrt(7.815);
    std::vector<P3> T(K), Tt(K);
    std::vector<double> X(3 * (size_t)P), Xt(3 * (size_t)P), echi(E, 0.0);
    for (int k = 0; k < K; k++)
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[k].R[3 * r + c] = Tcw[16 * k + 4 * r + c]; T[k].t[r] = Tcw[16 * k + 4 * r + 3]; }
    for (size_t i = 0; i < X.size(); i++) X[i] = Xw[i];
    memset(flags, 0, (size_t)E);
    std::vector<int> row(K), poff(P + 1, 0);
    for (int e = 0; e < E; e++) poff[ep[e] + 1]++;
    for (int q = 0; q < P; q++) poff[q + 1] += poff[q];
    std::vector<double> Hll(6 * (size_t)P), bl(3 * (size_t)P), W(18 * (size_t)E), Dinv(9 * (size_t)P), xl(3 * (size_t)P, 0.0), Hpp, bp, S, bS, xp;
    trials[0] = trials[1] = 0;
    for (int round = 0; round < 2; round++) {
        const bool robust = round == 0;
        std::vector<char> kact(K, 0), pact(P, 0);
        for (int e = 0; e < E; e++) if (!(flags[e] & 1)) { kact[ek[e]] = 1; pact[ep[e]] = 1; }
        int rows = 0, npts = 0;
        for (int k = 0; k < K; k++) row[k] = (kact[k] && !fixed[k]) ? rows++ : -1;
        for (int q = 0; q < P; q++) npts += pact[q];
        const int n = 6 * rows;
        Hpp.assign(36 * (size_t)rows, 0); bp.assign(n, 0); S.assign((size_t)n * n, 0); bS.assign(n, 0); xp.assign(n, 0);
        double lambda = 0, ni = 2, cur = 0;
        int nbad = 0;
        for (int it = 0; it < (round ? 10 : 5) && npts; it++) {
            std::fill(Hll.begin(), Hll.end(), 0.0); std::fill(bl.begin(), bl.end(), 0.0); std::fill(Hpp.begin(), Hpp.end(), 0.0); std::fill(bp.begin(), bp.end(), 0.0);
            cur = 0;
            for (int e = 0; e < E; e++) {
                if (flags[e] & 1) continue;
                const int k = ek[e], q = ep[e];
                double err[3], Pc[3], r0, r1;
                const double chi = edge_err(p, e, T[k], &X[3 * q], err, Pc);
                const bool st = !(mr[e] < 0.f);
                echi[e] = chi;
                rho(chi, st ? ds : dm, robust, r0, r1);
                cur += r0;
                const float *c = cam + 5 * k;
                const double x = Pc[0], y = Pc[1], z = Pc[2], z2 = z * z, fx = c[0], fy = c[1], bf = c[4];
                double B[3][6] = { { x * y / z2 * fx, -(1 + x * x / z2) * fx, y / z * fx, -fx / z, 0, x / z2 * fx },
                                   { (1 + y * y / z2) * fy, -x * y / z2 * fy, -x / z * fy, 0, -fy / z, y / z2 * fy }, { 0, 0, 0, 0, 0, 0 } };
                double J[3][3] = { { -fx / z, 0, fx * x / z2 }, { 0, -fy / z, fy * y / z2 }, { 0, 0, 0 } }, A[3][3];
                if (st) {
                    B[2][0] = B[0][0] - bf * y / z2; B[2][1] = B[0][1] + bf * x / z2; B[2][2] = B[0][2]; B[2][3] = B[0][3]; B[2][5] = B[0][5] - bf / z2;
                    J[2][0] = J[0][0]; J[2][2] = J[0][2] - bf / z2;
                }
                const int nr = st ? 3 : 2;
                for (int r = 0; r < nr; r++)
                    for (int cc = 0; cc < 3; cc++) A[r][cc] = J[r][0] * T[k].R[cc] + J[r][1] * T[k].R[3 + cc] + J[r][2] * T[k].R[6 + cc];
                const double rw = r1 * w[e];
                double *H = &Hll[6 * (size_t)q], *b = &bl[3 * (size_t)q];
                int h = 0;
                for (int r = 0; r < 3; r++) {
                    for (int cc = r; cc < 3; cc++, h++) for (int m = 0; m < nr; m++) H[h] += A[m][r] * rw * A[m][cc];
                    for (int m = 0; m < nr; m++) b[r] -= A[m][r] * rw * err[m];
                }
                const int rr = row[k];
                if (rr < 0) continue;
                double *Hp = &Hpp[36 * (size_t)rr], *Wp = &W[18 * (size_t)e];
                for (int r = 0; r < 6; r++) {
                    for (int cc = 0; cc < 6; cc++) { double s = 0; for (int m = 0; m < nr; m++) s += B[m][r] * rw * B[m][cc]; Hp[6 * r + cc] += s; }
                    for (int cc = 0; cc < 3; cc++) { double s = 0; for (int m = 0; m < nr; m++) s += B[m][r] * rw * A[m][cc]; Wp[3 * r + cc] = s; }
                    for (int m = 0; m < nr; m++) bp[6 * rr + r] -= B[m][r] * rw * err[m];
                }
            }
            const double ini = cur;
            if (it == 0) {
                double md = 0;
                for (int r = 0; r < n; r++) md = fmax(md, fabs(Hpp[36 * (size_t)(r / 6) + 7 * (r % 6)]));
                for (int q = 0; q < P; q++) if (pact[q]) { md = fmax(md, fabs(Hll[6 * (size_t)q])); md = fmax(md, fabs(Hll[6 * (size_t)q + 3])); md = fmax(md, fabs(Hll[6 * (size_t)q + 5])); }
                lambda = 1e-5 * md; ni = 2; nbad = 0;
            }
            double rh = 0;
            int qmax = 0;
            do {
                // Dinv, the Schur complement, b_S
                std::fill(S.begin(), S.end(), 0.0);
                for (int r = 0; r < rows; r++) {
                    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) S[(size_t)(6 * r + a) * n + 6 * r + b] = Hpp[36 * (size_t)r + 6 * a + b] + (a == b ? lambda : 0);
                    for (int a = 0; a < 6; a++) bS[6 * r + a] = bp[6 * r + a];
                }
                for (int q = 0; q < P; q++) {
                    if (!pact[q]) continue;
                    const double *H = &Hll[6 * (size_t)q];
                    const double m00 = H[0] + lambda, m01 = H[1], m02 = H[2], m11 = H[3] + lambda, m12 = H[4], m22 = H[5] + lambda;
                    const double c00 = m11 * m22 - m12 * m12, c01 = m12 * m02 - m01 * m22, c02 = m01 * m12 - m11 * m02;
                    const double inv = 1.0 / (c00 * m00 + c01 * m01 + c02 * m02);
                    double *D = &Dinv[9 * (size_t)q];
                    D[0] = c00 * inv; D[1] = D[3] = c01 * inv; D[2] = D[6] = c02 * inv; D[4] = (m00 * m22 - m02 * m02) * inv;
                    D[5] = D[7] = (m01 * m02 - m00 * m12) * inv; D[8] = (m00 * m11 - m01 * m01) * inv;
                    const double *b = &bl[3 * (size_t)q];
                    const double db[3] = { D[0] * b[0] + D[1] * b[1] + D[2] * b[2], D[3] * b[0] + D[4] * b[1] + D[5] * b[2], D[6] * b[0] + D[7] * b[1] + D[8] * b[2] };
                    for (int e1 = poff[q]; e1 < poff[q + 1]; e1++) {
                        const int r1_ = (flags[e1] & 1) ? -1 : row[ek[e1]];
                        if (r1_ < 0) continue;
                        const double *W1 = &W[18 * (size_t)e1];
                        double BD[18];
                        for (int a = 0; a < 6; a++) {
                            for (int c = 0; c < 3; c++) BD[3 * a + c] = W1[3 * a] * D[c] + W1[3 * a + 1] * D[3 + c] + W1[3 * a + 2] * D[6 + c];
                            bS[6 * r1_ + a] -= W1[3 * a] * db[0] + W1[3 * a + 1] * db[1] + W1[3 * a + 2] * db[2];
                        }
                        for (int e2 = poff[q]; e2 < poff[q + 1]; e2++) {
                            const int r2_ = (flags[e2] & 1) ? -1 : row[ek[e2]];
                            if (r2_ < r1_) continue;      // the upper block triangle; r2_ == -1 falls out here too
                            const double *W2 = &W[18 * (size_t)e2];
                            for (int a = 0; a < 6; a++)
                                for (int b = 0; b < 6; b++)
                                    S[(size_t)(6 * r1_ + a) * n + 6 * r2_ + b] -= BD[3 * a] * W2[3 * b] + BD[3 * a + 1] * W2[3 * b + 1] + BD[3 * a + 2] * W2[3 * b + 2];
                        }
                    }
                }
                // LDL^T on the upper triangle (row i of U = column i of L), then the two substitutions
                bool ok = true;
                for (int j = 0; j < n && ok; j++) {
                    const double d = S[(size_t)j * n + j];
                    if (!(d > 0)) { ok = false; break; }
                    for (int i = j + 1; i < n; i++) {
                        const double l = S[(size_t)j * n + i] / d;
                        if (l == 0) continue;
                        double *Si = &S[(size_t)i * n];
                        const double *Sj = &S[(size_t)j * n];
                        for (int k = i; k < n; k++) Si[k] -= l * Sj[k];
                        bS[i] -= l * bS[j];
                    }
                }
                if (ok) {
                    for (int i = n - 1; i >= 0; i--) {
                        double v = bS[i];
                        for (int k = i + 1; k < n; k++) v -= S[(size_t)i * n + k] * xp[k];
                        xp[i] = v / S[(size_t)i * n + i];
                    }
                }
                // update into the trial copy, the errors there, the scale
                double scale = 0, temp = 0;
                for (int k = 0; k < K; k++) { Tt[k] = T[k]; if (row[k] >= 0) exp_update(Tt[k], &xp[6 * row[k]]); }
                for (int r = 0; r < n; r++) scale += xp[r] * (lambda * xp[r] + bp[r]);
                for (int q = 0; q < P; q++) {
                    for (int c = 0; c < 3; c++) Xt[3 * (size_t)q + c] = X[3 * (size_t)q + c];
                    if (!pact[q]) continue;
                    if (ok) {
                        double c3[3] = { bl[3 * (size_t)q], bl[3 * (size_t)q + 1], bl[3 * (size_t)q + 2] };
                        for (int e = poff[q]; e < poff[q + 1]; e++) {
                            const int rr = (flags[e] & 1) ? -1 : row[ek[e]];
                            if (rr < 0) continue;
                            const double *We = &W[18 * (size_t)e];
                            for (int c = 0; c < 3; c++) for (int a = 0; a < 6; a++) c3[c] -= We[3 * a + c] * xp[6 * rr + a];
                        }
                        const double *D = &Dinv[9 * (size_t)q];
                        for (int c = 0; c < 3; c++) xl[3 * (size_t)q + c] = D[3 * c] * c3[0] + D[3 * c + 1] * c3[1] + D[3 * c + 2] * c3[2];
                    }
                    for (int c = 0; c < 3; c++) {
                        const double v = xl[3 * (size_t)q + c];
                        Xt[3 * (size_t)q + c] += v;
                        scale += v * (lambda * v + bl[3 * (size_t)q + c]);
                    }
                }
                for (int e = 0; e < E; e++) {
                    if (flags[e] & 1) continue;
                    double err[3], Pc[3], r0, r1;
                    echi[e] = edge_err(p, e, Tt[ek[e]], &Xt[3 * (size_t)ep[e]], err, Pc);
                    rho(echi[e], !(mr[e] < 0.f) ? ds : dm, robust, r0, r1);
                    temp += r0;
                }
                if (!ok) temp = DBL_MAX;
                trials[round]++;
                rh = (cur - temp) / (scale + 1e-3);
                if (rh > 0 && isfinite(temp)) {
                    const double t = 2 * rh - 1;
                    lambda *= fmax(1.0 / 3, fmin(1 - t * t * t, 2.0 / 3));
                    ni = 2; cur = temp;
                    T.swap(Tt); X.swap(Xt);
                } else { lambda *= ni; ni *= 2; }
                qmax++;
            } while (rh < 0 && qmax < 10);
            if (qmax == 10 || rh == 0) break;
            nbad = (ini - cur) * 1e3 < ini ? nbad + 1 : 0;
            if (nbad >= 3) break;
        }
        chi2_out[round] = cur;
        for (int e = 0; e < E; e++) {
            const double *Xq = &X[3 * (size_t)ep[e]];
            const P3 &Tk = T[ek[e]];
            const double z = Tk.R[6] * Xq[0] + Tk.R[7] * Xq[1] + Tk.R[8] * Xq[2] + Tk.t[2];
            if (echi[e] > (!(mr[e] < 0.f) ? 7.815 : 5.991) || !(z > 0)) flags[e] |= (uint8_t)(round == 0 ? 1 : 2);
        }
    }
    for (int k = 0; k < K; k++) {
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Tcw_out[16 * k + 4 * r + c] = (float)T[k].R[3 * r + c]; Tcw_out[16 * k + 4 * r + 3] = (float)T[k].t[r]; }
        Tcw_out[16 * k + 12] = Tcw_out[16 * k + 13] = Tcw_out[16 * k + 14] = 0.f; Tcw_out[16 * k + 15] = 1.f;
    }
    for (size_t i = 0; i < X.size(); i++) Xw_out[i] = (float)X[i];
    return 0;
}

// orbx_essential.hip — Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:885-1153) between :907 and :1152: a pose graph of 7-DoF
// VertexSim3Expmap vertices and binary EdgeSim3 edges, no points, then the correction of the map points.  The contract, operation by
// operation, is include/orbx.h (orbx_optimize_essential_graph); the numpy restatement is tests/eg_model.py.  The Levenberg loop runs on the
// host as the bundle adjustments' does (lm_host_loop of orbx_lm.h), one status record per linearisation and per trial; the
// system is 7 x the free keyframes: dense and solved by the panels of orbx_ldlt.hip, or (orbx_optimize_essential_graph2) the envelope of
// its lower triangle, solved by orbx_ldlt_env.hip with the same values.  fp64 on the plain VALU, no atomics.
//
//   k_eg_setup        vScw of every keyframe (the start estimates), the measurement of every edge, the 14 transforms Sim3(+-delta e_d)
//   k_eg_edges<true>  the linearisation.  An edge costs 29 evaluations of log(C * Si' * Sj'^-1): each gets its own lane, 32 lanes an edge,
//                     two edges a wave.  The errors meet in LDS, where the lanes of the edge turn them into the Jacobians [A | B] and then
//                     into the edge's record: the upper triangle of [A | B]^T [A | B] (105: A^T A, A^T B, B^T B), -[A | B]^T e (14), chi2.
//                     No lane keeps an indexed accumulator, so nothing goes to scratch.
//   k_eg_edges<false> a thread per edge: chi2 at the trial estimates
//   k_eg_rows         a workgroup per free vertex (its diagonal block and b over its incident edges, in edge order) and per unique pair of
//                     free vertices (its off-diagonal block over the pair's edges, in edge order), from host-built lists
//   k_eg_reduce       one workgroup: chi2, the sum of x (lambda x + b), the largest diagonal entry (for the report only)
//   k_eg_fill         phase 0 zeroes the lower triangle of S; phase 1 scatters the blocks, adds lambda, copies b to y
//   k_eg_fill_env     the envelope form of phase 1 (phase 0 is a memset of the envelope, one linear range)
//   k_eg_update       trial estimate = Sim3(x_k) * S_k, and the vertex's part of x (lambda x + b)
//   k_eg_finish       S_out and the SE3 recovery;  k_eg_points: a thread per map point
//   k_eg_probe        orbx_debug_eg_stages only: the 29 evaluations of every edge, a thread each, for the stage tests
#include "orbx_resident.h"
#include "orbx_lm.h"
#include "orbx_sim3.h"
#include "orbx_ldlt_env.h"
#include <float.h>
#include <math.h>
#include <algorithm>

namespace {

enum { EG_REC = 120 };   // doubles of an edge's record

// every pointer is a device address
struct Eg {
    int K, E, P, F, NP, fix;
    const float *Tcw; const uint8_t *fixed; const int32_t *corrected, *noncorrected; const double *Sc, *Snc;
    const int32_t *edge_i, *edge_j; const uint8_t *kind;
    const float *Xw; const int32_t *pref;
    const int32_t *row, *rowkf, *voff, *vedge, *poff, *pedge, *pair;   // vedge: 2 e + end; pedge: 2 e + (block read transposed); pair: hi row, lo row
    double *status;      // chi2, scale, largest diagonal, ok of the solve
    const int64_t *rowptr; const int32_t *first;   // the envelope of S (orbx_ldlt_env.h), or null: S is dense [7 F][7 F]
    double *S_out; float *Tcw_out; double *point_out; float *Xw_out;
    double *est[2], *vS, *meas, *xf, *rec, *echi, *Hd, *bv, *Off, *sc, *S, *y, *x;
};

// packed index of entry (r, c), r <= c, of the upper triangle of an N x N matrix in row order
template <int N> __device__ __forceinline__ int upk(int r, int c) { return r * N - r * (r - 1) / 2 + (c - r); }

// :923-937: the keyframe's start estimate
__device__ __forceinline__ Sim3 eg_vscw(const Eg &G, int k)
{
    const int ci = G.corrected[k];
    if (ci >= 0) return xf_load(G.Sc + 8 * (size_t)ci);
    const float *T = G.Tcw + 16 * (size_t)k;
    const double R[9] = { (double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10] };
    Sim3 S;
    quat_from_matrix(R, S.qx, S.qy, S.qz, S.qw);
    S.tx = (double)T[3]; S.ty = (double)T[7]; S.tz = (double)T[11]; S.s = 1.0;
    return S;
}

__device__ __forceinline__ Sim3 eg_normal_end(const Eg &G, int k)
{
    const int ni = G.noncorrected[k];
    return ni >= 0 ? xf_load(G.Snc + 8 * (size_t)ni) : eg_vscw(G, k);
}

__global__ __launch_bounds__(256) void k_eg_setup(Eg G)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < 14) {
        double u[7];
#pragma unroll
        for (int j = 0; j < 7; j++) u[j] = (t >> 1) == j ? ((t & 1) ? -1e-9 : 1e-9) : 0.0;
        if (G.fix) u[6] = 0.0;   // oplusImpl: update[6] = 0
        xf_store(G.xf + 8 * t, sim3_exp(u));
    }
    if (t < G.K) {
        const Sim3 S = eg_vscw(G, t);
        xf_store(G.vS + 8 * (size_t)t, S);
        xf_store(G.est[0] + 8 * (size_t)t, S);
        xf_store(G.est[1] + 8 * (size_t)t, S);
    }
    if (t < G.E) {
        const int i = G.edge_i[t], j = G.edge_j[t];
        const bool normal = G.kind[t] != 0;
        const Sim3 Siw = normal ? eg_normal_end(G, i) : eg_vscw(G, i);
        const Sim3 Sjw = normal ? eg_normal_end(G, j) : eg_vscw(G, j);
        xf_store(G.meas + 8 * (size_t)t, sim3_mul(Sjw, sim3_inverse(Siw)));
    }
}

// EdgeSim3::computeError: (C * Si * Sj^-1).log()
__device__ __forceinline__ void eg_error(const Sim3 &C, const Sim3 &Si, const Sim3 &Sj, double e[7])
{
    sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inverse(Sj)), e);
}

__device__ __forceinline__ double eg_chi2(const double e[7])
{
    return (((((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]) + e[4] * e[4]) + e[5] * e[5]) + e[6] * e[6];
}

template <bool LIN>
__global__ __launch_bounds__(256) void k_eg_edges(Eg G, int cur)
{
    if constexpr (!LIN) {
        const int e = blockIdx.x * 256 + threadIdx.x;
        if (e >= G.E) return;
        double err[7];
        eg_error(xf_load(G.meas + 8 * (size_t)e), xf_load(G.est[cur] + 8 * (size_t)G.edge_i[e]), xf_load(G.est[cur] + 8 * (size_t)G.edge_j[e]), err);
        G.echi[e] = eg_chi2(err);
    } else {
        __shared__ double errs[8][29][7];
        __shared__ double Jm[8][7][14];
        const int tid = threadIdx.x, slot = tid >> 5, lane = tid & 31;
        const int e = blockIdx.x * 8 + slot;
        const bool live = e < G.E;
        int i = 0, j = 0;
        bool free_i = false, free_j = false;
        if (live) {
            i = G.edge_i[e]; j = G.edge_j[e];
            free_i = G.row[i] >= 0; free_j = G.row[j] >= 0;
            // lane 0: the error itself; lanes 1 .. 14: vertex 0 through transform lane - 1; lanes 15 .. 28: vertex 1 through transform lane - 15
            const bool on_i = lane >= 1 && lane <= 14, on_j = lane >= 15 && lane <= 28;
            if (lane == 0 || (on_i && free_i) || (on_j && free_j)) {
                Sim3 Si = xf_load(G.est[cur] + 8 * (size_t)i), Sj = xf_load(G.est[cur] + 8 * (size_t)j);
                if (on_i) Si = sim3_mul(xf_load(G.xf + 8 * (lane - 1)), Si);
                if (on_j) Sj = sim3_mul(xf_load(G.xf + 8 * (lane - 15)), Sj);
                double err[7];
                eg_error(xf_load(G.meas + 8 * (size_t)e), Si, Sj, err);
#pragma unroll
                for (int m = 0; m < 7; m++) errs[slot][lane][m] = err[m];
            }
        }
        __syncthreads();
        if (live) {
            const double scalar = 1.0 / (2.0 * 1e-9);
            for (int q = lane; q < 98; q += 32) {
                const int m = q / 14, c = q % 14;
                const bool has = c < 7 ? free_i : free_j;
                Jm[slot][m][c] = has ? scalar * (errs[slot][1 + 2 * c][m] - errs[slot][2 + 2 * c][m]) : 0.0;
            }
        }
        __syncthreads();
        if (!live) return;
        double *rec = G.rec + (size_t)EG_REC * e;
        for (int k = lane; k < EG_REC; k += 32) {
            double v;
            if (k < 105) {
                int r = 0, q = k;
                while (q >= 14 - r) { q -= 14 - r; r++; }
                const int c = r + q;
                v = Jm[slot][0][r] * Jm[slot][0][c];
#pragma unroll
                for (int m = 1; m < 7; m++) v += Jm[slot][m][r] * Jm[slot][m][c];
            } else if (k < 119) {
                const int c = k - 105;
                v = Jm[slot][0][c] * -errs[slot][0][0];
#pragma unroll
                for (int m = 1; m < 7; m++) v += Jm[slot][m][c] * -errs[slot][0][m];
            } else {
                double err[7];
#pragma unroll
                for (int m = 0; m < 7; m++) err[m] = errs[slot][0][m];
                v = eg_chi2(err);
                G.echi[e] = v;
            }
            rec[k] = v;
        }
    }
}

// workgroup b < F: row b's H_ii (28) and b (7); workgroup F + p: pair p's 7 x 7 block, entry [a][c] for dof a of the higher row, c of the lower
__global__ __launch_bounds__(64) void k_eg_rows(Eg G)
{
    const int b = blockIdx.x, t = threadIdx.x;
    if (b < G.F) {
        if (t >= 35) return;
        int r = 0, c = 0;
        if (t < 28) {
            int q = t;
            while (q >= 7 - r) { q -= 7 - r; r++; }
            c = r + q;
        }
        double v = 0.0;
        for (int q = G.voff[b]; q < G.voff[b + 1]; q++) {
            const int ent = G.vedge[q], off = 7 * (ent & 1);
            const double *rec = G.rec + (size_t)EG_REC * (ent >> 1);
            v += t < 28 ? rec[upk<14>(off + r, off + c)] : rec[105 + off + (t - 28)];
        }
        if (t < 28) G.Hd[28 * (size_t)b + t] = v; else G.bv[7 * (size_t)b + (t - 28)] = v;
        return;
    }
    const int p = b - G.F;
    if (t >= 49) return;
    const int a = t / 7, c = t % 7;
    double v = 0.0;
    for (int q = G.poff[p]; q < G.poff[p + 1]; q++) {
        const int ent = G.pedge[q];
        const double *rec = G.rec + (size_t)EG_REC * (ent >> 1);
        // the record holds (A^T B)[r][s] at (r, 7 + s): vertex 0 is the higher row -> [a][c], else the transpose
        v += (ent & 1) ? rec[upk<14>(c, 7 + a)] : rec[upk<14>(a, 7 + c)];
    }
    G.Off[49 * (size_t)p + t] = v;
}

// status[0] = chi2 (edge e to partial e % 256), status[1] = sum of the vertices' x (lambda x + b) (trial), status[2] = largest diagonal
__global__ __launch_bounds__(256) void k_eg_reduce(Eg G, int trial)
{
    __shared__ double red[4 * 2];
    __shared__ double mx[4];
    const int tid = threadIdx.x;
    double a[2] = { 0.0, 0.0 };
    for (int e = tid; e < G.E; e += 256) a[0] += G.echi[e];
    double md = 0.0;
    if (trial) {
        for (int r = tid; r < G.F; r += 256) a[1] += G.sc[r];
    } else {
        for (int r = tid; r < G.F; r += 256)
#pragma unroll
            for (int d = 0; d < 7; d++) md = fmax(fabs(G.Hd[28 * (size_t)r + upk<7>(d, d)]), md);
    }
    block_sum(a, red);
    md = wave_max(md);
    if ((tid & 63) == 0) mx[tid >> 6] = md;
    __syncthreads();
    if (tid == 0) {
        G.status[0] = a[0];
        if (trial) G.status[1] = a[1];
        else G.status[2] = fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
    }
}

// phase 0: grid (ceil(n / 256), n), the lower triangle of S zeroed.  phase 1: grid F + NP, the blocks into S, lambda on the diagonal, b to y
__global__ __launch_bounds__(256) void k_eg_fill(Eg G, double lambda, int phase)
{
    const size_t n = 7 * (size_t)G.F;
    if (phase == 0) {
        const size_t row = blockIdx.y, col = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (col <= row) G.S[row * n + col] = 0.0;
        return;
    }
    const int b = blockIdx.x, t = threadIdx.x;
    if (t >= 49) return;
    const int a = t / 7, c = t % 7;
    if (b < G.F) {
        const size_t o = 7 * (size_t)b;
        if (c <= a) G.S[(o + a) * n + o + c] = a == c ? G.Hd[28 * (size_t)b + upk<7>(c, a)] + lambda : G.Hd[28 * (size_t)b + upk<7>(c, a)];
        if (t < 7) G.y[o + t] = G.bv[o + t];
        return;
    }
    const int p = b - G.F;
    const size_t hi = 7 * (size_t)G.pair[2 * p], lo = 7 * (size_t)G.pair[2 * p + 1];
    G.S[(hi + a) * n + lo + c] = G.Off[49 * (size_t)p + t];
}

// grid F + NP: k_eg_fill's phase 1 into the envelope.  A pair's block lies inside it: the higher row's first column is at or in front of
// 7 x the lowest row it is paired with (eg_envelope_rows).
__global__ __launch_bounds__(64) void k_eg_fill_env(Eg G, double lambda)
{
    const int b = blockIdx.x, t = threadIdx.x;
    if (t >= 49) return;
    const int a = t / 7, c = t % 7;
    if (b < G.F) {
        const int o = 7 * b;
        if (c <= a) G.S[G.rowptr[o + a] - G.first[o + a] + o + c] = a == c ? G.Hd[28 * (size_t)b + upk<7>(c, a)] + lambda : G.Hd[28 * (size_t)b + upk<7>(c, a)];
        if (t < 7) G.y[o + t] = G.bv[o + t];
        return;
    }
    const int p = b - G.F;
    const int hi = 7 * G.pair[2 * p], lo = 7 * G.pair[2 * p + 1];
    G.S[G.rowptr[hi + a] - G.first[hi + a] + lo + c] = G.Off[49 * (size_t)p + t];
}

// thread k: keyframe k's trial estimate (VertexSim3Expmap::oplusImpl for a row, a copy otherwise).  After a failed solve x is the previous one.
__global__ __launch_bounds__(256) void k_eg_update(Eg G, int cur, double lambda)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= G.K) return;
    Sim3 S = xf_load(G.est[cur] + 8 * (size_t)k);
    const int r = G.row[k];
    if (r >= 0) {
        double x[7];
#pragma unroll
        for (int d = 0; d < 7; d++) x[d] = G.x[7 * (size_t)r + d];
        if (G.fix) { x[6] = 0.0; G.x[7 * (size_t)r + 6] = 0.0; }   // oplusImpl writes into the solver's x
        S = sim3_mul(sim3_exp(x), S);
        double s = 0.0;
#pragma unroll
        for (int d = 0; d < 7; d++) s += x[d] * (lambda * x[d] + G.bv[7 * (size_t)r + d]);
        G.sc[r] = s;
    }
    xf_store(G.est[1 - cur] + 8 * (size_t)k, S);
}

// :1101-1118: S_out, and Tiw = [R | t * (1. / s)] through Converter::toCvSE3's float casts
__global__ __launch_bounds__(256) void k_eg_finish(Eg G, int cur)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= G.K) return;
    const Sim3 S = xf_load(G.est[cur] + 8 * (size_t)k);
    xf_store(G.S_out + 8 * (size_t)k, S);
    const Pose Q = { S.qx, S.qy, S.qz, S.qw, 0.0, 0.0, 0.0 };
    double R[9];
    quat_to_matrix(Q, R);
    const double inv = 1. / S.s;
    const double t[3] = { S.tx * inv, S.ty * inv, S.tz * inv };
    float *T = G.Tcw_out + 16 * (size_t)k;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
        T[4 * r + 3] = (float)t[r];
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// :1122-1152: correctedSwr.map(Srw.map(P3Dw)), behind k_eg_finish
__global__ __launch_bounds__(256) void k_eg_points(Eg G)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= G.P) return;
    const int ref = G.pref[p];
    const Sim3 Srw = xf_load(G.vS + 8 * (size_t)ref), Swr = sim3_inverse(xf_load(G.S_out + 8 * (size_t)ref));
    const float *X = G.Xw + 3 * (size_t)p;
    double x, y, z, cx, cy, cz;
    sim3_map(Srw, (double)X[0], (double)X[1], (double)X[2], x, y, z);
    sim3_map(Swr, x, y, z, cx, cy, cz);
    double *o = G.point_out + 3 * (size_t)p;
    o[0] = cx; o[1] = cy; o[2] = cz;
    float *f = G.Xw_out + 3 * (size_t)p;
    f[0] = (float)cx; f[1] = (float)cy; f[2] = (float)cz;
}

// orbx_debug_eg_stages only: a thread per (edge, evaluation), err[e][v][7].  Evaluation 0 is the error at the estimates; evaluation
// 1 + 2 c is column c's plus side and 2 + 2 c its minus side, column c = dof c of vertex 0 for c < 7 and dof c - 7 of vertex 1 above:
// that vertex's estimate goes through Sim3(+delta e_dof) (xf[2 dof]) or Sim3(-delta e_dof) (xf[2 dof + 1]), the other one stays.  The
// evaluations of a fixed end, which the linearisation never makes, are written as zeros.  Stated from the column, not from a lane.
__global__ __launch_bounds__(256) void k_eg_probe(Eg G, int cur, double *err)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 29 * (size_t)G.E) return;
    const int e = (int)(t / 29), v = (int)(t % 29);
    const int i = G.edge_i[e], j = G.edge_j[e];
    Sim3 Si = xf_load(G.est[cur] + 8 * (size_t)i), Sj = xf_load(G.est[cur] + 8 * (size_t)j);
    bool made = true;
    if (v > 0) {
        const int col = (v - 1) >> 1, minus = (v - 1) & 1;
        const bool second = col >= 7;
        const int dof = second ? col - 7 : col;
        const Sim3 T = xf_load(G.xf + 8 * (2 * dof + minus));
        if (second) { Sj = sim3_mul(T, Sj); made = G.row[j] >= 0; }
        else { Si = sim3_mul(T, Si); made = G.row[i] >= 0; }
    }
    double r[7];
    eg_error(xf_load(G.meas + 8 * (size_t)e), Si, Sj, r);
#pragma unroll
    for (int m = 0; m < 7; m++) err[7 * t + m] = made ? r[m] : 0.0;
}

}   // namespace

// ---------------------------------------------------------------- host side (include/orbx.h: orbx_optimize_essential_graph)

// orbx_debug_eg_profile: as orbx_debug_lba_profile, for the calling thread's orbx_optimize_essential_graph calls (tools/bench_eg.py)
enum { EG_K_SETUP, EG_K_LINEARIZE, EG_K_ROWS, EG_K_REDUCE, EG_K_FILL, EG_K_SOLVE, EG_K_UPDATE, EG_K_ERRORS, EG_K_FINISH, EG_K_POINTS, EG_K_COUNT };
static thread_local LaunchProfile<EG_K_COUNT> g_eg_prof;

extern "C" int orbx_debug_eg_profile(int enable, double *ms, int32_t *launches) { return g_eg_prof.entry(enable, ms, launches); }

// iterations: the options' where there are options; max_free: 1536 for the dense solve, 4095 (every n_kf that passes) for the envelope
static int eg_check(const char *who, const orbx_eg_problem *p, const int *iterations, const float *Tcw_out, const float *Xw_out, int max_free, int *n_free)
{
    if (!p || !Tcw_out) { orbx_set_error("%s: NULL problem or Tcw_out", who); return ORBX_E_INVALID; }
    if (p->n_kf < 1 || p->n_edges < 0 || p->n_points < 0 || p->n_corrected < 0 || p->n_noncorrected < 0) {
        orbx_set_error("%s: n_kf = %d, n_edges = %d, n_points = %d, n_corrected = %d, n_noncorrected = %d", who, p->n_kf, p->n_edges, p->n_points,
                       p->n_corrected, p->n_noncorrected);
        return ORBX_E_INVALID;
    }
    if (iterations && *iterations < 0) { orbx_set_error("%s: iterations = %d", who, *iterations); return ORBX_E_INVALID; }
    if (p->n_kf > 4096 || p->n_edges > (1 << 18) || p->n_points > (1 << 20) || p->n_corrected > 4096 || p->n_noncorrected > 4096) {
        orbx_set_error("%s: n_kf = %d, n_edges = %d, n_points = %d, n_corrected = %d, n_noncorrected = %d beyond 4096, 2^18, 2^20, 4096, 4096", who,
                       p->n_kf, p->n_edges, p->n_points, p->n_corrected, p->n_noncorrected);
        return ORBX_E_CAPACITY;
    }
    if (!p->Tcw || !p->fixed || !p->corrected || !p->noncorrected || (p->n_corrected && !p->S_corrected) || (p->n_noncorrected && !p->S_noncorrected) ||
        (p->n_edges && (!p->edge_i || !p->edge_j || !p->edge_kind)) || (p->n_points && (!p->Xw || !p->point_ref || !Xw_out))) {
        orbx_set_error("%s: a NULL array", who);
        return ORBX_E_INVALID;
    }
    int nfix = 0;
    for (int k = 0; k < p->n_kf; k++) {
        nfix += p->fixed[k] != 0;
        if (p->corrected[k] < -1 || p->corrected[k] >= p->n_corrected || p->noncorrected[k] < -1 || p->noncorrected[k] >= p->n_noncorrected) {
            orbx_set_error("%s: keyframe %d: corrected = %d or noncorrected = %d out of range", who, k, p->corrected[k], p->noncorrected[k]);
            return ORBX_E_INVALID;
        }
    }
    if (nfix != 1) { orbx_set_error("%s: %d keyframes with fixed != 0, not exactly one", who, nfix); return ORBX_E_INVALID; }
    for (int e = 0; e < p->n_edges; e++) {
        const int i = p->edge_i[e], j = p->edge_j[e];
        if (i < 0 || i >= p->n_kf || j < 0 || j >= p->n_kf || i == j || p->edge_kind[e] > 1) {
            orbx_set_error("%s: edge %d: vertices %d, %d (out of range or equal) or kind %d", who, e, i, j, (int)p->edge_kind[e]);
            return ORBX_E_INVALID;
        }
    }
    for (int q = 0; q < p->n_points; q++)
        if (p->point_ref[q] < 0 || p->point_ref[q] >= p->n_kf) { orbx_set_error("%s: point %d: reference keyframe %d out of range", who, q, p->point_ref[q]); return ORBX_E_INVALID; }
    if (p->n_kf - 1 > max_free) { orbx_set_error("%s: %d keyframes with fixed == 0, more than %d", who, p->n_kf - 1, max_free); return ORBX_E_CAPACITY; }
    *n_free = p->n_kf - 1;
    return ORBX_OK;
}

// The envelope of a checked problem's system, rows in keyframe order: block row r (a free keyframe's 7 rows) starts at 7 x the smallest
// row it shares an edge with, itself where there is none; orbx_ldlt_env_shape rounds that down to the panel width.  Every pair's block
// (higher row, lower row) and every diagonal block then lies inside.  Host only.
static void eg_envelope_rows(const orbx_eg_problem *p, std::vector<int32_t> *first)
{
    std::vector<int32_t> row(p->n_kf), lowest(p->n_kf);
    int F = 0;
    for (int k = 0; k < p->n_kf; k++) { row[k] = p->fixed[k] ? -1 : F; if (!p->fixed[k]) { lowest[F] = F; F++; } }
    for (int e = 0; e < p->n_edges; e++) {
        const int ri = row[p->edge_i[e]], rj = row[p->edge_j[e]];
        if (ri < 0 || rj < 0) continue;
        const int hi = ri > rj ? ri : rj, lo = ri > rj ? rj : ri;
        if (lo < lowest[hi]) lowest[hi] = lo;
    }
    first->resize(7 * (size_t)F);
    for (int r = 0; r < F; r++)
        for (int d = 0; d < 7; d++) (*first)[7 * (size_t)r + d] = 7 * lowest[r];
}

extern "C" int orbx_eg_envelope(const orbx_eg_problem *p, int64_t *entries, int64_t *triangle)
{
    const char *who = "orbx_eg_envelope";
    if (!entries || !triangle) { orbx_set_error("%s: NULL entries or triangle", who); return ORBX_E_INVALID; }
    int n_free = 0;
    static const float none = 0.f;   // this call has no Tcw_out and no Xw_out for eg_check to ask for
    const int rc = eg_check(who, p, nullptr, &none, &none, 4095, &n_free);
    if (rc) return rc;
    std::vector<int32_t> first;
    eg_envelope_rows(p, &first);
    LdltEnvPlan plan;
    orbx_ldlt_env_shape(7 * n_free, first.data(), &plan);
    *entries = plan.entries;
    *triangle = (int64_t)(7 * n_free) * (7 * n_free + 1) / 2;
    return ORBX_OK;
}

// A checked problem on the device, and the launch sequences over it: what orbx_optimize_essential_graph and orbx_debug_eg_stages share.
// stage() builds the row and pair lists, uploads the problem and lays out the work area (the download head first: the status record, then
// the four outputs); setup(), linearise() and trial() are the launches of the start, of a linearisation and of a Levenberg trial.
struct EgCall {
    CallCtx *c = nullptr, *pc = nullptr;
    hipStream_t s = nullptr;
    Eg G;
    size_t K = 0, E = 0, P = 0, F = 0, N = 0, NP = 0;
    size_t out = 0, w_Sout = 0, w_Tcw = 0, w_point = 0, w_Xw = 0;   // the download head and the outputs in it
    uint8_t *extra = nullptr;                                         // `extra_bytes` of device memory behind the work area (the probe's)
    std::vector<int32_t> pair;                                        // hi row, lo row of every unique pair, as the device has them
    LdltEnvPlan *env = nullptr;                                       // the envelope solve's plan, or null: the dense solve

    // env: the plan of the system's envelope (orbx_ldlt_env_plan over eg_envelope_rows): S is packed and solved by it
    int stage(int device, const orbx_eg_problem *p, int n_free, size_t extra_bytes, LdltEnvPlan *env = nullptr);

    int setup()
    {
        ORBX_HIP(hipMemsetAsync(G.status, 0, 64, s));
        if (N) ORBX_HIP(hipMemsetAsync(G.x, 0, 8 * N, s));   // the solver's x before the first solve: zeros, as in the other solvers
        g_eg_prof.launch(EG_K_SETUP, pc, [&] { hipLaunchKernelGGL(k_eg_setup, dim3(grid256((int)std::max(std::max(K, E), (size_t)14))), dim3(256), 0, s, G); });
        return ORBX_OK;
    }

    // the system at est[cur]: the records, the rows and pairs, chi2 and the largest diagonal entry; the status record fetched
    int linearise(int cur)
    {
        g_eg_prof.launch(EG_K_LINEARIZE, pc, [&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_eg_edges<true>), dim3((unsigned)((E + 7) / 8)), dim3(256), 0, s, G, cur); });
        g_eg_prof.launch(EG_K_ROWS, pc, [&] { hipLaunchKernelGGL(k_eg_rows, dim3((unsigned)(F + NP)), dim3(64), 0, s, G); });
        g_eg_prof.launch(EG_K_REDUCE, pc, [&] { hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(256), 0, s, G, 0); });
        return call_fetch(c, 64);
    }

    // a trial from est[cur] into est[1 - cur]; the status record fetched.  filled() runs between the fill and the solve, which factors S
    // in place; solve == false leaves x as it stands (orbx_debug_eg_stages with x_in).  A hook's failure ends the trial.
    template <class Filled>
    int trial(int cur, double lambda, bool solve, Filled filled)
    {
        g_eg_prof.launch(EG_K_FILL, pc, [&] {
            if (env) {
                (void)hipMemsetAsync(G.S, 0, 8 * (size_t)env->entries, s);   // a failure shows at call_fetch's hipGetLastError
                hipLaunchKernelGGL(k_eg_fill_env, dim3((unsigned)(F + NP)), dim3(64), 0, s, G, lambda);
                return;
            }
            hipLaunchKernelGGL(k_eg_fill, dim3(grid256((int)N), (unsigned)N), dim3(256), 0, s, G, lambda, 0);
            hipLaunchKernelGGL(k_eg_fill, dim3((unsigned)(F + NP)), dim3(64), 0, s, G, lambda, 1);
        });
        if (const int rc = filled()) return rc;
        if (solve) g_eg_prof.launch(EG_K_SOLVE, pc, [&] {
            if (env) orbx_ldlt_env_launch(G.S, G.y, G.x, G.status + 3, *env, s);
            else orbx_ldlt_panel_launch(G.S, G.y, G.x, G.status + 3, (int)N, s);
        });
        g_eg_prof.launch(EG_K_UPDATE, pc, [&] { hipLaunchKernelGGL(k_eg_update, dim3(grid256((int)K)), dim3(256), 0, s, G, cur, lambda); });
        g_eg_prof.launch(EG_K_ERRORS, pc, [&] { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_eg_edges<false>), dim3(grid256((int)E)), dim3(256), 0, s, G, 1 - cur); });
        g_eg_prof.launch(EG_K_REDUCE, pc, [&] { hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(256), 0, s, G, 1); });
        return call_fetch(c, 64);
    }
};

int EgCall::stage(int device, const orbx_eg_problem *p, int n_free, size_t extra_bytes, LdltEnvPlan *env_plan)
{
    int rc;
    env = env_plan;
    K = (size_t)p->n_kf; E = (size_t)p->n_edges; P = (size_t)p->n_points; F = (size_t)n_free; N = 7 * F;
    const size_t NC = (size_t)p->n_corrected, NN = (size_t)p->n_noncorrected;

    // rows: the free keyframes in keyframe order; a vertex's incident edges and a pair's edges in edge order
    std::vector<int32_t> row(K), rowkf(F ? F : 1), voff(F + 1, 0), vedge, poff, pedge;
    pair.clear();
    {
        int r = 0;
        for (size_t k = 0; k < K; k++) { row[k] = p->fixed[k] ? -1 : r; if (!p->fixed[k]) rowkf[r++] = (int32_t)k; }
    }
    std::vector<std::pair<uint64_t, int32_t>> pe;   // (hi row, lo row) -> 2 e + transposed
    for (size_t e = 0; e < E; e++) {
        const int ri = row[p->edge_i[e]], rj = row[p->edge_j[e]];
        if (ri >= 0) voff[ri + 1]++;
        if (rj >= 0) voff[rj + 1]++;
        if (ri >= 0 && rj >= 0) {
            const bool i_hi = ri > rj;
            pe.push_back({ ((uint64_t)(i_hi ? ri : rj) << 32) | (uint32_t)(i_hi ? rj : ri), (int32_t)(2 * e + (i_hi ? 0 : 1)) });
        }
    }
    for (size_t r = 0; r < F; r++) voff[r + 1] += voff[r];
    vedge.resize(voff[F] ? voff[F] : 1);
    {
        std::vector<int32_t> fill(voff.begin(), voff.end() - 1);
        for (size_t e = 0; e < E; e++) {
            const int ri = row[p->edge_i[e]], rj = row[p->edge_j[e]];
            if (ri >= 0) vedge[fill[ri]++] = (int32_t)(2 * e);
            if (rj >= 0) vedge[fill[rj]++] = (int32_t)(2 * e + 1);
        }
    }
    std::stable_sort(pe.begin(), pe.end(), [](const std::pair<uint64_t, int32_t> &a, const std::pair<uint64_t, int32_t> &b) { return a.first < b.first; });
    poff.push_back(0);
    for (size_t q = 0; q < pe.size(); q++) {
        if (q == 0 || pe[q].first != pe[q - 1].first) {
            if (q) poff.push_back((int32_t)q);
            pair.push_back((int32_t)(pe[q].first >> 32)); pair.push_back((int32_t)(pe[q].first & 0xffffffffu));
        }
        pedge.push_back(pe[q].second);
    }
    poff.push_back((int32_t)pe.size());
    NP = pair.size() / 2;
    if (pedge.empty()) pedge.push_back(0);
    if (pair.empty()) { pair.push_back(0); pair.push_back(0); }

    if ((rc = orbx_call_ctx(device, &c))) return rc;
    BlobCursor b = { nullptr, nullptr, 0 };
    const size_t o_T = b.take(64 * K), o_fix = b.take(K), o_cor = b.take(4 * K), o_non = b.take(4 * K), o_Sc = b.take(64 * NC), o_Sn = b.take(64 * NN),
                 o_ei = b.take(4 * E), o_ej = b.take(4 * E), o_kind = b.take(E), o_X = b.take(12 * P), o_ref = b.take(4 * P), o_row = b.take(4 * K),
                 o_rowkf = b.take(4 * rowkf.size()), o_voff = b.take(4 * voff.size()), o_vedge = b.take(4 * vedge.size()), o_poff = b.take(4 * poff.size()),
                 o_pedge = b.take(4 * pedge.size()), o_pair = b.take(4 * pair.size());
    const size_t o_rowptr = b.take(env ? 8 * env->rowptr.size() : 0), o_first = b.take(env ? 4 * env->first.size() : 0),
                 o_act = b.take(env ? 4 * env->act.size() : 0);
    const size_t blob = b.o;
    BlobCursor w = { nullptr, nullptr, 0 };
    const size_t w_status = w.take(64);
    w_Sout = w.take(64 * K); w_Tcw = w.take(64 * K); w_point = w.take(24 * P); w_Xw = w.take(12 * P);
    out = w.o;
    const size_t w_e0 = w.take(64 * K), w_e1 = w.take(64 * K), w_vS = w.take(64 * K), w_meas = w.take(64 * E), w_xf = w.take(14 * 64),
                 w_rec = w.take(8 * EG_REC * E), w_echi = w.take(8 * E), w_Hd = w.take(224 * F), w_bv = w.take(56 * F), w_Off = w.take(392 * NP),
                 w_sc = w.take(8 * F), w_S = w.take(env ? 8 * (size_t)env->entries : 8 * N * N), w_y = w.take(8 * N), w_x = w.take(8 * N);
    const size_t w_extra = w.take(extra_bytes);
    if ((rc = call_reserve(c, blob, w.o, out))) return rc;
    uint8_t *h = c->h_blob;
    memcpy(h + o_T, p->Tcw, 64 * K); memcpy(h + o_fix, p->fixed, K); memcpy(h + o_cor, p->corrected, 4 * K); memcpy(h + o_non, p->noncorrected, 4 * K);
    if (NC) memcpy(h + o_Sc, p->S_corrected, 64 * NC);
    if (NN) memcpy(h + o_Sn, p->S_noncorrected, 64 * NN);
    if (E) { memcpy(h + o_ei, p->edge_i, 4 * E); memcpy(h + o_ej, p->edge_j, 4 * E); memcpy(h + o_kind, p->edge_kind, E); }
    if (P) { memcpy(h + o_X, p->Xw, 12 * P); memcpy(h + o_ref, p->point_ref, 4 * P); }
    memcpy(h + o_row, row.data(), 4 * K); memcpy(h + o_rowkf, rowkf.data(), 4 * rowkf.size()); memcpy(h + o_voff, voff.data(), 4 * voff.size());
    memcpy(h + o_vedge, vedge.data(), 4 * vedge.size()); memcpy(h + o_poff, poff.data(), 4 * poff.size());
    memcpy(h + o_pedge, pedge.data(), 4 * pedge.size()); memcpy(h + o_pair, pair.data(), 4 * pair.size());
    if (env) {
        memcpy(h + o_rowptr, env->rowptr.data(), 8 * env->rowptr.size()); memcpy(h + o_first, env->first.data(), 4 * env->first.size());
        memcpy(h + o_act, env->act.data(), 4 * env->act.size());
    }
    if ((rc = call_upload(c, blob))) return rc;
    if ((rc = g_eg_prof.ctx(c, &pc))) return rc;

    memset(&G, 0, sizeof G);
    uint8_t *d = c->d_blob, *wk = c->d_work;
    G.K = (int)K; G.E = (int)E; G.P = (int)P; G.F = (int)F; G.NP = (int)NP; G.fix = p->fix_scale ? 1 : 0;
    G.Tcw = (const float *)(d + o_T); G.fixed = d + o_fix; G.corrected = (const int32_t *)(d + o_cor); G.noncorrected = (const int32_t *)(d + o_non);
    G.Sc = (const double *)(d + o_Sc); G.Snc = (const double *)(d + o_Sn);
    G.edge_i = (const int32_t *)(d + o_ei); G.edge_j = (const int32_t *)(d + o_ej); G.kind = d + o_kind;
    G.Xw = (const float *)(d + o_X); G.pref = (const int32_t *)(d + o_ref);
    G.row = (const int32_t *)(d + o_row); G.rowkf = (const int32_t *)(d + o_rowkf); G.voff = (const int32_t *)(d + o_voff); G.vedge = (const int32_t *)(d + o_vedge);
    G.poff = (const int32_t *)(d + o_poff); G.pedge = (const int32_t *)(d + o_pedge); G.pair = (const int32_t *)(d + o_pair);
    G.status = (double *)(wk + w_status); G.S_out = (double *)(wk + w_Sout); G.Tcw_out = (float *)(wk + w_Tcw);
    G.point_out = (double *)(wk + w_point); G.Xw_out = (float *)(wk + w_Xw);
    G.est[0] = (double *)(wk + w_e0); G.est[1] = (double *)(wk + w_e1); G.vS = (double *)(wk + w_vS); G.meas = (double *)(wk + w_meas);
    G.xf = (double *)(wk + w_xf); G.rec = (double *)(wk + w_rec); G.echi = (double *)(wk + w_echi); G.Hd = (double *)(wk + w_Hd);
    G.bv = (double *)(wk + w_bv); G.Off = (double *)(wk + w_Off); G.sc = (double *)(wk + w_sc); G.S = (double *)(wk + w_S);
    G.y = (double *)(wk + w_y); G.x = (double *)(wk + w_x);
    if (env) {
        G.rowptr = env->d_rowptr = (const int64_t *)(d + o_rowptr); G.first = env->d_first = (const int32_t *)(d + o_first);
        env->d_act = (const int32_t *)(d + o_act);
    }

    extra = wk + w_extra;
    s = c->stream;
    return ORBX_OK;
}

static int eg_run(int device, const orbx_eg_problem *p, int n_free, int iterations, LdltEnvPlan *env, float *Tcw_out, float *Xw_out, double *S_out,
                  double *point_out, orbx_eg_report *report);

// ORBX_EG_SOLVER_AUTO: the envelope solve beyond the dense solve's 1536 free keyframes, and where the envelope holds at most half of the
// lower triangle's entries
static bool eg_auto_takes_envelope(int n_free, int64_t entries)
{
    const int64_t n = 7 * (int64_t)n_free;
    return n_free > 1536 || 2 * entries <= n * (n + 1) / 2;
}

extern "C" int orbx_optimize_essential_graph(int device, const orbx_eg_problem *p, const orbx_eg_options *opt, float *Tcw_out, float *Xw_out,
                                             double *S_out, double *point_out, orbx_eg_report *report)
{
    const char *who = "orbx_optimize_essential_graph";
    int n_free = 0;
    int rc = eg_check(who, p, opt ? &opt->iterations : nullptr, Tcw_out, Xw_out, 1536, &n_free);
    if (rc) return rc;
    return eg_run(device, p, n_free, opt ? opt->iterations : 20 /* :1096 */, nullptr, Tcw_out, Xw_out, S_out, point_out, report);
}

extern "C" int orbx_optimize_essential_graph2(int device, const orbx_eg_problem *p, const orbx_eg_options2 *opt, float *Tcw_out, float *Xw_out,
                                              double *S_out, double *point_out, orbx_eg_report *report)
{
    const char *who = "orbx_optimize_essential_graph2";
    int solver = opt ? opt->solver : ORBX_EG_SOLVER_AUTO;
    if (solver != ORBX_EG_SOLVER_DENSE && solver != ORBX_EG_SOLVER_ENVELOPE && solver != ORBX_EG_SOLVER_AUTO) {
        orbx_set_error("%s: solver = %d", who, solver);
        return ORBX_E_INVALID;
    }
    int n_free = 0;
    int rc = eg_check(who, p, opt ? &opt->iterations : nullptr, Tcw_out, Xw_out, solver == ORBX_EG_SOLVER_DENSE ? 1536 : 4095, &n_free);
    if (rc) return rc;
    const int iterations = opt ? opt->iterations : 20;
    if (solver == ORBX_EG_SOLVER_DENSE) return eg_run(device, p, n_free, iterations, nullptr, Tcw_out, Xw_out, S_out, point_out, report);
    std::vector<int32_t> first;
    eg_envelope_rows(p, &first);
    LdltEnvPlan plan;
    orbx_ldlt_env_shape(7 * n_free, first.data(), &plan);
    if (solver == ORBX_EG_SOLVER_AUTO && !eg_auto_takes_envelope(n_free, plan.entries))
        return eg_run(device, p, n_free, iterations, nullptr, Tcw_out, Xw_out, S_out, point_out, report);
    if (plan.entries > ORBX_EG_MAX_ENVELOPE) {
        orbx_set_error("%s: the envelope of the system holds %lld entries, more than %lld (%d keyframes with fixed == 0 in this order; orbx_eg_envelope)",
                       who, (long long)plan.entries, (long long)ORBX_EG_MAX_ENVELOPE, n_free);
        return ORBX_E_CAPACITY;
    }
    orbx_ldlt_env_plan(7 * n_free, first.data(), &plan);
    return eg_run(device, p, n_free, iterations, &plan, Tcw_out, Xw_out, S_out, point_out, report);
}

// the call behind both entry points, on a checked problem.  env: the envelope solve's plan, or null for the dense solve.
static int eg_run(int device, const orbx_eg_problem *p, int n_free, int iterations, LdltEnvPlan *env, float *Tcw_out, float *Xw_out, double *S_out,
                  double *point_out, orbx_eg_report *report)
{
    int rc;
    EgCall q;
    if ((rc = q.stage(device, p, n_free, 0, env))) return rc;
    const size_t K = q.K, E = q.E, P = q.P, F = q.F;
    CallCtx *c = q.c;
    orbx_eg_report rep;
    memset(&rep, 0, sizeof rep);
    rep.n_free = n_free;
    if ((rc = q.setup())) return rc;

    int cur = 0;
    // no edge, or no free vertex: optimize() finds no active vertex and returns before the first iteration (sparse_optimizer.cpp:341-345)
    const LmRun r = lm_host_loop(
        E > 0 && F > 0 ? iterations : 0, 1e-16,   // setUserLambdaInit(1e-16), :899
        [&] { return q.linearise(cur); }, [&](double lambda) { return q.trial(cur, lambda, true, [] { return ORBX_OK; }); },
        [&] { return (const double *)c->h_out; }, [] { return false; }, [&] { cur = 1 - cur; });
    if (r.rc) return r.rc;
    rep.iterations = r.iterations; rep.trials = r.trials; rep.n_solve_failed = r.n_solve_failed;
    rep.chi2_start = r.chi2_start; rep.chi2 = r.chi2; rep.lambda = r.lambda;

    g_eg_prof.launch(EG_K_FINISH, q.pc, [&] { hipLaunchKernelGGL(k_eg_finish, dim3(grid256((int)K)), dim3(256), 0, q.s, q.G, cur); });
    if (P) g_eg_prof.launch(EG_K_POINTS, q.pc, [&] { hipLaunchKernelGGL(k_eg_points, dim3(grid256((int)P)), dim3(256), 0, q.s, q.G); });
    if ((rc = call_fetch(c, q.out))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    memcpy(Tcw_out, ho + q.w_Tcw, 64 * K);
    if (S_out) memcpy(S_out, ho + q.w_Sout, 64 * K);
    if (P) memcpy(Xw_out, ho + q.w_Xw, 12 * P);
    if (P && point_out) memcpy(point_out, ho + q.w_point, 24 * P);
    if (report) *report = rep;
    return ORBX_OK;
}

// orbx_debug_eg_stages (include/orbx.h): ONE linearisation at the start estimates and, where asked, ONE trial from them, through the
// launch sequences of the call above; what each kernel left in device memory is copied out between them.
extern "C" int orbx_debug_eg_stages(int device, const orbx_eg_problem *p, double lambda, const double *x_in, int trial, orbx_eg_stages *d)
{
    const char *who = "orbx_debug_eg_stages";
    if (!d) { orbx_set_error("%s: NULL dump", who); return ORBX_E_INVALID; }
    int n_free = 0;
    static const float none = 0.f;   // this call has no Tcw_out and no Xw_out for eg_check to ask for
    int rc = eg_check(who, p, nullptr, &none, &none, 1536, &n_free);
    if (rc) return rc;
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) { orbx_set_error("%s: lambda = %g", who, lambda); return ORBX_E_INVALID; }
    if (d->S && 7 * n_free > ORBX_EG_STAGES_MAX_N) {
        orbx_set_error("%s: S asked for with n = %d, more than %d", who, 7 * n_free, ORBX_EG_STAGES_MAX_N);
        return ORBX_E_CAPACITY;
    }
    if (d->err && p->n_edges > ORBX_EG_STAGES_MAX_PROBED) {
        orbx_set_error("%s: err asked for with %d edges, more than %d", who, p->n_edges, ORBX_EG_STAGES_MAX_PROBED);
        return ORBX_E_CAPACITY;
    }
    EgCall q;
    if ((rc = q.stage(device, p, n_free, d->err ? 8 * 29 * 7 * (size_t)p->n_edges : 0))) return rc;
    const size_t K = q.K, E = q.E, F = q.F, N = q.N, NP = q.NP;
    const Eg &G = q.G;
    // device memory -> the caller's array, where there is one
    auto copy = [&](void *dst, const void *src, size_t bytes) -> int {
        if (!dst || !bytes) return ORBX_OK;
        ORBX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, q.s));
        ORBX_HIP(hipStreamSynchronize(q.s));
        return ORBX_OK;
    };
    if ((rc = q.setup())) return rc;
    if ((rc = copy(d->vS, G.vS, 64 * K)) || (rc = copy(d->meas, G.meas, 64 * E)) || (rc = copy(d->xf, G.xf, 14 * 64))) return rc;
    if (d->n_pairs) *d->n_pairs = (int32_t)NP;
    if (E == 0 || F == 0) { ORBX_HIP(hipStreamSynchronize(q.s)); return ORBX_OK; }   // the full call runs no iteration on such a graph

    if ((rc = q.linearise(0))) return rc;
    if (d->status_lin) memcpy(d->status_lin, q.c->h_out, 32);
    if (d->pair && NP) memcpy(d->pair, q.pair.data(), 8 * NP);
    if ((rc = copy(d->rec, G.rec, 8 * EG_REC * E)) || (rc = copy(d->echi, G.echi, 8 * E)) || (rc = copy(d->Hd, G.Hd, 224 * F)) ||
        (rc = copy(d->bv, G.bv, 56 * F)) || (rc = copy(d->Off, G.Off, 392 * NP))) return rc;
    if (d->err) {
        double *err = (double *)q.extra;
        hipLaunchKernelGGL(k_eg_probe, dim3(grid256((int)(29 * E))), dim3(256), 0, q.s, G, 0, err);
        ORBX_HIP(hipGetLastError());
        if ((rc = copy(d->err, err, 8 * 29 * 7 * E))) return rc;
    }
    if (!trial) return ORBX_OK;

    rc = q.trial(0, lambda, x_in == nullptr, [&]() -> int {
        int r;
        if ((r = copy(d->S, G.S, 8 * N * N)) || (r = copy(d->y, G.y, 8 * N))) return r;   // above S's diagonal: whatever the memory held
        if (x_in) ORBX_HIP(hipMemcpyAsync(G.x, x_in, 8 * N, hipMemcpyHostToDevice, q.s));
        return ORBX_OK;
    });
    if (rc) return rc;
    if (d->status_trial) memcpy(d->status_trial, q.c->h_out, 32);
    if (d->solve_ok) *d->solve_ok = x_in ? -1 : (((const double *)q.c->h_out)[3] != 0.0);
    if ((rc = copy(d->x, G.x, 8 * N)) || (rc = copy(d->trial, G.est[1], 64 * K)) || (rc = copy(d->sc, G.sc, 8 * F)) ||
        (rc = copy(d->echi_trial, G.echi, 8 * E))) return rc;
    return ORBX_OK;
}

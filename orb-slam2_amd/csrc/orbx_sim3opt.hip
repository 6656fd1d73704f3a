// orbx_sim3opt.hip — k_sim3_opt: Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1164-1365) in one launch.
// Every VertexSBAPointXYZ of that function is fixed; the one free vertex is a 7-DoF VertexSim3Expmap, so a Levenberg step is a dense
// 7x7 normal equation reduced over two reprojection edges per correspondence (EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ).  The
// structure is k_pose_opt's (orbx_pose.hip): one workgroup of 256 threads per job, the estimate (an UNNORMALISED quaternion, a
// translation and a scale, as g2o::Sim3 keeps them) and every scalar of the Levenberg loop in registers of EVERY thread, the 7x7 solve,
// the exponential and the bookkeeping run redundantly on sums that block_sum (orbx_lm.h) hands every thread bit for bit, correspondences
// strided over the threads, fp64, no atomics.  A linearisation reduces 28 + 7 + 1 doubles, a trial one; a job's result does not depend on
// the run or on the other jobs of the launch.
// The Jacobian is the reference's: both edge types leave linearizeOplus commented out (types_seven_dof_expmap.h:147,169), so g2o takes
// the central difference of base_binary_edge.hpp:131-205, column d = (e(exp(+1e-9 e_d) * S) - e(exp(-1e-9 e_d) * S)) * (1 / 2e-9).  The
// 14 perturbed transforms and their inverses do not depend on the edge: threads 0..13 build one pair each per linearisation into LDS
// (28 x 8 doubles), and an edge thread reads them back as broadcasts -- 28 map + project evaluations on top of its own two.
// The rounds (src/Optimizer.cc:1305-1364), unlike PoseOptimization's: optimize(5), then optimize(nBad > 0 ? 10 : 5) CONTINUING from the
// first round's estimate; Huber stays on in both; an edge pair removed after round 1 never comes back; fewer than 10 pairs left after
// round 1 returns 0 with g2oS12 untouched.  Per-pair state is one byte, the flag in the job's output array; the error an edge "keeps"
// (the one of the last evaluated trial: linearizeOplus restores _error itself, :150,:200) is recomputed from that trial's estimate.
// The solver's x DOES survive from the first optimize() to the second: BlockSolver::buildStructure calls resize -> Solver::resizeVector
// (solver.cpp:46-70), which allocates only when the size outgrows _maxXSize (twice the first size), and nothing else clears _x; so a
// failed factorisation in round 2 re-applies the last solution of round 1.  (Before the first solve g2o's _x is uninitialised in a
// release build; zeros here, as in k_pose_opt.)  VertexSim3Expmap::oplusImpl writes update[6] = 0 INTO that x when _fix_scale.
// The arithmetic is restated in include/orbx.h (orbx_sim3_optimize) and, in numpy, in tests/sim3opt_model.py.
#include "orbx_resident.h"
#include "orbx_lm.h"
#include "orbx_sim3.h"
#include <float.h>
#include <math.h>

// One job of k_sim3_opt.  Every pointer is a device address.  inlier[n] is the kernel's per-pair state and its output.
struct Sim3OptJob {
    int n, fix_scale;
    float th2, delta;    // delta = (float)sqrt(th2), src/Optimizer.cc:1217
    const uint8_t *has_pair;
    const float *P1c, *P2c, *x1, *y1, *w1, *x2, *y2, *w2;
    uint8_t *inlier;
    float cam1[4], cam2[4];
    double S12[8];       // qx qy qz qw tx ty tz s
};
struct Sim3OptOut { double S12[8], chi2[2]; int32_t n_corr, rounds, n_bad, more_iterations, iterations[2], n_inliers, pad; };

namespace {

struct Cam4 { double fx, fy, cx, cy; };
struct Pair { double p1x, p1y, p1z, p2x, p2y, p2z, m1x, m1y, w1, m2x, m2y, w2; };

__device__ __forceinline__ Pair pair_load(const Sim3OptJob &J, int i)
{
    const long long k = 3 * (long long)i;
    Pair p;
    p.p1x = (double)J.P1c[k]; p.p1y = (double)J.P1c[k + 1]; p.p1z = (double)J.P1c[k + 2];
    p.p2x = (double)J.P2c[k]; p.p2y = (double)J.P2c[k + 1]; p.p2z = (double)J.P2c[k + 2];
    p.m1x = (double)J.x1[i]; p.m1y = (double)J.y1[i]; p.w1 = (double)J.w1[i];
    p.m2x = (double)J.x2[i]; p.m2y = (double)J.y2[i]; p.w2 = (double)J.w2[i];
    return p;
}

// error = obs - cam_map(project(T.map(P))) (types_seven_dof_expmap.h:138-167); returns chi2 = e . (w e)
__device__ __forceinline__ double edge_err(const Sim3 &T, const Cam4 &K, double X, double Y, double Z, double mx, double my, double w, double &e0, double &e1)
{
    double x, y, z;
    sim3_map(T, X, Y, Z, x, y, z);
    e0 = mx - ((x / z) * K.fx + K.cx);
    e1 = my - ((y / z) * K.fy + K.cy);
    return e0 * (w * e0) + e1 * (w * e1);
}

// the two chi2 of a pair at estimate S (edge 12: P2c through S into camera 1) and its inverse Si (edge 21: P1c into camera 2)
__device__ __forceinline__ void pair_chi2(const Pair &p, const Sim3 &S, const Sim3 &Si, const Cam4 &K1, const Cam4 &K2, double &c12, double &c21)
{
    double e0, e1;
    c12 = edge_err(S, K1, p.p2x, p.p2y, p.p2z, p.m1x, p.m1y, p.w1, e0, e1);
    c21 = edge_err(Si, K2, p.p1x, p.p1y, p.p1z, p.m2x, p.m2y, p.w2, e0, e1);
}

// one edge into the system: its error and chi2 at T0, the central-difference Jacobian from the 14 transforms at xf (xf[16 * d] is
// exp(+delta e_d) * S, xf[16 * d + 8] the minus one; for edge 21 the caller passes their inverses), then
// H += A^T (rho1 w) A, b -= rho1 A^T (w e), chi2 += rho0 (base_binary_edge.hpp:55-120)
__device__ __forceinline__ void edge_accumulate(double (&acc)[36], const double *xf, const Sim3 &T0, const Cam4 &K, double X, double Y, double Z,
                                                double mx, double my, double w, double delta)
{
    double e0, e1;
    const double chi = edge_err(T0, K, X, Y, Z, mx, my, w, e0, e1);
    double rho0, rho1;
    huber(chi, delta, rho0, rho1);
    acc[35] += rho0;
    const double scalar = 1.0 / (2.0 * 1e-9);
    double A0[7], A1[7];
#pragma unroll
    for (int d = 0; d < 7; d++) {
        double p0, p1, m0, m1;
        edge_err(xf_load(xf + 16 * d), K, X, Y, Z, mx, my, w, p0, p1);
        edge_err(xf_load(xf + 16 * d + 8), K, X, Y, Z, mx, my, w, m0, m1);
        A0[d] = scalar * (p0 - m0);
        A1[d] = scalar * (p1 - m1);
        // the transforms stay in LDS, 16 doubles of them live at a time: without this fence the compiler hoists all 224 loads out of
        // the edge loop (they are loop invariant), and without the operands it runs the seven columns' divisions side by side; both spill
        asm volatile("" : "+v"(A0[d]), "+v"(A1[d]) : : "memory");
    }
    const double rw = rho1 * w, we0 = w * e0, we1 = w * e1;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 7; r++) {
#pragma unroll
        for (int c = r; c < 7; c++, k++) acc[k] += (A0[r] * rw) * A0[c] + (A1[r] * rw) * A1[c];
        acc[28 + r] -= rho1 * (A0[r] * we0 + A1[r] * we1);
    }
}

__global__ __launch_bounds__(256) void k_sim3_opt(const Sim3OptJob *__restrict__ jobs, Sim3OptOut *__restrict__ outs)
{
    __shared__ double red[4 * 36];
    __shared__ double xf[28 * 8];   // [0, 112): pair d at 16 d (plus), 16 d + 8 (minus); [112, 224): their inverses, same order
    const Sim3OptJob &J = jobs[blockIdx.x];
    Sim3OptOut &out = outs[blockIdx.x];
    const int tid = threadIdx.x, n = J.n;
    const bool fix = J.fix_scale != 0;
    const Cam4 K1 = { (double)J.cam1[0], (double)J.cam1[1], (double)J.cam1[2], (double)J.cam1[3] };
    const Cam4 K2 = { (double)J.cam2[0], (double)J.cam2[1], (double)J.cam2[2], (double)J.cam2[3] };
    const double delta = (double)J.delta, th2 = (double)J.th2;

    double cnt[1] = { 0.0 };
    for (int i = tid; i < n; i += 256)
        if (J.has_pair[i]) { cnt[0] += 1.0; J.inlier[i] = 1; }
    block_sum(cnt, red);
    const int n_corr = (int)cnt[0];

    const Sim3 start = { J.S12[0], J.S12[1], J.S12[2], J.S12[3], J.S12[4], J.S12[5], J.S12[6], J.S12[7] };   // as handed in: setEstimate(g2oS12)
    Sim3 S = start, Strial = start;
    int rounds = 0, n_bad = 0, more = 5, left = n_corr;
    double x[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    double chi2_of[2] = { 0.0, 0.0 };
    int iters_of[2] = { 0, 0 };
    for (int round = 0; round < 2 && n_corr > 0; round++) {
        const int max_iter = round == 0 ? 5 : more;
        double lambda = 0.0, ni = 2.0, cur_chi = 0.0;
        int stop_bad = 0, iters = 0;
        for (int iter = 0; iter < max_iter; iter++) {
            // the 14 perturbed estimates and their inverses, one pair per thread
            if (tid < 14) {
                double u[7];
#pragma unroll
                for (int j = 0; j < 7; j++) u[j] = (tid >> 1) == j ? ((tid & 1) ? -1e-9 : 1e-9) : 0.0;
                if (fix) u[6] = 0.0;   // oplusImpl: update[6] = 0, so column 6 is exactly 0
                const Sim3 T = sim3_mul(sim3_exp(u), S);
                xf_store(xf + 8 * tid, T);
                xf_store(xf + 112 + 8 * tid, sim3_inverse(T));
            }
            __syncthreads();
            // computeActiveErrors + buildSystem at S
            const Sim3 Si = sim3_inverse(S);
            double acc[36];
#pragma unroll
            for (int k = 0; k < 36; k++) acc[k] = 0.0;
            for (int i = tid; i < n; i += 256) {
                if (!J.has_pair[i] || !J.inlier[i]) continue;
                const Pair p = pair_load(J, i);
                edge_accumulate(acc, xf, S, K1, p.p2x, p.p2y, p.p2z, p.m1x, p.m1y, p.w1, delta);
                edge_accumulate(acc, xf + 112, Si, K2, p.p1x, p.p1y, p.p1z, p.m2x, p.m2y, p.w2, delta);
            }
            block_sum(acc, red);
            cur_chi = acc[35];
            const double ini_chi = cur_chi;
            if (iter == 0) {   // optimization_algorithm_levenberg.cpp:93-97, :166-180
                lm_start(hu_max_diag<7>(acc), lambda, ni, stop_bad);
            }
            double rho = 0.0;
            int qmax = 0;
            do {
                const Sim3 backup = S;
                const bool ok = ldlt_small<7>(acc, acc + 28, lambda, x);
                if (fix) x[6] = 0.0;
                S = sim3_mul(sim3_exp(x), S);
                Strial = S;
                const Sim3 Ti = sim3_inverse(S);
                double tc[1] = { 0.0 };
                for (int i = tid; i < n; i += 256) {
                    if (!J.has_pair[i] || !J.inlier[i]) continue;
                    const Pair p = pair_load(J, i);
                    double c12, c21, r0, r1;
                    pair_chi2(p, S, Ti, K1, K2, c12, c21);
                    huber(c12, delta, r0, r1); tc[0] += r0;
                    huber(c21, delta, r0, r1); tc[0] += r0;
                }
                block_sum(tc, red);
                const double temp_chi = ok ? tc[0] : DBL_MAX;
                double scale = 0.0;
#pragma unroll
                for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + acc[28 + j]);
                rho = lm_gain(cur_chi, temp_chi, scale);
                if (lm_accepts(rho, temp_chi)) {
                    lm_accept(rho, lambda, ni);
                    cur_chi = temp_chi;
                } else {
                    lm_reject(lambda, ni);
                    S = backup;   // pop(): the vertex goes back, the edges keep the errors of the rejected estimate
                }
                qmax++;
            } while (rho < 0.0 && qmax < 10);
            iters++;
            if (lm_done(qmax, rho, ini_chi, cur_chi, stop_bad)) break;
        }
        // :1308-1327 / :1343-1358: every pair still in the graph, at the errors of the last evaluated trial
        const Sim3 Ti = sim3_inverse(Strial);
        double bad[1] = { 0.0 };
        for (int i = tid; i < n; i += 256) {
            if (!J.has_pair[i] || !J.inlier[i]) continue;
            const Pair p = pair_load(J, i);
            double c12, c21;
            pair_chi2(p, Strial, Ti, K1, K2, c12, c21);
            if (c12 > th2 || c21 > th2) { J.inlier[i] = 0; bad[0] += 1.0; }
        }
        block_sum(bad, red);
        chi2_of[round] = cur_chi; iters_of[round] = iters;
        rounds = round + 1;
        left -= (int)bad[0];
        if (round == 0) {
            n_bad = (int)bad[0];
            more = n_bad > 0 ? 10 : 5;
            if (n_corr - n_bad < 10) break;   // :1335-1336
        }
    }
    if (tid == 0) {
        const bool kept = rounds == 2;   // g2oS12 is assigned only behind the second round
        const Sim3 R = kept ? S : start;
        out.S12[0] = R.qx; out.S12[1] = R.qy; out.S12[2] = R.qz; out.S12[3] = R.qw;
        out.S12[4] = R.tx; out.S12[5] = R.ty; out.S12[6] = R.tz; out.S12[7] = R.s;
        out.chi2[0] = chi2_of[0]; out.chi2[1] = chi2_of[1];
        out.iterations[0] = iters_of[0]; out.iterations[1] = iters_of[1];
        out.n_corr = n_corr; out.rounds = rounds; out.n_bad = n_bad; out.more_iterations = more;
        out.n_inliers = kept ? left : 0; out.pad = 0;
    }
}

}   // namespace

// ---------------------------------------------------------------- host side (include/orbx.h: orbx_sim3_optimize)

struct Sim3OptArgs {
    const orbx_sim3opt_obs *obs; const float *cam1, *cam2; const double *S12;
    float th2; int fix_scale;
    double *S12_out; uint8_t *inlier; int *n_inliers; orbx_sim3opt_report *report;
};

static int sim3opt_check(const char *who, int job, const Sim3OptArgs &a)
{
    if (!a.obs || !a.cam1 || !a.cam2 || !a.S12 || !a.S12_out || !a.n_inliers) {
        orbx_set_error("%s: job %d: NULL obs, cam1, cam2, S12, S12_out or n_inliers", who, job);
        return ORBX_E_INVALID;
    }
    const orbx_sim3opt_obs &o = *a.obs;
    if (o.n < 0 || o.n > 65535) { orbx_set_error("%s: job %d: n = %d outside [0, 65535]", who, job, o.n); return ORBX_E_INVALID; }
    if (!(a.th2 > 0.f) || !isfinite(a.th2)) { orbx_set_error("%s: job %d: th2 is not positive and finite", who, job); return ORBX_E_INVALID; }
    if (o.n && (!o.has_pair || !o.P1c || !o.P2c || !o.x1 || !o.y1 || !o.inv_sigma2_1 || !o.x2 || !o.y2 || !o.inv_sigma2_2 || !a.inlier)) {
        orbx_set_error("%s: job %d: observation arrays or inlier missing", who, job);
        return ORBX_E_INVALID;
    }
    return ORBX_OK;
}

static void sim3opt_deliver(const Sim3OptOut &o, const uint8_t *flags, const Sim3OptArgs &a)
{
    memcpy(a.S12_out, o.S12, sizeof o.S12);
    const orbx_sim3opt_obs &ob = *a.obs;
    for (int i = 0; i < ob.n; i++)
        if (ob.has_pair[i]) a.inlier[i] = flags[i];
    *a.n_inliers = o.n_inliers;
    if (!a.report) return;
    orbx_sim3opt_report &r = *a.report;
    r.n_corr = o.n_corr; r.rounds = o.rounds; r.n_bad = o.n_bad; r.more_iterations = o.more_iterations;
    for (int k = 0; k < 2; k++) { r.iterations[k] = o.iterations[k]; r.chi2[k] = o.chi2[k]; }
    memcpy(r.S12, o.S12, sizeof o.S12);
}

// nothing to optimise in any job: what the kernel would have written, without a launch
static void sim3opt_empty(const Sim3OptArgs &a)
{
    Sim3OptOut o;
    memset(&o, 0, sizeof o);
    memcpy(o.S12, a.S12, sizeof o.S12);
    o.more_iterations = 5;
    sim3opt_deliver(o, nullptr, a);
}

static bool sim3opt_has_pairs(const orbx_sim3opt_obs &o)
{
    for (int i = 0; i < o.n; i++)
        if (o.has_pair[i]) return true;
    return false;
}

// a job's arrays, stated once (JobArrays, orbx_resident.h): what goes up, then the flag bytes that come down behind the Sim3OptOuts.
// Returns where the flags were fetched to (DELIVER)
static const uint8_t *sim3opt_arrays(JobArrays &w, const orbx_sim3opt_obs &ob, Sim3OptJob &J)
{
    const size_t n = (size_t)ob.n;
    w.in(J.has_pair, ob.has_pair, n); w.in(J.P1c, ob.P1c, 12 * n); w.in(J.P2c, ob.P2c, 12 * n);
    w.in(J.x1, ob.x1, 4 * n); w.in(J.y1, ob.y1, 4 * n); w.in(J.w1, ob.inv_sigma2_1, 4 * n);
    w.in(J.x2, ob.x2, 4 * n); w.in(J.y2, ob.y2, 4 * n); w.in(J.w2, ob.inv_sigma2_2, 4 * n);
    return w.out(J.inlier, nullptr, n);
}

// staging: up [Sim3OptJob x njobs | the jobs' arrays], down [Sim3OptOut x njobs | the jobs' flag bytes]
static int sim3opt_run(const char *who, int device, const Sim3OptArgs *a, int njobs)
{
    bool any = false;
    for (int j = 0; j < njobs; j++) {
        const int rc = sim3opt_check(who, j, a[j]);
        if (rc) return rc;
        any = any || sim3opt_has_pairs(*a[j].obs);
    }
    if (!any) {
        for (int j = 0; j < njobs; j++) sim3opt_empty(a[j]);
        return ORBX_OK;
    }
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    const size_t jobs_b = a16(sizeof(Sim3OptJob) * (size_t)njobs), outs_b = a16(sizeof(Sim3OptOut) * (size_t)njobs);
    Sim3OptJob none = {};
    JobArrays size(JobArrays::MEASURE, c, jobs_b, outs_b);
    for (int j = 0; j < njobs; j++) sim3opt_arrays(size, *a[j].obs, none);
    const size_t blob = size.up.o, out = size.down.o;
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    JobArrays stage(JobArrays::STAGE, c, jobs_b, outs_b);
    for (int j = 0; j < njobs; j++) {
        Sim3OptJob &J = ((Sim3OptJob *)c->h_blob)[j];
        memset(&J, 0, sizeof J);
        J.n = a[j].obs->n; J.fix_scale = a[j].fix_scale ? 1 : 0;
        J.th2 = a[j].th2; J.delta = sqrtf(a[j].th2);
        sim3opt_arrays(stage, *a[j].obs, J);
        memcpy(J.cam1, a[j].cam1, sizeof J.cam1); memcpy(J.cam2, a[j].cam2, sizeof J.cam2); memcpy(J.S12, a[j].S12, sizeof J.S12);
    }
    if ((rc = call_upload(c, blob))) return rc;
    hipLaunchKernelGGL(k_sim3_opt, dim3(njobs), dim3(256), 0, c->stream, (const Sim3OptJob *)c->d_blob, (Sim3OptOut *)c->d_work);
    if ((rc = call_fetch(c, out))) return rc;
    JobArrays deliver(JobArrays::DELIVER, c, jobs_b, outs_b);
    for (int j = 0; j < njobs; j++) sim3opt_deliver(((const Sim3OptOut *)c->h_out)[j], sim3opt_arrays(deliver, *a[j].obs, none), a[j]);
    return ORBX_OK;
}

extern "C" int orbx_sim3_optimize(int device, const orbx_sim3opt_obs *obs, const float *cam1, const float *cam2, const double *S12, float th2,
                                  int fix_scale, double *S12_out, uint8_t *inlier, int *n_inliers, orbx_sim3opt_report *report)
{
    const Sim3OptArgs a = { obs, cam1, cam2, S12, th2, fix_scale, S12_out, inlier, n_inliers, report };
    return sim3opt_run("orbx_sim3_optimize", device, &a, 1);
}

extern "C" int orbx_sim3_optimize_batch(int device, orbx_sim3opt_job *jobs, int njobs)
{
    if (!jobs || njobs < 1 || njobs > 64) { orbx_set_error("orbx_sim3_optimize_batch: invalid argument (1 <= njobs <= 64)"); return ORBX_E_INVALID; }
    std::vector<Sim3OptArgs> a((size_t)njobs);
    for (int j = 0; j < njobs; j++)
        a[j] = { jobs[j].obs, jobs[j].cam1, jobs[j].cam2, jobs[j].S12, jobs[j].th2, jobs[j].fix_scale, jobs[j].S12_out, jobs[j].inlier, &jobs[j].n_inliers, jobs[j].report };
    return sim3opt_run("orbx_sim3_optimize_batch", device, a.data(), njobs);
}

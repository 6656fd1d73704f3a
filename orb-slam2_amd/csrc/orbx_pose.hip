// orbx_pose.hip — k_pose_opt: Optimizer::PoseOptimization (reference src/Optimizer.cc:286-513) in one launch.
// One workgroup of 256 threads per job.  The pose (a unit quaternion and a translation, as g2o's SE3Quat keeps it) and every scalar of the
// Levenberg loop live in registers of EVERY thread: each thread runs the 6x6 solve, the exponential and the bookkeeping redundantly on
// values that are bit-identical across the workgroup (they come out of block_sum, which hands every thread the same sums), so the loop
// trip counts are uniform and nothing but the partial sums crosses the LDS.  The observations are strided over the threads; a
// linearisation reduces 28 doubles (21 of H's upper triangle, 6 of b, the robust chi2), a trial one.
// The reduction order is a fixed function of (n, thread index): per thread ascending i, then the xor butterfly across the wave (both
// partners add the same two numbers, so all 64 lanes hold the same bits), then ((w0 + w1) + (w2 + w3)) over the four waves.  No atomics:
// a job's result does not depend on the run or on the other jobs of the launch.
// Per-edge state is one byte, the outlier flag in the job's output array; the error an active edge "keeps" between rounds (the one of the
// last evaluated trial, base of the classification at :441-502) is recomputed from that trial's pose, which gives the same bits.
// The arithmetic is restated in include/orbx.h (orbx_pose_optimize) and, in numpy, in tests/pose_model.py.  Behind the kernel: the
// refusals, the staging and the delivery of the three calls (pose_check, pose_run, pose_deliver and the entry points).
#include "orbx_resident.h"
#include "orbx_lm.h"
#include <float.h>

// One job of k_pose_opt.  Every pointer is a device address.  The host-pointer calls give
// inv_sigma2 / Xw / has_point and leave octave / geom / slot NULL; the resident call gives octave (with lvl_isig), the table's geom and
// slot (a feature has a point where slot >= 0) and leaves the other three NULL.  outlier[n] is the kernel's per-edge state and its output.
struct PoseJob {
    int n, nlevels;      // nlevels: entries of lvl_isig (resident form)
    const float *x, *y, *u_right;
    const float *inv_sigma2; const int32_t *octave;
    const float *Xw; const float4 *geom; const int32_t *slot;
    const uint8_t *has_point;
    uint8_t *outlier;
    float lvl_isig[ORBX_MAX_LEVELS];
    float cam[5];        // fx fy cx cy mbf
    float Tcw[16];
};
struct PoseOut { double pose[12], chi2[4]; float Tcw[16]; int32_t n_corr, rounds, n_bad[4], iterations[4], n_inliers, bad_octave; };

namespace {

struct Edge : Obs { double X, Y, Z; };   // an observation and its map point

__device__ __forceinline__ bool edge_present(const PoseJob &J, int i) { return J.slot ? J.slot[i] >= 0 : J.has_point[i] != 0; }

__device__ __forceinline__ Edge edge_load(const PoseJob &J, int i)
{
    Edge e;
    e.mx = (double)J.x[i]; e.my = (double)J.y[i];
    const float ur = J.u_right[i];
    e.stereo = !(ur < 0.f);   // src/Optimizer.cc:335
    e.mr = (double)ur;
    e.w = (double)(J.inv_sigma2 ? J.inv_sigma2[i] : J.lvl_isig[J.octave[i]]);
    if (J.slot) {
        const float4 g = J.geom[2 * (long long)J.slot[i]];
        e.X = (double)g.x; e.Y = (double)g.y; e.Z = (double)g.z;
    } else {
        e.X = (double)J.Xw[3 * (long long)i]; e.Y = (double)J.Xw[3 * (long long)i + 1]; e.Z = (double)J.Xw[3 * (long long)i + 2];
    }
    return e;
}

__device__ __forceinline__ double edge_chi2(const PoseJob &J, int i, const Pose &P, const Cam &K, bool *stereo)
{
    const Edge e = edge_load(J, i);
    double x, y, z, err[3];
    se3_map(P, e.X, e.Y, e.Z, x, y, z);
    *stereo = e.stereo;
    return edge_error(e, K, x, y, z, err);
}

__global__ __launch_bounds__(256) void k_pose_opt(const PoseJob *__restrict__ jobs, PoseOut *__restrict__ outs)
{
    __shared__ double red[4 * 28];
    const PoseJob &J = jobs[blockIdx.x];
    PoseOut &out = outs[blockIdx.x];
    const int tid = threadIdx.x, n = J.n;
    const Cam K = cam_load(J.cam);
    const double delta_mono = (double)(float)sqrt(5.991), delta_stereo = (double)(float)sqrt(7.815);   // src/Optimizer.cc:322-323

    double cnt[2] = { 0.0, 0.0 };   // correspondences; those whose octave names no level (resident form)
    for (int i = tid; i < n; i += 256)
        if (edge_present(J, i)) {
            cnt[0] += 1.0; J.outlier[i] = 0;
            if (J.octave && (unsigned)J.octave[i] >= (unsigned)J.nlevels) cnt[1] += 1.0;
        }
    block_sum(cnt, red);
    const int n_corr = (int)cnt[0];
    if (cnt[1] != 0.0) {   // refused: the host reports it, nothing else is written
        if (tid == 0) out.bad_octave = 1;
        return;
    }

    Pose start;
    {
        double m[9];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) m[3 * r + c] = (double)J.Tcw[4 * r + c];
        quat_from_matrix(m, start.qx, start.qy, start.qz, start.qw);   // Converter::toSE3Quat: SE3Quat(R, t)
        quat_normalize(start.qx, start.qy, start.qz, start.qw);
        start.tx = (double)J.Tcw[3]; start.ty = (double)J.Tcw[7]; start.tz = (double)J.Tcw[11];
    }

    if (n_corr < 3) {   // :423-424: nothing is optimised, SetPose is not called
        if (tid == 0) {
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 4; c++) out.pose[4 * r + c] = (double)J.Tcw[4 * r + c];
            for (int k = 0; k < 16; k++) out.Tcw[k] = J.Tcw[k];
            for (int k = 0; k < 4; k++) { out.chi2[k] = 0.0; out.n_bad[k] = 0; out.iterations[k] = 0; }
            out.n_corr = n_corr; out.rounds = 0; out.n_inliers = 0; out.bad_octave = 0;
        }
        return;
    }

    Pose P = start;
    int rounds = 0, n_bad = 0;
    double x[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };   // the solver's x: a failed factorisation leaves the previous solution in it
    for (int it = 0; it < 4; it++) {
        const bool robust = it < 3;   // :468-469, :497-498: the kernels go after the third round
        P = start;                    // :437
        Pose Ptrial = start;
        double lambda = 0.0, ni = 2.0, cur_chi = 0.0;
        int stop_bad = 0, iters = 0;
        for (int iter = 0; iter < 10; iter++) {
            // computeActiveErrors + buildSystem at P
            double acc[28];
#pragma unroll
            for (int k = 0; k < 28; k++) acc[k] = 0.0;
            for (int i = tid; i < n; i += 256) {
                if (!edge_present(J, i) || J.outlier[i]) continue;
                const Edge e = edge_load(J, i);
                double X, Y, Z, err[3];
                se3_map(P, e.X, e.Y, e.Z, X, Y, Z);
                const double chi = edge_error(e, K, X, Y, Z, err);
                double rho0 = chi, rho1 = 1.0;
                if (robust) huber(chi, e.stereo ? delta_stereo : delta_mono, rho0, rho1);
                acc[27] += rho0;
                const double invz = 1.0 / Z, invz_2 = invz * invz;   // types_six_dof_expmap.cpp:266-288, :335-364
                double A[3][6];
                A[0][0] = X * Y * invz_2 * K.fx; A[0][1] = -(1.0 + (X * X * invz_2)) * K.fx; A[0][2] = Y * invz * K.fx;
                A[0][3] = -invz * K.fx; A[0][4] = 0.0; A[0][5] = X * invz_2 * K.fx;
                A[1][0] = (1.0 + Y * Y * invz_2) * K.fy; A[1][1] = -X * Y * invz_2 * K.fy; A[1][2] = -X * invz * K.fy;
                A[1][3] = 0.0; A[1][4] = -invz * K.fy; A[1][5] = Y * invz_2 * K.fy;
                A[2][0] = A[0][0] - K.bf * Y * invz_2; A[2][1] = A[0][1] + K.bf * X * invz_2; A[2][2] = A[0][2];
                A[2][3] = A[0][3]; A[2][4] = 0.0; A[2][5] = A[0][5] - K.bf * invz_2;
                const double rw = rho1 * e.w, we0 = e.w * err[0], we1 = e.w * err[1], we2 = e.w * err[2];
                int k = 0;
                if (e.stereo) {
#pragma unroll
                    for (int r = 0; r < 6; r++) {
#pragma unroll
                        for (int c = r; c < 6; c++, k++) acc[k] += ((A[0][r] * rw) * A[0][c] + (A[1][r] * rw) * A[1][c]) + (A[2][r] * rw) * A[2][c];
                        acc[21 + r] -= rho1 * ((A[0][r] * we0 + A[1][r] * we1) + A[2][r] * we2);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 6; r++) {
#pragma unroll
                        for (int c = r; c < 6; c++, k++) acc[k] += (A[0][r] * rw) * A[0][c] + (A[1][r] * rw) * A[1][c];
                        acc[21 + r] -= rho1 * (A[0][r] * we0 + A[1][r] * we1);
                    }
                }
            }
            block_sum(acc, red);
            cur_chi = acc[27];
            const double ini_chi = cur_chi;
            if (iter == 0) lm_start(hu_max_diag<6>(acc), lambda, ni, stop_bad);
            double rho = 0.0;
            int qmax = 0;
            do {
                const Pose backup = P;
                const bool ok = ldlt_small<6>(acc, acc + 21, lambda, x);
                P = pose_update(P, x);
                Ptrial = P;
                double tc[1] = { 0.0 };
                for (int i = tid; i < n; i += 256) {
                    if (!edge_present(J, i) || J.outlier[i]) continue;
                    bool st;
                    const double chi = edge_chi2(J, i, P, K, &st);
                    double rho0 = chi, rho1 = 1.0;
                    if (robust) huber(chi, st ? delta_stereo : delta_mono, rho0, rho1);
                    tc[0] += rho0;
                }
                block_sum(tc, red);
                const double temp_chi = ok ? tc[0] : DBL_MAX;
                double scale = 0.0;
#pragma unroll
                for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + acc[21 + j]);
                rho = lm_gain(cur_chi, temp_chi, scale);
                if (lm_accepts(rho, temp_chi)) {
                    lm_accept(rho, lambda, ni);
                    cur_chi = temp_chi;
                } else {
                    lm_reject(lambda, ni);
                    P = backup;   // pop(): the vertex goes back, the edges keep the errors of the rejected pose
                }
                qmax++;
            } while (rho < 0.0 && qmax < 10);
            iters++;
            if (lm_done(qmax, rho, ini_chi, cur_chi, stop_bad)) break;
        }
        // :441-502: an outlier gets a fresh error at the round's pose, an active edge keeps the error of the last evaluated trial
        double bad[1] = { 0.0 };
        for (int i = tid; i < n; i += 256) {
            if (!edge_present(J, i)) continue;
            bool st;
            const double chi = edge_chi2(J, i, J.outlier[i] ? P : Ptrial, K, &st);
            const bool o = (float)chi > (st ? 7.815f : 5.991f);
            J.outlier[i] = o ? 1 : 0;
            if (o) bad[0] += 1.0;
        }
        block_sum(bad, red);
        n_bad = (int)bad[0];
        rounds = it + 1;
        if (tid == 0) { out.chi2[it] = cur_chi; out.n_bad[it] = n_bad; out.iterations[it] = iters; }
        if (n_corr < 10) break;   // :501: optimizer.edges().size(), all edges
    }
    if (tid == 0) {
        for (int k = rounds; k < 4; k++) { out.chi2[k] = 0.0; out.n_bad[k] = 0; out.iterations[k] = 0; }
        double R[9];
        quat_to_matrix(P, R);
        const double t[3] = { P.tx, P.ty, P.tz };
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) { out.pose[4 * r + c] = R[3 * r + c]; out.Tcw[4 * r + c] = (float)R[3 * r + c]; }
            out.pose[4 * r + 3] = t[r]; out.Tcw[4 * r + 3] = (float)t[r];
        }
        out.Tcw[12] = 0.f; out.Tcw[13] = 0.f; out.Tcw[14] = 0.f; out.Tcw[15] = 1.f;
        out.n_corr = n_corr; out.rounds = rounds; out.n_inliers = n_corr - n_bad; out.bad_octave = 0;
    }
}

}   // namespace

// ---------------------------------------------------------------- host side (include/orbx.h: orbx_pose_optimize)

struct PoseArgs {
    const orbx_pose_obs *obs; const float *cam, *Tcw;
    float *Tcw_out; uint8_t *outlier; int *n_inliers; orbx_pose_report *report;
};

static int pose_check(const char *who, int job, const PoseArgs &a)
{
    if (!a.obs || !a.cam || !a.Tcw || !a.Tcw_out || !a.n_inliers) { orbx_set_error("%s: job %d: NULL obs, cam, Tcw, Tcw_out or n_inliers", who, job); return ORBX_E_INVALID; }
    const orbx_pose_obs &o = *a.obs;
    if (o.n < 0 || o.n > 65535) { orbx_set_error("%s: job %d: n = %d outside [0, 65535]", who, job, o.n); return ORBX_E_INVALID; }
    if (o.n && (!o.x || !o.y || !o.u_right || !o.inv_sigma2 || !o.Xw || !o.has_point || !a.outlier)) {
        orbx_set_error("%s: job %d: observation arrays or outlier missing", who, job);
        return ORBX_E_INVALID;
    }
    return ORBX_OK;
}

// what a job's PoseOut and flag bytes (present(i) says where they count) give the caller
template <typename Present>
static void pose_deliver(const PoseOut &o, const uint8_t *flags, int n, const PoseArgs &a, Present present)
{
    memcpy(a.Tcw_out, o.Tcw, sizeof o.Tcw);
    for (int i = 0; i < n; i++)
        if (present(i)) a.outlier[i] = flags[i];
    *a.n_inliers = o.n_inliers;
    if (!a.report) return;
    orbx_pose_report &r = *a.report;
    r.n_corr = o.n_corr; r.rounds = o.rounds;
    for (int k = 0; k < 4; k++) { r.n_bad[k] = o.n_bad[k]; r.iterations[k] = o.iterations[k]; r.chi2[k] = o.chi2[k]; }
    memcpy(r.pose, o.pose, sizeof o.pose);
}

// staging of the two forms: up [PoseJob x njobs | the jobs' arrays], down [PoseOut x njobs | the jobs' flag bytes]
static int pose_launch_and_fetch(CallCtx *c, size_t blob, size_t out, int njobs)
{
    int rc = call_upload(c, blob);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pose_opt, dim3(njobs), dim3(256), 0, c->stream, (const PoseJob *)c->d_blob, (PoseOut *)c->d_work);
    return call_fetch(c, out);
}

// a job's arrays, stated once (JobArrays, orbx_resident.h): what goes up, then the flag bytes that come down behind the PoseOuts.  Returns
// where the flags were fetched to (DELIVER)
static const uint8_t *pose_arrays(JobArrays &w, const orbx_pose_obs &ob, PoseJob &J)
{
    const size_t n = (size_t)ob.n;
    w.in(J.x, ob.x, 4 * n); w.in(J.y, ob.y, 4 * n); w.in(J.u_right, ob.u_right, 4 * n); w.in(J.inv_sigma2, ob.inv_sigma2, 4 * n);
    w.in(J.Xw, ob.Xw, 12 * n); w.in(J.has_point, ob.has_point, n);
    return w.out(J.outlier, nullptr, n);
}

static int pose_run(const char *who, int device, const PoseArgs *a, int njobs)
{
    size_t total = 0;
    for (int j = 0; j < njobs; j++) {
        const int rc = pose_check(who, j, a[j]);
        if (rc) return rc;
        total += (size_t)a[j].obs->n;
    }
    if (total > ((size_t)1 << 22)) { orbx_set_error("%s: %zu features in all, more than 2^22", who, total); return ORBX_E_CAPACITY; }
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    const size_t jobs_b = a16(sizeof(PoseJob) * (size_t)njobs), outs_b = a16(sizeof(PoseOut) * (size_t)njobs);
    PoseJob none = {};
    JobArrays size(JobArrays::MEASURE, c, jobs_b, outs_b);
    for (int j = 0; j < njobs; j++) pose_arrays(size, *a[j].obs, none);
    const size_t blob = size.up.o, out = size.down.o;
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    JobArrays stage(JobArrays::STAGE, c, jobs_b, outs_b);
    for (int j = 0; j < njobs; j++) {
        PoseJob &J = ((PoseJob *)c->h_blob)[j];
        memset(&J, 0, sizeof J);
        J.n = a[j].obs->n;
        pose_arrays(stage, *a[j].obs, J);
        memcpy(J.cam, a[j].cam, sizeof J.cam); memcpy(J.Tcw, a[j].Tcw, sizeof J.Tcw);
    }
    if ((rc = pose_launch_and_fetch(c, blob, out, njobs))) return rc;
    JobArrays deliver(JobArrays::DELIVER, c, jobs_b, outs_b);
    for (int j = 0; j < njobs; j++) {
        const orbx_pose_obs &ob = *a[j].obs;
        pose_deliver(((const PoseOut *)c->h_out)[j], pose_arrays(deliver, ob, none), ob.n, a[j], [&](int i) { return ob.has_point[i] != 0; });
    }
    return ORBX_OK;
}

extern "C" int orbx_pose_optimize(int device, const orbx_pose_obs *obs, const float *cam, const float *Tcw, float *Tcw_out, uint8_t *outlier,
                                  int *n_inliers, orbx_pose_report *report)
{
    const PoseArgs a = { obs, cam, Tcw, Tcw_out, outlier, n_inliers, report };
    return pose_run("orbx_pose_optimize", device, &a, 1);
}

extern "C" int orbx_pose_optimize_batch(int device, orbx_pose_job *jobs, int njobs)
{
    if (!jobs || njobs < 1 || njobs > 1024) { orbx_set_error("orbx_pose_optimize_batch: invalid argument (1 <= njobs <= 1024)"); return ORBX_E_INVALID; }
    std::vector<PoseArgs> a((size_t)njobs);
    for (int j = 0; j < njobs; j++) a[j] = { jobs[j].obs, jobs[j].cam, jobs[j].Tcw, jobs[j].Tcw_out, jobs[j].outlier, &jobs[j].n_inliers, jobs[j].report };
    return pose_run("orbx_pose_optimize_batch", device, a.data(), njobs);
}

extern "C" int orbx_frame_pose_optimize(const orbx_frame *cur, const orbx_mappoints *m, const int32_t *slot_of_feature,
                                        const float *inv_level_sigma2, int nlevels, const float *cam, const float *Tcw, float *Tcw_out,
                                        uint8_t *outlier, int *n_inliers, orbx_pose_report *report)
{
    const char *who = "orbx_frame_pose_optimize";
    if (!cur || !m || !inv_level_sigma2 || !cam || !Tcw || !Tcw_out || !n_inliers || nlevels < 1 || nlevels > ORBX_MAX_LEVELS ||
        (cur->n && (!slot_of_feature || !outlier))) {
        orbx_set_error("%s: invalid argument (a frame, a table, slots and outlier for its features, 1 <= nlevels <= %d, cam, Tcw, Tcw_out, n_inliers)", who, ORBX_MAX_LEVELS);
        return ORBX_E_INVALID;
    }
    if (cur->device != m->device) { orbx_set_error("%s: the frame and the table live on different devices", who); return ORBX_E_INVALID; }
    std::shared_lock<std::shared_timed_mutex> lk(m->mu);
    const int n = cur->n;
    for (int i = 0; i < n; i++) {
        const int s = slot_of_feature[i];
        if (s == -1) continue;
        if (s < 0 || s >= m->capacity) { orbx_set_error("%s: feature %d: slot %d outside [0, %d)", who, i, s, m->capacity); return ORBX_E_INVALID; }
        if (m->have[s] != 3) { orbx_set_error("%s: feature %d: slot %d is not set", who, i, s); return ORBX_E_INVALID; }
        if (!cur->h_oct.empty() && (cur->h_oct[i] < 0 || cur->h_oct[i] >= nlevels)) {
            orbx_set_error("%s: feature %d: octave %d outside [0, %d)", who, i, cur->h_oct[i], nlevels);
            return ORBX_E_INVALID;
        }
    }
    CallCtx *c;
    int rc = orbx_call_ctx(cur->device, &c);
    if (rc) return rc;
    const size_t nn = (size_t)n, jobs_b = a16(sizeof(PoseJob)), outs_b = a16(sizeof(PoseOut));
    const size_t blob = jobs_b + a16(4 * nn), out = outs_b + a16(nn);
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    PoseJob &J = *(PoseJob *)c->h_blob;
    memset(&J, 0, sizeof J);
    const DevFrame F = frame_dev(cur);
    J.n = n; J.nlevels = nlevels;
    J.x = F.x; J.y = F.y; J.u_right = F.u_right; J.octave = F.octave;
    J.geom = m->d_geom; J.slot = (const int32_t *)(c->d_blob + jobs_b);
    J.outlier = c->d_work + outs_b;
    memcpy(J.lvl_isig, inv_level_sigma2, sizeof(float) * (size_t)nlevels);
    memcpy(J.cam, cam, sizeof J.cam); memcpy(J.Tcw, Tcw, sizeof J.Tcw);
    if (n) memcpy(c->h_blob + jobs_b, slot_of_feature, 4 * nn);
    if ((rc = frame_order_before(cur, c->stream))) return rc;
    if ((rc = mappoints_order_before(m, c->stream))) return rc;
    if ((rc = pose_launch_and_fetch(c, blob, out, 1))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    const PoseOut &po = *(const PoseOut *)ho;
    if (po.bad_octave) {   // a frame made from extraction outputs has its octaves on the device only: the kernel checks them first and stops
        orbx_set_error("%s: a feature with a point has an octave outside [0, %d)", who, nlevels);
        return ORBX_E_INVALID;
    }
    const PoseArgs a = { nullptr, cam, Tcw, Tcw_out, outlier, n_inliers, report };
    pose_deliver(po, ho + outs_b, n, a, [&](int i) { return slot_of_feature[i] >= 0; });
    return ORBX_OK;
}

// orbx_sim3.hip — k_sim3: every hypothesis of Sim3Solver's RANSAC (reference src/Sim3Solver.cc:233-371) for every job of one call.
// One wave64 per (job, hypothesis), four waves per workgroup.  A wave finds its job by bisecting the jobs' first-wave numbers (at most 64),
// reads its three sample indices and the six points, and solves Horn's closed form lane-uniformly in registers: centroids, M, N, a cyclic
// Jacobi on the symmetric 4x4 (every matrix index is a constant: no scratch), the rotation from the quaternion, scale, translation, T12 and
// T21.  Its lanes then stride over the job's points, 64 at a time: both reprojections, both strict comparisons, and __ballot of the
// predicate IS the mask word (lane 0 stores it, __popcll adds it to the count).  No LDS, no atomics; a job's points are a few KB that
// many waves read: L2 serves them.
// The arithmetic is restated in include/orbx.h (orbx_sim3_hypotheses) and, in numpy, in tests/sim3_model.py.  Behind the kernel: the
// refusals, the staging (one blob up, one block down) and the delivery of the two calls (sim3_check, sim3_run and the entry points).
#include "orbx_resident.h"
#include "orbx_wave.h"

// One job of k_sim3.  Every pointer is a device address.  first = the number of this job's
// first wave: wave first + h evaluates hypothesis h; the jobs of a call are in rising order of it.
struct Sim3Job {
    int n, n_hyp, fix_scale, first;
    const float *X1, *X2, *max_err1, *max_err2;
    const int32_t *samples;
    int32_t *n_inliers; float *srt; uint64_t *inlier_bits;
    float K1[4], K2[4];
};

namespace {

// where OpenCV calls hypot
__device__ __forceinline__ float hyp(float a, float b)
{
    return (float)sqrt((double)a * (double)a + (double)b * (double)b);
}

__device__ __forceinline__ void rot(float &a, float &b, float c, float s)
{
    const float a0 = a, b0 = b;
    a = a0 * c - b0 * s;
    b = a0 * s + b0 * c;
}

// One Jacobi rotation on the pivot A[K][L], K < L, of the upper triangle A with diagonal W; eigenvectors are the rows of V.
template <int K, int L>
__device__ __forceinline__ bool jacobi_rot(float (&A)[4][4], float (&W)[4], float (&V)[4][4])
{
    const float p = A[K][L];
    if ((double)p * (double)p <= 0x1p-46 * fabs((double)W[K] * (double)W[L])) return false;
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
#pragma unroll
    for (int i = 0; i < K; i++) rot(A[i][K], A[i][L], c, s);
#pragma unroll
    for (int i = K + 1; i < L; i++) rot(A[K][i], A[i][L], c, s);
#pragma unroll
    for (int i = L + 1; i < 4; i++) rot(A[K][i], A[L][i], c, s);
#pragma unroll
    for (int i = 0; i < 4; i++) rot(V[K][i], V[L][i], c, s);
    return true;
}

// the eigenvector of N's largest eigenvalue (of equal ones the earlier) -> q[4]
__device__ __forceinline__ void top_eigenvector(float (&A)[4][4], float q[4])
{
    float V[4][4], W[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        W[i] = A[i][i];
#pragma unroll
        for (int k = 0; k < 4; k++) V[i][k] = i == k ? 1.0f : 0.0f;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        changed |= jacobi_rot<0, 1>(A, W, V);
        changed |= jacobi_rot<0, 2>(A, W, V);
        changed |= jacobi_rot<0, 3>(A, W, V);
        changed |= jacobi_rot<1, 2>(A, W, V);
        changed |= jacobi_rot<1, 3>(A, W, V);
        changed |= jacobi_rot<2, 3>(A, W, V);
        if (!changed) break;
    }
    float best = W[0];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = V[0][k];
#pragma unroll
    for (int i = 1; i < 4; i++) {
        if (W[i] > best) {
            best = W[i];
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = V[i][k];
        }
    }
}

// Project / FromCameraToImage (:389-433): one axis of the pinhole
__device__ __forceinline__ float pix(float f, float c, float X, float invz)
{
    const float x = X * invz;
    return f * x + c;
}

__device__ __forceinline__ float err2(float u0, float v0, float u1, float v1)
{
    const float d0 = u0 - u1, d1 = v0 - v1;
    return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}

__global__ __launch_bounds__(256) void k_sim3(const Sim3Job *__restrict__ jobs, int njobs, int total)
{
    const int g = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (g >= total) return;
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = njobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g >= jobs[mid].first) lo = mid; else hi = mid;
    }
    const Sim3Job &J = jobs[lo];
    const int h = g - J.first, n = J.n;
    const int32_t *sm = J.samples + 3 * (long long)h;

    // ---- ComputeSim3 (:233-344), the same in every lane
    float P1[3][3], P2[3][3], O1[3], O2[3];   // [row][point]
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const long long idx = sm[i];
#pragma unroll
        for (int r = 0; r < 3; r++) { P1[r][i] = J.X1[3 * idx + r]; P2[r][i] = J.X2[3 * idx + r]; }
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        O1[r] = (float)((double)((P1[r][0] + P1[r][1]) + P1[r][2]) * (1.0 / 3.0));
        O2[r] = (float)((double)((P2[r][0] + P2[r][1]) + P2[r][2]) * (1.0 / 3.0));
#pragma unroll
        for (int i = 0; i < 3; i++) { P1[r][i] -= O1[r]; P2[r][i] -= O2[r]; }   // Pr1, Pr2
    }
    float M[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[r][c] = (float)dotd(P2[r][0], P2[r][1], P2[r][2], P1[c][0], P1[c][1], P1[c][2]);
    float A[4][4];
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
    A[1][0] = A[2][0] = A[2][1] = A[3][0] = A[3][1] = A[3][2] = 0.f;   // the lower triangle is never read
    float q[4];
    top_eigenvector(A, q);
    const bool degenerate = q[1] == 0.f && q[2] == 0.f && q[3] == 0.f;   // norm(vec) == 0 (:285-287 divide by it)

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
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float p3 = (float)dotd(R[r][0], R[r][1], R[r][2], P2[0][i], P2[1][i], P2[2][i]);
                nom += (double)P1[r][i] * (double)p3;
                den += (double)(p3 * p3);
            }
        s12 = (float)(nom / den);
    }
    const double sd = (double)s12, si = 1.0 / (double)s12;
    float t12[3], sR[3][3], sRi[3][3], t21[3];
#pragma unroll
    for (int r = 0; r < 3; r++) t12[r] = (float)((double)O1[r] - sd * dotd(R[r][0], R[r][1], R[r][2], O2[0], O2[1], O2[2]));
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) { sR[r][c] = (float)(sd * (double)R[r][c]); sRi[r][c] = (float)(si * (double)R[c][r]); }
#pragma unroll
    for (int r = 0; r < 3; r++) t21[r] = (float)(-dotd(sRi[r][0], sRi[r][1], sRi[r][2], t12[0], t12[1], t12[2]));

    // ---- CheckInliers (:347-371): lane i % 64 takes point i
    const int words = (n + 63) >> 6;
    uint64_t *bits = J.inlier_bits + (long long)h * words;
    const float fx1 = J.K1[0], fy1 = J.K1[1], cx1 = J.K1[2], cy1 = J.K1[3];
    const float fx2 = J.K2[0], fy2 = J.K2[1], cx2 = J.K2[2], cy2 = J.K2[3];
    int count = 0;
    for (int wd = 0; wd < words; wd++) {
        const int i = wd * 64 + lane;
        bool in = false;
        if (i < n && !degenerate) {
            const float a0 = J.X1[3 * i], a1 = J.X1[3 * i + 1], a2 = J.X1[3 * i + 2];
            const float b0 = J.X2[3 * i], b1 = J.X2[3 * i + 1], b2 = J.X2[3 * i + 2];
            const float ia = 1.0f / a2, ib = 1.0f / b2;
            const float u11 = pix(fx1, cx1, a0, ia), v11 = pix(fy1, cy1, a1, ia);   // mvP1im1
            const float u22 = pix(fx2, cx2, b0, ib), v22 = pix(fy2, cy2, b1, ib);   // mvP2im2
            const float c0 = (float)(dotd(sR[0][0], sR[0][1], sR[0][2], b0, b1, b2) + (double)t12[0]);
            const float c1 = (float)(dotd(sR[1][0], sR[1][1], sR[1][2], b0, b1, b2) + (double)t12[1]);
            const float c2 = (float)(dotd(sR[2][0], sR[2][1], sR[2][2], b0, b1, b2) + (double)t12[2]);
            const float ic = 1.0f / c2;
            const float e1 = err2(u11, v11, pix(fx1, cx1, c0, ic), pix(fy1, cy1, c1, ic));    // mvP1im1 - vP2im1
            const float d0 = (float)(dotd(sRi[0][0], sRi[0][1], sRi[0][2], a0, a1, a2) + (double)t21[0]);
            const float d1 = (float)(dotd(sRi[1][0], sRi[1][1], sRi[1][2], a0, a1, a2) + (double)t21[1]);
            const float d2 = (float)(dotd(sRi[2][0], sRi[2][1], sRi[2][2], a0, a1, a2) + (double)t21[2]);
            const float id = 1.0f / d2;
            const float e2 = err2(pix(fx2, cx2, d0, id), pix(fy2, cy2, d1, id), u22, v22);    // vP1im2 - mvP2im2
            in = e1 < J.max_err1[i] && e2 < J.max_err2[i];
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) bits[wd] = m;
        count += __popcll(m);
    }
    if (lane == 0) J.n_inliers[h] = count;
    if (lane < 13) {
        float v = lane == 0 ? s12 : lane < 10 ? R[0][0] : t12[0];
#pragma unroll
        for (int k = 1; k < 10; k++) if (lane == k) v = R[(k - 1) / 3][(k - 1) % 3];
#pragma unroll
        for (int k = 10; k < 13; k++) if (lane == k) v = t12[k - 10];
        J.srt[13 * (long long)h + lane] = degenerate ? __uint_as_float(0x7fc00000u) : v;
    }
}

}   // namespace

// ---------------------------------------------------------------- host side (include/orbx.h: orbx_sim3_hypotheses)

static int sim3_check(const char *who, int j, const orbx_sim3_job &J)
{
    if (!J.X1 || !J.X2 || !J.max_err1 || !J.max_err2 || !J.samples || !J.n_inliers || !J.srt || !J.inlier_bits) {
        orbx_set_error("%s: job %d: a NULL array", who, j);
        return ORBX_E_INVALID;
    }
    if (J.n < 3 || J.n > 65535) { orbx_set_error("%s: job %d: n = %d outside [3, 65535]", who, j, J.n); return ORBX_E_INVALID; }
    if (J.n_hyp < 1 || J.n_hyp > 1024) { orbx_set_error("%s: job %d: n_hyp = %d outside [1, 1024]", who, j, J.n_hyp); return ORBX_E_INVALID; }
    for (int h = 0; h < J.n_hyp; h++) {
        const int32_t *s = J.samples + 3 * (size_t)h;
        if (s[0] < 0 || s[0] >= J.n || s[1] < 0 || s[1] >= J.n || s[2] < 0 || s[2] >= J.n) {
            orbx_set_error("%s: job %d: hypothesis %d: a sample index outside [0, %d)", who, j, h, J.n);
            return ORBX_E_INVALID;
        }
        if (s[0] == s[1] || s[0] == s[2] || s[1] == s[2]) {
            orbx_set_error("%s: job %d: hypothesis %d: two equal sample indices", who, j, h);
            return ORBX_E_INVALID;
        }
    }
    return ORBX_OK;
}

// a job's arrays, stated once (JobArrays, orbx_resident.h): what goes up, and the results, which lie in the work area
static void sim3_arrays(JobArrays &w, const orbx_sim3_job &in, Sim3Job &J)
{
    const size_t n = (size_t)in.n, nh = (size_t)in.n_hyp;
    w.in(J.X1, in.X1, 12 * n); w.in(J.X2, in.X2, 12 * n); w.in(J.max_err1, in.max_err1, 4 * n); w.in(J.max_err2, in.max_err2, 4 * n);
    w.in(J.samples, in.samples, 12 * nh);
    w.out(J.n_inliers, in.n_inliers, 4 * nh); w.out(J.srt, in.srt, 52 * nh); w.out(J.inlier_bits, in.inlier_bits, 8 * nh * ((n + 63) / 64));
}

static int sim3_run(const char *who, int device, orbx_sim3_job *jobs, int njobs)
{
    if (!jobs || njobs < 1 || njobs > 64) { orbx_set_error("%s: invalid argument (jobs, 1 <= njobs <= 64)", who); return ORBX_E_INVALID; }
    size_t words = 0, total = 0;
    for (int j = 0; j < njobs; j++) {
        const int rc = sim3_check(who, j, jobs[j]);
        if (rc) return rc;
        words += (size_t)jobs[j].n_hyp * (((size_t)jobs[j].n + 63) / 64);
        total += (size_t)jobs[j].n_hyp;
    }
    if (words > ((size_t)1 << 22)) { orbx_set_error("%s: %zu mask words in all, more than 2^22", who, words); return ORBX_E_CAPACITY; }
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    const size_t jobs_b = a16(sizeof(Sim3Job) * (size_t)njobs);
    Sim3Job none = {};
    JobArrays size(JobArrays::MEASURE, c, jobs_b, 0);
    for (int j = 0; j < njobs; j++) sim3_arrays(size, jobs[j], none);
    const size_t blob = size.up.o, out = size.down.o;
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    JobArrays stage(JobArrays::STAGE, c, jobs_b, 0);
    int first = 0;
    for (int j = 0; j < njobs; j++) {
        const orbx_sim3_job &in = jobs[j];
        Sim3Job &J = ((Sim3Job *)c->h_blob)[j];
        memset(&J, 0, sizeof J);
        J.n = in.n; J.n_hyp = in.n_hyp; J.fix_scale = in.fix_scale ? 1 : 0; J.first = first;
        first += in.n_hyp;
        sim3_arrays(stage, in, J);
        memcpy(J.K1, in.K1, sizeof J.K1); memcpy(J.K2, in.K2, sizeof J.K2);
    }
    if ((rc = call_upload(c, blob))) return rc;
    hipLaunchKernelGGL(k_sim3, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, c->stream, (const Sim3Job *)c->d_blob, njobs, (int)total);   // one wave per hypothesis
    if ((rc = call_fetch(c, out))) return rc;
    JobArrays deliver(JobArrays::DELIVER, c, jobs_b, 0);
    for (int j = 0; j < njobs; j++) sim3_arrays(deliver, jobs[j], none);
    return ORBX_OK;
}

extern "C" int orbx_sim3_hypotheses(int device, orbx_sim3_job *job)
{
    if (!job) { orbx_set_error("orbx_sim3_hypotheses: a NULL job"); return ORBX_E_INVALID; }
    return sim3_run("orbx_sim3_hypotheses", device, job, 1);
}

extern "C" int orbx_sim3_hypotheses_batch(int device, orbx_sim3_job *jobs, int njobs)
{
    return sim3_run("orbx_sim3_hypotheses_batch", device, jobs, njobs);
}

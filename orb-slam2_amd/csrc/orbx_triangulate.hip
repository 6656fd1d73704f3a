// orbx_triangulate.hip — k_triangulate, k_tri_resolve: the body of LocalMapping::CreateNewMapPoints' match loop (reference
// src/LocalMapping.cc:327-511) for every (current keyframe, neighbour) pair list of one call.
// k_triangulate: one pair per thread, workgroups of 256.  A thread finds its neighbour by bisecting the prefix table of the pair lists (at
// most 65 entries), reads the two features and the two views and runs parallax test, 4x4 Jacobi SVD or UnprojectStereo, the depth tests,
// the reprojection gates and the scale gate on registers alone: no LDS, no atomics, no scratch (the Jacobi's pair loop is unrolled so that
// every matrix index is a constant).  It writes one status byte and three floats.
// k_tri_resolve<0 / 1>: first neighbour wins.  Pass 0: a created pair does atomicMin(first[idx1], neighbour); pass 1: a created pair whose
// neighbour is larger than first[idx1] becomes 32 + status.  An integer minimum does not depend on the order of the threads.
// The arithmetic is restated in include/orbx.h (orbx_triangulate_pairs) and, in numpy, in tests/triangulate_model.py; the host side of
// the calls is in orbx_proj.hip, beside the frame handle it reads.
#include "orbx_internal.h"

namespace {

struct V3 { float x, y, z; };

// (double) a . b, left to right
__device__ __forceinline__ double dotd(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}

// Rwc * v (+ add): Rwc is the transpose of the rotation block of Tcw[3][4]; one cast per row
__device__ __forceinline__ V3 rot_wc(const float *T, float v0, float v1, float v2, double a0, double a1, double a2)
{
    V3 r;
    r.x = (float)(dotd(T[0], T[4], T[8], v0, v1, v2) + a0);
    r.y = (float)(dotd(T[1], T[5], T[9], v0, v1, v2) + a1);
    r.z = (float)(dotd(T[2], T[6], T[10], v0, v1, v2) + a2);
    return r;
}

// row r of [R | t] applied to X: (float)(R.row(r) . X + t[r])
__device__ __forceinline__ float cam_row(const float *T, int r, const V3 &X)
{
    return (float)(dotd(T[4 * r], T[4 * r + 1], T[4 * r + 2], X.x, X.y, X.z) + (double)T[4 * r + 3]);
}

// cos(2 atan2(mb / 2, depth)) as (d^2 - h^2) / (d^2 + h^2)
__device__ __forceinline__ float stereo_cos(float mb, float depth)
{
    const double h = (double)(mb / 2.0f), d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

__device__ __forceinline__ float norm3(float x, float y, float z)
{
    return (float)sqrt(((double)x * (double)x + (double)y * (double)y) + (double)z * (double)z);
}

// One Jacobi rotation of columns i < j of A (rows i, j of At) and of the same rows of V; W holds the columns' squared norms.
__device__ __forceinline__ bool jacobi_pair(float (&Ai)[4], float (&Aj)[4], float (&Vi)[4], float (&Vj)[4], double &Wi, double &Wj)
{
    double a = Wi, b = Wj, p = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) p += (double)Ai[k] * (double)Aj[k];
    if (fabs(p) <= (double)(2.0f * 1.1920928955078125e-7f) * sqrt(a * b)) return false;
    p *= 2.0;
    const double beta = a - b, gamma = sqrt(p * p + beta * beta);
    float c, s;
    if (beta < 0.0) {
        const double delta = (gamma - beta) * 0.5;
        s = (float)sqrt(delta / gamma);
        c = (float)(p / ((gamma * (double)s) * 2.0));
    } else {
        c = (float)sqrt((gamma + beta) / (gamma * 2.0));
        s = (float)(p / ((gamma * (double)c) * 2.0));
    }
    a = 0.0; b = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float t0 = c * Ai[k] + s * Aj[k], t1 = (-s) * Ai[k] + c * Aj[k];
        Ai[k] = t0; Aj[k] = t1;
        a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
    }
    Wi = a; Wj = b;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float t0 = c * Vi[k] + s * Vj[k], t1 = (-s) * Vi[k] + c * Vj[k];
        Vi[k] = t0; Vj[k] = t1;
    }
    return true;
}

// the right singular vector of A's smallest singular value (At[i] = column i of A) -> v[4]
__device__ __forceinline__ void null_vector(float (&At)[4][4], float v[4])
{
    float V[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) { sd += (double)At[i][k] * (double)At[i][k]; V[i][k] = i == k ? 1.0f : 0.0f; }
        W[i] = sd;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        changed |= jacobi_pair(At[0], At[1], V[0], V[1], W[0], W[1]);
        changed |= jacobi_pair(At[0], At[2], V[0], V[2], W[0], W[2]);
        changed |= jacobi_pair(At[0], At[3], V[0], V[3], W[0], W[3]);
        changed |= jacobi_pair(At[1], At[2], V[1], V[2], W[1], W[2]);
        changed |= jacobi_pair(At[1], At[3], V[1], V[3], W[1], W[3]);
        changed |= jacobi_pair(At[2], At[3], V[2], V[3], W[2], W[3]);
        if (!changed) break;
    }
    double best = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) sd += (double)At[i][k] * (double)At[i][k];
        if (i == 0 || sd <= best) {   // a tie takes the later column
            best = sd;
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = V[i][k];
        }
    }
}

// the reprojection gate of one keyframe (:418-445 / :449-472); mbf is ALWAYS the current keyframe's (:465)
__device__ __forceinline__ bool reproj_ok(const orbx_tri_view &v, const V3 &X, float z, float kx, float ky, float ur, bool stereo, float sigma2, float mbf)
{
    const float x = cam_row(v.Tcw, 0, X), y = cam_row(v.Tcw, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = v.fx * x * invz + v.cx, w = v.fy * y * invz + v.cy;
    const float ex = u - kx, ey = w - ky;
    if (!stereo) return !((double)(ex * ex + ey * ey) > 5.991 * (double)sigma2);
    const float u_r = u - mbf * invz;
    const float er = u_r - ur;
    return !((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2);
}

__device__ __forceinline__ int pair_neighbour(const TriHead &H, int g)
{
    int lo = 0, hi = H.n2;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g >= H.prefix[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_triangulate(const TriHead *__restrict__ Hp, const int32_t *__restrict__ pairs,
                                                     uint8_t *__restrict__ status, float *__restrict__ x3d, int *__restrict__ bad)
{
    const TriHead &H = *Hp;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= H.total) return;
    const int nb = pair_neighbour(H, g);
    const int i1 = pairs[2 * (long long)g], i2 = pairs[2 * (long long)g + 1];
    const orbx_tri_view &v1 = H.v1;
    const orbx_tri_view &v2 = H.nb[nb].v;
    const TriFeat &f1 = H.f1;
    const TriFeat &f2 = H.nb[nb].f;

    const float k1x = f1.x[i1], k1y = f1.y[i1], ur1 = f1.u_right[i1];
    const float k2x = f2.x[i2], k2y = f2.y[i2], ur2 = f2.u_right[i2];
    const int o1 = f1.octave[i1], o2 = f2.octave[i2];
    const bool st1 = ur1 >= 0.f, st2 = ur2 >= 0.f;
    int st = -1;
    V3 X = { 0.f, 0.f, 0.f };
    bool have_x = false;
    do {
        if ((unsigned)o1 >= (unsigned)H.nlevels || (unsigned)o2 >= (unsigned)H.nlevels) { *bad = 1; st = 255; break; }   // resident octaves the host never saw
        const float xn1x = (k1x - v1.cx) * v1.invfx, xn1y = (k1y - v1.cy) * v1.invfy;
        const float xn2x = (k2x - v2.cx) * v2.invfx, xn2y = (k2y - v2.cy) * v2.invfy;
        const V3 r1 = rot_wc(v1.Tcw, xn1x, xn1y, 1.0f, 0.0, 0.0, 0.0), r2 = rot_wc(v2.Tcw, xn2x, xn2y, 1.0f, 0.0, 0.0, 0.0);
        const double dot = dotd(r1.x, r1.y, r1.z, r2.x, r2.y, r2.z);
        const double n1 = sqrt(dotd(r1.x, r1.y, r1.z, r1.x, r1.y, r1.z)), n2 = sqrt(dotd(r2.x, r2.y, r2.z, r2.x, r2.y, r2.z));
        const float cos_rays = (float)(dot / (n1 * n2));
        float cs1 = cos_rays + 1.0f, cs2 = cs1;
        if (st1) cs1 = stereo_cos(v1.mb, f1.depth[i1]);
        else if (st2) cs2 = stereo_cos(v2.mb, f2.depth[i2]);
        const float cos_stereo = cs2 < cs1 ? cs2 : cs1;
        if (cos_rays < cos_stereo && cos_rays > 0.f && (st1 || st2 || (double)cos_rays < 0.9998)) {
            float At[4][4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                At[c][0] = xn1x * v1.Tcw[8 + c] - v1.Tcw[c];
                At[c][1] = xn1y * v1.Tcw[8 + c] - v1.Tcw[4 + c];
                At[c][2] = xn2x * v2.Tcw[8 + c] - v2.Tcw[c];
                At[c][3] = xn2y * v2.Tcw[8 + c] - v2.Tcw[4 + c];
            }
            float v[4];
            null_vector(At, v);
            if (v[3] == 0.f) { st = 17; break; }
            X.x = v[0] / v[3]; X.y = v[1] / v[3]; X.z = v[2] / v[3];
            st = 0;
        } else if (st1 && cs1 < cs2) {
            const float z = f1.depth[i1];
            if (!(z > 0.f)) { st = 24; break; }
            const float x = (f1.raw_x[i1] - v1.cx) * z * v1.invfx, y = (f1.raw_y[i1] - v1.cy) * z * v1.invfy;
            X = rot_wc(v1.Tcw, x, y, z, (double)v1.Ow[0], (double)v1.Ow[1], (double)v1.Ow[2]);
            st = 1;
        } else if (st2 && cs2 < cs1) {
            const float z = f2.depth[i2];
            if (!(z > 0.f)) { st = 24; break; }
            const float x = (f2.raw_x[i2] - v2.cx) * z * v2.invfx, y = (f2.raw_y[i2] - v2.cy) * z * v2.invfy;
            X = rot_wc(v2.Tcw, x, y, z, (double)v2.Ow[0], (double)v2.Ow[1], (double)v2.Ow[2]);
            st = 2;
        } else { st = 16; break; }
        have_x = true;
        const int created = st;
        const float z1 = cam_row(v1.Tcw, 2, X);
        if (z1 <= 0.f) { st = 18; break; }
        const float z2 = cam_row(v2.Tcw, 2, X);
        if (z2 <= 0.f) { st = 19; break; }
        if (!reproj_ok(v1, X, z1, k1x, k1y, ur1, st1, H.sigma2[o1], v1.mbf)) { st = 20; break; }
        if (!reproj_ok(v2, X, z2, k2x, k2y, ur2, st2, H.sigma2[o2], v1.mbf)) { st = 21; break; }
        const float d1 = norm3(X.x - v1.Ow[0], X.y - v1.Ow[1], X.z - v1.Ow[2]);
        const float d2 = norm3(X.x - v2.Ow[0], X.y - v2.Ow[1], X.z - v2.Ow[2]);
        if (d1 == 0.f || d2 == 0.f) { st = 22; break; }
        const float ratio_dist = d2 / d1, ratio_oct = H.sf[o1] / H.sf[o2];
        if (ratio_dist * H.ratio_factor < ratio_oct || ratio_dist > ratio_oct * H.ratio_factor) { st = 23; break; }
        st = created;
    } while (0);
    status[g] = (uint8_t)st;
    x3d[3 * (long long)g] = have_x ? X.x : 0.f;
    x3d[3 * (long long)g + 1] = have_x ? X.y : 0.f;
    x3d[3 * (long long)g + 2] = have_x ? X.z : 0.f;
}

template <int PASS>
__global__ __launch_bounds__(256) void k_tri_resolve(const TriHead *__restrict__ Hp, const int32_t *__restrict__ pairs,
                                                     uint8_t *__restrict__ status, int *__restrict__ first)
{
    const TriHead &H = *Hp;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= H.total) return;
    const int s = status[g];
    if (s > 2) return;
    const int nb = pair_neighbour(H, g), i1 = pairs[2 * (long long)g];
    if (PASS == 0) atomicMin(&first[i1], nb);
    else if (nb > first[i1]) status[g] = (uint8_t)(32 + s);
}

}   // namespace

void orbx_triangulate_launch(const TriHead *d_head, const int32_t *d_pairs, int total, uint8_t *d_status, float *d_x3d, int *d_bad, int *d_first,
                             hipStream_t s)
{
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_triangulate, grid, block, 0, s, d_head, d_pairs, d_status, d_x3d, d_bad);
    hipLaunchKernelGGL(k_tri_resolve<0>, grid, block, 0, s, d_head, d_pairs, d_status, d_first);
    hipLaunchKernelGGL(k_tri_resolve<1>, grid, block, 0, s, d_head, d_pairs, d_status, d_first);
}

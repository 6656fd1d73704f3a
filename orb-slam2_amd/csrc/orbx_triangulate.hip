// orbx_triangulate.hip — k_triangulate, k_tri_resolve: the body of LocalMapping::CreateNewMapPoints' match loop (reference
// src/LocalMapping.cc:327-511) for every (current keyframe, neighbour) pair list of one call.
// k_triangulate: one pair per thread, workgroups of 256.  A thread finds its neighbour by bisecting the prefix table of the pair lists (at
// most 65 entries), reads the two features and the two views and runs parallax test, 4x4 Jacobi SVD or UnprojectStereo, the depth tests,
// the reprojection gates and the scale gate on registers alone: no LDS, no atomics, no scratch (the Jacobi's pair loop is unrolled so that
// every matrix index is a constant).  It writes one status byte and three floats.
// k_tri_resolve<0 / 1>: first neighbour wins.  Pass 0: a created pair does atomicMin(first[idx1], neighbour); pass 1: a created pair whose
// neighbour is larger than first[idx1] becomes 32 + status.  An integer minimum does not depend on the order of the threads.
// The arithmetic is restated in include/orbx.h (orbx_triangulate_pairs) and, in numpy, in tests/triangulate_model.py.  Behind the kernels:
// the refusals, the staging and the delivery of the two calls (tri_check, tri_run and the entry points).
#include "orbx_resident.h"
#include "orbx_wave.h"
#include <stddef.h>

// What k_triangulate reads besides the pair list.  Every pointer is a device address; raw_x / raw_y are x / y and
// depth is NULL (never read: no stereo feature) where a keyframe has no depth attached.  prefix[i] = pairs of the neighbours before i,
// prefix[n2] = total; the call uploads the head up to nb[n2].
struct TriFeat { const float *x, *y, *u_right, *depth, *raw_x, *raw_y; const int32_t *octave; };
struct TriHead {
    int n2, total, nlevels;
    float ratio_factor;
    int prefix[65];
    float sf[ORBX_MAX_LEVELS], sigma2[ORBX_MAX_LEVELS];
    orbx_tri_view v1; TriFeat f1;
    struct Nb { orbx_tri_view v; TriFeat f; } nb[64];
};

namespace {

struct V3 { float x, y, z; };

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

#include "orbx_svd4.h"   // jacobi_pair, null_vector: the 4x4 routine of the contract, shared with orbx_initializer.hip

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

// ---------------------------------------------------------------- host side (include/orbx.h: orbx_triangulate_pairs)

// what the host knows of one keyframe of a call (NULL: only the device has it)
struct TriHostKf { int n; const int32_t *octave; const float *u_right; bool has_depth; };

struct TriArgs {
    int n2, cap, nlevels;
    const int32_t *pairs; const int *npairs;
    const orbx_tri_view *v1, *v2s;
    const float *sf, *sigma2;
    float ratio_factor;
    uint8_t *status; float *x3d; int *n_new;
};

// the refusals of both forms, in their order: the arguments, the keyframes (host_kfs(h) fills h[0] for k1 and h[1 + i] for k2s[i], or
// refuses), the pair lists; *total = the pairs of all lists
template <class HostKfs>
static int tri_check(const char *who, const void *k1, const void *k2s, const TriArgs &a, HostKfs host_kfs, size_t *total)
{
    if (!k1 || !a.v1 || !k2s || !a.v2s || !a.pairs || !a.npairs || !a.sf || !a.sigma2 || !a.status || !a.x3d || !a.n_new || a.n2 < 1 || a.n2 > 64) {
        orbx_set_error("%s: invalid argument (no NULL argument, 1 <= n2 <= 64)", who);
        return ORBX_E_INVALID;
    }
    TriHostKf h[65];
    if (const int rc = host_kfs(h)) return rc;
    const TriHostKf &h1 = h[0], *h2 = h + 1;
    if (a.cap < 1 || a.nlevels < 1 || a.nlevels > ORBX_MAX_LEVELS) {
        orbx_set_error("%s: invalid argument (cap >= 1, 1 <= nlevels <= %d)", who, ORBX_MAX_LEVELS);
        return ORBX_E_INVALID;
    }
    size_t t = 0;
    for (int i = 0; i < a.n2; i++) {
        const int np = a.npairs[i];
        if (np < 0 || np > a.cap) { orbx_set_error("%s: npairs[%d] = %d outside [0, cap = %d]", who, i, np, a.cap); return ORBX_E_INVALID; }
        t += (size_t)np;
        const int32_t *p = a.pairs + 2 * (size_t)i * (size_t)a.cap;
        for (int k = 0; k < np; k++) {
            const int i1 = p[2 * k], i2 = p[2 * k + 1];
            if (i1 < 0 || i1 >= h1.n || i2 < 0 || i2 >= h2[i].n) {
                orbx_set_error("%s: neighbour %d, pair %d: (%d, %d) outside the keyframes (%d, %d features)", who, i, k, i1, i2, h1.n, h2[i].n);
                return ORBX_E_INVALID;
            }
            if ((h1.octave && (h1.octave[i1] < 0 || h1.octave[i1] >= a.nlevels)) || (h2[i].octave && (h2[i].octave[i2] < 0 || h2[i].octave[i2] >= a.nlevels))) {
                orbx_set_error("%s: neighbour %d, pair %d: an octave outside [0, %d)", who, i, k, a.nlevels);
                return ORBX_E_INVALID;
            }
            if ((h1.u_right && !h1.has_depth && h1.u_right[i1] >= 0.f) || (h2[i].u_right && !h2[i].has_depth && h2[i].u_right[i2] >= 0.f)) {
                orbx_set_error("%s: neighbour %d, pair %d: a stereo feature of a keyframe without depth", who, i, k);
                return ORBX_E_INVALID;
            }
        }
    }
    if (t > ((size_t)1 << 22)) { orbx_set_error("%s: %zu pairs in all, more than 2^22", who, t); return ORBX_E_CAPACITY; }
    *total = t;
    return ORBX_OK;
}

// blob: [TriHead up to nb[n2]] [pairs, packed] [whatever stage() adds]; work / download: [status] [x3d] [bad flag] | [first[n1]]
// stage(H, cursor) fills the TriFeat records (and, for host pointers, the blob at the cursor)
template <class Stage>
static int tri_run(const char *who, CallCtx *c, const TriArgs &a, int n1, size_t total, size_t extra_blob, Stage stage,
                   const orbx_frame *const *wait, int nwait)
{
    *a.n_new = 0;
    if (total == 0) return ORBX_OK;
    const size_t head_b = a16(offsetof(TriHead, nb) + sizeof(TriHead::Nb) * (size_t)a.n2), pairs_b = a16(8 * total);
    const size_t blob = head_b + pairs_b + extra_blob;
    const size_t o_x3d = a16(total), o_bad = o_x3d + a16(12 * total), out = o_bad + 16, work = out + a16(4 * (size_t)n1);
    int rc = call_reserve(c, blob, work, out);
    if (rc) return rc;
    TriHead &H = *(TriHead *)c->h_blob;
    memset(&H, 0, head_b);
    H.n2 = a.n2; H.total = (int)total; H.nlevels = a.nlevels; H.ratio_factor = a.ratio_factor;
    memcpy(H.sf, a.sf, sizeof(float) * (size_t)a.nlevels); memcpy(H.sigma2, a.sigma2, sizeof(float) * (size_t)a.nlevels);
    H.v1 = *a.v1;
    int32_t *hp = (int32_t *)(c->h_blob + head_b);
    size_t at = 0;
    for (int i = 0; i < a.n2; i++) {
        H.prefix[i] = (int)at;
        H.nb[i].v = a.v2s[i];
        memcpy(hp + 2 * at, a.pairs + 2 * (size_t)i * (size_t)a.cap, 8 * (size_t)a.npairs[i]);
        at += (size_t)a.npairs[i];
    }
    H.prefix[a.n2] = (int)at;
    BlobCursor b = { c->h_blob, c->d_blob, head_b + pairs_b };
    stage(H, b);
    for (int i = 0; i < nwait; i++)
        if ((rc = frame_order_before(wait[i], c->stream))) return rc;
    if ((rc = call_upload(c, blob))) return rc;
    // 0x7f7f7f7f: larger than any neighbour index in first[], and not the 1 the kernel writes into the flag
    ORBX_HIP(hipMemsetAsync(c->d_work + o_bad, 0x7f, work - o_bad, c->stream));
    // k_triangulate, then first neighbour wins: d_work = status[total] | x3d[total][3] | bad flag | first[n1]
    const TriHead *d_head = (const TriHead *)c->d_blob;
    const int32_t *d_pairs = (const int32_t *)(c->d_blob + head_b);
    int *d_first = (int *)(c->d_work + out);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_triangulate, grid, block, 0, c->stream, d_head, d_pairs, c->d_work, (float *)(c->d_work + o_x3d), (int *)(c->d_work + o_bad));
    hipLaunchKernelGGL(k_tri_resolve<0>, grid, block, 0, c->stream, d_head, d_pairs, c->d_work, d_first);
    hipLaunchKernelGGL(k_tri_resolve<1>, grid, block, 0, c->stream, d_head, d_pairs, c->d_work, d_first);
    if ((rc = call_fetch(c, out))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    if (*(const int32_t *)(ho + o_bad) == 1) { orbx_set_error("%s: a paired feature has an octave outside [0, %d)", who, a.nlevels); return ORBX_E_INVALID; }
    const float *hx = (const float *)(ho + o_x3d);
    int n_new = 0;
    at = 0;
    for (int i = 0; i < a.n2; i++) {
        const size_t np = (size_t)a.npairs[i], row = (size_t)i * (size_t)a.cap;
        memcpy(a.status + row, ho + at, np);
        memcpy(a.x3d + 3 * row, hx + 3 * at, 12 * np);
        for (size_t k = 0; k < np; k++) n_new += ho[at + k] <= 2;
        at += np;
    }
    *a.n_new = n_new;
    return ORBX_OK;
}

extern "C" int orbx_triangulate_pairs(int device, const orbx_tri_feats *k1, const orbx_tri_view *v1, const orbx_tri_feats *const *k2s,
                                      const orbx_tri_view *v2s, int n2, const int32_t *pairs, int cap, const int *npairs,
                                      const float *scale_factors, const float *level_sigma2, int nlevels, float ratio_factor,
                                      uint8_t *status, float *x3d, int *n_new)
{
    const char *who = "orbx_triangulate_pairs";
    const TriArgs a = { n2, cap, nlevels, pairs, npairs, v1, v2s, scale_factors, level_sigma2, ratio_factor, status, x3d, n_new };
    size_t total;
    int rc = tri_check(who, k1, k2s, a, [&](TriHostKf *h) -> int {
        for (int i = 0; i <= n2; i++) {
            const orbx_tri_feats *k = i ? k2s[i - 1] : k1;
            if (!k || k->n < 0 || (k->n && (!k->x || !k->y || !k->octave || !k->u_right)) || (!k->raw_x) != (!k->raw_y)) {
                orbx_set_error("%s: a keyframe is NULL, has n < 0, lacks x / y / octave / u_right or gives one raw array only", who);
                return ORBX_E_INVALID;
            }
            h[i].n = k->n; h[i].octave = k->octave; h[i].u_right = k->u_right; h[i].has_depth = k->depth != nullptr;
        }
        return ORBX_OK;
    }, &total);
    if (rc) return rc;
    CallCtx *c;
    if ((rc = orbx_call_ctx(device, &c))) return rc;
    auto kf_bytes = [](const orbx_tri_feats *k) { return (size_t)(4 + (k->depth ? 1 : 0) + (k->raw_x ? 2 : 0)) * a16(4 * (size_t)k->n); };
    size_t extra = kf_bytes(k1);
    for (int i = 0; i < n2; i++) extra += kf_bytes(k2s[i]);
    return tri_run(who, c, a, k1->n, total, extra, [&](TriHead &H, BlobCursor &b) {
        auto put_kf = [&](const orbx_tri_feats *k, TriFeat &f) {
            const size_t nb = 4 * (size_t)k->n;
            f.x = (const float *)b.put(k->x, nb); f.y = (const float *)b.put(k->y, nb);
            f.octave = (const int32_t *)b.put(k->octave, nb); f.u_right = (const float *)b.put(k->u_right, nb);
            f.depth = k->depth ? (const float *)b.put(k->depth, nb) : nullptr;
            f.raw_x = k->raw_x ? (const float *)b.put(k->raw_x, nb) : f.x; f.raw_y = k->raw_y ? (const float *)b.put(k->raw_y, nb) : f.y;
        };
        put_kf(k1, H.f1);
        for (int i = 0; i < n2; i++) put_kf(k2s[i], H.nb[i].f);
    }, nullptr, 0);
}

extern "C" int orbx_frame_triangulate(const orbx_frame *k1, const orbx_tri_view *v1, const orbx_frame *const *k2s, const orbx_tri_view *v2s,
                                      int n2, const int32_t *pairs, int cap, const int *npairs, const float *scale_factors,
                                      const float *level_sigma2, int nlevels, float ratio_factor, uint8_t *status, float *x3d, int *n_new)
{
    const char *who = "orbx_frame_triangulate";
    const orbx_frame *fr[65];
    const TriArgs a = { n2, cap, nlevels, pairs, npairs, v1, v2s, scale_factors, level_sigma2, ratio_factor, status, x3d, n_new };
    size_t total;
    int rc = tri_check(who, k1, k2s, a, [&](TriHostKf *h) -> int {
        for (int i = 0; i <= n2; i++) {
            const orbx_frame *f = fr[i] = i ? k2s[i - 1] : k1;
            if (!f) { orbx_set_error("%s: a NULL frame", who); return ORBX_E_INVALID; }
            if (f->device != k1->device) { orbx_set_error("%s: the frames live on different devices", who); return ORBX_E_INVALID; }
            if ((f->has_stereo || f->from_extraction) && !f->depth_set) {
                orbx_set_error("%s: frame %d has stereo features or comes from an extraction, and no depth (orbx_frame_set_depth)", who, i);
                return ORBX_E_INVALID;
            }
            h[i].n = f->n; h[i].octave = f->h_oct.empty() ? nullptr : f->h_oct.data(); h[i].u_right = nullptr; h[i].has_depth = f->depth_set;
        }
        return ORBX_OK;
    }, &total);
    if (rc) return rc;
    CallCtx *c;
    if ((rc = orbx_call_ctx(k1->device, &c))) return rc;
    return tri_run(who, c, a, k1->n, total, 0, [&](TriHead &H, BlobCursor &) {
        for (int i = 0; i <= n2; i++) {
            const orbx_frame *f = fr[i];
            const DevFrame F = frame_dev(f);
            TriFeat &t = i ? H.nb[i - 1].f : H.f1;
            t.x = F.x; t.y = F.y; t.octave = F.octave; t.u_right = F.u_right;
            t.depth = f->d_depth;
            t.raw_x = f->d_raw_x ? f->d_raw_x : F.x; t.raw_y = f->d_raw_y ? f->d_raw_y : F.y;
        }
    }, fr, n2 + 1);
}

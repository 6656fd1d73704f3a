// tools/tri_baseline.cc -- the match loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:271-511) restated in plain
// C++ WITHOUT cv::Mat: the arithmetic of include/orbx.h (orbx_triangulate_pairs) on a host core, neighbour by neighbour, with the flag
// of a feature that got a point updated between two neighbours as the reference's loop does.  tools/bench_triangulate.py compiles it
// (g++ -O2 -ffp-contract=off -shared) and times it beside the device calls: a LOWER BOUND on what the reference's loop body costs, whose
// cv::Mat temporaries, cv::SVD and allocations are all absent here.  It is not the reference and says nothing about OpenCV's speed.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include <orbx.h>

namespace {

struct V3 { float x, y, z; };

inline double dotd(float a0, float a1, float a2, float b0, float b1, float b2) { return ((double)a0 * b0 + (double)a1 * b1) + (double)a2 * b2; }

inline V3 rot_wc(const float *T, float v0, float v1, float v2, double a0, double a1, double a2)
{
    V3 r;
    r.x = (float)(dotd(T[0], T[4], T[8], v0, v1, v2) + a0);
    r.y = (float)(dotd(T[1], T[5], T[9], v0, v1, v2) + a1);
    r.z = (float)(dotd(T[2], T[6], T[10], v0, v1, v2) + a2);
    return r;
}

inline float cam_row(const float *T, int r, const V3 &X) { return (float)(dotd(T[4 * r], T[4 * r + 1], T[4 * r + 2], X.x, X.y, X.z) + (double)T[4 * r + 3]); }

inline float stereo_cos(float mb, float depth)
{
    const double h = (double)(mb / 2.0f), d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

inline float norm3(float x, float y, float z) { return (float)sqrt(((double)x * x + (double)y * y) + (double)z * z); }

void null_vector(float At[4][4], float v[4])
{
    float V[4][4];
    double W[4];
    for (int i = 0; i < 4; i++) {
        double sd = 0.0;
        for (int k = 0; k < 4; k++) { sd += (double)At[i][k] * At[i][k]; V[i][k] = i == k ? 1.0f : 0.0f; }
        W[i] = sd;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; j < 4; j++) {
                double a = W[i], b = W[j], p = 0.0;
                for (int k = 0; k < 4; k++) p += (double)At[i][k] * At[j][k];
                if (fabs(p) <= (double)(2.0f * 1.1920928955078125e-7f) * sqrt(a * b)) continue;
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
                a = b = 0.0;
                for (int k = 0; k < 4; k++) {
                    const float t0 = c * At[i][k] + s * At[j][k], t1 = (-s) * At[i][k] + c * At[j][k];
                    At[i][k] = t0; At[j][k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                for (int k = 0; k < 4; k++) {
                    const float t0 = c * V[i][k] + s * V[j][k], t1 = (-s) * V[i][k] + c * V[j][k];
                    V[i][k] = t0; V[j][k] = t1;
                }
                changed = true;
            }
        if (!changed) break;
    }
    double best = 0.0;
    for (int i = 0; i < 4; i++) {
        double sd = 0.0;
        for (int k = 0; k < 4; k++) sd += (double)At[i][k] * At[i][k];
        if (i == 0 || sd <= best) { best = sd; memcpy(v, V[i], sizeof V[i]); }
    }
}

inline bool reproj_ok(const orbx_tri_view &v, const V3 &X, float z, float kx, float ky, float ur, bool stereo, float sigma2, float mbf)
{
    const float x = cam_row(v.Tcw, 0, X), y = cam_row(v.Tcw, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = v.fx * x * invz + v.cx, w = v.fy * y * invz + v.cy;
    const float ex = u - kx, ey = w - ky;
    if (!stereo) return !((double)(ex * ex + ey * ey) > 5.991 * (double)sigma2);
    const float er = (u - mbf * invz) - ur;
    return !((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2);
}

int one_pair(const orbx_tri_feats &f1, const orbx_tri_view &v1, int i1, const orbx_tri_feats &f2, const orbx_tri_view &v2, int i2, const float *sf,
             const float *sigma2, float ratio_factor, V3 &X, bool &have_x)
{
    const float k1x = f1.x[i1], k1y = f1.y[i1], ur1 = f1.u_right[i1], k2x = f2.x[i2], k2y = f2.y[i2], ur2 = f2.u_right[i2];
    const int o1 = f1.octave[i1], o2 = f2.octave[i2];
    const bool st1 = ur1 >= 0.f, st2 = ur2 >= 0.f;
    have_x = false;
    const float xn1x = (k1x - v1.cx) * v1.invfx, xn1y = (k1y - v1.cy) * v1.invfy, xn2x = (k2x - v2.cx) * v2.invfx, xn2y = (k2y - v2.cy) * v2.invfy;
    const V3 r1 = rot_wc(v1.Tcw, xn1x, xn1y, 1.0f, 0, 0, 0), r2 = rot_wc(v2.Tcw, xn2x, xn2y, 1.0f, 0, 0, 0);
    const float cos_rays = (float)(dotd(r1.x, r1.y, r1.z, r2.x, r2.y, r2.z) /
                                   (sqrt(dotd(r1.x, r1.y, r1.z, r1.x, r1.y, r1.z)) * sqrt(dotd(r2.x, r2.y, r2.z, r2.x, r2.y, r2.z))));
    float cs1 = cos_rays + 1.0f, cs2 = cs1;
    if (st1) cs1 = stereo_cos(v1.mb, f1.depth[i1]);
    else if (st2) cs2 = stereo_cos(v2.mb, f2.depth[i2]);
    const float cos_stereo = cs2 < cs1 ? cs2 : cs1;
    int created;
    if (cos_rays < cos_stereo && cos_rays > 0.f && (st1 || st2 || (double)cos_rays < 0.9998)) {
        float At[4][4], v[4];
        for (int c = 0; c < 4; c++) {
            At[c][0] = xn1x * v1.Tcw[8 + c] - v1.Tcw[c]; At[c][1] = xn1y * v1.Tcw[8 + c] - v1.Tcw[4 + c];
            At[c][2] = xn2x * v2.Tcw[8 + c] - v2.Tcw[c]; At[c][3] = xn2y * v2.Tcw[8 + c] - v2.Tcw[4 + c];
        }
        null_vector(At, v);
        if (v[3] == 0.f) return 17;
        X.x = v[0] / v[3]; X.y = v[1] / v[3]; X.z = v[2] / v[3];
        created = 0;
    } else if ((st1 && cs1 < cs2) || (st2 && cs2 < cs1)) {
        const bool one = st1 && cs1 < cs2;
        const orbx_tri_feats &f = one ? f1 : f2;
        const orbx_tri_view &v = one ? v1 : v2;
        const int i = one ? i1 : i2;
        const float z = f.depth[i];
        if (!(z > 0.f)) return 24;
        const float x = ((f.raw_x ? f.raw_x : f.x)[i] - v.cx) * z * v.invfx, y = ((f.raw_y ? f.raw_y : f.y)[i] - v.cy) * z * v.invfy;
        X = rot_wc(v.Tcw, x, y, z, (double)v.Ow[0], (double)v.Ow[1], (double)v.Ow[2]);
        created = one ? 1 : 2;
    } else return 16;
    have_x = true;
    const float z1 = cam_row(v1.Tcw, 2, X);
    if (z1 <= 0.f) return 18;
    const float z2 = cam_row(v2.Tcw, 2, X);
    if (z2 <= 0.f) return 19;
    if (!reproj_ok(v1, X, z1, k1x, k1y, ur1, st1, sigma2[o1], v1.mbf)) return 20;
    if (!reproj_ok(v2, X, z2, k2x, k2y, ur2, st2, sigma2[o2], v1.mbf)) return 21;
    const float d1 = norm3(X.x - v1.Ow[0], X.y - v1.Ow[1], X.z - v1.Ow[2]), d2 = norm3(X.x - v2.Ow[0], X.y - v2.Ow[1], X.z - v2.Ow[2]);
    if (d1 == 0.f || d2 == 0.f) return 22;
    const float ratio_dist = d2 / d1, ratio_oct = sf[o1] / sf[o2];
    if (ratio_dist * ratio_factor < ratio_oct || ratio_dist > ratio_oct * ratio_factor) return 23;
    return created;
}

}   // namespace

// the arguments of orbx_triangulate_pairs without the device; a pair whose feature got a point at an earlier neighbour is skipped as the
// reference's next search would have skipped it (its status stays 255, its x3d untouched)
extern "C" int tri_loop(const orbx_tri_feats *k1, const orbx_tri_view *v1, const orbx_tri_feats *const *k2s, const orbx_tri_view *v2s, int n2,
                        const int32_t *pairs, int cap, const int *npairs, const float *sf, const float *sigma2, float ratio_factor, uint8_t *status,
                        float *x3d)
{
    std::vector<uint8_t> has_point((size_t)k1->n, 0), created_here;
    int n_new = 0;
    for (int i = 0; i < n2; i++) {
        created_here.assign((size_t)k1->n, 0);
        for (int k = 0; k < npairs[i]; k++) {
            const size_t at = (size_t)i * cap + k;
            const int i1 = pairs[2 * at], i2 = pairs[2 * at + 1];
            status[at] = 255;
            if (has_point[i1]) continue;
            V3 X = { 0.f, 0.f, 0.f };
            bool have_x;
            const int st = one_pair(*k1, *v1, i1, *k2s[i], v2s[i], i2, sf, sigma2, ratio_factor, X, have_x);
            status[at] = (uint8_t)st;
            x3d[3 * at] = have_x ? X.x : 0.f; x3d[3 * at + 1] = have_x ? X.y : 0.f; x3d[3 * at + 2] = have_x ? X.z : 0.f;
            if (st <= 2) { created_here[i1] = 1; n_new++; }
        }
        for (int j = 0; j < k1->n; j++) has_point[j] |= created_here[j];
    }
    return n_new;
}

// orbx_frame.hip — Frame::UndistortKeyPoints (reference src/Frame.cc:470-515; SURVEY.md 8f row f2, "plus" part).
// cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) on the N keypoint positions: per point, in double,
//   x = (u - cx)/fx, y = (v - cy)/fy (as multiplications by ifx = 1./fx, ify = 1./fy), five fixed-point iterations of
//   the inverse Brown-Conrady model (k1 k2 p1 p2 k3), then back through P = mK, result rounded to float
// [OpenCV 3.2 cvUndistortPoints restated from memory -- parity unpinned; 2.4.11's loop is the same arithmetic for the
// 4/5-coefficient models ORB-SLAM2's settings files carry: the rational, thin-prism and tilt terms are exact no-ops at
// zero].  Points are independent: one thread each, fp64 VALU (-ffp-contract=off keeps the oracle's rounding).
#include "orbx_device.h"
#include <string.h>
#include <vector>

__global__ __launch_bounds__(256) void k_undistort(const float2 *__restrict__ in, float2 *__restrict__ out, int n, UndistortParams p)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = dev_undistort(in[i], p);   // orbx_device.h: the same arithmetic the resident-frame ingest runs (orbx_resident.hip)
}

struct FrameCtx : ThreadCtx {
    float2 *d_in = nullptr; size_t in_cap = 0;
    float2 *d_out = nullptr; size_t out_cap = 0;
    float2 *h = nullptr; size_t h_cap = 0;
    void release()
    {
        if (orbx_ctx_leave(this)) {
            if (d_in) (void)hipFree(d_in);
            if (d_out) (void)hipFree(d_out);
            if (h) (void)hipHostFree(h);
        }
        d_in = d_out = h = nullptr;
        in_cap = out_cap = h_cap = 0;
    }
    ~FrameCtx() { release(); }
};
static thread_local FrameCtx g_frame[ORBX_MAX_DEVICES];
void orbx_frame_thread_release() { for (FrameCtx &c : g_frame) c.release(); }

extern "C" int orbx_undistort_keypoints(int device, const float *xy, int n, float fx, float fy, float cx, float cy,
                                        const float *dist_coef, int ndist, float *xy_out)
{
    if (n < 0 || (n && (!xy || !xy_out)) || !dist_coef || (ndist != 4 && ndist != 5) || fx == 0.f || fy == 0.f) {
        orbx_set_error("orbx_undistort_keypoints: invalid argument (4 or 5 distortion coefficients)");
        return ORBX_E_INVALID;
    }
    if (n == 0) return ORBX_OK;
    if (dist_coef[0] == 0.0f) { // src/Frame.cc:472-476: mvKeysUn = mvKeys
        if (xy_out != xy) memcpy(xy_out, xy, sizeof(float) * 2 * (size_t)n);
        return ORBX_OK;
    }
    FrameCtx *c;
    int rc = orbx_ctx_get(g_frame, device, &c);
    const size_t bytes = sizeof(float2) * (size_t)n;
    if (!rc && bytes > c->in_cap) rc = ensure(&c->d_in, &c->in_cap, 2 * bytes);
    if (!rc && bytes > c->out_cap) rc = ensure(&c->d_out, &c->out_cap, 2 * bytes);
    if (!rc && bytes > c->h_cap) rc = ensure_pinned(&c->h, &c->h_cap, 2 * bytes);
    if (rc) return rc;
    const UndistortParams p = orbx_undistort_params(fx, fy, cx, cy, dist_coef, ndist);
    memcpy(c->h, xy, bytes);
    ORBX_HIP(hipMemcpyAsync(c->d_in, c->h, bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_in, c->d_out, n, p);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(c->h, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    ORBX_HIP(hipStreamSynchronize(c->stream));
    memcpy(xy_out, c->h, bytes);
    return ORBX_OK;
}

// ---- Frame::ComputeStereoFromRGBD (src/Frame.cc:754-774) with UndistortKeyPoints (:152) and Tracking::GrabImageRGBD's depth conversion
// (src/Tracking.cc:232-233) folded in.  One thread per keypoint, a (ceil(cap/256), batch) grid; the count is read on the device, so a launch
// needs no host synchronisation.  A latency-bound gather: one 28-byte record read, the fp64 undistortion of k_undistort (dev_undistort, same
// bits), one 2- or 4-byte depth read, three stores.  -ffp-contract=off and the default correctly rounded fp32 division keep the reference's
// rounding: d = raw * scale is one fp32 multiply, u_right = kpU.x - bf / d one division and one subtraction.
__global__ __launch_bounds__(256) void k_rgbd_depth(const RgbdArgs a)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.cap || i >= a.n[b]) return;
    const long long k = (long long)b * a.cap + i;
    const orbx_keypoint *kp = a.kps + k;
    const float2 pos = make_float2(kp->x, kp->y);
    const float2 un = a.undistort ? dev_undistort(pos, a.up) : pos;
    if (a.xy_un) a.xy_un[k] = un;
    float ur = -1.f, z = -1.f;
    // imDepth.at<float>(v, u) with u = (int)kp.x, v = (int)kp.y (truncation).  A position whose truncation falls outside the image (NaN
    // included) reads nothing and gets -1 / -1: the defined deviation for caller-supplied keypoints (the reference reads out of bounds)
    if (pos.x > -1.f && pos.x < (float)a.w && pos.y > -1.f && pos.y < (float)a.h) {
        const int u = (int)pos.x, v = (int)pos.y;
        const uint8_t *row = a.depth + (long long)b * a.depth_img_stride + (long long)v * a.depth_pitch;
        float d;
        if (a.depth_type == ORBX_DEPTH_U16) d = (float)reinterpret_cast<const uint16_t *>(row)[u] * a.scale;   // convertTo(CV_32F, scale): always
        else {
            d = reinterpret_cast<const float *>(row)[u];
            if (a.apply_scale) d = d * a.scale;       // only when fabs(mDepthMapFactor - 1.0f) > 1e-5 (src/Tracking.cc:232)
        }
        if (d > 0) { z = d; ur = un.x - a.bf / d; }
    }
    a.u_right[k] = ur;
    a.z[k] = z;
}

int orbx_rgbd_args(const char *fn, const orbx_rgbd_params *p, int w, int h, size_t depth_pitch, RgbdArgs *a)
{
    if (!p || (p->depth_type != ORBX_DEPTH_U16 && p->depth_type != ORBX_DEPTH_F32) || (p->ndist != 4 && p->ndist != 5) || w < 1 || h < 1) {
        orbx_set_error("%s: invalid argument (params, depth_type, ndist 4 or 5, image size)", fn);
        return ORBX_E_INVALID;
    }
    const size_t es = p->depth_type == ORBX_DEPTH_U16 ? 2 : 4;
    if (depth_pitch < (size_t)w * es || depth_pitch % es) {
        orbx_set_error("%s: depth row stride %zu is below a row (%zu bytes) or not a multiple of the element size", fn, depth_pitch, (size_t)w * es);
        return ORBX_E_INVALID;
    }
    memset(a, 0, sizeof(*a));
    a->undistort = p->dist_coef[0] != 0.0f;
    if (a->undistort) {
        if (p->fx == 0.f || p->fy == 0.f) { orbx_set_error("%s: fx / fy is 0", fn); return ORBX_E_INVALID; }
        a->up = orbx_undistort_params(p->fx, p->fy, p->cx, p->cy, p->dist_coef, p->ndist);
    }
    a->depth_type = p->depth_type;
    a->scale = p->depth_scale;
    // src/Tracking.cc:232: (fabs(mDepthMapFactor - 1.0f) > 1e-5) || imDepth.type() != CV_32F -- the difference in float, the compare in double
    a->apply_scale = p->depth_type == ORBX_DEPTH_U16 || (double)fabsf(p->depth_scale - 1.0f) > 1e-5;
    a->bf = p->bf;
    a->w = w; a->h = h; a->depth_pitch = (long long)depth_pitch;
    return ORBX_OK;
}

int orbx_rgbd_launch(const RgbdArgs &a, int batch, hipStream_t s)
{
    hipLaunchKernelGGL(k_rgbd_depth, dim3((unsigned)((a.cap + 255) / 256), (unsigned)batch), dim3(256), 0, s, a);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbx_rgbd_depth_batch_device(int device, const void *d_kps, const void *d_n, int cap, int batch,
                                            const void *d_depth, size_t depth_img_stride, size_t depth_pitch, int w, int h,
                                            const orbx_rgbd_params *p, void *d_xy_un, void *d_u_right, void *d_depth_out, void *stream)
{
    if (!d_kps || !d_n || !d_depth || !d_u_right || !d_depth_out || cap < 1 || batch < 1 || batch > 65535 ||
        (batch > 1 && depth_img_stride < depth_pitch * (size_t)h)) {
        orbx_set_error("orbx_rgbd_depth_batch_device: invalid argument");
        return ORBX_E_INVALID;
    }
    RgbdArgs a;
    int rc = orbx_rgbd_args("orbx_rgbd_depth_batch_device", p, w, h, depth_pitch, &a);
    if (rc) return rc;
    if ((rc = orbx_check_device(device))) return rc;
    ORBX_HIP(orbx_use_device(device));
    a.depth = (const uint8_t *)d_depth; a.depth_img_stride = (long long)depth_img_stride;
    a.kps = (const orbx_keypoint *)d_kps; a.n = (const int *)d_n; a.cap = cap;
    a.xy_un = (float2 *)d_xy_un; a.u_right = (float *)d_u_right; a.z = (float *)d_depth_out;
    return orbx_rgbd_launch(a, batch, (hipStream_t)stream);
}

// orbx_hostapi.hip — the host-pointer entry points of the extractor: frames that arrive in host memory are staged through pinned
// buffers, uploaded, extracted (orbx_extract.hip through orbx_extract_batch_device; orbx_stereo.hip, orbx_remap.hip and orbx_frame.hip through
// their device entry points) and their results brought back, either in one call behind one synchronisation (orbx_extract, orbx_extract_batch,
// orbx_extract_color, orbx_extract_rectified, orbx_extract_stereo, orbx_extract_rgbd) or pipelined (the _submit / _wait forms).
// Host code, but for the two transport kernels k_gray and k_copy_bytes.
#include "orbx_device.h"
#include <atomic>
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int orbx_ensure_out_staging(orbx_extractor *e, int batch, int cap)
{
    if (e->d_out_kps && e->out_cap >= cap && e->out_batch >= batch) return ORBX_OK;
    { const int qrc = orbx_quiesce(e); if (qrc) return qrc; }
    void **ps[] = { &e->d_out_kps, &e->d_out_desc, &e->d_out_n, (void **)&e->d_out_ur, (void **)&e->d_out_depth };
    for (void **p : ps) if (*p) { ORBX_HIP(hipFree(*p)); *p = nullptr; }
    const size_t n = (size_t)batch * cap;
    ORBX_HIP(hipMalloc(&e->d_out_kps, n * sizeof(orbx_keypoint)));
    ORBX_HIP(hipMalloc(&e->d_out_desc, n * 32));
    ORBX_HIP(hipMalloc(&e->d_out_n, sizeof(int) * batch));
    ORBX_HIP(hipMalloc((void **)&e->d_out_ur, n * 4));
    ORBX_HIP(hipMalloc((void **)&e->d_out_depth, n * 4));
    e->out_cap = cap; e->out_batch = batch;
    return ORBX_OK;
}

// What the synchronous host-pointer forms share.  begin: device, geometry, capacity check, level-0 and output staging on the device, the
// layout of the pinned result block.  stage: rows repitched into the pinned input staging (a pageable 2-D copy is executed row by row by
// the runtime); the caller uploads them to where its form wants them.  extract: the extraction of the staged level 0.  finish: the whole
// capacity back in a copy per array, ONE synchronisation, the first n entries of each array out to the caller.
namespace {
struct HostCall {
    orbx_extractor *e;
    int images, need;                   // images of this call; keypoint capacity per image of the geometry
    size_t pitch, img_bytes;            // level 0 in d_stage_in
    ResultLayout out;                   // of the pinned h_out

    int begin(orbx_extractor *e_, int w, int h, int cap, int images_)
    {
        e = e_; images = images_;
        ORBX_HIP(orbx_use_device(e->device));
        int rc = orbx_prepare_geometry(e, w, h);
        if (rc) return rc;
        need = e->geom.kp_total;
        if (cap < need) { orbx_set_error("keypoint capacity %d < orbx_max_keypoints() = %d", cap, need); return ORBX_E_CAPACITY; }
        pitch = align_up(w, 64); img_bytes = pitch * h;
        if ((rc = ensure(&e->d_stage_in, &e->stage_in_cap, img_bytes * e->max_batch))) return rc;
        if ((rc = orbx_ensure_out_staging(e, e->max_batch, need))) return rc;
        out = orbx_result_layout(images, need);
        return ensure_pinned(&e->h_out, &e->h_out_cap, out.bytes);
    }

    // `rows` rows of row_bytes from src (rows `stride` apart) to h_stage_in + offset, rows dpitch apart.  Everything of a call is staged
    // before its first upload: growing the buffer keeps what the call has staged below `offset`, but not a copy in flight
    int stage(const void *src, size_t stride, size_t row_bytes, int rows, size_t dpitch, size_t offset)
    {
        if (offset + dpitch * rows > e->h_stage_in_cap || !e->h_stage_in) {
            uint8_t *grown = nullptr; size_t cap = 0;
            const int rc = ensure_pinned(&grown, &cap, offset + dpitch * rows);
            if (rc) return rc;
            if (e->h_stage_in) { memcpy(grown, e->h_stage_in, offset < e->h_stage_in_cap ? offset : e->h_stage_in_cap); ORBX_HIP(hipHostFree(e->h_stage_in)); }
            e->h_stage_in = grown; e->h_stage_in_cap = cap;
        }
        uint8_t *dst = e->h_stage_in + offset;
        for (int y = 0; y < rows; y++) memcpy(dst + (size_t)y * dpitch, (const uint8_t *)src + (size_t)y * stride, row_bytes);
        return ORBX_OK;
    }

    int extract(int w, int h)
    {
        e->prof_chain = false; // the uploads (and k_gray / the remap) are not part of the first launch
        return orbx_extract_batch_device(e, e->d_stage_in, img_bytes, pitch, images, w, h, e->d_out_kps, e->d_out_desc, need, e->d_out_n, nullptr);
    }

    int finish(orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out, float *u_right = nullptr, float *depth = nullptr,
               float *xy_un = nullptr, const void *d_xy = nullptr)
    {
        uint8_t *ho = e->h_out;
        const size_t n = (size_t)need;
        ORBX_HIP(hipMemcpyAsync(ho, e->d_out_n, sizeof(int) * images, hipMemcpyDeviceToHost, e->stream));
        ORBX_HIP(hipMemcpyAsync(ho + out.kps, e->d_out_kps, sizeof(orbx_keypoint) * n * images, hipMemcpyDeviceToHost, e->stream));
        ORBX_HIP(hipMemcpyAsync(ho + out.desc, e->d_out_desc, 32 * n * images, hipMemcpyDeviceToHost, e->stream));
        if (u_right) ORBX_HIP(hipMemcpyAsync(ho + out.ur, e->d_out_ur, 4 * n, hipMemcpyDeviceToHost, e->stream));
        if (depth) ORBX_HIP(hipMemcpyAsync(ho + out.z, e->d_out_depth, 4 * n, hipMemcpyDeviceToHost, e->stream));
        if (xy_un) ORBX_HIP(hipMemcpyAsync(ho + out.xy, d_xy, 8 * n, hipMemcpyDeviceToHost, e->stream));
        const int rc = orbx_sync(e, nullptr);
        if (rc) return rc;
        const int *hn = reinterpret_cast<const int *>(ho);
        for (int i = 0; i < images; i++) {
            n_out[i] = hn[i];
            memcpy(kps + (size_t)i * cap, ho + out.kps + sizeof(orbx_keypoint) * n * i, sizeof(orbx_keypoint) * (size_t)hn[i]);
            memcpy(desc + (size_t)i * cap * 32, ho + out.desc + 32 * n * i, (size_t)32 * hn[i]);
        }
        if (u_right) memcpy(u_right, ho + out.ur, 4 * (size_t)hn[0]);
        if (depth) memcpy(depth, ho + out.z, 4 * (size_t)hn[0]);
        if (xy_un) memcpy(xy_un, ho + out.xy, 8 * (size_t)hn[0]);
        return ORBX_OK;
    }
};
}

extern "C" int orbx_extract_batch(orbx_extractor *e, const uint8_t *const *imgs, int batch, int w, int h, size_t stride,
                                  orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out)
{
    if (!e || !imgs || !kps || !desc || !n_out || batch < 1 || batch > e->max_batch || w < 0 || h < 0) {
        orbx_set_error("orbx_extract_batch: invalid argument");
        return ORBX_E_INVALID;
    }
    if (w == 0 || h == 0) { for (int i = 0; i < batch; i++) n_out[i] = 0; return ORBX_OK; } // reference :1264
    if (stride < (size_t)w) { orbx_set_error("stride < width"); return ORBX_E_INVALID; }
    HostCall hc;
    int rc = hc.begin(e, w, h, cap, batch);
    if (rc) return rc;
    for (int i = 0; i < batch; i++) {
        if (!imgs[i]) { orbx_set_error("imgs[%d] is NULL", i); return ORBX_E_INVALID; }
        if ((rc = hc.stage(imgs[i], stride, (size_t)w, h, hc.pitch, hc.img_bytes * i))) return rc;
    }
    ORBX_HIP(hipMemcpyAsync(e->d_stage_in, e->h_stage_in, hc.img_bytes * batch, hipMemcpyHostToDevice, e->stream));
    if ((rc = hc.extract(w, h))) return rc;
    return hc.finish(kps, desc, cap, n_out);
}

extern "C" int orbx_extract(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride,
                            orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out)
{
    const uint8_t *imgs[1] = { img };
    if (!img && w > 0 && h > 0) { orbx_set_error("img is NULL"); return ORBX_E_INVALID; }
    return orbx_extract_batch(e, imgs, 1, w, h, stride, kps, desc, cap, n_out);
}

// cv::cvtColor colour -> grey for 8U (call sites src/Tracking.cc:177-202): fixed point, yuv_shift 14
__global__ __launch_bounds__(256) void k_gray(const uint8_t *__restrict__ src, int w, int h, int spitch, int channels, int rgb_order,
                                              uint8_t *__restrict__ dst, int dpitch)
{
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h || x4 >= dpitch) return;
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int x = x4 + i;
        if (x < w) {
            const uint8_t *p = src + (long long)y * spitch + (long long)x * channels;
            const int r = rgb_order ? p[0] : p[2], g = p[1], bl = rgb_order ? p[2] : p[0];
            out |= (uint32_t)((r * 4899 + g * 9617 + bl * 1868 + (1 << 13)) >> 14) << (8 * i);
        }
    }
    *reinterpret_cast<uint32_t *>(dst + (long long)y * dpitch + x4) = out;
}


extern "C" int orbx_extract_color(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride, int channels, int rgb_order,
                                  orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out, uint8_t *gray_out, size_t gray_stride)
{
    if (!e || !kps || !desc || !n_out || w < 0 || h < 0 || (channels != 3 && channels != 4) || (gray_out && gray_stride < (size_t)w)) {
        orbx_set_error("orbx_extract_color: invalid argument");
        return ORBX_E_INVALID;
    }
    if (w == 0 || h == 0) { *n_out = 0; return ORBX_OK; }
    if (!img || stride < (size_t)w * channels) { orbx_set_error("orbx_extract_color: bad image / stride"); return ORBX_E_INVALID; }
    HostCall hc;
    int rc = hc.begin(e, w, h, cap, 1);
    if (rc) return rc;
    const size_t pitch = hc.pitch, cpitch = align_up((size_t)w * channels, 64), cbytes = cpitch * h;
    void *d_color;
    if ((rc = orbx_scratch(e, 6, cbytes, &d_color))) return rc;
    if ((rc = hc.stage(img, stride, (size_t)w * channels, h, cpitch, 0))) return rc;
    ORBX_HIP(hipMemcpyAsync(d_color, e->h_stage_in, cbytes, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_gray, dim3((unsigned)((pitch / 4 + 63) / 64), (h + 3) / 4), dim3(256), 0, e->stream, (const uint8_t *)d_color, w, h, (int)cpitch,
                       channels, rgb_order, e->d_stage_in, (int)pitch);
    if ((rc = hc.extract(w, h)) || (rc = hc.finish(kps, desc, cap, n_out))) return rc;
    if (gray_out) ORBX_HIP(hipMemcpy2D(gray_out, gray_stride, e->d_stage_in, pitch, w, h, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

// EuRoC stereo front end (Examples/Stereo/stereo_euroc.cc:136-137 then Tracking::GrabImageStereo): the raw grey frame is
// uploaded, rectified on device (orbx_remap.hip) straight into the level-0 staging, and extracted.
extern "C" int orbx_extract_rectified(orbx_extractor *e, const orbx_rectifier *r, const uint8_t *img, int w, int h, size_t stride,
                                      orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out, uint8_t *rect_out, size_t rect_stride)
{
    int rw = 0, rh = 0;
    if (!e || !r || !img || !kps || !desc || !n_out || w < 1 || h < 1 || stride < (size_t)w || orbx_rectifier_size(r, &rw, &rh) ||
        (rect_out && rect_stride < (size_t)rw)) {
        orbx_set_error("orbx_extract_rectified: invalid argument");
        return ORBX_E_INVALID;
    }
    HostCall hc;
    int rc = hc.begin(e, rw, rh, cap, 1);
    if (rc) return rc;
    const size_t spitch = align_up((size_t)w, 64), sbytes = spitch * h;
    void *d_raw;
    if ((rc = orbx_scratch(e, 6, sbytes, &d_raw))) return rc;
    if ((rc = hc.stage(img, stride, (size_t)w, h, spitch, 0))) return rc;
    ORBX_HIP(hipMemcpyAsync(d_raw, e->h_stage_in, sbytes, hipMemcpyHostToDevice, e->stream));
    if ((rc = orbx_remap_batch_device(r, d_raw, sbytes, spitch, 1, e->d_stage_in, hc.img_bytes, hc.pitch, e->stream))) return rc;
    if ((rc = hc.extract(rw, rh)) || (rc = hc.finish(kps, desc, cap, n_out))) return rc;
    if (rect_out) ORBX_HIP(hipMemcpy2D(rect_out, rect_stride, e->d_stage_in, hc.pitch, rw, rh, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

// One stereo frame through host pointers in one call: what Frame::Frame(imLeft, imRight, ...) does with two ExtractORB
// threads and ComputeStereoMatches (src/Frame.cc:82-97): both eyes in one H2D copy and one batch-of-2 extraction, the
// stereo matcher on the still device-resident keypoints, everything back in one group of copies behind ONE
// synchronisation (the separate calls cost three synchronisations and an extra round trip of both eyes' features).
extern "C" int orbx_extract_stereo(orbx_extractor *e, const uint8_t *img_left, const uint8_t *img_right, int w, int h, size_t stride,
                                   float bf, float min_z, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out,
                                   float *u_right, float *depth)
{
    if (!e || !img_left || !img_right || !kps || !desc || !n_out || !u_right || !depth || w < 1 || h < 1 || stride < (size_t)w ||
        !(min_z > 0)) {
        orbx_set_error("orbx_extract_stereo: invalid argument");
        return ORBX_E_INVALID;
    }
    if (e->max_batch < 2) { orbx_set_error("orbx_extract_stereo needs an extractor created with max_batch >= 2"); return ORBX_E_INVALID; }
    HostCall hc;
    int rc = hc.begin(e, w, h, cap, 2);
    if (rc) return rc;
    if ((rc = hc.stage(img_left, stride, (size_t)w, h, hc.pitch, 0)) || (rc = hc.stage(img_right, stride, (size_t)w, h, hc.pitch, hc.img_bytes))) return rc;
    ORBX_HIP(hipMemcpyAsync(e->d_stage_in, e->h_stage_in, hc.img_bytes * 2, hipMemcpyHostToDevice, e->stream));
    if ((rc = hc.extract(w, h))) return rc;
    const int need = hc.need;
    orbx_keypoint *dk = (orbx_keypoint *)e->d_out_kps;
    uint8_t *dd = (uint8_t *)e->d_out_desc;
    int *dn = (int *)e->d_out_n;
    // the right keypoints are what the launch above wrote into the handle's own buffer: its by-product row table serves when it built one
    rc = orbx_stereo_match_batch_device(e, 0, e, 1, 1, dk, dd, dn, dk + need, dd + (size_t)32 * need, dn + 1, need, bf, min_z,
                                        e->d_out_ur, e->d_out_depth,
                                        orbx_stereo_row_table_available(e, dk + need, 1, 1, need) ? ORBX_ROWTAB_OF_EXTRACTION : ORBX_ROWTAB_FROM_KEYPOINTS, nullptr);
    if (rc) return rc;
    return hc.finish(kps, desc, cap, n_out, u_right, depth);
}

// One RGB-D frame through host pointers in one call: Tracking::GrabImageRGBD's cvtColor and depth convertTo (src/Tracking.cc:217-233) and
// the RGB-D constructor's ExtractORB / UndistortKeyPoints / ComputeStereoFromRGBD (src/Frame.cc:145-154).  The depth is uploaded right
// behind the image, k_rgbd_depth runs on the still device-resident keypoints, and everything comes back behind ONE synchronisation.
extern "C" int orbx_extract_rgbd(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride, int channels, int rgb_order,
                                 const void *depth, size_t depth_stride, const orbx_rgbd_params *p,
                                 orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out, float *xy_un, float *u_right, float *depth_out)
{
    if (!e || !img || !depth || !kps || !desc || !n_out || !u_right || !depth_out || w < 1 || h < 1 ||
        (channels != 1 && channels != 3 && channels != 4) || stride < (size_t)w * channels) {
        orbx_set_error("orbx_extract_rgbd: invalid argument");
        return ORBX_E_INVALID;
    }
    RgbdArgs a;
    int rc = orbx_rgbd_args("orbx_extract_rgbd", p, w, h, depth_stride, &a);
    if (rc) return rc;
    HostCall hc;
    if ((rc = hc.begin(e, w, h, cap, 1))) return rc;
    const size_t pitch = hc.pitch, cpitch = align_up((size_t)w * channels, 64), cbytes = cpitch * h;            // channels 1: cbytes == img_bytes
    const size_t drow = (size_t)w * (p->depth_type == ORBX_DEPTH_U16 ? 2 : 4), dpitch = align_up(drow, 64), dbytes = dpitch * h;
    void *d_color = nullptr, *d_depth, *d_xy;
    if (channels > 1 && (rc = orbx_scratch(e, 6, cbytes, &d_color))) return rc;
    if ((rc = orbx_scratch(e, 8, dbytes, &d_depth)) || (rc = orbx_scratch(e, 9, 8 * (size_t)hc.need, &d_xy))) return rc;
    if ((rc = hc.stage(img, stride, (size_t)w * channels, h, cpitch, 0)) || (rc = hc.stage(depth, depth_stride, drow, h, dpitch, cbytes))) return rc;
    ORBX_HIP(hipMemcpyAsync(channels > 1 ? d_color : (void *)e->d_stage_in, e->h_stage_in, cbytes, hipMemcpyHostToDevice, e->stream));
    ORBX_HIP(hipMemcpyAsync(d_depth, e->h_stage_in + cbytes, dbytes, hipMemcpyHostToDevice, e->stream));
    if (channels > 1)
        hipLaunchKernelGGL(k_gray, dim3((unsigned)((pitch / 4 + 63) / 64), (h + 3) / 4), dim3(256), 0, e->stream, (const uint8_t *)d_color, w, h, (int)cpitch,
                           channels, rgb_order, e->d_stage_in, (int)pitch);
    if ((rc = hc.extract(w, h))) return rc;
    a.depth = (const uint8_t *)d_depth; a.depth_img_stride = (long long)dbytes; a.depth_pitch = (long long)dpitch;
    a.kps = (const orbx_keypoint *)e->d_out_kps; a.n = (const int *)e->d_out_n; a.cap = hc.need;
    a.xy_un = (float2 *)d_xy; a.u_right = e->d_out_ur; a.z = e->d_out_depth;
    if ((rc = orbx_rgbd_launch(a, 1, e->stream))) return rc;
    return hc.finish(kps, desc, cap, n_out, u_right, depth_out, xy_un, d_xy);
}

// ---- pipelined host-pointer stereo frames (a camera stream fed from host memory)

static_assert((ORBX_PIPE_DEPTH & (ORBX_PIPE_DEPTH - 1)) == 0, "tickets wrap at 2^31: the depth must divide it");

extern "C" int orbx_pipeline_depth(void) { return ORBX_PIPE_DEPTH; }

extern "C" void *orbx_pinned_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) { orbx_set_error("hipHostMalloc(%zu) failed", bytes); return nullptr; }
    return p;
}
extern "C" void orbx_pinned_free(void *p) { if (p) hipHostFree(p); }

// the address a kernel reads pinned (page-locked, mapped) host memory at, or nullptr for anything else
static const uint8_t *pinned_device_ptr(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return a.type == hipMemoryTypeHost ? (const uint8_t *)a.devicePointer : nullptr;
}

static int pipe_slot_prepare(orbx_extractor *e, PipeSlot &s, size_t in_bytes, int need)
{
    if (!s.ev_h2d) {
        ORBX_HIP(hipEventCreateWithFlags(&s.ev_h2d, hipEventDisableTiming));
        ORBX_HIP(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
        ORBX_HIP(hipEventCreateWithFlags(&s.ev_d2h, hipEventDisableTiming));
    }
    int rc;
    if (in_bytes > s.h_in_cap) {
        if ((rc = ensure_pinned(&s.h_in, &s.h_in_cap, in_bytes))) return rc;
        ORBX_HIP(hipHostGetDevicePointer((void **)&s.h_in_dev, s.h_in, 0));
    }
    if ((rc = ensure(&s.d_in, &s.d_in_cap, in_bytes))) return rc;
    const ResultLayout L = orbx_result_layout(2, need);
    if ((rc = ensure(&s.d_out, &s.d_out_cap, L.bytes))) return rc;
    if (L.bytes > s.h_out_cap) {
        if ((rc = ensure_pinned(&s.h_out, &s.h_out_cap, L.bytes))) return rc;
        ORBX_HIP(hipHostGetDevicePointer((void **)&s.h_out_dev, s.h_out, 0));
    }
    // the views follow `need` (the layout of this frame), not the capacity the block was allocated for
    s.d_n = s.d_out; s.d_kps = s.d_out + L.kps; s.d_desc = s.d_out + L.desc;
    s.d_ur = reinterpret_cast<float *>(s.d_out + L.ur); s.d_z = reinterpret_cast<float *>(s.d_out + L.z);
    return ORBX_OK;
}

// Frame transport of the pipelined forms by KERNEL: the caller's pinned images are read over PCIe by a copy kernel on the frame's own
// lane stream, and the result block is written to the slot's pinned buffer the same way.  The copy engines move a 466 KB image in
// ~25 us each (0.93 MB per stereo frame: a ceiling of ~15 k frames/s whatever the number of lanes) and need a stream hop with two
// events each way; a kernel with enough loads in flight moves the frame in ~20 us and is just one more launch of the chain.
__global__ __launch_bounds__(256) void k_copy_bytes(const uint8_t *__restrict__ src0, const uint8_t *__restrict__ src1, uint8_t *__restrict__ dst0,
                                                    uint8_t *__restrict__ dst1, unsigned long long bytes)
{
    const uint8_t *src = blockIdx.y ? src1 : src0;
    uint8_t *dst = blockIdx.y ? dst1 : dst0;
    const unsigned long long n16 = bytes >> 4, stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
        uint4 v;
        __builtin_memcpy(&v, src + 16 * i, 16);             // any byte alignment (global memory takes unaligned dwordx4)
        __builtin_memcpy(dst + 16 * i, &v, 16);
    }
    if (blockIdx.x == 0) for (unsigned long long i = (n16 << 4) + threadIdx.x; i < bytes; i += 256) dst[i] = src[i];
}

static std::atomic<int> g_pipe_handles{0};   // handles of this process that have submitted pipelined frames and still exist
void orbx_pipe_handle_released() { g_pipe_handles.fetch_sub(1, std::memory_order_relaxed); }

// one frame into the next pipeline slot: eyes = 2 (stereo: both extractions + ComputeStereoMatches) or 1 (mono: extraction only)
// ORBX_PIPE_PROF: host nanoseconds per section of pipe_submit / pipe_wait, summed over every client thread (relaxed atomics: diagnostic only)
static std::atomic<long long> g_pp[8]; static std::atomic<long> g_pp_n;
static inline double pp_now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static const bool g_pp_on = getenv("ORBX_PIPE_PROF") != nullptr;
struct PpScope {    // charges the time since construction / the last next() to section k
    int k; double t0;
    explicit PpScope(int k_) : k(k_), t0(g_pp_on ? pp_now() : 0) {}
    void next(int k_) { if (g_pp_on) { const double t = pp_now(); g_pp[k].fetch_add((long long)((t - t0) * 1e3), std::memory_order_relaxed); t0 = t; } k = k_; }
    ~PpScope() { if (g_pp_on) g_pp[k].fetch_add((long long)((pp_now() - t0) * 1e3), std::memory_order_relaxed); }
};
extern "C" void orbx_debug_pipe_prof_print()
{
    const long frames = g_pp_n.load();
    if (!g_pp_on || !frames) return;
    const char *nm[8] = { "setdevice+lane+geometry", "pinned test + slot", "upload enqueue", "extract launches", "stereo launch", "download enqueue + event", "wait: event sync", "wait: copy out" };
    for (int i = 0; i < 8; i++) fprintf(stderr, "pipe prof: %-28s %7.2f us per frame\n", nm[i], g_pp[i].load() * 1e-3 / frames);
}

// the RGB-D part of a pipelined frame (eyes == ORBX_PIPE_RGBD): img_left is the grey or colour image, `depth` its depth map
struct RgbdIn { const void *depth; size_t depth_stride; int channels, rgb_order; RgbdArgs a; };
// an RGB-D slot's input block: level 0 (grey) | the colour image (up to 4 channels) | the depth map (up to 4 bytes a pixel), each row-aligned;
// sized for the largest form whatever the frame, so that one warm-up frame per slot makes every later RGB-D frame of the size allocation-free
static size_t rgbd_in_bytes(int w, int h) { return (align_up(w, 64) + 2 * align_up((size_t)w * 4, 64)) * (size_t)h; }

static int pipe_submit(orbx_extractor *e, const uint8_t *img_left, const uint8_t *img_right, int eyes, int w, int h, size_t stride,
                       float bf, float min_z, int *ticket, const RgbdIn *rg = nullptr)
{
    if (g_pp_on) g_pp_n.fetch_add(1, std::memory_order_relaxed);
    PpScope pp(0);
#define PP_NEXT(K) pp.next(K)
    ORBX_HIP(orbx_use_device(e->device));
    // Kernel lanes: a single stereo frame is a chain of dependent launches (~70 us) that keeps a few percent of the chip busy, so
    // consecutive frames go round the handle and its shadow handles (own stream, own pyramid / candidate / quadtree workspaces,
    // created on first use) and their chains overlap.  Slots, tickets and the order of results are unchanged.
    // (With the copy-engine transport of round 2 lanes only paid for a lone handle -- four client threads: 11.3 k frames/s with one lane
    // each, 8.2 k with two --; with the kernel transport they pay for every handle: two camera streams 14.7 k -> 17.3 k, four 20 k either way.)
    if (!e->pipe_counted) { e->pipe_counted = true; g_pipe_handles.fetch_add(1, std::memory_order_relaxed); }
    orbx_extractor *x = e;
    const int nl = e->pipe_lanes, li = (int)(e->pipe_next % (unsigned)nl);
    if (li) {
        orbx_extractor *&sh = e->lanes[li - 1];
        if (!sh) {
            const int lrc = orbx_extractor_create(&sh, e->nfeatures, (float)e->scale_factor, e->nlevels, e->ini_th, e->min_th, e->device, e->max_w, e->max_h, 2);
            if (lrc) return lrc;
        }
        x = sh;
        if (x->cv_profile != e->cv_profile) orbx_extractor_set_cv_profile(x, e->cv_profile);
        x->pyr_group_max_images = e->pyr_group_max_images; x->pyr_group_mid_images = e->pyr_group_mid_images;
    }
    int rc = orbx_prepare_geometry(x, w, h);   // waits for everything in flight only when the image size changes
    if (rc) return rc;
    PP_NEXT(1);
    PipeSlot &s = e->pipe[e->pipe_next % ORBX_PIPE_DEPTH];
    if (s.busy) { orbx_set_error("all %d pipeline slots are in flight: wait for the oldest ticket first", ORBX_PIPE_DEPTH); return ORBX_E_INVALID; }
    const int need = x->geom.kp_total;
    const int nimg = eyes == 2 ? 2 : 1;                 // images extracted per frame
    const ResultLayout L = orbx_result_layout(2, need);
    if (rg && L.xy + 8 * (size_t)need > L.desc) {       // the xy rows of an RGB-D slot must fit the unused second-eye keypoint rows
        orbx_set_error("keypoint capacity %d too small for the RGB-D result block", need);
        return ORBX_E_INVALID;
    }
    const uint8_t *pin[2] = { stride == (size_t)w ? pinned_device_ptr(img_left) : nullptr, stride == (size_t)w && eyes == 2 ? pinned_device_ptr(img_right) : nullptr };
    const bool in_place = pin[0] && (eyes == 1 || pin[1]);
    size_t pitch = in_place ? (size_t)w : align_up(w, 64), img_bytes = pitch * h;
    if (!e->copy_in) {
        ORBX_HIP(hipStreamCreateWithFlags(&e->copy_in, hipStreamNonBlocking));
        ORBX_HIP(hipStreamCreateWithFlags(&e->copy_out, hipStreamNonBlocking));
    }
    {
        const size_t in_bytes = 2 * align_up(w, 64) * (size_t)h, in_rgbd = rg ? rgbd_in_bytes(w, h) : 0;
        if ((rc = pipe_slot_prepare(e, s, in_rgbd > in_bytes ? in_rgbd : in_bytes, need))) return rc;
    }
    // upload: the slot's device input was last read by the kernels of the frame that used it ORBX_PIPE_DEPTH submissions ago,
    // which its _wait has already seen finish (ev_d2h follows ev_done), so the copy stream may overwrite it right away
    const uint8_t *eye_ptr[2] = { img_left, img_right };
    PP_NEXT(2);
    // (inline form: upload, kernels and download of a frame all on its lane's stream -- no events, no stream hops; the lanes overlap each other)
    hipStream_t s_in = e->pipe_inline ? x->stream : e->copy_in, s_out = e->pipe_inline ? x->stream : e->copy_out;
    const bool kcopy = e->pipe_inline && e->pipe_kcopy;
    // host -> slot: pinned source (device-visible address `pin`, or nullptr) or staged through the slot's pinned h_in at offset `off`
    auto upload = [&](const uint8_t *src, const uint8_t *pin_src, size_t spitch, size_t row, int rows, size_t dpitch, size_t off) -> int {
        const size_t bytes = dpitch * rows;
        if (!pin_src) {
            uint8_t *dst = s.h_in + off;
            if (spitch == dpitch) memcpy(dst, src, dpitch * (rows - 1) + row);   // (the source's last row may end at its row bytes)
            else for (int y = 0; y < rows; y++) memcpy(dst + (size_t)y * dpitch, src + (size_t)y * spitch, row);
        }
        if (kcopy) hipLaunchKernelGGL(k_copy_bytes, dim3(128, 1), dim3(256), 0, x->stream, pin_src ? pin_src : (const uint8_t *)s.h_in_dev + off, (const uint8_t *)nullptr,
                                      s.d_in + off, (uint8_t *)nullptr, (unsigned long long)bytes);
        else ORBX_HIP(hipMemcpyAsync(s.d_in + off, pin_src ? src : s.h_in + off, bytes, hipMemcpyHostToDevice, s_in));
        return ORBX_OK;
    };
    const uint8_t *rg_depth = nullptr;                  // RGB-D: where k_rgbd_depth reads the depth map (slot or mapped host memory)
    size_t rg_dpitch = 0, rg_cpitch = 0, off_col = align_up(w, 64) * (size_t)h;
    if (rg) {
        // level 0 at s.d_in (pitch align_up(w, 64) after k_gray, or the grey image itself), the colour image behind it, the depth map last
        const size_t row = (size_t)w * rg->channels, off_dep = off_col + align_up((size_t)w * 4, 64) * (size_t)h;
        const uint8_t *ipin = stride == row ? pinned_device_ptr(img_left) : nullptr;
        const size_t ipitch = ipin ? row : align_up(row, 64);
        if (rg->channels == 1) { pitch = ipitch; img_bytes = pitch * h; }
        else { pitch = align_up(w, 64); img_bytes = pitch * h; rg_cpitch = ipitch; }
        if ((rc = upload(img_left, ipin, stride, row, h, ipitch, rg->channels == 1 ? 0 : off_col))) return rc;
        const size_t drow = (size_t)w * (rg->a.depth_type == ORBX_DEPTH_U16 ? 2 : 4);
        const uint8_t *dpin = rg->depth_stride == drow ? pinned_device_ptr(rg->depth) : nullptr;
        rg_dpitch = drow;
        if (e->pipe_rgbd_gather) {                      // the depth stays in host memory: only the values at the keypoints cross PCIe
            if (!dpin) {
                const uint8_t *src = (const uint8_t *)rg->depth;
                if (rg->depth_stride == drow) memcpy(s.h_in + off_dep, src, drow * h);
                else for (int y = 0; y < h; y++) memcpy(s.h_in + off_dep + (size_t)y * drow, src + (size_t)y * rg->depth_stride, drow);
            }
            rg_depth = dpin ? dpin : s.h_in_dev + off_dep;
        } else {
            if ((rc = upload((const uint8_t *)rg->depth, dpin, rg->depth_stride, drow, h, drow, off_dep))) return rc;
            rg_depth = s.d_in + off_dep;
        }
    } else if (in_place && kcopy) {
        hipLaunchKernelGGL(k_copy_bytes, dim3(128, eyes), dim3(256), 0, x->stream, pin[0], pin[1], s.d_in, s.d_in + img_bytes, (unsigned long long)img_bytes);
    } else if (in_place) {
        for (int i = 0; i < eyes; i++) ORBX_HIP(hipMemcpyAsync(s.d_in + img_bytes * i, eye_ptr[i], img_bytes, hipMemcpyHostToDevice, s_in));
    } else {
        for (int i = 0; i < eyes; i++) {
            uint8_t *dst = s.h_in + img_bytes * i;
            if (stride == pitch) memcpy(dst, eye_ptr[i], img_bytes);
            else for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * pitch, eye_ptr[i] + (size_t)y * stride, (size_t)w);
        }
        if (kcopy) hipLaunchKernelGGL(k_copy_bytes, dim3(128, eyes), dim3(256), 0, x->stream, (const uint8_t *)s.h_in_dev, (const uint8_t *)s.h_in_dev + img_bytes, s.d_in, s.d_in + img_bytes,
                                      (unsigned long long)img_bytes);
        else ORBX_HIP(hipMemcpyAsync(s.d_in, s.h_in, img_bytes * eyes, hipMemcpyHostToDevice, s_in));
    }
    if (!e->pipe_inline) {
        ORBX_HIP(hipEventRecord(s.ev_h2d, e->copy_in));
        ORBX_HIP(hipStreamWaitEvent(x->stream, s.ev_h2d, 0));
    }
    if (rg && rg->channels > 1)     // cvtColor (src/Tracking.cc:217-231) from the slot's colour image into its level 0
        hipLaunchKernelGGL(k_gray, dim3((unsigned)((pitch / 4 + 63) / 64), (h + 3) / 4), dim3(256), 0, x->stream, (const uint8_t *)s.d_in + off_col, w, h,
                           (int)rg_cpitch, rg->channels, rg->rgb_order, s.d_in, (int)pitch);
    x->prof_chain = false;
    orbx_keypoint *dk = (orbx_keypoint *)s.d_kps;
    uint8_t *dd = (uint8_t *)s.d_desc;
    int *dn = (int *)s.d_n;
    // the kernel error flag of this frame travels with its counts (k_desc drops it into the slot's block).  It is sticky on the device
    // (a node-table overflow is a configuration error, not a per-frame event): pipe_wait clears it when it reports it
    x->flag_out = dn + 2;
    PP_NEXT(3);
    rc = orbx_extract_batch_device(x, s.d_in, img_bytes, pitch, nimg, w, h, s.d_kps, s.d_desc, need, s.d_n, nullptr);
    x->flag_out = nullptr;
    if (rc) return rc;
    PP_NEXT(4);
    if (rg) {   // UndistortKeyPoints + ComputeStereoFromRGBD (src/Frame.cc:152-154); the undistorted positions take the unused second-eye keypoint rows
        RgbdArgs a = rg->a;
        a.depth = rg_depth; a.depth_img_stride = 0; a.depth_pitch = (long long)rg_dpitch;
        a.kps = dk; a.n = dn; a.cap = need;
        a.xy_un = reinterpret_cast<float2 *>(s.d_out + L.xy); a.u_right = s.d_ur; a.z = s.d_z;
        if ((rc = orbx_rgbd_launch(a, 1, x->stream))) return rc;
    }
    if (eyes == 2) {
        rc = orbx_stereo_match_batch_device(x, 0, x, 1, 1, dk, dd, dn, dk + need, dd + (size_t)32 * need, dn + 1, need, bf, min_z, s.d_ur, s.d_z,
                                            orbx_stereo_row_table_available(x, dk + need, 1, 1, need) ? ORBX_ROWTAB_OF_EXTRACTION : ORBX_ROWTAB_FROM_KEYPOINTS, nullptr);
        if (rc) return rc;
    }
    PP_NEXT(5);
    // download: one copy of the slot's block (counts + flag, both eyes' keypoints and descriptors, uRight, depth)
    if (!e->pipe_inline) {
        ORBX_HIP(hipEventRecord(s.ev_done, x->stream));
        ORBX_HIP(hipStreamWaitEvent(e->copy_out, s.ev_done, 0));
    }
    {
        const size_t out_bytes = eyes != 1 ? L.z + 4 * (size_t)need : L.desc + (size_t)32 * need;
        if (kcopy) hipLaunchKernelGGL(k_copy_bytes, dim3(64, 1), dim3(256), 0, x->stream, (const uint8_t *)s.d_out, (const uint8_t *)nullptr, s.h_out_dev, (uint8_t *)nullptr,
                                      (unsigned long long)out_bytes);
        else ORBX_HIP(hipMemcpyAsync(s.h_out, s.d_out, out_bytes, hipMemcpyDeviceToHost, s_out));
    }
    s.lane = x;
    ORBX_HIP(hipEventRecord(s.ev_d2h, s_out));
    // tickets are the low 31 bits of an unsigned submit counter: never negative, and (the depth divides 2^31) still congruent to the slot
    s.busy = true; s.cap = need; s.ticket = (int)(e->pipe_next & 0x7FFFFFFFu); s.eyes = eyes;
    *ticket = s.ticket;
    e->pipe_next++;
    return ORBX_OK;
#undef PP_NEXT
}

static int pipe_wait(orbx_extractor *e, int ticket, int eyes, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out, float *u_right, float *depth,
                     float *xy_un = nullptr)
{
    PipeSlot &s = e->pipe[ticket % ORBX_PIPE_DEPTH];
    if (!s.busy || s.ticket != ticket || s.eyes != eyes) { orbx_set_error("ticket %d is not in flight (or was submitted through the other form)", ticket); return ORBX_E_INVALID; }
    ORBX_HIP(orbx_use_device(e->device));
    const int need = s.cap;
    if (cap < need) { orbx_set_error("keypoint capacity %d < orbx_max_keypoints() = %d (the ticket stays valid)", cap, need); return ORBX_E_CAPACITY; }
    { PpScope w6(6); ORBX_HIP(hipEventSynchronize(s.ev_d2h)); }
    PpScope w7(7);
    s.busy = false;
    const ResultLayout L = orbx_result_layout(2, need);
    const int *hn = reinterpret_cast<const int *>(s.h_out);
    if (hn[2]) {
        orbx_extractor *x = s.lane ? s.lane : e;
        hipMemsetAsync(x->d_lvl_cnt + (size_t)x->max_batch * ORBX_MAX_LEVELS, 0, sizeof(int), x->stream);
        orbx_set_error("quadtree kernel reported a node-table overflow");
        return ORBX_E_CAPACITY;
    }
    for (int i = 0; i < (eyes == 2 ? 2 : 1); i++) {
        n_out[i] = hn[i];
        memcpy(kps + (size_t)i * cap, s.h_out + L.kps + sizeof(orbx_keypoint) * (size_t)need * i, sizeof(orbx_keypoint) * (size_t)hn[i]);
        memcpy(desc + (size_t)i * cap * 32, s.h_out + L.desc + (size_t)32 * need * i, (size_t)32 * hn[i]);
    }
    if (eyes != 1) {
        memcpy(u_right, s.h_out + L.ur, 4 * (size_t)hn[0]);
        memcpy(depth, s.h_out + L.z, 4 * (size_t)hn[0]);
    }
    if (eyes == ORBX_PIPE_RGBD && xy_un) memcpy(xy_un, s.h_out + L.xy, 8 * (size_t)hn[0]);
    return ORBX_OK;
}

// Every pipeline slot and every kernel lane (the handle and its shadow handles: own stream, pyramid / candidate / quadtree / stereo workspaces,
// pinned result block) of the pipelined forms is made and touched by running ONE frame of a textured scratch image through each, so that the
// frames that follow all see the steady-state latency.  Called by the first submit of a handle (and again when the image size changes); a
// caller that wants even its first frame on time calls it beforehand.  Round 3 made lanes and slots lazily, one per frame: the first four
// frames of a stream -- inside any timed window -- took 3-19 ms each against 0.2 ms.
extern "C" int orbx_pipeline_warm(orbx_extractor *e, int w, int h)
{
    if (!e || w < 1 || h < 1) { orbx_set_error("orbx_pipeline_warm: invalid argument"); return ORBX_E_INVALID; }
    if (e->max_batch < 2) { orbx_set_error("orbx_pipeline_warm needs an extractor created with max_batch >= 2"); return ORBX_E_INVALID; }
    if (e->pipe_warm_w == w && e->pipe_warm_h == h) return ORBX_OK;
    for (const PipeSlot &s : e->pipe) if (s.busy) { orbx_set_error("orbx_pipeline_warm: frames are in flight"); return ORBX_E_INVALID; }
    std::vector<uint8_t> img((size_t)w * h);
    unsigned lcg = 2463534242u;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            lcg = lcg * 1664525u + 1013904223u;
            img[(size_t)y * w + x] = (uint8_t)((((x >> 4) * 37 + (y >> 4) * 91) & 127) + 40 + (lcg >> 29));   // 16-px blocks: corners on every level
        }
    e->pipe_warm_w = w; e->pipe_warm_h = h;      // (set first: the submits below must not come back here)
    const int need = orbx_max_keypoints(e, w, h);
    int rc = need < 0 ? need : ORBX_OK;
    std::vector<orbx_keypoint> kps(rc ? 0 : 2 * (size_t)need);
    std::vector<uint8_t> desc(rc ? 0 : (size_t)64 * need);
    std::vector<float> ur(rc ? 0 : (size_t)need), z(rc ? 0 : (size_t)need);
    int tickets[ORBX_PIPE_DEPTH], n[2], nsub = 0;
    for (int i = 0; i < ORBX_PIPE_DEPTH && !rc; i++) {          // one frame per slot; the lanes go round with the slots
        rc = pipe_submit(e, img.data(), img.data(), 2, w, h, (size_t)w, 386.1448f, 0.5372f, &tickets[i]);
        if (!rc) nsub++;
    }
    for (int i = 0; i < nsub; i++) {
        const int wrc = pipe_wait(e, tickets[i], 2, kps.data(), desc.data(), need, n, ur.data(), z.data());
        if (wrc && !rc) rc = wrc;
    }
    if (rc) { e->pipe_warm_w = 0; e->pipe_warm_h = 0; }
    return rc;
}

extern "C" int orbx_extract_stereo_submit(orbx_extractor *e, const uint8_t *img_left, const uint8_t *img_right, int w, int h, size_t stride,
                                          float bf, float min_z, int *ticket)
{
    if (!e || !img_left || !img_right || !ticket || w < 1 || h < 1 || stride < (size_t)w || !(min_z > 0)) {
        orbx_set_error("orbx_extract_stereo_submit: invalid argument");
        return ORBX_E_INVALID;
    }
    if (e->max_batch < 2) { orbx_set_error("orbx_extract_stereo_submit needs an extractor created with max_batch >= 2"); return ORBX_E_INVALID; }
    if (e->pipe_warm_w != w || e->pipe_warm_h != h) {           // first frame of this size: make every lane and slot now, not one per frame
        bool idle = true;
        for (const PipeSlot &s : e->pipe) idle = idle && !s.busy;
        if (idle) { const int wrc = orbx_pipeline_warm(e, w, h); if (wrc) return wrc; }
    }
    return pipe_submit(e, img_left, img_right, 2, w, h, stride, bf, min_z, ticket);
}

extern "C" int orbx_extract_stereo_wait(orbx_extractor *e, int ticket, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out,
                                        float *u_right, float *depth)
{
    if (!e || !kps || !desc || !n_out || !u_right || !depth || ticket < 0) { orbx_set_error("orbx_extract_stereo_wait: invalid argument"); return ORBX_E_INVALID; }
    return pipe_wait(e, ticket, 2, kps, desc, cap, n_out, u_right, depth);
}

extern "C" int orbx_extract_rgbd_submit(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride, int channels, int rgb_order,
                                        const void *depth, size_t depth_stride, const orbx_rgbd_params *p, int *ticket)
{
    if (!e || !img || !depth || !ticket || w < 1 || h < 1 || (channels != 1 && channels != 3 && channels != 4) || stride < (size_t)w * channels) {
        orbx_set_error("orbx_extract_rgbd_submit: invalid argument");
        return ORBX_E_INVALID;
    }
    RgbdIn rg;
    int rc = orbx_rgbd_args("orbx_extract_rgbd_submit", p, w, h, depth_stride, &rg.a);
    if (rc) return rc;
    if (e->max_batch < 2) { orbx_set_error("orbx_extract_rgbd_submit needs an extractor created with max_batch >= 2"); return ORBX_E_INVALID; }
    rg.depth = depth; rg.depth_stride = depth_stride; rg.channels = channels; rg.rgb_order = rgb_order;
    if (e->pipe_rgbd_warm_w != w || e->pipe_rgbd_warm_h != h) {
        bool idle = true;
        for (const PipeSlot &s : e->pipe) idle = idle && !s.busy;
        if (idle) {
            // first RGB-D frame of this size: every lane and slot as orbx_pipeline_warm makes them, then one RGB-D frame through each slot
            // (the larger input block, k_gray and k_rgbd_depth on every lane) -- colour + float depth, the largest input form
            if ((rc = orbx_pipeline_warm(e, w, h))) return rc;
            e->pipe_rgbd_warm_w = w; e->pipe_rgbd_warm_h = h;
            std::vector<uint8_t> img4((size_t)w * h * 4);
            for (size_t i = 0; i < img4.size(); i++) img4[i] = (uint8_t)((((i / 4 % w) >> 4) * 37 + ((i / 4 / w) >> 4) * 91 + (i & 3) * 17) & 127) + 40;
            std::vector<float> dep((size_t)w * h, 1.0f);
            RgbdIn wr = rg;
            wr.depth = dep.data(); wr.depth_stride = (size_t)w * 4; wr.channels = 4; wr.rgb_order = 1; wr.a.depth_type = ORBX_DEPTH_F32;
            const int need = orbx_max_keypoints(e, w, h);
            if (need < 0) return need;
            std::vector<orbx_keypoint> kps(need); std::vector<uint8_t> desc((size_t)32 * need); std::vector<float> ur(need), z(need), xy(2 * (size_t)need);
            int tickets[ORBX_PIPE_DEPTH], n = 0, nsub = 0;
            for (int i = 0; i < ORBX_PIPE_DEPTH && !rc; i++) { rc = pipe_submit(e, img4.data(), nullptr, ORBX_PIPE_RGBD, w, h, (size_t)w * 4, 0.f, 1.f, &tickets[i], &wr); if (!rc) nsub++; }
            for (int i = 0; i < nsub; i++) {
                const int wrc = pipe_wait(e, tickets[i], ORBX_PIPE_RGBD, kps.data(), desc.data(), need, &n, ur.data(), z.data(), xy.data());
                if (wrc && !rc) rc = wrc;
            }
            if (rc) { e->pipe_rgbd_warm_w = 0; e->pipe_rgbd_warm_h = 0; return rc; }
        }
    }
    return pipe_submit(e, img, nullptr, ORBX_PIPE_RGBD, w, h, stride, 0.f, 1.f, ticket, &rg);
}

extern "C" int orbx_extract_rgbd_wait(orbx_extractor *e, int ticket, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out,
                                      float *xy_un, float *u_right, float *depth_out)
{
    if (!e || !kps || !desc || !n_out || !u_right || !depth_out || ticket < 0) { orbx_set_error("orbx_extract_rgbd_wait: invalid argument"); return ORBX_E_INVALID; }
    return pipe_wait(e, ticket, ORBX_PIPE_RGBD, kps, desc, cap, n_out, u_right, depth_out, xy_un);
}

extern "C" int orbx_extract_submit(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride, int *ticket)
{
    if (!e || !img || !ticket || w < 1 || h < 1 || stride < (size_t)w) { orbx_set_error("orbx_extract_submit: invalid argument"); return ORBX_E_INVALID; }
    return pipe_submit(e, img, nullptr, 1, w, h, stride, 0.f, 1.f, ticket);
}

extern "C" int orbx_extract_wait(orbx_extractor *e, int ticket, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out)
{
    if (!e || !kps || !desc || !n_out || ticket < 0) { orbx_set_error("orbx_extract_wait: invalid argument"); return ORBX_E_INVALID; }
    return pipe_wait(e, ticket, 1, kps, desc, cap, n_out, nullptr, nullptr);
}

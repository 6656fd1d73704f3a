// orbx_resident.hip — the two resident handles (include/orbx.h: orbx_frame, orbx_mappoints), what builds them, and the per-thread
// staging context every call on them shares (orbx_resident.h).
//
// In file order:
//   device   the grid build of Frame::AssignFeaturesToGrid (src/Frame.cc:261-279, :444-457): grid_build_body, k_grid_build
//            the frame ingest from extraction buffers: k_frame_ingest, k_frame_ingest_grid
//            the map-point table: k_mappoints_scatter (orbx_mappoints_set), k_frustum (Frame::isInFrustum from a pose, :310-380)
//   host     the CallCtx array, orbx_call_ctx; the launches orbx_proj.hip uses (orbx_grid_build_launch, orbx_frustum_launch)
//            the frame pool and the orbx_frame handle (create, create_from_extraction, size, read, destroy, set_depth)
//            the orbx_mappoints handle (create, destroy, capacity, set, read), the level thresholds, orbx_frustum_args,
//            orbx_mappoints_frustum
#include "orbx_device.h"
#include "orbx_resident.h"
#include <algorithm>
#include <math.h>
#include <mutex>

#define PG_LDS_FEATS 8192
// ---- Frame::AssignFeaturesToGrid: CSR over the 64x48 cells, ascending feature index inside a cell.  cell_of(i) = the cell of feature i
// (PosInGrid, src/Frame.cc:444-457) or -1; one 256-thread workgroup.
struct GridLds {
    int cnt[PG_CELLS];
    int cur[PG_CELLS];
    int s_w[4];
    uint16_t idx_l[PG_LDS_FEATS];     // the cell lists while they are being ordered (frames of up to PG_LDS_FEATS features)
};

__device__ __forceinline__ int grid_cell(float x, float y, float min_x, float min_y, float inv_w, float inv_h)
{
    const int px = (int)roundf((x - min_x) * inv_w), py = (int)roundf((y - min_y) * inv_h); // PosInGrid :444-457
    return (px >= 0 && px < PG_COLS && py >= 0 && py < PG_ROWS) ? px * PG_ROWS + py : -1;
}

template <typename CellOf>
__device__ __forceinline__ void grid_build_body(int n, CellOf cell_of, GridLds &L, int *__restrict__ cell_off, int *__restrict__ cell_idx)
{
    int *cnt = L.cnt, *cur = L.cur;
    uint16_t *idx_l = L.idx_l;
    const int tid = threadIdx.x;
    const bool in_lds = n <= PG_LDS_FEATS;
    for (int c = tid; c < PG_CELLS; c += 256) { cnt[c] = 0; cur[c] = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int c = cell_of(i);
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    const int total = lds_excl_scan(cnt, PG_CELLS, L.s_w);
    for (int c = tid; c < PG_CELLS; c += 256) cell_off[c] = cnt[c];
    if (tid == 0) cell_off[PG_CELLS] = total;
    for (int i = tid; i < n; i += 256) {
        const int c = cell_of(i);
        if (c >= 0) {
            const int slot = cnt[c] + atomicAdd(&cur[c], 1);
            if (in_lds) idx_l[slot] = (uint16_t)i; else cell_idx[slot] = i;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (in_lds) {
        // push_back order = ascending i: insertion sort of the (short) cell lists in LDS, then ONE coalesced copy to memory (sorting them in
        // global memory was a chain of dependent loads and stores per cell with two entries or more: half of this kernel's 10.8 us)
        for (int c = tid; c < PG_CELLS; c += 256) {
            const int b = cnt[c], e = b + cur[c];
            for (int a = b + 1; a < e; a++) {
                const uint16_t v = idx_l[a];
                int j = a - 1;
                while (j >= b && idx_l[j] > v) { idx_l[j + 1] = idx_l[j]; j--; }
                idx_l[j + 1] = v;
            }
        }
        __syncthreads();
        for (int j = tid; j < total; j += 256) cell_idx[j] = idx_l[j];
        return;
    }
    for (int c = tid; c < PG_CELLS; c += 256) { // (larger frames: the same in global memory)
        const int b = cnt[c], e = b + cur[c];
        for (int a = b + 1; a < e; a++) {
            const int v = cell_idx[a];
            int j = a - 1;
            while (j >= b && cell_idx[j] > v) { cell_idx[j + 1] = cell_idx[j]; j--; }
            cell_idx[j + 1] = v;
        }
    }
}

__global__ __launch_bounds__(256) void k_grid_build(DevFrame F, int *__restrict__ cell_off, int *__restrict__ cell_idx)
{
    __shared__ GridLds L;
    grid_build_body(F.n, [&](int i) { return grid_cell(F.x[i], F.y[i], F.min_x, F.min_y, F.inv_w, F.inv_h); }, L, cell_off, cell_idx);
}

// ---- resident frame (orbx_frame): the frame's block in HBM is x[n] y[n] octave[n] angle[n] u_right[n] desc[n][32] cell_off[3073]
// cell_idx[n].  The ingest turns orbx_extract_batch_device's keypoint records (28 B, orbx_keypoint) into those arrays, undistorts the
// positions when asked (dev_undistort: orbx_undistort_keypoints' arithmetic), copies the descriptors and u_right (-1 without one).
struct FrameIngest {
    const float *kps;        // [n][7] orbx_keypoint
    const uint4 *desc;       // [n][2]
    const float *u_right;    // [n] or NULL (monocular)
    int undistort;
    UndistortParams up;
};
struct FrameBlockPtrs {
    float *x, *y, *angle, *u_right;
    int32_t *octave;
    uint4 *desc;
    int *cell_off, *cell_idx;
};

__device__ __forceinline__ float2 ingest_feature(const FrameIngest &in, const FrameBlockPtrs &o, int i)
{
    const float *k = in.kps + 7 * (long long)i;
    float2 p = make_float2(k[0], k[1]);
    if (in.undistort) p = dev_undistort(p, in.up);
    o.x[i] = p.x; o.y[i] = p.y; o.angle[i] = k[3]; o.octave[i] = __float_as_int(k[5]);
    o.u_right[i] = in.u_right ? in.u_right[i] : -1.0f;
    return p;
}

// frames of more than PG_LDS_FEATS features: the ingest on its own (k_grid_build follows)
__global__ __launch_bounds__(256) void k_frame_ingest(FrameIngest in, FrameBlockPtrs o, int n)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) ingest_feature(in, o, t);
    if (t < 2 * n) o.desc[t] = in.desc[t];
}

// A frame's creation is a chain of dependent launches; up to PG_LDS_FEATS features ingest and grid build are ONE workgroup: the cell of
// every feature is taken from the position the ingest has in a register and parked in LDS, so the grid never reads back what the
// ingest wrote (one launch and one dependent global round trip less than ingest + k_grid_build).
__global__ __launch_bounds__(256) void k_frame_ingest_grid(FrameIngest in, FrameBlockPtrs o, int n, float min_x, float min_y, float inv_w,
                                                           float inv_h)
{
    __shared__ GridLds L;
    __shared__ uint16_t cell_l[PG_LDS_FEATS];
    for (int i = threadIdx.x; i < n; i += 256) {
        const float2 p = ingest_feature(in, o, i);
        cell_l[i] = (uint16_t)grid_cell(p.x, p.y, min_x, min_y, inv_w, inv_h);   // -1 -> 0xFFFF
    }
    for (int t = threadIdx.x; t < 2 * n; t += 256) o.desc[t] = in.desc[t];
    __syncthreads();
    grid_build_body(n, [&](int i) { const int c = cell_l[i]; return c == 0xFFFF ? -1 : c; }, L, o.cell_off, o.cell_idx);
}

// ---- resident map points (include/orbx.h: orbx_mappoints).  The table is geom[capacity] (32 B: X Y Z dmin | nx ny nz dmax) and
// desc[capacity] (32 B); a slot is a map point.  orbx_mappoints_set uploads the changed records densely and this kernel scatters them: four
// threads per point, one 16-byte move each (q = 0, 1: the geometry halves, 2, 3: the descriptor halves; a half not given is NULL).
__global__ __launch_bounds__(256) void k_mappoints_scatter(const int32_t *__restrict__ slots, const uint4 *__restrict__ geom_in,
                                                           const uint4 *__restrict__ desc_in, int n, uint4 *__restrict__ geom,
                                                           uint4 *__restrict__ desc)
{
    const int t = blockIdx.x * 256 + threadIdx.x, i = t >> 2, q = t & 3;
    if (i >= n) return;
    const long long s = slots[i];   // in [0, capacity): checked on the host
    if (q < 2) { if (geom_in) geom[2 * s + q] = geom_in[2 * (long long)i + q]; }
    else if (desc_in) desc[2 * s + (q - 2)] = desc_in[2 * (long long)i + (q - 2)];
}

// ---- Frame::isInFrustum (src/Frame.cc:310-380) from a pose, one thread per point; the arithmetic is the contract stated in include/orbx.h
// (float unless a step says double, no contraction, correctly rounded division and square root).  The scale level is NOT a logarithm here:
// thr[k] is the smallest float r with ceilf(logf(r) / mfLogScaleFactor) > k, found on the host with the C library's logf, and the level is
// the number of thresholds at or below dmax / dist -- no device logf equals the host's bit for bit.
__global__ __launch_bounds__(256) void k_frustum(const float4 *__restrict__ geom, const uint4 *__restrict__ tdesc,
                                                 const int32_t *__restrict__ slots, const uint8_t *__restrict__ flags, int n, FrustumArgs A,
                                                 FrustumOut o)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned fl = flags[i];   // bit 0: eligible, bit 1: Observations() > 0
    float u = 0.f, v = 0.f, xr = 0.f, vc = 0.f;
    int level = 0;
    bool in = false;
    long long s = 0;
    if (fl & 1) do {
        s = slots[i];               // in [0, capacity) and set: checked on the host
        const float4 g0 = geom[2 * s], g1 = geom[2 * s + 1];
        const float X = g0.x, Y = g0.y, Z = g0.z, dmin = g0.w, nx = g1.x, ny = g1.y, nz = g1.z, dmax = g1.w;
        const float pcx = ((A.R[0] * X + A.R[1] * Y) + A.R[2] * Z) + A.t[0];
        const float pcy = ((A.R[3] * X + A.R[4] * Y) + A.R[5] * Z) + A.t[1];
        const float pcz = ((A.R[6] * X + A.R[7] * Y) + A.R[8] * Z) + A.t[2];
        if (pcz < 0.0f) break;
        const float invz = 1.0f / pcz;
        const float pu = (A.fx * pcx) * invz + A.cx, pv = (A.fy * pcy) * invz + A.cy;
        if (pu < A.min_x || pu > A.max_x || pv < A.min_y || pv > A.max_y) break;
        if (!isfinite(pu) || !isfinite(pv)) break;                                        // (a NaN passes every comparison above)
        const float pox = X - A.Ow[0], poy = Y - A.Ow[1], poz = Z - A.Ow[2];
        const float dist = (float)__dsqrt_rn(((double)pox * pox + (double)poy * poy) + (double)poz * poz);   // cv::norm: double accumulation
        if (dist < 0.8f * dmin || dist > 1.2f * dmax) break;
        const float c = (float)((((double)pox * nx + (double)poy * ny) + (double)poz * nz) / (double)dist);   // Mat::dot in double
        if (!isfinite(c) || c < A.view_cos_limit) break;
        const float ratio = dmax / dist;                                                  // MapPoint::PredictScale
        int l = 0;
        for (int k = 0; k < A.nlevels - 1; k++) l += A.thr[k] <= ratio ? 1 : 0;
        u = pu; v = pv; xr = pu - A.mbf * invz; vc = c; level = l; in = true;
    } while (0);
    o.u[i] = u; o.v[i] = v; o.xr[i] = xr; o.view_cos[i] = vc; o.level[i] = level; o.in_view[i] = in ? 1 : 0;
    if (o.has_obs) o.has_obs[i] = (fl >> 1) & 1;
    if (o.desc && in) { o.desc[2 * (long long)i] = tdesc[2 * s]; o.desc[2 * (long long)i + 1] = tdesc[2 * s + 1]; }
}

// ---------------------------------------------------------------- host side

void CallCtx::release()
{
    if (orbx_ctx_leave(this)) {
        if (h_blob) (void)hipHostFree(h_blob);
        if (d_blob) (void)hipFree(d_blob);
        if (d_work) (void)hipFree(d_work);
        if (d_entries) (void)hipFree(d_entries);
        if (h_out) (void)hipHostFree(h_out);
        if (h_n) (void)hipHostFree(h_n);
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
    ev_a = ev_b = nullptr;
    h_blob = d_blob = d_work = nullptr; d_entries = nullptr; h_out = h_n = nullptr;
    h_cap = d_cap = work_cap = ent_cap = out_cap = 0;
}
static thread_local CallCtx g_call[ORBX_MAX_DEVICES];
void orbx_proj_thread_release() { for (CallCtx &c : g_call) c.release(); }
int orbx_call_ctx(int device, CallCtx **out) { return orbx_ctx_get(g_call, device, out); }

void orbx_grid_build_launch(const DevFrame &F, int *d_cell_off, int *d_cell_idx, hipStream_t s)
{
    hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(256), 0, s, F, d_cell_off, d_cell_idx);
}

void orbx_frustum_launch(const orbx_mappoints *m, const int32_t *d_slots, const uint8_t *d_flags, int n, const FrustumArgs &A,
                         const FrustumOut &o, hipStream_t s)
{
    hipLaunchKernelGGL(k_frustum, dim3((n + 255) / 256), dim3(256), 0, s, m->d_geom, m->d_desc, d_slots, d_flags, n, A, o);
}

// ---------------------------------------------------------------- resident current frame (include/orbx.h: orbx_frame)

// Frame blocks and their events are recycled: a frame lives one frame time, and hipFree would synchronise the device every frame.  A block
// returns to its device's pool only after the work that wrote it has completed (its event).
static std::mutex g_fpool_mu;
static std::vector<FrameBlock> g_fpool[ORBX_MAX_DEVICES];
#define FRAME_POOL_MAX 8

static int frame_block_get(int device, size_t bytes, FrameBlock *out)
{
    {
        std::lock_guard<std::mutex> lk(g_fpool_mu);
        std::vector<FrameBlock> &v = g_fpool[device];
        int best = -1;
        for (int i = 0; i < (int)v.size(); i++)
            if (v[i].cap >= bytes && (best < 0 || v[i].cap < v[best].cap)) best = i;
        if (best >= 0) { *out = v[best]; v.erase(v.begin() + best); return ORBX_OK; }
    }
    FrameBlock b;
    b.cap = (bytes + 65535) & ~(size_t)65535;   // frames of similar size share blocks
    ORBX_HIP(hipMalloc((void **)&b.d, b.cap));
    if (hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess) {
        hipFree(b.d);
        orbx_set_error("orbx_frame: hipEventCreateWithFlags failed");
        return ORBX_E_HIP;
    }
    *out = b;
    return ORBX_OK;
}

static void frame_block_put(int device, FrameBlock b)
{
    hipEventSynchronize(b.ev);   // the creation that wrote the block (searches of the frame have synchronised already)
    std::lock_guard<std::mutex> lk(g_fpool_mu);
    std::vector<FrameBlock> &v = g_fpool[device];
    if (v.size() < FRAME_POOL_MAX) { v.push_back(b); return; }
    hipEventDestroy(b.ev);
    hipFree(b.d);
}

static orbx_frame *frame_new(int device, int n, int has_angle, float min_x, float min_y, float max_x, float max_y)
{
    orbx_frame *f = new orbx_frame();
    static_cast<FrameLayout &>(*f) = frame_layout((size_t)n);
    f->device = device; f->n = n; f->has_angle = has_angle;
    f->bounds[0] = min_x; f->bounds[1] = min_y; f->bounds[2] = max_x; f->bounds[3] = max_y;
    f->pending = false;
    return f;
}

extern "C" int orbx_frame_create(int device, const orbx_frame_feats *cur, orbx_frame **out)
{
    if (!out || !cur || cur->n < 0 || cur->n >= 65536) { orbx_set_error("orbx_frame_create: invalid argument"); return ORBX_E_INVALID; }
    *out = nullptr;
    if (cur->n && (!cur->x || !cur->y || !cur->octave || !cur->u_right || !cur->desc)) { orbx_set_error("orbx_frame_create: frame arrays missing"); return ORBX_E_INVALID; }
    if (!(cur->max_x > cur->min_x) || !(cur->max_y > cur->min_y)) { orbx_set_error("orbx_frame_create: empty image bounds"); return ORBX_E_INVALID; }
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    orbx_frame *f = frame_new(device, cur->n, cur->n == 0 || cur->angle ? 1 : 0, cur->min_x, cur->min_y, cur->max_x, cur->max_y);
    rc = frame_block_get(device, f->bytes, &f->blk);
    if (rc) { delete f; return rc; }
    // the frame arrays of the block are the head of a host-pointer call's staging blob (one frame_layout): frame_stage puts them there, one upload
    rc = call_reserve(c, f->o_coff, 0, 0);
    if (!rc) {
        const DevFrame F = frame_dev(f);
        if (cur->n) {
            frame_stage(c, cur);
            if (hipMemcpyAsync(f->blk.d, c->h_blob, f->o_coff, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = ORBX_E_HIP;
        }
        if (!rc) hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(256), 0, c->stream, F, (int *)(f->blk.d + f->o_coff), (int *)(f->blk.d + f->o_cidx));
        if (!rc && (hipGetLastError() != hipSuccess || hipEventRecord(f->blk.ev, c->stream) != hipSuccess ||
                    hipStreamSynchronize(c->stream) != hipSuccess)) rc = ORBX_E_HIP;   // the staging blob is reused by the next call
        if (rc) orbx_set_error("orbx_frame_create: upload / grid build failed");
    }
    if (rc) { frame_block_put(device, f->blk); delete f; return rc; }
    if (cur->n) f->h_oct.assign(cur->octave, cur->octave + cur->n);
    for (int i = 0; i < cur->n; i++)
        if (cur->u_right[i] >= 0.f) { f->has_stereo = true; break; }
    *out = f;
    return ORBX_OK;
}

extern "C" int orbx_frame_create_from_extraction(int device, const void *d_kps, const void *d_desc, const void *d_n, int cap, int index,
                                                 const void *d_u_right, const float *K, const float *dist_coef, int ndist,
                                                 float min_x, float min_y, float max_x, float max_y, void *stream, orbx_frame **out)
{
    if (!out || !d_kps || !d_desc || !d_n || cap < 1 || index < 0) {
        orbx_set_error("orbx_frame_create_from_extraction: invalid argument (null buffer, cap < 1 or index < 0)");
        return ORBX_E_INVALID;
    }
    *out = nullptr;
    if (K && (!dist_coef || (ndist != 4 && ndist != 5) || K[0] == 0.f || K[1] == 0.f)) {
        orbx_set_error("orbx_frame_create_from_extraction: K needs fx, fy != 0 and 4 or 5 distortion coefficients");
        return ORBX_E_INVALID;
    }
    if (!(max_x > min_x) || !(max_y > min_y)) { orbx_set_error("orbx_frame_create_from_extraction: empty image bounds"); return ORBX_E_INVALID; }
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!c->h_n) ORBX_HIP(hipHostMalloc((void **)&c->h_n, 64, hipHostMallocDefault));
    ORBX_HIP(hipMemcpyAsync(c->h_n, (const int32_t *)d_n + index, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));   // the one synchronisation: the count sizes the frame
    const int n = c->h_n[0];
    if (n < 0 || n > cap || n >= 65536) {
        orbx_set_error("orbx_frame_create_from_extraction: image %d holds %d keypoints, outside [0, cap = %d] (wrong index / cap?)", index, n, cap);
        return ORBX_E_INVALID;
    }
    orbx_frame *f = frame_new(device, n, 1, min_x, min_y, max_x, max_y);
    rc = frame_block_get(device, f->bytes, &f->blk);
    if (rc) { delete f; return rc; }
    FrameIngest in;
    memset(&in, 0, sizeof in);
    in.kps = (const float *)((const uint8_t *)d_kps + (size_t)index * cap * sizeof(orbx_keypoint));
    in.desc = (const uint4 *)((const uint8_t *)d_desc + (size_t)index * cap * 32);
    in.u_right = (const float *)d_u_right;
    in.undistort = K && dist_coef[0] != 0.0f;   // src/Frame.cc:472-476: mvKeysUn = mvKeys
    if (in.undistort) in.up = orbx_undistort_params(K[0], K[1], K[2], K[3], dist_coef, ndist);
    uint8_t *d = f->blk.d;
    FrameBlockPtrs o;
    o.x = (float *)(d + f->o_x); o.y = (float *)(d + f->o_y); o.octave = (int32_t *)(d + f->o_oct); o.angle = (float *)(d + f->o_ang);
    o.u_right = (float *)(d + f->o_ur); o.desc = (uint4 *)(d + f->o_desc); o.cell_off = (int *)(d + f->o_coff); o.cell_idx = (int *)(d + f->o_cidx);
    const DevFrame F = frame_dev(f);
    if (n <= PG_LDS_FEATS) {
        hipLaunchKernelGGL(k_frame_ingest_grid, dim3(1), dim3(256), 0, st, in, o, n, F.min_x, F.min_y, F.inv_w, F.inv_h);
    } else {
        hipLaunchKernelGGL(k_frame_ingest, dim3((2 * n + 255) / 256), dim3(256), 0, st, in, o, n);
        hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(256), 0, st, F, o.cell_off, o.cell_idx);
    }
    if (hipGetLastError() != hipSuccess || hipEventRecord(f->blk.ev, st) != hipSuccess) {
        orbx_set_error("orbx_frame_create_from_extraction: launch failed");
        frame_block_put(device, f->blk);
        delete f;
        return ORBX_E_HIP;
    }
    f->pending = true;
    f->from_extraction = true;
    *out = f;
    return ORBX_OK;
}

extern "C" int orbx_frame_size(const orbx_frame *f) { return f ? f->n : ORBX_E_INVALID; }

extern "C" int orbx_frame_read(const orbx_frame *f, float *x, float *y, int32_t *octave, float *angle, float *u_right, uint8_t *desc)
{
    if (!f) { orbx_set_error("orbx_frame_read: null frame"); return ORBX_E_INVALID; }
    if (f->n == 0) return ORBX_OK;
    ORBX_HIP(orbx_use_device(f->device));
    ORBX_HIP(hipEventSynchronize(f->blk.ev));
    const size_t nc = (size_t)f->n;
    const uint8_t *d = f->blk.d;
    if (x) ORBX_HIP(hipMemcpy(x, d + f->o_x, 4 * nc, hipMemcpyDeviceToHost));
    if (y) ORBX_HIP(hipMemcpy(y, d + f->o_y, 4 * nc, hipMemcpyDeviceToHost));
    if (octave) ORBX_HIP(hipMemcpy(octave, d + f->o_oct, 4 * nc, hipMemcpyDeviceToHost));
    if (angle) ORBX_HIP(hipMemcpy(angle, d + f->o_ang, 4 * nc, hipMemcpyDeviceToHost));
    if (u_right) ORBX_HIP(hipMemcpy(u_right, d + f->o_ur, 4 * nc, hipMemcpyDeviceToHost));
    if (desc) ORBX_HIP(hipMemcpy(desc, d + f->o_desc, 32 * nc, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" void orbx_frame_destroy(orbx_frame *f)
{
    if (!f) return;
    if (orbx_use_device(f->device) == hipSuccess) {
        frame_block_put(f->device, f->blk);
        if (f->d_depth) (void)hipFree(f->d_depth);
    }
    delete f;
}

extern "C" int orbx_frame_set_depth(orbx_frame *f, const float *depth, const float *raw_x, const float *raw_y)
{
    if (!f || !depth || (!raw_x) != (!raw_y)) { orbx_set_error("orbx_frame_set_depth: invalid argument (a frame, depth, raw_x and raw_y both or neither)"); return ORBX_E_INVALID; }
    if (f->depth_set) { orbx_set_error("orbx_frame_set_depth: the frame has its depth already"); return ORBX_E_INVALID; }
    if (f->n) {
        ORBX_HIP(orbx_use_device(f->device));
        const size_t b = 4 * (size_t)f->n, s = a16(b);
        uint8_t *d = nullptr;
        ORBX_HIP(hipMalloc((void **)&d, (raw_x ? 3 : 1) * s));
        hipError_t e = hipMemcpy(d, depth, b, hipMemcpyHostToDevice);
        if (e == hipSuccess && raw_x) e = hipMemcpy(d + s, raw_x, b, hipMemcpyHostToDevice);
        if (e == hipSuccess && raw_x) e = hipMemcpy(d + 2 * s, raw_y, b, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); orbx_set_error("orbx_frame_set_depth: upload failed: %s", hipGetErrorString(e)); return ORBX_E_HIP; }
        f->d_depth = (float *)d;
        if (raw_x) { f->d_raw_x = (float *)(d + s); f->d_raw_y = (float *)(d + 2 * s); }
    }
    f->depth_set = true;
    return ORBX_OK;
}

// ---------------------------------------------------------------- resident map points (include/orbx.h: orbx_mappoints)

#define MP_STAGE_RECORDS 65536

extern "C" int orbx_mappoints_create(int device, int capacity, orbx_mappoints **out)
{
    if (!out || capacity < 1 || capacity > (1 << 24)) { orbx_set_error("orbx_mappoints_create: invalid argument (1 <= capacity <= 2^24)"); return ORBX_E_INVALID; }
    *out = nullptr;
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    const size_t cap = (size_t)capacity;
    orbx_mappoints *m = new orbx_mappoints();
    m->device = device; m->capacity = capacity;
    m->stage_records = capacity < MP_STAGE_RECORDS ? capacity : MP_STAGE_RECORDS;
    m->st_bytes = a16(4 * (size_t)m->stage_records) + 64 * (size_t)m->stage_records;
    const size_t table = 64 * cap, total = table + m->st_bytes;
    m->d_blob = nullptr; m->h_stage = nullptr; m->ev = nullptr; m->ev_stream = nullptr; m->ev_set = false; m->gen = 0;
    const hipError_t e1 = hipMalloc((void **)&m->d_blob, total);
    const hipError_t e2 = e1 == hipSuccess ? hipHostMalloc((void **)&m->h_stage, m->st_bytes, hipHostMallocDefault) : e1;
    const hipError_t e3 = e2 == hipSuccess ? hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) : e2;
    const hipError_t e4 = e3 == hipSuccess ? hipMemset(m->d_blob, 0, table) : e3;   // a half never given reads 0
    if (e4 != hipSuccess) {
        orbx_set_error("orbx_mappoints_create: HIP allocation of %zu bytes failed: %s", total, hipGetErrorString(e4));
        if (m->ev) hipEventDestroy(m->ev);
        if (m->h_stage) hipHostFree(m->h_stage);
        if (m->d_blob) hipFree(m->d_blob);
        delete m;
        return ORBX_E_HIP;
    }
    m->d_geom = (float4 *)m->d_blob; m->d_desc = (uint4 *)(m->d_blob + 32 * cap); m->d_stage = m->d_blob + table;
    m->have.assign(cap, 0); m->stamp.assign(cap, 0);
    *out = m;
    return ORBX_OK;
}

extern "C" void orbx_mappoints_destroy(orbx_mappoints *m)
{
    if (!m) return;
    if (orbx_use_device(m->device) == hipSuccess) {
        if (m->ev_set) hipEventSynchronize(m->ev);
        hipEventDestroy(m->ev);
        hipHostFree(m->h_stage);
        hipFree(m->d_blob);
    }
    delete m;
}

extern "C" int orbx_mappoints_capacity(const orbx_mappoints *m) { return m ? m->capacity : ORBX_E_INVALID; }

extern "C" int orbx_mappoints_set(orbx_mappoints *m, const int32_t *slots, int n, const float *geom, const uint8_t *desc, void *stream)
{
    if (!m || n < 0 || (n && (!slots || (!geom && !desc)))) { orbx_set_error("orbx_mappoints_set: invalid argument (a table, n slots, geom and / or desc)"); return ORBX_E_INVALID; }
    if (n == 0) return ORBX_OK;
    std::unique_lock<std::shared_timed_mutex> lk(m->mu);
    // refusals first: the table and its bitmap stay as they were
    if (++m->gen == 0) { std::fill(m->stamp.begin(), m->stamp.end(), 0u); m->gen = 1; }
    const unsigned give = (geom ? 1u : 0u) | (desc ? 2u : 0u);
    for (int i = 0; i < n; i++) {
        const int s = slots[i];
        if (s < 0) { orbx_set_error("orbx_mappoints_set: entry %d: negative slot %d", i, s); return ORBX_E_INVALID; }
        if (s >= m->capacity) { orbx_set_error("orbx_mappoints_set: entry %d: slot %d, capacity %d", i, s, m->capacity); return ORBX_E_CAPACITY; }
        if (m->stamp[s] == m->gen) { orbx_set_error("orbx_mappoints_set: slot %d named twice", s); return ORBX_E_INVALID; }
        m->stamp[s] = m->gen;
        if ((m->have[s] | give) != 3) { orbx_set_error("orbx_mappoints_set: slot %d has never been given its %s", s, geom ? "descriptor" : "geometry"); return ORBX_E_INVALID; }
    }
    CallCtx *c;
    int rc = orbx_call_ctx(m->device, &c);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // one upload and one scatter launch per MP_STAGE_RECORDS records (a frame's changes are one), each packed by its own count
    for (int first = 0; first < n; first += m->stage_records) {
        const int k = n - first < m->stage_records ? n - first : m->stage_records;
        const size_t kk = (size_t)k, o_geom = a16(4 * kk), o_desc = o_geom + (geom ? 32 * kk : 0), bytes = o_desc + (desc ? 32 * kk : 0);
        if (m->ev_set) ORBX_HIP(hipEventSynchronize(m->ev));   // the previous upload has read the staging
        memcpy(m->h_stage, slots + first, 4 * kk);
        if (geom) memcpy(m->h_stage + o_geom, geom + 8 * (size_t)first, 32 * kk);
        if (desc) memcpy(m->h_stage + o_desc, desc + 32 * (size_t)first, 32 * kk);
        ORBX_HIP(hipMemcpyAsync(m->d_stage, m->h_stage, bytes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mappoints_scatter, dim3((4 * k + 255) / 256), dim3(256), 0, st, (const int32_t *)m->d_stage,
                           geom ? (const uint4 *)(m->d_stage + o_geom) : nullptr, desc ? (const uint4 *)(m->d_stage + o_desc) : nullptr, k,
                           (uint4 *)m->d_geom, m->d_desc);
        ORBX_HIP(hipGetLastError());
        ORBX_HIP(hipEventRecord(m->ev, st));
        m->ev_stream = st; m->ev_set = true;
        for (int i = first; i < first + k; i++) m->have[slots[i]] |= (uint8_t)give;   // what has been enqueued is in the table for every later call
    }
    return ORBX_OK;
}

extern "C" int orbx_mappoints_read(const orbx_mappoints *m, const int32_t *slots, int n, float *geom, uint8_t *desc)
{
    if (!m || n < 0 || (n && !slots)) { orbx_set_error("orbx_mappoints_read: invalid argument"); return ORBX_E_INVALID; }
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= m->capacity) { orbx_set_error("orbx_mappoints_read: entry %d: slot %d outside [0, %d)", i, slots[i], m->capacity); return ORBX_E_INVALID; }
    if (n == 0) return ORBX_OK;
    std::shared_lock<std::shared_timed_mutex> lk(m->mu);
    ORBX_HIP(orbx_use_device(m->device));
    if (m->ev_set) ORBX_HIP(hipEventSynchronize(m->ev));
    // one copy per run of consecutive ascending slots and half: proportional to n, not to the capacity
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && slots[j] == slots[j - 1] + 1) j++;
        const size_t run = 32 * (size_t)(j - i), src = 32 * (size_t)slots[i], dst = 32 * (size_t)i;
        if (geom) ORBX_HIP(hipMemcpy((uint8_t *)geom + dst, (const uint8_t *)m->d_geom + src, run, hipMemcpyDeviceToHost));
        if (desc) ORBX_HIP(hipMemcpy(desc + dst, (const uint8_t *)m->d_desc + src, run, hipMemcpyDeviceToHost));
        i = j;
    }
    return ORBX_OK;
}

// the smallest positive float r with ceilf(logf(r) / lsf) > k: bisection over float bit patterns (the predicate is monotone in r; it is
// false at 0, where logf is -inf, and true at +inf)
static float level_threshold(float lsf, int k)
{
    uint32_t lo = 0, hi = 0x7F800000u;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float r;
        memcpy(&r, &mid, 4);
        if (ceilf(logf(r) / lsf) > (float)k) hi = mid; else lo = mid;
    }
    float r;
    memcpy(&r, &hi, 4);
    return r;
}

struct LevelThr { float lsf; int nlevels; float thr[ORBX_MAX_LEVELS - 1]; };
static std::mutex g_thr_mu;
static std::vector<LevelThr> g_thr;   // one entry per (log_scale_factor, nlevels) seen: a SLAM system has one or two

static void level_thresholds(float lsf, int nlevels, float *thr)
{
    std::lock_guard<std::mutex> lk(g_thr_mu);
    for (const LevelThr &t : g_thr)
        if (memcmp(&t.lsf, &lsf, 4) == 0 && t.nlevels == nlevels) { memcpy(thr, t.thr, sizeof t.thr); return; }
    LevelThr t;
    memset(&t, 0, sizeof t);
    t.lsf = lsf; t.nlevels = nlevels;
    for (int k = 0; k < nlevels - 1; k++) t.thr[k] = level_threshold(lsf, k);
    if (g_thr.size() >= 64) g_thr.clear();
    g_thr.push_back(t);
    memcpy(thr, t.thr, sizeof t.thr);
}

int orbx_frustum_args(const char *who, const orbx_mappoints *m, const int32_t *slots, const uint8_t *flags, int n, bool any_bit,
                      const float *pose, const float *cam, float view_cos_limit, float lsf, int nlevels, FrustumArgs *A)
{
    if (!m || n < 0 || n > (1 << 20) || (n && (!slots || !flags)) || !pose || !cam || nlevels < 1 || nlevels > ORBX_MAX_LEVELS ||
        !(lsf > 0.f) || !isfinite(lsf)) {
        orbx_set_error("%s: invalid argument (a table, n <= 2^20 slots and flags, pose, cam, 1 <= nlevels <= %d, log_scale_factor > 0)", who, ORBX_MAX_LEVELS);
        return ORBX_E_INVALID;
    }
    for (int i = 0; i < n; i++) {
        if (!(any_bit ? flags[i] != 0 : (flags[i] & 1) != 0)) continue;   // not eligible: the slot is never looked at
        const int s = slots[i];
        if (s < 0 || s >= m->capacity) { orbx_set_error("%s: point %d: slot %d outside [0, %d)", who, i, s, m->capacity); return ORBX_E_INVALID; }
        if (m->have[s] != 3) { orbx_set_error("%s: point %d: slot %d is not set", who, i, s); return ORBX_E_INVALID; }
    }
    memset(A, 0, sizeof *A);
    memcpy(A->R, pose, 9 * sizeof(float)); memcpy(A->t, pose + 9, 3 * sizeof(float)); memcpy(A->Ow, pose + 12, 3 * sizeof(float));
    A->fx = cam[0]; A->fy = cam[1]; A->cx = cam[2]; A->cy = cam[3]; A->mbf = cam[4];
    A->min_x = cam[5]; A->min_y = cam[6]; A->max_x = cam[7]; A->max_y = cam[8];
    A->view_cos_limit = view_cos_limit; A->nlevels = nlevels;
    level_thresholds(lsf, nlevels, A->thr);
    return ORBX_OK;
}

extern "C" int orbx_mappoints_frustum(const orbx_mappoints *m, const int32_t *slots, const uint8_t *eligible, int n, const float *pose,
                                      const float *cam, float view_cos_limit, float log_scale_factor, int nlevels, uint8_t *in_view,
                                      float *u, float *v, float *xr, int32_t *level, float *view_cos)
{
    if (n > 0 && !in_view) { orbx_set_error("orbx_mappoints_frustum: in_view missing"); return ORBX_E_INVALID; }
    if (!m) { orbx_set_error("orbx_mappoints_frustum: null table"); return ORBX_E_INVALID; }
    std::shared_lock<std::shared_timed_mutex> lk(m->mu);
    FrustumArgs A;
    int rc = orbx_frustum_args("orbx_mappoints_frustum", m, slots, eligible, n, true, pose, cam, view_cos_limit, log_scale_factor, nlevels, &A);
    if (rc) return rc;
    if (n == 0) return ORBX_OK;
    CallCtx *c;
    if ((rc = orbx_call_ctx(m->device, &c))) return rc;
    const size_t np = (size_t)n, col = a16(4 * np);
    const size_t blob = col + a16(np), out = 5 * col + a16(np);   // up: slots | flags   down: u v xr view_cos level | in_view
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    memcpy(c->h_blob, slots, 4 * np);
    for (size_t i = 0; i < np; i++) c->h_blob[col + i] = eligible[i] ? 1 : 0;
    if ((rc = mappoints_order_before(m, c->stream))) return rc;
    if ((rc = call_upload(c, blob))) return rc;
    uint8_t *wk = c->d_work;
    FrustumOut fo;
    memset(&fo, 0, sizeof fo);
    fo.u = (float *)wk; fo.v = (float *)(wk + col); fo.xr = (float *)(wk + 2 * col); fo.view_cos = (float *)(wk + 3 * col);
    fo.level = (int32_t *)(wk + 4 * col); fo.in_view = wk + 5 * col;
    orbx_frustum_launch(m, (const int32_t *)c->d_blob, c->d_blob + col, n, A, fo, c->stream);
    if ((rc = call_fetch(c, out))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    if (u) memcpy(u, ho, 4 * np);
    if (v) memcpy(v, ho + col, 4 * np);
    if (xr) memcpy(xr, ho + 2 * col, 4 * np);
    if (view_cos) memcpy(view_cos, ho + 3 * col, 4 * np);
    if (level) memcpy(level, ho + 4 * col, 4 * np);
    memcpy(in_view, ho + 5 * col, np);
    return ORBX_OK;
}

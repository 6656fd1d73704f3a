// orbx_proj.hip — the projection-guided searches of ORB-SLAM2, seven in all, reference src/ORBmatcher.cc:
//   SearchByProjection(Frame&, const Frame&, th, bMono)                 :1396-1553   last frame
//   SearchByProjection(Frame&, const vector<MapPoint*>&, th)            :48-129      local map points
//   SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)   :1555-1685   relocalisation
//   SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)         :305-415     loop closing
//   Fuse x2 (search half) and each direction of SearchBySim3            :873-1164, :1218-1372   ("window best": independent points)
//   SearchBySim3                                                        :1166-1394
//   SearchForInitialization                                             :430-556
// with Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea (src/Frame.cc:261-279, :386-457).
//
// In file order:
//   device   DevFrame, DevPoints, ProjParams (one parameter block describes every search)
//            the grid build: grid_build_body, k_grid_build
//            the frame ingest from extraction buffers: k_frame_ingest, k_frame_ingest_grid
//            a point's window and candidate test: point_window, cand_ok; the window walk both per-point kernels share: window_walk
//            k_proj_lists (candidate lists), k_proj_resolve (claim fixpoint + rotation filter), k_init_resolve (SearchForInitialization)
//            k_window_best (independent points against resident keyframes, many jobs per launch)
//            the resident map-point table: k_mappoints_scatter (orbx_mappoints_set), k_frustum (Frame::isInFrustum from a pose)
//   host     ProjCtx (per-thread staging); frame_layout, dev_frame (one layout of a frame's arrays); proj_stage_frame, points_stage;
//            proj_search (upload, grid, lists, resolve, download); points_check, proj_run; the parameter blocks params_*; sim3_agree
//            the host-pointer entry points of the seven searches
//            the frame pool and the orbx_frame handle (create, create_from_extraction, read, destroy)
//            the searches on a resident current frame; the searches on resident keyframes (orbx_frame_window_best_batch and its users)
//            the resident map points (orbx_mappoints: create, set, read, frustum) and orbx_frame_search_local_points
//
// The reference walks the map points sequentially and lets every accepted match claim its feature
// (later points skip features whose holder has Observations() > 0), so the result depends on the order.
// Exact parallel form: the per-point candidate lists (window, level, uRight tests and Hamming distances) do
// not depend on the claims and are built in parallel, in GetFeaturesInArea's traversal order; the claims are
// then the unique fixpoint of
//     choice(i) = best candidate f of i with  !occupied(f)  and no j < i, has_obs(j), choice(j) == f,
// a recursion on i, reached by iterating all points in parallel until nothing changes (at most one round
// per link of the longest conflict chain).  Projections (u, v, 1/z) come from the adaptor, which has the
// poses: restating cv::gemm's accumulation is not needed.
#include "orbx_device.h"
#include <algorithm>
#include <math.h>
#include <mutex>
#include <shared_mutex>
#include <string.h>
#include <vector>

#define PG_COLS 64 // FRAME_GRID_COLS, include/Frame.h:38
#define PG_ROWS 48 // FRAME_GRID_ROWS, include/Frame.h:37
#define PG_CELLS (PG_COLS * PG_ROWS)

struct DevFrame {
    int n;
    const float *x, *y, *angle, *u_right;
    const int32_t *octave;
    const uint32_t *desc;
    const uint8_t *occupied;
    float min_x, min_y, max_x, max_y, inv_w, inv_h;
};
struct DevPoints {
    int n;
    const float *u, *v, *aux, *angle, *view_cos;
    const int32_t *level;
    const uint32_t *desc;
    const uint8_t *valid, *has_obs;
};
// One parameter block describes every projection-type search of src/ORBmatcher.cc (which tests, which window, which
// claim rule); the extern "C" entry points below fill it per reference function.
struct ProjParams {
    int radius_mode;   // 0: th * sf[level]   1: RadiusByViewingCos(view_cos) [* th] * sf[level]   2: th (a fixed window)
    int bounds;        // 0: none  1: Frame bounds, inclusive (:1431-1434)  2: KeyFrame::IsInImage (src/KeyFrame.cc:649-652)
    int need_pos_aux;  // 1: reject aux (= invzc) < 0 (:1426)
    int lo_off, hi_off;// candidate levels [level + lo_off, level + hi_off] unless direction != 0
    int direction;     // last-frame search: 1 bForward, 2 bBackward
    int ur_mode;       // 0: none  1: |u - mbf*aux - uR| > r (:1467-1471)  2: |aux - uR| > r (:88-92)
    int chi2;          // Fuse: reprojection gate 5.99 / 7.8 with inv_sigma2[octave], aux = ur (:967-992)
    int max_dist;      // TH_HIGH, TH_LOW or ORBdist
    int ratio;         // 1: same-level ratio test of the map-point search (:117-121)
    int check_ori;
    int mark_cleared;  // 1: a feature whose match the rotation filter cleared reads -2 instead of -1 (the reference leaves NULL there, not the old holder)
    int init_search;   // 1: SearchForInitialization's sequential rule (k_init_resolve)
    int claims;        // 0: points are independent (Fuse, SearchBySim3)  1: an accepted match of a point with
                       // Observations() > 0 blocks its feature  2: every accepted match blocks it
    float th, mbf, nnratio;
    float sf[ORBX_MAX_LEVELS], inv_sigma2[ORBX_MAX_LEVELS];
};

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

// window of a point: radius, level range, cell range; false if the point takes no part
struct Win { float u, v, r; int min_l, max_l, cx0, cx1, cy0, cy1; };

__device__ __forceinline__ bool point_window(const DevFrame &F, const DevPoints &P, const ProjParams &pp, int i, Win *w)
{
    if (!P.valid[i]) return false;
    const float u = P.u[i], v = P.v[i];
    const int lvl = P.level[i] & (ORBX_MAX_LEVELS - 1);
    float r;
    int min_l, max_l;
    if (pp.need_pos_aux && P.aux[i] < 0) return false;                 // invzc < 0 (:1426)
    if (pp.bounds == 1) { if (u < F.min_x || u > F.max_x || v < F.min_y || v > F.max_y) return false; } // :1431-1434
    else if (pp.bounds == 2) { if (!(u >= F.min_x && u < F.max_x && v >= F.min_y && v < F.max_y)) return false; }
    if (pp.radius_mode == 0) {
        r = pp.th * pp.sf[lvl];                                        // :1439
    } else if (pp.radius_mode == 2) {
        r = pp.th;                                                     // SearchForInitialization's windowSize (:461)
    } else {
        float rr = (double)P.view_cos[i] > 0.998 ? 2.5f : 4.0f;        // RadiusByViewingCos (:131-137)
        if ((double)pp.th != 1.0) rr *= pp.th;                         // bFactor (:52, :66-67)
        r = rr * pp.sf[lvl];
    }
    if (pp.direction == 1) { min_l = lvl; max_l = -1; }                // bForward  (:1443)
    else if (pp.direction == 2) { min_l = 0; max_l = lvl; }            // bBackward (:1445)
    else { min_l = lvl + pp.lo_off; max_l = lvl + pp.hi_off; }
    // GetFeaturesInArea cell range (src/Frame.cc:391-406)
    const int a = (int)floorf((u - F.min_x - r) * F.inv_w);
    const int cx0 = a > 0 ? a : 0;
    if (cx0 >= PG_COLS) return false;
    int cx1 = (int)ceilf((u - F.min_x + r) * F.inv_w);
    cx1 = cx1 < PG_COLS - 1 ? cx1 : PG_COLS - 1;
    if (cx1 < 0) return false;
    const int b = (int)floorf((v - F.min_y - r) * F.inv_h);
    const int cy0 = b > 0 ? b : 0;
    if (cy0 >= PG_ROWS) return false;
    int cy1 = (int)ceilf((v - F.min_y + r) * F.inv_h);
    cy1 = cy1 < PG_ROWS - 1 ? cy1 : PG_ROWS - 1;
    if (cy1 < 0) return false;
    w->u = u; w->v = v; w->r = r; w->min_l = min_l; w->max_l = max_l;
    w->cx0 = cx0; w->cx1 = cx1; w->cy0 = cy0; w->cy1 = cy1;
    return true;
}

// claim-independent part of the candidate test: level range, box, right-image coordinate
__device__ __forceinline__ bool cand_ok(const DevFrame &F, const DevPoints &P, const ProjParams &pp, const Win &w, int i, int k)
{
    if (pp.claims && F.occupied[k]) return false;   // the feature holds an observed map point: skipped by every point (:80-82, :1453-1455); filtered here, once, not in every round of the resolve kernel
    const int oct = F.octave[k];
    if (w.min_l > 0 || w.max_l >= 0) { // bCheckLevels (:408)
        if (oct < w.min_l) return false;
        if (w.max_l >= 0 && oct > w.max_l) return false;
    }
    const float distx = F.x[k] - w.u, disty = F.y[k] - w.v;
    if (!(fabsf(distx) < w.r && fabsf(disty) < w.r)) return false; // :434
    const float ur_k = F.u_right[k];
    if (pp.ur_mode && ur_k > 0) {
        if (pp.ur_mode == 1) {
            const float ur = w.u - pp.mbf * P.aux[i];                  // :1467-1471
            if (fabsf(ur - ur_k) > w.r) return false;
        } else {
            if (fabsf(P.aux[i] - ur_k) > w.r) return false;            // :88-92 (r * scale == w.r)
        }
    }
    if (pp.chi2) {                                                     // Fuse, :961-992 (float products, double compare)
        const float inv = pp.inv_sigma2[oct & (ORBX_MAX_LEVELS - 1)];
        const float ex = -distx, ey = -disty;
        if (ur_k >= 0) {
            const float er = P.aux[i] - ur_k;
            const float e2 = ex * ex + ey * ey + er * er;
            if ((double)(e2 * inv) > 7.8) return false;
        } else {
            const float e2 = ex * ex + ey * ey;
            if ((double)(e2 * inv) > 5.99) return false;
        }
    }
    return true;
}

// ---- the window walk of one point by one wave, shared by k_proj_lists and k_window_best.  For a fixed grid column ix the cells
// (ix, cy0..cy1) are consecutive in the CSR (cells are stored column by column), so the window is a handful of contiguous index runs
// whose concatenation is exactly GetFeaturesInArea's traversal order (ix, iy, position in cell).  Lane q fetches the run of column
// cx0 + q (the grid has 64 columns), a wave prefix sum flattens the runs, and the candidates are then taken 64 at a time ACROSS columns
// -- in the order the column-by-column walk had (the order decides every tie downstream).  That walk was four dependent memory round
// trips per column; this is four per point.
// Returns upper, the window's total run length (wave-uniform).  admit(upper) is asked once, when upper > 0, whether the walk takes place
// (k_proj_lists reserves its pool space there).  visit(ok, jf, k, dist) is then called once per 64-candidate chunk on ALL lanes (a
// visitor may ballot): jf = the lane's position in the flattened candidate sequence, ok = the position exists and the candidate passed
// cand_ok; then k is the feature and dist its Hamming distance to the point's descriptor (loaded once, before the chunks).
template <typename Admit, typename Visit>
__device__ __forceinline__ int window_walk(const DevFrame &F, const int *__restrict__ cell_off, const int *__restrict__ cell_idx,
                                           const DevPoints &P, const ProjParams &pp, const Win &w, int i, int lane, Admit admit, Visit visit)
{
    const int ncol = w.cx1 - w.cx0 + 1;
    int c_lo = 0, c_n = 0;
    if (lane < ncol) {
        const int ix = w.cx0 + lane;
        c_lo = cell_off[ix * PG_ROWS + w.cy0];
        c_n = cell_off[ix * PG_ROWS + w.cy1 + 1] - c_lo;
    }
    const int c_incl = wave_incl_scan(c_n), c_excl = c_incl - c_n;
    const int upper = __builtin_amdgcn_readlane(c_incl, 63);
    if (!upper || !admit(upper)) return upper;
    uint32_t d[8];
    const uint4 *s = reinterpret_cast<const uint4 *>(P.desc + (long long)i * 8);
    const uint4 q0 = s[0], q1 = s[1];
    d[0] = q0.x; d[1] = q0.y; d[2] = q0.z; d[3] = q0.w; d[4] = q1.x; d[5] = q1.y; d[6] = q1.z; d[7] = q1.w;
    for (int jb = 0; jb < upper; jb += 64) {
        const int jf = jb + lane;            // position in the flattened candidate sequence
        int j = -1;
        for (int q = 0; q < ncol; q++) {     // which column's run holds it (a handful of columns; their runs ride in lanes 0 .. ncol - 1)
            const int e_ = __builtin_amdgcn_readlane(c_excl, q), n_ = __builtin_amdgcn_readlane(c_n, q), l_ = __builtin_amdgcn_readlane(c_lo, q);
            if (jf >= e_ && jf < e_ + n_) j = l_ + (jf - e_);
        }
        bool ok = false;
        int k = -1, dist = 0;
        if (jf < upper) {
            k = cell_idx[j];
            if (cand_ok(F, P, pp, w, i, k)) {
                ok = true;
                const uint4 *t = reinterpret_cast<const uint4 *>(F.desc + (long long)k * 8);
                const uint4 v0 = t[0], v1 = t[1];
                const uint32_t e[8] = { v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w };
                dist = hamming256(d, e);
            }
        }
        visit(ok, jf, k, dist);
    }
    return upper;
}

// Candidate list of every point, one wave per point: the survivors of the window walk are appended behind a ballot, which keeps
// the walk's order (entry = feature | dist<<16 | octave<<25).  The wave reserves the window's total run length in the pool with
// one atomicAdd (an upper bound of its list); beg[i] / cnt[i] locate the list.  If the pool overflows the host
// grows it and repeats the call (pool_used = entries needed).
__global__ __launch_bounds__(256) void k_proj_lists(DevFrame F, DevPoints P, ProjParams pp, const int *__restrict__ cell_off,
                                                    const int *__restrict__ cell_idx, int *__restrict__ beg, int *__restrict__ cnt,
                                                    uint32_t *__restrict__ entries, int pool_cap, int *__restrict__ pool_used)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= P.n) return; // wave-uniform
    Win w;
    int n = 0, base = 0;
    if (point_window(F, P, pp, i, &w)) {
        window_walk(F, cell_off, cell_idx, P, pp, w, i, lane,
            [&](int upper) {
                if (lane == 0) base = atomicAdd(pool_used, upper);
                base = __builtin_amdgcn_readfirstlane(base);
                return base + upper <= pool_cap;   // overflow: no entry is written, the host repeats the call with a larger pool
            },
            [&](bool ok, int, int k, int dist) {
                const unsigned long long m = __ballot(ok);
                if (ok) entries[base + n + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0))] =
                    (uint32_t)k | ((uint32_t)dist << 16) | ((uint32_t)(F.octave[k] & 31) << 25);
                n += __popcll(m);
            });
    }
    if (lane == 0) { beg[i] = base; cnt[i] = n; }
}

// the claim fixpoint + output, one workgroup.  owner[] (the earliest observed point currently choosing each
// feature) lives in LDS; points below the first index that changed in a round are final and are not evaluated again.
extern __shared__ __align__(16) int resolve_smem[];

__global__ __launch_bounds__(1024) void k_proj_resolve(DevFrame F, DevPoints P, ProjParams pp, const int *__restrict__ beg,
                                                       const int *__restrict__ cnt, const uint32_t *__restrict__ entries,
                                                       int *__restrict__ choice_a, int *__restrict__ choice_b,
                                                       int32_t *__restrict__ match, int *__restrict__ out_n,
                                                       int32_t *__restrict__ pt_choice, int32_t *__restrict__ pt_dist)
{
    __shared__ int s_first, s_cnt;
    __shared__ int hist[30];
    __shared__ int keep3[3];
    int *owner = resolve_smem; // [F.n]
    const int tid = threadIdx.x, nt = 1024;
    int *cur = choice_a, *nxt = choice_b;
    for (int i = tid; i < P.n; i += nt) { cur[i] = -1; nxt[i] = -1; }
    __threadfence_block();
    __syncthreads();
    int stable = 0; // points [0, stable) are final
    for (int round = 0; round <= P.n; round++) {
        for (int f = tid; f < F.n; f += nt) owner[f] = 0x7FFFFFFF;
        if (tid == 0) s_first = 0x7FFFFFFF;
        __syncthreads();
        for (int i = tid; i < P.n; i += nt)
            if (cur[i] >= 0 && pp.claims && (pp.claims == 2 || P.has_obs[i])) atomicMin(&owner[cur[i]], i);
        __syncthreads();
        int first = 0x7FFFFFFF;
        for (int i = stable + tid; i < P.n; i += nt) {
            int b1 = 256, b2 = 256, l1 = -1, l2 = -1, bi = -1;
            const int e0 = beg[i], e1 = e0 + cnt[i];
            for (int eb = e0; eb < e1; eb += 8) {      // eight entries per trip: their loads travel together (one by one the walk was a memory round trip per entry and round)
                uint32_t en8[8];
#pragma unroll
                for (int q = 0; q < 8; q++) en8[q] = eb + q < e1 ? entries[eb + q] : 0xFFFFFFFFu;
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const uint32_t en = en8[q];
                    if (eb + q >= e1) break;
                    const int f = en & 0xFFFF, dist = (en >> 16) & 0x1FF, lv = en >> 25;
                    if (pp.claims && owner[f] < i) continue; // the feature is held by an earlier point (see ProjParams::claims; occupied features never enter the lists)
                    if (dist < b1) { b2 = b1; l2 = l1; b1 = dist; l1 = lv; bi = f; }
                    else if (dist < b2) { b2 = dist; l2 = lv; }
                }
            }
            int c = -1;
            if (b1 <= pp.max_dist) {
                if (!pp.ratio) c = bi;
                else if (!(l1 == l2 && (float)b1 > pp.nnratio * (float)b2)) c = bi; // :117-121
            }
            nxt[i] = c;
            pt_dist[i] = c >= 0 ? b1 : 256; // final once the point is stable: an unchanged choice keeps its distance
            if (c != cur[i] && i < first) first = i;
        }
        if (first != 0x7FFFFFFF) atomicMin(&s_first, first);
        for (int i = tid; i < stable; i += nt) nxt[i] = cur[i]; // the stable prefix keeps its choices in both buffers
        __threadfence_block();
        __syncthreads();
        const int fc = s_first;
        { int *t = cur; cur = nxt; nxt = t; }
        __syncthreads();
        if (fc == 0x7FFFFFFF) break;
        stable = fc; // nothing below the first change moved: those points depend only on earlier ones and are final
    }
    // ---- outputs: a feature ends up with the LAST point that chose it (:1488 overwrites); every choice counts
    for (int f = tid; f < F.n; f += nt) match[f] = -1;
    if (tid < 30) hist[tid] = 0;
    if (tid == 0) s_cnt = 0;
    __threadfence_block();
    __syncthreads();
    int local = 0;
    for (int i = tid; i < P.n; i += nt) {
        const int f = cur[i];
        pt_choice[i] = f;
        if (f < 0) continue;
        atomicMax(&match[f], i);
        local++;
        if (pp.check_ori) {
            const int bin = rot_bin(P.angle[i], F.angle[f]);   // :1493-1500
            atomicAdd(&hist[bin], 1);
            nxt[i] = bin;
        }
    }
    if (local) atomicAdd(&s_cnt, local);
    __threadfence_block();
    __syncthreads();
    if (pp.check_ori) {
        if (tid == 0) {
            int i1, i2, i3;
            three_maxima(hist, &i1, &i2, &i3);
            keep3[0] = i1; keep3[1] = i2; keep3[2] = i3;
        }
        __syncthreads();
        int removed = 0;
        for (int i = tid; i < P.n; i += nt) {
            const int f = cur[i];
            if (f < 0) continue;
            const int b = nxt[i];
            if (b != keep3[0] && b != keep3[1] && b != keep3[2]) { match[f] = pp.mark_cleared ? -2 : -1; pt_choice[i] = -1; removed++; } // :1518-1523, one decrement per entry
        }
        if (removed) atomicSub(&s_cnt, removed);
        __threadfence_block();
        __syncthreads();
    }
    if (tid == 0) *out_n = s_cnt;
}

// ORBmatcher::SearchForInitialization's matching loop (src/ORBmatcher.cc:447-511) is sequential by construction: a
// candidate is skipped when the match it already holds is at least as good (vMatchedDistance, :470) and an accepted
// match steals the feature from its previous holder (:491-496).  The candidate lists with their distances come from
// k_proj_lists (all pairs in parallel); this kernel replays the decisions in order with ONE wave: per point a
// coalesced sweep over its list, the two smallest distances and the first position of the minimum by wave
// reductions, then the scalar bookkeeping.  md / m21 (vMatchedDistance, vnMatches21) live in LDS.
__global__ __launch_bounds__(64) void k_init_resolve(DevFrame F, DevPoints P, ProjParams pp, const int *__restrict__ beg,
                                                     const int *__restrict__ cnt, const uint32_t *__restrict__ entries,
                                                     int *__restrict__ bins, int32_t *__restrict__ pt_choice,
                                                     int32_t *__restrict__ pt_dist, int *__restrict__ out_n)
{
    uint16_t *md = reinterpret_cast<uint16_t *>(resolve_smem);          // [F.n] 0xFFFF = INT_MAX
    uint16_t *m21 = md + ((F.n + 7) & ~7);                               // [F.n] holder + 1, 0 = none
    float *fang = reinterpret_cast<float *>(m21 + ((F.n + 7) & ~7));     // [F.n] the frame's keypoint angles (read per accepted match)
    __shared__ int hist[30];
    const int lane = threadIdx.x;
    for (int f = lane; f < F.n; f += 64) { md[f] = 0xFFFF; m21[f] = 0; fang[f] = pp.check_ori ? F.angle[f] : 0.f; }
    for (int i = lane; i < P.n; i += 64) { pt_choice[i] = -1; pt_dist[i] = 256; bins[i] = -1; }
    if (lane < 30) hist[lane] = 0;
    __threadfence_block();
    __syncthreads();
    int nm = 0;
    // The walk is sequential, its memory traffic need not be: list heads (cnt, beg) are fetched 64 points at a time and handed out by
    // v_readlane, and while point j is decided the first two 64-entry chunks of the NEXT point with a list are already on their way
    // (a point's list is ~80 entries at 1000-2000 features and the reference's window of 100 px).  The per-point chain is then two wave
    // minima, the LDS look-ups and lane 0's bookkeeping -- not three dependent global round trips.  Only LDS state (md, m21, hist) orders
    // the points; the global result arrays are written as we go and read back after the walk, behind one fence.
    for (int base = 0; base < P.n; base += 64) {
        const int ip = base + lane;
        const int my_cnt = ip < P.n ? cnt[ip] : 0, my_beg = ip < P.n ? beg[ip] : 0;
        const float my_ang = ip < P.n && pp.check_ori ? P.angle[ip] : 0.f;
        unsigned long long todo = __ballot(my_cnt > 0);
        uint32_t nx0 = 0, nx1 = 0;                              // chunks 0 and 1 of the next point's list
        if (todo) {
            const int j = (int)__builtin_ctzll(todo);
            const int c = __builtin_amdgcn_readlane(my_cnt, j), e0 = __builtin_amdgcn_readlane(my_beg, j);
            if (lane < c) nx0 = entries[e0 + lane];
            if (64 + lane < c) nx1 = entries[e0 + 64 + lane];
        }
        while (todo) {
            const int j = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            const int i1 = base + j;
            const int c = __builtin_amdgcn_readlane(my_cnt, j), e0 = __builtin_amdgcn_readlane(my_beg, j);
            const uint32_t en0 = nx0, en1 = nx1;
            if (todo) {                                         // the next point's chunks leave now
                const int jn = (int)__builtin_ctzll(todo);
                const int cn = __builtin_amdgcn_readlane(my_cnt, jn), en_ = __builtin_amdgcn_readlane(my_beg, jn);
                nx0 = lane < cn ? entries[en_ + lane] : 0u;
                nx1 = 64 + lane < cn ? entries[en_ + 64 + lane] : 0u;
            }
            unsigned k1 = 0xFFFFFFFFu, d2 = 0x7FFFFFFFu; // lane-local: smallest (dist<<16 | position), second smallest distance
            for (int eb = 0; eb < c; eb += 64) {
                const int e = eb + lane;
                if (e < c) {
                    const uint32_t en = eb == 0 ? en0 : eb == 64 ? en1 : entries[e0 + e];
                    const unsigned f = en & 0xFFFF, d = (en >> 16) & 0x1FF;
                    if (!(md[f] <= d)) {                                   // :470
                        const unsigned key = (d << 16) | (unsigned)e;     // lists are shorter than 65536 (host check)
                        if (key < k1) { d2 = k1 >> 16; k1 = key; }
                        else if (d < d2) d2 = d;
                    }
                }
            }
            if (k1 == 0xFFFFFFFFu) d2 = 0x7FFFFFFFu; else if (d2 == 0xFFFFu) d2 = 0x7FFFFFFFu;
            const unsigned best = wave_min_u32(k1);
            // second smallest over the wave: the winner lane contributes its own second, every other lane its first
            const unsigned mine = (k1 == best) ? d2 : (k1 == 0xFFFFFFFFu ? 0x7FFFFFFFu : (k1 >> 16));
            const unsigned second = wave_min_u32(mine);
            if (best == 0xFFFFFFFFu) continue;
            const int bd = (int)(best >> 16), be = (int)(best & 0xFFFF);
            if (bd <= 50 && (float)bd < (float)(int)second * pp.nnratio) {  // TH_LOW (:485), ratio (:487)
                // the winning entry sits in a register of lane be % 64 (chunks 0 / 1) or, beyond them, in memory
                const uint32_t wen = be < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)en0, be) : be < 128 ? (uint32_t)__builtin_amdgcn_readlane((int)en1, be - 64) : entries[e0 + be];
                const int f = (int)(wen & 0xFFFF);
                if (lane == 0) {
                    const int prev = (int)m21[f] - 1;
                    if (prev >= 0) pt_choice[prev] = -1;                   // :489-493
                    pt_choice[i1] = f; pt_dist[i1] = bd;
                    m21[f] = (uint16_t)(i1 + 1); md[f] = (uint16_t)bd;
                    if (pp.check_ori) {
                        const int bin = rot_bin(__uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(my_ang), j)), fang[f]);   // :501-509
                        hist[bin]++; bins[i1] = bin;
                    }
                }
                // lane 0's LDS writes before the next point's LDS reads: one wave, in-order LDS -- a compiler barrier is all it takes
                // (the workgroup fence that stood here also waited for the global stores: a memory round trip per accepted match)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    // nmatches = matches still standing (every steal removed one, :492), then the orientation filter (:514-541)
    int i1k = -1, i2k = -1, i3k = -1;
    if (pp.check_ori) three_maxima(hist, &i1k, &i2k, &i3k);
    int local = 0;
    for (int i = lane; i < P.n; i += 64) {
        if (pt_choice[i] < 0) continue;
        if (pp.check_ori) {
            const int b = bins[i];
            if (b != i1k && b != i2k && b != i3k) { pt_choice[i] = -1; continue; }
        }
        local++;
    }
    nm = wave_sum(local);
    if (lane == 0) *out_n = nm;
}

// ---- independent points against resident keyframes (Fuse x2 :873-1164, each direction of SearchBySim3 :1218-1372): with
// ProjParams::claims == 0 a point's answer is the first minimum of its own candidate list, so list and decision fuse into ONE kernel --
// no pool, no atomics, no second launch -- and one launch serves many (keyframe, points) jobs.  Job j owns the workgroups
// wg_first[j] .. wg_first[j + 1] (four points each, one wave per point, as k_proj_lists); the job table lives in device memory and is
// found by a wave-uniform search.  The window, the level range and the walk (window_walk) are those of k_proj_lists; instead of
// appending the survivors every lane keeps its smallest (dist << 16 | position in GetFeaturesInArea's traversal), dist <= 256 and
// position < 65536 (a frame holds fewer features than that), and one wave minimum gives the reference's strict '<' (:995-999): the
// smallest distance and, among equals, the FIRST candidate in traversal order.
struct WinJob {
    DevFrame F;
    const int *cell_off, *cell_idx;
    DevPoints P;
    ProjParams pp;       // th, chi2, max_dist, sf[], inv_sigma2[] of the job; bounds = 2, levels [level - 1, level], claims = 0
    int out_off;         // the job's first entry in best_idx / best_dist
};

__global__ __launch_bounds__(256) void k_window_best(const WinJob *__restrict__ jobs, const int *__restrict__ wg_first, int njobs,
                                                     int32_t *__restrict__ best_idx, int32_t *__restrict__ best_dist)
{
    const int wg = blockIdx.x;
    int lo = 0, hi = njobs;                 // the last job with wg_first[j] <= wg (jobs without workgroups are passed over)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (wg_first[mid] <= wg) lo = mid; else hi = mid;
    }
    const WinJob &J = jobs[lo];
    const int i = (wg - wg_first[lo]) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= J.P.n) return; // wave-uniform
    unsigned key = 0xFFFFFFFFu;             // lane-local: smallest (dist << 16 | position), and the feature it belongs to
    int key_k = -1;
    Win w;
    if (point_window(J.F, J.P, J.pp, i, &w)) {
        window_walk(J.F, J.cell_off, J.cell_idx, J.P, J.pp, w, i, lane, [](int) { return true; },
            [&](bool ok, int jf, int k, int dist) {
                const unsigned nk = ((unsigned)dist << 16) | (unsigned)jf;
                if (ok && nk < key) { key = nk; key_k = k; }   // a lane's positions ascend: '<' keeps its first minimum
            });
    }
    const unsigned best = wave_min_u32(key);
    int out_k = -1, out_d = 256;
    if (best != 0xFFFFFFFFu && (int)(best >> 16) <= J.pp.max_dist) {
        const int src = (int)__builtin_ctzll(__ballot(key == best));   // positions are unique: exactly one lane holds the minimum
        out_k = __builtin_amdgcn_readlane(key_k, src);
        out_d = (int)(best >> 16);
    }
    if (lane == 0) { best_idx[J.out_off + i] = out_k; best_dist[J.out_off + i] = out_d; }
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
struct FrustumArgs {
    float R[9], t[3], Ow[3];
    float fx, fy, cx, cy, mbf, min_x, min_y, max_x, max_y;
    float view_cos_limit;
    int nlevels;
    float thr[ORBX_MAX_LEVELS - 1];   // [nlevels - 1] used
};
// what k_frustum writes: the arrays of a dense DevPoints (aux = xr, valid = in_view).  has_obs / desc are NULL for orbx_mappoints_frustum.
struct FrustumOut {
    float *u, *v, *xr, *view_cos;
    int32_t *level;
    uint8_t *in_view, *has_obs;
    uint4 *desc;
};

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

struct ProjCtx : ThreadCtx {
    uint8_t *h_blob = nullptr; size_t h_cap = 0;   // the staging blob, pinned
    uint8_t *d_blob = nullptr; size_t d_cap = 0;
    uint8_t *d_work = nullptr; size_t work_cap = 0;
    uint32_t *d_entries = nullptr; size_t ent_cap = 0;   // bytes, like every capacity here
    int32_t *h_out = nullptr; size_t out_cap = 0;
    int32_t *h_n = nullptr;    // pinned: the feature count a frame created from extraction outputs reads back
    void release()
    {
        if (orbx_ctx_leave(this)) {
            if (h_blob) (void)hipHostFree(h_blob);
            if (d_blob) (void)hipFree(d_blob);
            if (d_work) (void)hipFree(d_work);
            if (d_entries) (void)hipFree(d_entries);
            if (h_out) (void)hipHostFree(h_out);
            if (h_n) (void)hipHostFree(h_n);
        }
        h_blob = d_blob = d_work = nullptr; d_entries = nullptr; h_out = h_n = nullptr;
        h_cap = d_cap = work_cap = ent_cap = out_cap = 0;
    }
    ~ProjCtx() { release(); }
};
static thread_local ProjCtx g_proj[ORBX_MAX_DEVICES];
void orbx_proj_thread_release() { for (ProjCtx &c : g_proj) c.release(); }

// the staging blob of one call: [frame arrays (host-pointer calls only)] [occupied] [point arrays], one upload
static int proj_blob_reserve(ProjCtx *c, size_t blob)
{
    int rc = ORBX_OK;
    if (blob > c->h_cap) rc = ensure_pinned(&c->h_blob, &c->h_cap, 2 * blob);
    if (!rc && blob > c->d_cap) rc = ensure(&c->d_blob, &c->d_cap, 2 * blob);
    return rc;
}
// ---- the arrays of a frame, as they lie in a resident frame's block and, up to o_coff, at the head of a host-pointer call's staging
// blob: x[n] y[n] octave[n] angle[n] u_right[n] desc[n][32] | cell_off[3073] cell_idx[n]
struct FrameLayout { size_t o_x, o_y, o_oct, o_ang, o_ur, o_desc, o_coff, o_cidx, bytes; };

static FrameLayout frame_layout(size_t nc)
{
    FrameLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += a16(bytes); return r; };
    L.o_x = take(4 * nc); L.o_y = take(4 * nc); L.o_oct = take(4 * nc); L.o_ang = take(4 * nc); L.o_ur = take(4 * nc);
    L.o_desc = take(32 * nc); L.o_coff = take(4 * (PG_CELLS + 1)); L.o_cidx = take(4 * nc);
    L.bytes = o;
    return L;
}

// the DevFrame of n features laid out by L behind `base` (a device address), image bounds b = min_x, min_y, max_x, max_y; occupied is
// the search's to set
static DevFrame dev_frame(const uint8_t *base, const FrameLayout &L, int n, const float b[4])
{
    DevFrame F;
    F.n = n; F.x = (const float *)(base + L.o_x); F.y = (const float *)(base + L.o_y); F.octave = (const int32_t *)(base + L.o_oct);
    F.angle = (const float *)(base + L.o_ang); F.u_right = (const float *)(base + L.o_ur); F.desc = (const uint32_t *)(base + L.o_desc);
    F.occupied = nullptr;
    F.min_x = b[0]; F.min_y = b[1]; F.max_x = b[2]; F.max_y = b[3];
    F.inv_w = (float)PG_COLS / (b[2] - b[0]);  // src/Frame.cc:164-165
    F.inv_h = (float)PG_ROWS / (b[3] - b[1]);
    return F;
}

static size_t proj_tail_bytes(size_t nc, size_t np) { return a16(nc) + 6 * a16(4 * np) + a16(32 * np) + 2 * a16(np); }

// ---- part 1 of a host-pointer search: the frame's arrays into the head of the staging blob (frame_layout(n).o_coff bytes); the DevFrame
// addresses them where the upload of part 2 will put them (the grid is then built by part 2 into its work area)
static DevFrame proj_stage_frame(ProjCtx *c, const orbx_frame_feats *cur)
{
    const size_t nc = (size_t)cur->n;
    const FrameLayout L = frame_layout(nc);
    uint8_t *h = c->h_blob;
    memcpy(h + L.o_x, cur->x, 4 * nc); memcpy(h + L.o_y, cur->y, 4 * nc); memcpy(h + L.o_oct, cur->octave, 4 * nc);
    if (cur->angle) memcpy(h + L.o_ang, cur->angle, 4 * nc); else memset(h + L.o_ang, 0, 4 * nc);
    memcpy(h + L.o_ur, cur->u_right, 4 * nc); memcpy(h + L.o_desc, cur->desc, 32 * nc);
    const float b[4] = { cur->min_x, cur->min_y, cur->max_x, cur->max_y };
    return dev_frame(c->d_blob, L, cur->n, b);
}

// ---- the arrays of a point set into a staging blob at *o (advanced; sub-blocks in the order of DevPoints): u v level valid always, of
// the others those that `want` names.  A wanted array the caller left NULL reads 0 (has_obs: 1).  The DevPoints addresses them behind
// `d`, where the upload will put them; an array not wanted is NULL there.
enum { PT_AUX = 1, PT_ANGLE = 2, PT_VIEW_COS = 4, PT_DESC = 8, PT_HAS_OBS = 16, PT_ALL = 31 };

static DevPoints points_stage(uint8_t *h, const uint8_t *d, size_t *o, const orbx_proj_points *p, unsigned want)
{
    const size_t np = (size_t)p->n;
    auto put = [&](bool wanted, const void *src, size_t bytes, int absent) -> const uint8_t * {
        if (!wanted) return nullptr;
        const size_t at = *o;
        *o += a16(bytes);
        if (src) memcpy(h + at, src, bytes); else memset(h + at, absent, bytes);
        return d + at;
    };
    DevPoints P;
    P.n = p->n;
    P.u = (const float *)put(true, p->u, 4 * np, 0); P.v = (const float *)put(true, p->v, 4 * np, 0);
    P.aux = (const float *)put(want & PT_AUX, p->aux, 4 * np, 0);
    P.level = (const int32_t *)put(true, p->level, 4 * np, 0);
    P.angle = (const float *)put(want & PT_ANGLE, p->angle, 4 * np, 0);
    P.view_cos = (const float *)put(want & PT_VIEW_COS, p->view_cos, 4 * np, 0);
    P.desc = (const uint32_t *)put(want & PT_DESC, p->desc, 32 * np, 0);
    P.valid = put(true, p->valid, np, 0);
    P.has_obs = put(want & PT_HAS_OBS, p->has_obs, np, 1);
    return P;
}

// ---- the resident map-point table (include/orbx.h: orbx_mappoints).  ONE device allocation made at creation: geom[capacity][8] |
// desc[capacity][32] | the staging of one upload of orbx_mappoints_set, MP_STAGE_RECORDS records at most (a larger set goes in several
// uploads); nothing grows.  An upload is packed by its own record count, slots[k] | geom[k][8] | desc[k][32] with a half not given left
// out, so what crosses PCIe is 4 + 32 or 4 + 64 bytes per record sent, whatever the capacity.
// Host state: which halves every slot has been given, and the event of the most recent _set.  A _set holds `mu` exclusively while it
// enqueues, a search holds it shared until its stream has drained: a slot is never rewritten under a search in flight, and a search on
// another stream than the _set's waits for the event, not for the device.
#define MP_STAGE_RECORDS 65536
struct orbx_mappoints {
    int device, capacity;
    uint8_t *d_blob;
    float4 *d_geom; uint4 *d_desc;
    uint8_t *d_stage, *h_stage;          // h_stage: pinned, as large as d_stage
    int stage_records; size_t st_bytes;  // records one upload holds; bytes of the staging
    std::vector<uint8_t> have;           // bit 0: geom given, bit 1: desc given; 3 = set
    std::vector<uint32_t> stamp; uint32_t gen;   // duplicate slots of one _set
    mutable hipEvent_t ev; mutable hipStream_t ev_stream; mutable bool ev_set;
    mutable std::shared_timed_mutex mu;
};

// the points of orbx_frame_search_local_points: slots of a resident table, in view or not by k_frustum -- nothing but the slot and a flag
// byte per point is staged, the dense DevPoints is written on the device (into the work area)
struct LocalPts {
    const orbx_mappoints *m;
    const int32_t *slots;
    const uint8_t *flags;
    int n;
    FrustumArgs A;
    uint8_t *in_view;   // [n] out
};

// ---- part 2: occupied + points staged behind `head` bytes, one upload of the whole blob, the grid build when the frame is not resident
// (grid == NULL), lists, resolve, download.  F.occupied is set here (it points into the blob).  lp != NULL: the points are lp's (pts is
// NULL) and k_frustum runs in front of the lists.
static int proj_search(ProjCtx *c, DevFrame F, size_t head, const int *grid_off, const int *grid_idx, const uint8_t *occupied,
                       const orbx_proj_points *pts, const float *sf, int nlevels, const ProjParams &pp_in, int32_t *match_cur,
                       int *nmatches, const float *inv_sigma2, int32_t *pt_choice, int32_t *pt_dist, const LocalPts *lp = nullptr)
{
    const size_t nc = (size_t)F.n, np = (size_t)(lp ? lp->n : pts->n);
    const size_t blob = head + (lp ? a16(nc) + a16(4 * np) + a16(np) : proj_tail_bytes(nc, np));
    int rc = proj_blob_reserve(c, blob);
    if (rc) return rc;
    uint8_t *h = c->h_blob;
    const uint8_t *d = c->d_blob;
    size_t o = head + a16(nc);
    if (occupied) memcpy(h + head, occupied, nc); else memset(h + head, 0, nc);
    F.occupied = d + head;
    DevPoints P;
    size_t o_slots = 0, o_flags = 0;
    if (lp) {
        o_slots = o; o += a16(4 * np); o_flags = o; o += a16(np);
        memcpy(h + o_slots, lp->slots, 4 * np); memcpy(h + o_flags, lp->flags, np);
        memset(&P, 0, sizeof P);
        P.n = lp->n;            // its arrays: in the work area, below
    } else {
        P = points_stage(h, d, &o, pts, PT_ALL);
    }
    ORBX_HIP(hipMemcpyAsync(c->d_blob, h, blob, hipMemcpyHostToDevice, c->stream));
    ProjParams pp = pp_in;
    for (int i = 0; i < ORBX_MAX_LEVELS; i++) {
        pp.sf[i] = i < nlevels ? sf[i] : 0.f;
        pp.inv_sigma2[i] = (inv_sigma2 && i < nlevels) ? inv_sigma2[i] : 0.f;
    }
    // work: cell_off[3073] | cell_idx[nc] | beg[np] | cnt[np] | pool_used | choice_a[np] | choice_b[np] | match[nc] | out_n |
    //       pt_choice[np] | pt_dist[np] | (lp: valid[np] u v aux level view_cos has_obs desc of the DevPoints k_frustum writes)
    size_t w = 0;
    auto wtake = [&](size_t bytes) { const size_t r = w; w += a16(bytes); return r; };
    const size_t w_coff = wtake(4 * (PG_CELLS + 1)), w_cidx = wtake(4 * nc), w_beg = wtake(4 * np), w_cnt = wtake(4 * np), w_used = wtake(16),
                 w_ca = wtake(4 * np), w_cb = wtake(4 * np), w_match = wtake(4 * nc), w_n = wtake(16), w_pc = wtake(4 * np),
                 w_pd = wtake(4 * np);
    FrustumOut fo;
    memset(&fo, 0, sizeof fo);
    size_t w_valid = 0, w_lp[7] = { 0 };
    if (lp) {
        w_valid = wtake(np);
        for (int q = 0; q < 5; q++) w_lp[q] = wtake(4 * np);
        w_lp[5] = wtake(np); w_lp[6] = wtake(32 * np);
    }
    const size_t out = sizeof(int32_t) * (nc + 2 * np + 8) + (lp ? a16(np) : 0);
    if (w > c->work_cap && (rc = ensure(&c->d_work, &c->work_cap, 2 * w))) return rc;
    if (out > c->out_cap && (rc = ensure_pinned(&c->h_out, &c->out_cap, 2 * out))) return rc;
    const size_t resolve_lds = pp.init_search ? (2 * sizeof(uint16_t) + sizeof(float)) * ((nc + 7) & ~(size_t)7) + 16 : sizeof(int) * (nc + 4);   // init: md, m21, the frame's angles
    if (resolve_lds > 150 * 1024 || (pp.init_search && np >= 65535)) { orbx_set_error("too many features for one search"); return ORBX_E_INVALID; }
    if (pp.init_search)
        ORBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_init_resolve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)resolve_lds));
    else
        ORBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_proj_resolve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)resolve_lds));
    uint8_t *wk = c->d_work;
    int *d_beg = (int *)(wk + w_beg), *d_cnt = (int *)(wk + w_cnt), *d_used = (int *)(wk + w_used);
    if (lp) {
        fo.in_view = wk + w_valid; fo.u = (float *)(wk + w_lp[0]); fo.v = (float *)(wk + w_lp[1]); fo.xr = (float *)(wk + w_lp[2]);
        fo.level = (int32_t *)(wk + w_lp[3]); fo.view_cos = (float *)(wk + w_lp[4]); fo.has_obs = wk + w_lp[5]; fo.desc = (uint4 *)(wk + w_lp[6]);
        P.u = fo.u; P.v = fo.v; P.aux = fo.xr; P.level = fo.level; P.view_cos = fo.view_cos; P.valid = fo.in_view; P.has_obs = fo.has_obs;
        P.desc = (const uint32_t *)fo.desc;
        hipLaunchKernelGGL(k_frustum, dim3((lp->n + 255) / 256), dim3(256), 0, c->stream, lp->m->d_geom, lp->m->d_desc,
                           (const int32_t *)(d + o_slots), d + o_flags, lp->n, lp->A, fo);
    }
    const int *d_coff = grid_off, *d_cidx = grid_idx;
    if (!grid_off) {   // a host-pointer frame: Frame::AssignFeaturesToGrid, once per call
        d_coff = (int *)(wk + w_coff); d_cidx = (int *)(wk + w_cidx);
        hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(256), 0, c->stream, F, (int *)(wk + w_coff), (int *)(wk + w_cidx));
    }
    // entry pool: grown on demand, the lists and the resolve are simply repeated after an overflow
    if (!c->d_entries && (rc = ensure(&c->d_entries, &c->ent_cap, sizeof(uint32_t) << 20))) return rc;
    for (int attempt = 0; attempt < 2; attempt++) {
        ORBX_HIP(hipMemsetAsync(d_used, 0, 16, c->stream));
        hipLaunchKernelGGL(k_proj_lists, dim3((P.n + 3) / 4), dim3(256), 0, c->stream, F, P, pp, d_coff, d_cidx, d_beg, d_cnt,
                           c->d_entries, (int)(c->ent_cap / sizeof(uint32_t)), d_used);
        if (pp.init_search)
            hipLaunchKernelGGL(k_init_resolve, dim3(1), dim3(64), resolve_lds, c->stream, F, P, pp, d_beg, d_cnt, c->d_entries,
                               (int *)(wk + w_ca), (int32_t *)(wk + w_pc), (int32_t *)(wk + w_pd), (int *)(wk + w_n));
        else
            hipLaunchKernelGGL(k_proj_resolve, dim3(1), dim3(1024), resolve_lds, c->stream, F, P, pp, d_beg, d_cnt, c->d_entries,
                               (int *)(wk + w_ca), (int *)(wk + w_cb), (int32_t *)(wk + w_match), (int *)(wk + w_n),
                               (int32_t *)(wk + w_pc), (int32_t *)(wk + w_pd));
        ORBX_HIP(hipGetLastError());
        ORBX_HIP(hipMemcpyAsync(c->h_out, wk + w_match, 4 * nc, hipMemcpyDeviceToHost, c->stream));
        ORBX_HIP(hipMemcpyAsync(c->h_out + nc, wk + w_n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        ORBX_HIP(hipMemcpyAsync(c->h_out + nc + 1, d_used, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (pt_choice) ORBX_HIP(hipMemcpyAsync(c->h_out + nc + 8, wk + w_pc, 4 * np, hipMemcpyDeviceToHost, c->stream));
        if (pt_dist) ORBX_HIP(hipMemcpyAsync(c->h_out + nc + 8 + np, wk + w_pd, 4 * np, hipMemcpyDeviceToHost, c->stream));
        if (lp && attempt == 0) ORBX_HIP(hipMemcpyAsync(c->h_out + nc + 8 + 2 * np, wk + w_valid, np, hipMemcpyDeviceToHost, c->stream));
        ORBX_HIP(hipStreamSynchronize(c->stream));
        const size_t used = (size_t)(unsigned)c->h_out[nc + 1];
        if (used <= c->ent_cap / sizeof(uint32_t)) break;
        if (attempt == 1) { orbx_set_error("candidate pool overflow"); return ORBX_E_CAPACITY; }
        if ((rc = ensure(&c->d_entries, &c->ent_cap, sizeof(uint32_t) * used * 2))) return rc;
    }
    memcpy(match_cur, c->h_out, 4 * nc);
    *nmatches = c->h_out[nc];
    if (pt_choice) memcpy(pt_choice, c->h_out + nc + 8, 4 * np);
    if (pt_dist) memcpy(pt_dist, c->h_out + nc + 8 + np, 4 * np);
    if (lp) memcpy(lp->in_view, c->h_out + nc + 8 + 2 * np, np);
    return ORBX_OK;
}

// the refusals of a point set against a parameter block, for every search: its size (worded as `who`'s invalid argument), the arrays the
// block makes the kernels read, the level of every valid point.  job >= 0: the set belongs to that job of a batch.
static int points_check(const orbx_proj_points *p, const ProjParams &pp, int nlevels, const char *who, int job)
{
    char pre[32] = "", pre_pt[32] = "";
    auto name_job = [&] { if (job >= 0) { snprintf(pre, sizeof pre, "job %d: ", job); snprintf(pre_pt, sizeof pre_pt, "job %d, ", job); } };   // on a refusal only
    if (!p || p->n < 0 || p->n > (1 << 20)) { name_job(); orbx_set_error("%s: %sinvalid argument", who, pre); return ORBX_E_INVALID; }
    const bool need_aux = pp.need_pos_aux || pp.ur_mode || pp.chi2;
    if (p->n && (!p->u || !p->v || !p->level || !p->desc || !p->valid || (need_aux && !p->aux) || (pp.claims == 1 && !p->has_obs) ||
                 (pp.check_ori && !p->angle) || (pp.radius_mode == 1 && !p->view_cos))) { name_job(); orbx_set_error("%spoint arrays missing", pre); return ORBX_E_INVALID; }
    for (int i = 0; i < p->n; i++)
        if (p->valid[i] && (p->level[i] < 0 || p->level[i] >= nlevels)) { name_job(); orbx_set_error("%spoint %d: level %d out of range", pre_pt, i, p->level[i]); return ORBX_E_INVALID; }
    return ORBX_OK;
}

static int proj_run(int device, const orbx_frame_feats *cur, const orbx_proj_points *pts, const float *sf, int nlevels,
                    const ProjParams &pp_in, int32_t *match_cur, int *nmatches, const float *inv_sigma2 = nullptr,
                    int32_t *pt_choice = nullptr, int32_t *pt_dist = nullptr)
{
    int nm_dummy = 0;
    std::vector<int32_t> mc_dummy;
    if (!nmatches) nmatches = &nm_dummy;
    if (!match_cur && cur && cur->n >= 0) { mc_dummy.resize((size_t)cur->n + 1); match_cur = mc_dummy.data(); }
    if (!cur || !pts || !sf || !match_cur || !nmatches || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || cur->n < 0 || cur->n >= 65536) {
        orbx_set_error("search_by_projection: invalid argument");
        return ORBX_E_INVALID;
    }
    if (cur->n && (!cur->x || !cur->y || !cur->octave || !cur->u_right || !cur->desc || (pp_in.check_ori && !cur->angle) ||
                   (pp_in.claims && !cur->occupied))) { orbx_set_error("frame arrays missing"); return ORBX_E_INVALID; }
    int rc = points_check(pts, pp_in, nlevels, "search_by_projection", -1);
    if (rc) return rc;
    if (pp_in.chi2 && !inv_sigma2) { orbx_set_error("inv_sigma2 missing"); return ORBX_E_INVALID; }
    if (!(cur->max_x > cur->min_x) || !(cur->max_y > cur->min_y)) { orbx_set_error("empty image bounds"); return ORBX_E_INVALID; }
    for (int i = 0; i < cur->n; i++) match_cur[i] = -1;
    *nmatches = 0;
    for (int i = 0; i < pts->n; i++) { if (pt_choice) pt_choice[i] = -1; if (pt_dist) pt_dist[i] = 256; }
    if (cur->n == 0 || pts->n == 0) return ORBX_OK;
    ProjCtx *c;
    rc = orbx_ctx_get(g_proj, device, &c);
    if (rc) return rc;
    const size_t head = frame_layout((size_t)cur->n).o_coff;
    rc = proj_blob_reserve(c, head + proj_tail_bytes((size_t)cur->n, (size_t)pts->n));
    if (rc) return rc;
    const DevFrame F = proj_stage_frame(c, cur);                                   // part 1
    return proj_search(c, F, head, nullptr, nullptr, cur->occupied, pts, sf, nlevels, pp_in, match_cur, nmatches, inv_sigma2,
                       pt_choice, pt_dist);                                        // part 2
}

// the parameter blocks of the three per-frame searches (shared by the host-pointer and the resident entry points)
static ProjParams params_last_frame(float th, int direction, float mbf, int check_orientation)
{
    ProjParams pp;
    memset(&pp, 0, sizeof pp);
    pp.radius_mode = 0; pp.bounds = 1; pp.need_pos_aux = 1; pp.lo_off = -1; pp.hi_off = 1; pp.direction = direction;
    pp.ur_mode = 1; pp.max_dist = 100; pp.check_ori = check_orientation & 1; pp.mark_cleared = (check_orientation >> 1) & 1; pp.claims = 1;
    pp.th = th; pp.mbf = mbf;
    return pp;
}
static ProjParams params_map_points(float th, float nnratio)
{
    ProjParams pp;
    memset(&pp, 0, sizeof pp);
    pp.radius_mode = 1; pp.lo_off = -1; pp.hi_off = 0; pp.ur_mode = 2; pp.max_dist = 100; pp.ratio = 1; pp.claims = 1;
    pp.th = th; pp.nnratio = nnratio;
    return pp;
}
static ProjParams params_keyframe(float th, int orb_dist, int check_orientation)
{
    ProjParams pp;
    memset(&pp, 0, sizeof pp);
    pp.bounds = 1; pp.lo_off = -1; pp.hi_off = 1; pp.max_dist = orb_dist; pp.check_ori = check_orientation & 1; pp.mark_cleared = (check_orientation >> 1) & 1; pp.claims = 2;
    pp.th = th;
    return pp;
}

static ProjParams params_sim3(float th)   // SearchByProjection(KeyFrame, Scw, ...), :305-415
{
    ProjParams pp;
    memset(&pp, 0, sizeof pp);
    pp.bounds = 2; pp.lo_off = -1; pp.hi_off = 0; pp.max_dist = 50; pp.claims = 2;
    pp.th = th;
    return pp;
}
static ProjParams params_window(float th, int chi2, int max_dist)   // Fuse x2 and each direction of SearchBySim3: independent points
{
    ProjParams pp;
    memset(&pp, 0, sizeof pp);
    pp.bounds = 2; pp.lo_off = -1; pp.hi_off = 0; pp.max_dist = max_dist; pp.chi2 = chi2 ? 1 : 0; pp.claims = 0;
    pp.th = th;
    return pp;
}

// the agreement check of SearchBySim3 (:1375-1391) on the two directions' best candidates
static int sim3_agree(const int32_t *m1, const int32_t *m2, int n1, int32_t *match12)
{
    int found = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        const int idx2 = m1[i1];
        match12[i1] = -1;
        if (idx2 >= 0 && m2[idx2] == i1) { match12[i1] = idx2; found++; }
    }
    return found;
}

extern "C" int orbx_search_by_projection_last_frame(int device, const orbx_frame_feats *cur, const orbx_proj_points *pts,
                                                    const float *scale_factors, int nlevels, float th, int direction, float mbf,
                                                    int check_orientation, int32_t *match_cur, int *nmatches)
{
    if (direction < 0 || direction > 2) { orbx_set_error("direction must be 0 (none), 1 (forward) or 2 (backward)"); return ORBX_E_INVALID; }
    return proj_run(device, cur, pts, scale_factors, nlevels, params_last_frame(th, direction, mbf, check_orientation), match_cur, nmatches);
}

extern "C" int orbx_search_by_projection_map_points(int device, const orbx_frame_feats *cur, const orbx_proj_points *pts,
                                                    const float *scale_factors, int nlevels, float th, float nnratio,
                                                    int32_t *match_cur, int *nmatches)
{
    return proj_run(device, cur, pts, scale_factors, nlevels, params_map_points(th, nnratio), match_cur, nmatches);
}

extern "C" int orbx_search_by_projection_keyframe(int device, const orbx_frame_feats *cur, const orbx_proj_points *pts,
                                                  const float *scale_factors, int nlevels, float th, int orb_dist,
                                                  int check_orientation, int32_t *match_cur, int *nmatches)
{
    return proj_run(device, cur, pts, scale_factors, nlevels, params_keyframe(th, orb_dist, check_orientation), match_cur, nmatches);
}

extern "C" int orbx_search_by_projection_sim3(int device, const orbx_frame_feats *kf, const orbx_proj_points *pts,
                                              const float *scale_factors, int nlevels, float th, int32_t *match_kf, int *nmatches)
{
    return proj_run(device, kf, pts, scale_factors, nlevels, params_sim3(th), match_kf, nmatches);
}

extern "C" int orbx_window_best(int device, const orbx_frame_feats *kf, const orbx_proj_points *pts, const float *scale_factors,
                                const float *inv_sigma2, int nlevels, float th, int chi2, int max_dist, int32_t *best_idx,
                                int32_t *best_dist, int *nfound)
{
    if (!best_idx || max_dist < 0 || max_dist > 256) { orbx_set_error("orbx_window_best: invalid argument"); return ORBX_E_INVALID; }
    return proj_run(device, kf, pts, scale_factors, nlevels, params_window(th, chi2, max_dist), nullptr, nfound, inv_sigma2, best_idx, best_dist);
}

extern "C" int orbx_search_for_initialization(int device, const orbx_frame_feats *f1, const orbx_frame_feats *f2,
                                              const float *prev_matched_xy, int window_size, float nnratio, int check_orientation,
                                              int32_t *matches12, int *nmatches)
{
    if (!f1 || !f2 || !prev_matched_xy || !matches12 || !nmatches || f1->n < 0 || window_size < 0) {
        orbx_set_error("orbx_search_for_initialization: invalid argument");
        return ORBX_E_INVALID;
    }
    if (f1->n && (!f1->octave || !f1->desc || (check_orientation && !f1->angle))) { orbx_set_error("frame arrays missing"); return ORBX_E_INVALID; }
    const size_t n1 = (size_t)f1->n;
    std::vector<float> u(n1 + 1), v(n1 + 1);
    std::vector<int32_t> lvl(n1 + 1, 0);
    std::vector<uint8_t> valid(n1 + 1);
    for (size_t i = 0; i < n1; i++) {
        u[i] = prev_matched_xy[2 * i]; v[i] = prev_matched_xy[2 * i + 1];
        valid[i] = f1->octave[i] > 0 ? 0 : 1;                          // :451-453
    }
    orbx_proj_points pts;
    memset(&pts, 0, sizeof pts);
    pts.n = f1->n; pts.u = u.data(); pts.v = v.data(); pts.level = lvl.data(); pts.angle = f1->angle; pts.desc = f1->desc;
    pts.valid = valid.data();
    ProjParams pp;
    memset(&pp, 0, sizeof pp);
    pp.radius_mode = 2; pp.lo_off = 0; pp.hi_off = 0; pp.max_dist = 50; pp.check_ori = check_orientation; pp.init_search = 1;
    pp.th = (float)window_size; pp.nnratio = nnratio;
    const float sf1[1] = { 1.0f };
    return proj_run(device, f2, &pts, sf1, 1, pp, nullptr, nmatches, nullptr, matches12, nullptr);
}

extern "C" int orbx_search_by_sim3(int device, const orbx_frame_feats *kf1, const orbx_frame_feats *kf2,
                                   const orbx_proj_points *pts12, const orbx_proj_points *pts21, const float *scale_factors1,
                                   const float *scale_factors2, int nlevels, float th, int32_t *match12, int *nfound)
{
    if (!kf1 || !kf2 || !pts12 || !pts21 || !match12 || !nfound || pts12->n != kf1->n || pts21->n != kf2->n) {
        orbx_set_error("orbx_search_by_sim3: invalid argument (one projected point per keypoint on each side)");
        return ORBX_E_INVALID;
    }
    std::vector<int32_t> m1((size_t)pts12->n + 1), m2((size_t)pts21->n + 1);
    int n1 = 0, n2 = 0;
    int rc = orbx_window_best(device, kf2, pts12, scale_factors2, nullptr, nlevels, th, 0, 100, m1.data(), nullptr, &n1); // :1218-1292
    if (rc) return rc;
    rc = orbx_window_best(device, kf1, pts21, scale_factors1, nullptr, nlevels, th, 0, 100, m2.data(), nullptr, &n2);     // :1295-1372
    if (rc) return rc;
    *nfound = sim3_agree(m1.data(), m2.data(), pts12->n, match12);
    return ORBX_OK;
}

// ---------------------------------------------------------------- resident current frame (include/orbx.h: orbx_frame)

// Frame blocks and their events are recycled: a frame lives one frame time, and hipFree would synchronise the device every frame.  A block
// returns to its device's pool only after the work that wrote it has completed (its event).
struct FrameBlock { uint8_t *d = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; };
static std::mutex g_fpool_mu;
static std::vector<FrameBlock> g_fpool[16];
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

struct orbx_frame : FrameLayout {   // the block's layout: frame_layout(n)
    int device, n, has_angle;
    float bounds[4];   // min_x, min_y, max_x, max_y
    FrameBlock blk;
    bool pending;   // the creation may still be running: the first search waits for blk.ev on its own stream
    std::vector<int32_t> h_oct;   // a frame made from host pointers keeps its octaves: orbx_frame_pose_optimize checks them before any device work
    // orbx_frame_set_depth: mvDepth and the raw positions in one allocation of the frame's own (raw == nullptr: x / y); has_stereo = some
    // u_right >= 0 as far as the host saw them, from_extraction = it saw none
    float *d_depth = nullptr, *d_raw_x = nullptr, *d_raw_y = nullptr;
    bool depth_set = false, has_stereo = false, from_extraction = false;
};

static DevFrame frame_dev(const orbx_frame *f) { return dev_frame(f->blk.d, *f, f->n, f->bounds); }

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
    ProjCtx *c;
    int rc = orbx_ctx_get(g_proj, device, &c);
    if (rc) return rc;
    orbx_frame *f = frame_new(device, cur->n, cur->n == 0 || cur->angle ? 1 : 0, cur->min_x, cur->min_y, cur->max_x, cur->max_y);
    rc = frame_block_get(device, f->bytes, &f->blk);
    if (rc) { delete f; return rc; }
    // the frame arrays of the block are the head of a host-pointer call's staging blob (one frame_layout): part 1 stages them, one upload
    rc = proj_blob_reserve(c, f->o_coff);
    if (!rc) {
        const DevFrame F = frame_dev(f);
        if (cur->n) {
            proj_stage_frame(c, cur);
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
    ProjCtx *c;
    int rc = orbx_ctx_get(g_proj, device, &c);
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

// the resident twin of proj_run: the same point validation; the frame's arrays and grid come from its block, only part 2 runs
// (the handle is only read: *synced says whether the search ran, and with it synchronised behind the frame's creation)
static int proj_run_resident(const orbx_frame *f, const uint8_t *occupied, const orbx_proj_points *pts, const float *sf, int nlevels,
                             const ProjParams &pp, int32_t *match_cur, int *nmatches, bool *synced)
{
    *synced = false;
    if (!f || !pts || !sf || !match_cur || !nmatches || nlevels < 1 || nlevels > ORBX_MAX_LEVELS) {
        orbx_set_error("orbx_frame_search_by_projection: invalid argument");
        return ORBX_E_INVALID;
    }
    if (pp.check_ori && !f->has_angle) { orbx_set_error("orbx_frame_search_by_projection: the frame was created without angles"); return ORBX_E_INVALID; }
    int rc = points_check(pts, pp, nlevels, "orbx_frame_search_by_projection", -1);
    if (rc) return rc;
    for (int i = 0; i < f->n; i++) match_cur[i] = -1;
    *nmatches = 0;
    if (f->n == 0 || pts->n == 0) return ORBX_OK;
    ProjCtx *c;
    rc = orbx_ctx_get(g_proj, f->device, &c);
    if (rc) return rc;
    if (f->pending) ORBX_HIP(hipStreamWaitEvent(c->stream, f->blk.ev, 0));   // the creation, ordered by its event (no device synchronisation)
    const uint8_t *d = f->blk.d;
    rc = proj_search(c, frame_dev(f), 0, (const int *)(d + f->o_coff), (const int *)(d + f->o_cidx), occupied, pts, sf, nlevels, pp,
                     match_cur, nmatches, nullptr, nullptr, nullptr);
    if (!rc) *synced = true;
    return rc;
}

// the per-frame searches: one thread at a time on a frame, so the search that synchronised behind the creation may say so in the handle
static int proj_run_resident_own(orbx_frame *f, const uint8_t *occupied, const orbx_proj_points *pts, const float *sf, int nlevels,
                                 const ProjParams &pp, int32_t *match_cur, int *nmatches)
{
    bool synced;
    const int rc = proj_run_resident(f, occupied, pts, sf, nlevels, pp, match_cur, nmatches, &synced);
    if (synced) f->pending = false;
    return rc;
}

extern "C" int orbx_frame_search_by_projection_last_frame(orbx_frame *cur, const uint8_t *occupied, const orbx_proj_points *pts,
                                                          const float *scale_factors, int nlevels, float th, int direction, float mbf,
                                                          int check_orientation, int32_t *match_cur, int *nmatches)
{
    if (direction < 0 || direction > 2) { orbx_set_error("direction must be 0 (none), 1 (forward) or 2 (backward)"); return ORBX_E_INVALID; }
    return proj_run_resident_own(cur, occupied, pts, scale_factors, nlevels, params_last_frame(th, direction, mbf, check_orientation), match_cur, nmatches);
}

extern "C" int orbx_frame_search_by_projection_map_points(orbx_frame *cur, const uint8_t *occupied, const orbx_proj_points *pts,
                                                          const float *scale_factors, int nlevels, float th, float nnratio,
                                                          int32_t *match_cur, int *nmatches)
{
    return proj_run_resident_own(cur, occupied, pts, scale_factors, nlevels, params_map_points(th, nnratio), match_cur, nmatches);
}

extern "C" int orbx_frame_search_by_projection_keyframe(orbx_frame *cur, const uint8_t *occupied, const orbx_proj_points *pts,
                                                        const float *scale_factors, int nlevels, float th, int orb_dist,
                                                        int check_orientation, int32_t *match_cur, int *nmatches)
{
    return proj_run_resident_own(cur, occupied, pts, scale_factors, nlevels, params_keyframe(th, orb_dist, check_orientation), match_cur, nmatches);
}

// ---------------------------------------------------------------- resident keyframes: Fuse, SearchBySim3, Sim3 SearchByProjection
// A keyframe's keypoints and descriptors never change (src/KeyFrame.cc:29-60): an orbx_frame serves as the keyframe.  These calls only
// read the handle, so LocalMapping and LoopClosing may search one keyframe at the same time; the staging is the calling thread's ProjCtx.

extern "C" int orbx_frame_search_by_projection_sim3(const orbx_frame *kf, const uint8_t *occupied, const orbx_proj_points *pts,
                                                    const float *scale_factors, int nlevels, float th, int32_t *match_kf, int *nmatches)
{
    bool synced;
    return proj_run_resident(kf, occupied, pts, scale_factors, nlevels, params_sim3(th), match_kf, nmatches, &synced);
}

// the refusals of one job, before any device call and without reading the handle
static int window_job_check(const orbx_window_job &jb, int j)
{
    if (!jb.kf || !jb.pts || !jb.scale_factors || !jb.best_idx || jb.nlevels < 1 || jb.nlevels > ORBX_MAX_LEVELS || jb.max_dist < 0 ||
        jb.max_dist > 256) {
        orbx_set_error("orbx_frame_window_best: job %d: invalid argument", j);
        return ORBX_E_INVALID;
    }
    const int rc = points_check(jb.pts, params_window(jb.th, jb.chi2, jb.max_dist), jb.nlevels, "orbx_frame_window_best", j);
    if (rc) return rc;
    if (jb.chi2 && !jb.inv_sigma2) { orbx_set_error("job %d: inv_sigma2 missing", j); return ORBX_E_INVALID; }
    return ORBX_OK;
}

extern "C" int orbx_frame_window_best_batch(orbx_window_job *jobs, int njobs)
{
    if (!jobs || njobs < 1 || njobs > 1024) { orbx_set_error("orbx_frame_window_best_batch: 1 to 1024 jobs"); return ORBX_E_INVALID; }
    size_t total_in = 0;
    for (int j = 0; j < njobs; j++) {
        const int rc = window_job_check(jobs[j], j);
        if (rc) return rc;
        total_in += (size_t)jobs[j].pts->n;
    }
    if (total_in > ((size_t)1 << 20)) { orbx_set_error("orbx_frame_window_best_batch: more than 2^20 points in one call"); return ORBX_E_INVALID; }
    const int device = jobs[0].kf->device;
    for (int j = 1; j < njobs; j++)
        if (jobs[j].kf->device != device) { orbx_set_error("orbx_frame_window_best_batch: the keyframes live on different devices"); return ORBX_E_INVALID; }
    // jobs with work, their workgroups and output offsets; the points' staging: u v [aux] level valid per job (points_stage), descriptors once per
    // distinct host array (the jobs of one FuseBatch share the map points' descriptors)
    std::vector<int> wg_first((size_t)njobs + 1, 0);
    std::vector<size_t> o_desc((size_t)njobs, 0);
    size_t blob = a16(sizeof(WinJob) * (size_t)njobs);
    const size_t o_wg = blob;
    blob += a16(sizeof(int) * ((size_t)njobs + 1));
    size_t total = 0;
    for (int j = 0; j < njobs; j++) {
        orbx_window_job &jb = jobs[j];
        jb.nfound = 0;
        const size_t np = (size_t)jb.pts->n;
        for (size_t i = 0; i < np; i++) { jb.best_idx[i] = -1; if (jb.best_dist) jb.best_dist[i] = 256; }
        const bool work = np && jb.kf->n;
        wg_first[j + 1] = wg_first[j] + (work ? (int)((np + 3) / 4) : 0);
        if (!work) continue;
        total += np;
        int same = -1;
        for (int q = 0; q < j && same < 0; q++)
            if (o_desc[q] && jobs[q].pts->desc == jb.pts->desc && jobs[q].pts->n == jb.pts->n) same = q;
        if (same >= 0) o_desc[j] = o_desc[same];
        else { o_desc[j] = blob; blob += a16(32 * np); }
    }
    if (total == 0) return ORBX_OK;
    ProjCtx *c;
    int rc = orbx_ctx_get(g_proj, device, &c);
    if (rc) return rc;
    const size_t o_pts = blob;
    for (int j = 0; j < njobs; j++)
        if (wg_first[j + 1] > wg_first[j]) { const size_t np = (size_t)jobs[j].pts->n; blob += 3 * a16(4 * np) + a16(np) + (jobs[j].chi2 ? a16(4 * np) : 0); }
    if ((rc = proj_blob_reserve(c, blob))) return rc;
    const size_t out = 2 * sizeof(int32_t) * total;
    if (out > c->work_cap && (rc = ensure(&c->d_work, &c->work_cap, 2 * out))) return rc;
    if (out > c->out_cap && (rc = ensure_pinned(&c->h_out, &c->out_cap, 2 * out))) return rc;
    uint8_t *h = c->h_blob;
    const uint8_t *d = c->d_blob;
    WinJob *wj = reinterpret_cast<WinJob *>(h);
    memcpy(h + o_wg, wg_first.data(), sizeof(int) * ((size_t)njobs + 1));
    size_t o = o_pts, off = 0;
    bool pending = false;
    for (int j = 0; j < njobs; j++) {
        const orbx_window_job &jb = jobs[j];
        WinJob &W = wj[j];
        memset(&W, 0, sizeof W);
        if (wg_first[j + 1] == wg_first[j]) continue;   // no workgroup reads the record
        const orbx_frame *f = jb.kf;
        const orbx_proj_points *p = jb.pts;
        const size_t np = (size_t)p->n;
        W.P = points_stage(h, d, &o, p, jb.chi2 ? PT_AUX : 0);
        bool first = true;
        for (int q = 0; q < j; q++) if (o_desc[q] == o_desc[j]) first = false;
        if (first) memcpy(h + o_desc[j], p->desc, 32 * np);
        W.F = frame_dev(f);
        W.cell_off = (const int *)(f->blk.d + f->o_coff); W.cell_idx = (const int *)(f->blk.d + f->o_cidx);
        W.P.desc = (const uint32_t *)(d + o_desc[j]);
        W.pp = params_window(jb.th, jb.chi2, jb.max_dist);
        for (int i = 0; i < ORBX_MAX_LEVELS; i++) {
            W.pp.sf[i] = i < jb.nlevels ? jb.scale_factors[i] : 0.f;
            W.pp.inv_sigma2[i] = (jb.chi2 && i < jb.nlevels) ? jb.inv_sigma2[i] : 0.f;
        }
        W.out_off = (int)off;
        off += np;
        pending = pending || f->pending;
    }
    if (pending)   // a keyframe made from extraction buffers whose creation may still run: ordered by its event, the handle is not written
        for (int j = 0; j < njobs; j++)
            if (wg_first[j + 1] > wg_first[j] && jobs[j].kf->pending) ORBX_HIP(hipStreamWaitEvent(c->stream, jobs[j].kf->blk.ev, 0));
    int32_t *d_idx = (int32_t *)c->d_work, *d_dist = d_idx + total;
    ORBX_HIP(hipMemcpyAsync(c->d_blob, h, blob, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_window_best, dim3(wg_first[njobs]), dim3(256), 0, c->stream, (const WinJob *)d, (const int *)(d + o_wg), njobs, d_idx, d_dist);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(c->h_out, c->d_work, out, hipMemcpyDeviceToHost, c->stream));
    ORBX_HIP(hipStreamSynchronize(c->stream));
    off = 0;
    for (int j = 0; j < njobs; j++) {
        orbx_window_job &jb = jobs[j];
        if (wg_first[j + 1] == wg_first[j]) continue;
        const size_t np = (size_t)jb.pts->n;
        memcpy(jb.best_idx, c->h_out + off, 4 * np);
        if (jb.best_dist) memcpy(jb.best_dist, c->h_out + total + off, 4 * np);
        int nf = 0;
        for (size_t i = 0; i < np; i++) nf += jb.best_idx[i] >= 0;
        jb.nfound = nf;
        off += np;
    }
    return ORBX_OK;
}

extern "C" int orbx_frame_window_best(const orbx_frame *kf, const orbx_proj_points *pts, const float *scale_factors,
                                      const float *inv_sigma2, int nlevels, float th, int chi2, int max_dist, int32_t *best_idx,
                                      int32_t *best_dist, int *nfound)
{
    orbx_window_job jb;
    memset(&jb, 0, sizeof jb);
    jb.kf = kf; jb.pts = pts; jb.scale_factors = scale_factors; jb.inv_sigma2 = inv_sigma2; jb.nlevels = nlevels; jb.th = th;
    jb.chi2 = chi2; jb.max_dist = max_dist; jb.best_idx = best_idx; jb.best_dist = best_dist;
    const int rc = orbx_frame_window_best_batch(&jb, 1);
    if (!rc && nfound) *nfound = jb.nfound;
    return rc;
}

extern "C" int orbx_frame_search_by_sim3(const orbx_frame *kf1, const orbx_frame *kf2, const orbx_proj_points *pts12,
                                         const orbx_proj_points *pts21, const float *scale_factors1, const float *scale_factors2,
                                         int nlevels, float th, int32_t *match12, int *nfound)
{
    if (!kf1 || !kf2 || !pts12 || !pts21 || !match12 || !nfound || pts12->n != kf1->n || pts21->n != kf2->n) {
        orbx_set_error("orbx_frame_search_by_sim3: invalid argument (one projected point per keypoint on each side)");
        return ORBX_E_INVALID;
    }
    std::vector<int32_t> m1((size_t)pts12->n + 1), m2((size_t)pts21->n + 1);
    orbx_window_job jb[2];
    memset(jb, 0, sizeof jb);
    jb[0].kf = kf2; jb[0].pts = pts12; jb[0].scale_factors = scale_factors2; jb[0].best_idx = m1.data();   // :1218-1292
    jb[1].kf = kf1; jb[1].pts = pts21; jb[1].scale_factors = scale_factors1; jb[1].best_idx = m2.data();   // :1295-1372
    for (int j = 0; j < 2; j++) { jb[j].nlevels = nlevels; jb[j].th = th; jb[j].max_dist = 100; }
    const int rc = orbx_frame_window_best_batch(jb, 2);
    if (rc) return rc;
    *nfound = sim3_agree(m1.data(), m2.data(), pts12->n, match12);
    return ORBX_OK;
}

// ---------------------------------------------------------------- resident map points (include/orbx.h: orbx_mappoints)

extern "C" int orbx_mappoints_create(int device, int capacity, orbx_mappoints **out)
{
    if (!out || capacity < 1 || capacity > (1 << 24)) { orbx_set_error("orbx_mappoints_create: invalid argument (1 <= capacity <= 2^24)"); return ORBX_E_INVALID; }
    *out = nullptr;
    ProjCtx *c;
    int rc = orbx_ctx_get(g_proj, device, &c);
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
    ProjCtx *c;
    int rc = orbx_ctx_get(g_proj, m->device, &c);
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

// the refusals of a frustum call, before any launch, and its kernel arguments.  bit0: which bit pattern of flags[i] makes point i eligible
// (orbx_mappoints_frustum: any non-zero byte; the fused search: bit 0)
static int frustum_args(const char *who, const orbx_mappoints *m, const int32_t *slots, const uint8_t *flags, int n, bool any_bit,
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

// a search's stream behind the table's most recent _set (the caller holds m->mu shared)
static int mappoints_order_before(const orbx_mappoints *m, hipStream_t s)
{
    if (m->ev_set && m->ev_stream != s) ORBX_HIP(hipStreamWaitEvent(s, m->ev, 0));
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
    int rc = frustum_args("orbx_mappoints_frustum", m, slots, eligible, n, true, pose, cam, view_cos_limit, log_scale_factor, nlevels, &A);
    if (rc) return rc;
    if (n == 0) return ORBX_OK;
    ProjCtx *c;
    if ((rc = orbx_ctx_get(g_proj, m->device, &c))) return rc;
    const size_t np = (size_t)n, col = a16(4 * np);
    const size_t blob = col + a16(np), out = 5 * col + a16(np);   // up: slots | flags   down: u v xr view_cos level | in_view
    if ((rc = proj_blob_reserve(c, blob))) return rc;
    if (out > c->work_cap && (rc = ensure(&c->d_work, &c->work_cap, 2 * out))) return rc;
    if (out > c->out_cap && (rc = ensure_pinned(&c->h_out, &c->out_cap, 2 * out))) return rc;
    memcpy(c->h_blob, slots, 4 * np);
    for (size_t i = 0; i < np; i++) c->h_blob[col + i] = eligible[i] ? 1 : 0;
    if ((rc = mappoints_order_before(m, c->stream))) return rc;
    ORBX_HIP(hipMemcpyAsync(c->d_blob, c->h_blob, blob, hipMemcpyHostToDevice, c->stream));
    uint8_t *wk = c->d_work;
    FrustumOut fo;
    memset(&fo, 0, sizeof fo);
    fo.u = (float *)wk; fo.v = (float *)(wk + col); fo.xr = (float *)(wk + 2 * col); fo.view_cos = (float *)(wk + 3 * col);
    fo.level = (int32_t *)(wk + 4 * col); fo.in_view = wk + 5 * col;
    hipLaunchKernelGGL(k_frustum, dim3((n + 255) / 256), dim3(256), 0, c->stream, m->d_geom, m->d_desc, (const int32_t *)c->d_blob,
                       c->d_blob + col, n, A, fo);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(c->h_out, wk, out, hipMemcpyDeviceToHost, c->stream));
    ORBX_HIP(hipStreamSynchronize(c->stream));
    const uint8_t *ho = (const uint8_t *)c->h_out;
    if (u) memcpy(u, ho, 4 * np);
    if (v) memcpy(v, ho + col, 4 * np);
    if (xr) memcpy(xr, ho + 2 * col, 4 * np);
    if (view_cos) memcpy(view_cos, ho + 3 * col, 4 * np);
    if (level) memcpy(level, ho + 4 * col, 4 * np);
    memcpy(in_view, ho + 5 * col, np);
    return ORBX_OK;
}

extern "C" int orbx_frame_search_local_points(orbx_frame *cur, const uint8_t *occupied, const orbx_mappoints *m, const int32_t *slots,
                                              const uint8_t *flags, int n, const float *pose, const float *cam, float view_cos_limit,
                                              float log_scale_factor, const float *scale_factors, int nlevels, float th, float nnratio,
                                              int32_t *match_cur, int *nmatches, uint8_t *in_view)
{
    if (!cur || !m || !scale_factors || !match_cur || !nmatches || (n > 0 && !in_view)) {
        orbx_set_error("orbx_frame_search_local_points: invalid argument");
        return ORBX_E_INVALID;
    }
    if (cur->device != m->device) { orbx_set_error("orbx_frame_search_local_points: the frame and the table live on different devices"); return ORBX_E_INVALID; }
    std::shared_lock<std::shared_timed_mutex> lk(m->mu);
    LocalPts lp;
    int rc = frustum_args("orbx_frame_search_local_points", m, slots, flags, n, false, pose, cam, view_cos_limit, log_scale_factor, nlevels, &lp.A);
    if (rc) return rc;
    for (int i = 0; i < cur->n; i++) match_cur[i] = -1;
    *nmatches = 0;
    if (n) memset(in_view, 0, (size_t)n);
    if (cur->n == 0 || n == 0) return ORBX_OK;
    lp.m = m; lp.slots = slots; lp.flags = flags; lp.n = n; lp.in_view = in_view;
    ProjCtx *c;
    if ((rc = orbx_ctx_get(g_proj, cur->device, &c))) return rc;
    if (cur->pending) ORBX_HIP(hipStreamWaitEvent(c->stream, cur->blk.ev, 0));
    if ((rc = mappoints_order_before(m, c->stream))) return rc;
    const uint8_t *d = cur->blk.d;
    rc = proj_search(c, frame_dev(cur), 0, (const int *)(d + cur->o_coff), (const int *)(d + cur->o_cidx), occupied, nullptr, scale_factors,
                     nlevels, params_map_points(th, nnratio), match_cur, nmatches, nullptr, nullptr, nullptr, &lp);
    if (!rc) cur->pending = false;
    return rc;
}

// ---------------------------------------------------------------- Optimizer::PoseOptimization (include/orbx.h: orbx_pose_optimize)
// The kernel and its arithmetic are in orbx_pose.hip; here are the refusals, the staging and the delivery of the three calls.

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
static int pose_reserve(ProjCtx *c, size_t blob, size_t out)
{
    int rc = proj_blob_reserve(c, blob);
    if (!rc && out > c->work_cap) rc = ensure(&c->d_work, &c->work_cap, 2 * out);
    if (!rc && out > c->out_cap) rc = ensure_pinned(&c->h_out, &c->out_cap, 2 * out);
    return rc;
}

static int pose_launch_and_fetch(ProjCtx *c, size_t blob, size_t out, int njobs)
{
    ORBX_HIP(hipMemcpyAsync(c->d_blob, c->h_blob, blob, hipMemcpyHostToDevice, c->stream));
    orbx_pose_launch((const PoseJob *)c->d_blob, (PoseOut *)c->d_work, njobs, c->stream);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(c->h_out, c->d_work, out, hipMemcpyDeviceToHost, c->stream));
    ORBX_HIP(hipStreamSynchronize(c->stream));
    return ORBX_OK;
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
    ProjCtx *c;
    int rc = orbx_ctx_get(g_proj, device, &c);
    if (rc) return rc;
    const size_t jobs_b = a16(sizeof(PoseJob) * (size_t)njobs), outs_b = a16(sizeof(PoseOut) * (size_t)njobs);
    size_t blob = jobs_b, out = outs_b;
    for (int j = 0; j < njobs; j++) {
        const size_t n = (size_t)a[j].obs->n;
        blob += 4 * a16(4 * n) + a16(12 * n) + a16(n);
        out += a16(n);
    }
    if ((rc = pose_reserve(c, blob, out))) return rc;
    uint8_t *h = c->h_blob;
    const uint8_t *d = c->d_blob;
    PoseJob *hj = (PoseJob *)h;
    size_t o = jobs_b, fo = outs_b;
    for (int j = 0; j < njobs; j++) {
        const orbx_pose_obs &ob = *a[j].obs;
        const size_t n = (size_t)ob.n;
        auto put = [&](const void *src, size_t bytes) { const size_t at = o; o += a16(bytes); if (bytes) memcpy(h + at, src, bytes); return d + at; };
        PoseJob &J = hj[j];
        memset(&J, 0, sizeof J);
        J.n = ob.n;
        J.x = (const float *)put(ob.x, 4 * n); J.y = (const float *)put(ob.y, 4 * n); J.u_right = (const float *)put(ob.u_right, 4 * n);
        J.inv_sigma2 = (const float *)put(ob.inv_sigma2, 4 * n); J.Xw = (const float *)put(ob.Xw, 12 * n);
        J.has_point = put(ob.has_point, n);
        J.outlier = c->d_work + fo;
        fo += a16(n);
        memcpy(J.cam, a[j].cam, sizeof J.cam); memcpy(J.Tcw, a[j].Tcw, sizeof J.Tcw);
    }
    if ((rc = pose_launch_and_fetch(c, blob, out, njobs))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    fo = outs_b;
    for (int j = 0; j < njobs; j++) {
        const orbx_pose_obs &ob = *a[j].obs;
        pose_deliver(((const PoseOut *)ho)[j], ho + fo, ob.n, a[j], [&](int i) { return ob.has_point[i] != 0; });
        fo += a16((size_t)ob.n);
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
    ProjCtx *c;
    int rc = orbx_ctx_get(g_proj, cur->device, &c);
    if (rc) return rc;
    const size_t nn = (size_t)n, jobs_b = a16(sizeof(PoseJob)), outs_b = a16(sizeof(PoseOut));
    const size_t blob = jobs_b + a16(4 * nn), out = outs_b + a16(nn);
    if ((rc = pose_reserve(c, blob, out))) return rc;
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
    if (cur->pending) ORBX_HIP(hipStreamWaitEvent(c->stream, cur->blk.ev, 0));   // the handle is not written: every call on a pending frame waits
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

// ---------------------------------------------------------------- CreateNewMapPoints' triangulation (include/orbx.h: orbx_triangulate_pairs)
// The kernels and their arithmetic are in orbx_triangulate.hip; here are the refusals, the staging and the delivery of the two calls.

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

// the refusals both forms share; *total = the pairs of all lists
static int tri_check(const char *who, const TriArgs &a, const TriHostKf &h1, const TriHostKf *h2, size_t *total)
{
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
// stage(H, h_blob, d_blob, offset) fills the TriFeat records (and, for host pointers, the blob behind offset)
template <class Stage>
static int tri_run(const char *who, ProjCtx *c, const TriArgs &a, int n1, size_t total, size_t extra_blob, Stage stage,
                   const orbx_frame *const *wait, int nwait)
{
    *a.n_new = 0;
    if (total == 0) return ORBX_OK;
    const size_t head_b = a16(offsetof(TriHead, nb) + sizeof(TriHead::Nb) * (size_t)a.n2), pairs_b = a16(8 * total);
    const size_t blob = head_b + pairs_b + extra_blob;
    const size_t o_x3d = a16(total), o_bad = o_x3d + a16(12 * total), out = o_bad + 16, work = out + a16(4 * (size_t)n1);
    int rc = proj_blob_reserve(c, blob);
    if (!rc && work > c->work_cap) rc = ensure(&c->d_work, &c->work_cap, 2 * work);
    if (!rc && out > c->out_cap) rc = ensure_pinned(&c->h_out, &c->out_cap, 2 * out);
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
    stage(H, c->h_blob, c->d_blob, head_b + pairs_b);
    for (int i = 0; i < nwait; i++)
        if (wait[i]->pending) ORBX_HIP(hipStreamWaitEvent(c->stream, wait[i]->blk.ev, 0));   // the handles are not written: every call on a pending frame waits
    ORBX_HIP(hipMemcpyAsync(c->d_blob, c->h_blob, blob, hipMemcpyHostToDevice, c->stream));
    // 0x7f7f7f7f: larger than any neighbour index in first[], and not the 1 the kernel writes into the flag
    ORBX_HIP(hipMemsetAsync(c->d_work + o_bad, 0x7f, work - o_bad, c->stream));
    orbx_triangulate_launch((const TriHead *)c->d_blob, (const int32_t *)(c->d_blob + head_b), (int)total, c->d_work, (float *)(c->d_work + o_x3d),
                            (int *)(c->d_work + o_bad), (int *)(c->d_work + out), c->stream);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(c->h_out, c->d_work, out, hipMemcpyDeviceToHost, c->stream));
    ORBX_HIP(hipStreamSynchronize(c->stream));
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
    if (!k1 || !v1 || !k2s || !v2s || !pairs || !npairs || !scale_factors || !level_sigma2 || !status || !x3d || !n_new || n2 < 1 || n2 > 64) {
        orbx_set_error("%s: invalid argument (no NULL argument, 1 <= n2 <= 64)", who);
        return ORBX_E_INVALID;
    }
    auto host_kf = [&](const orbx_tri_feats *k, TriHostKf *h) {
        if (!k || k->n < 0 || (k->n && (!k->x || !k->y || !k->octave || !k->u_right)) || (!k->raw_x) != (!k->raw_y)) return false;
        h->n = k->n; h->octave = k->octave; h->u_right = k->u_right; h->has_depth = k->depth != nullptr;
        return true;
    };
    TriHostKf h1, h2[64];
    bool ok = host_kf(k1, &h1);
    for (int i = 0; ok && i < n2; i++) ok = host_kf(k2s[i], &h2[i]);
    if (!ok) { orbx_set_error("%s: a keyframe is NULL, has n < 0, lacks x / y / octave / u_right or gives one raw array only", who); return ORBX_E_INVALID; }
    const TriArgs a = { n2, cap, nlevels, pairs, npairs, v1, v2s, scale_factors, level_sigma2, ratio_factor, status, x3d, n_new };
    size_t total;
    int rc = tri_check(who, a, h1, h2, &total);
    if (rc) return rc;
    ProjCtx *c;
    if ((rc = orbx_ctx_get(g_proj, device, &c))) return rc;
    auto kf_bytes = [](const orbx_tri_feats *k) { return (size_t)(4 + (k->depth ? 1 : 0) + (k->raw_x ? 2 : 0)) * a16(4 * (size_t)k->n); };
    size_t extra = kf_bytes(k1);
    for (int i = 0; i < n2; i++) extra += kf_bytes(k2s[i]);
    return tri_run(who, c, a, k1->n, total, extra, [&](TriHead &H, uint8_t *h, const uint8_t *d, size_t o) {
        auto put_kf = [&](const orbx_tri_feats *k, TriFeat &f) {
            const size_t b = 4 * (size_t)k->n;
            auto put = [&](const void *src) { const size_t at = o; o += a16(b); if (b) memcpy(h + at, src, b); return (const float *)(d + at); };
            f.x = put(k->x); f.y = put(k->y); f.octave = (const int32_t *)put(k->octave); f.u_right = put(k->u_right);
            f.depth = k->depth ? put(k->depth) : nullptr;
            f.raw_x = k->raw_x ? put(k->raw_x) : f.x; f.raw_y = k->raw_y ? put(k->raw_y) : f.y;
        };
        put_kf(k1, H.f1);
        for (int i = 0; i < n2; i++) put_kf(k2s[i], H.nb[i].f);
    }, nullptr, 0);
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

extern "C" int orbx_frame_triangulate(const orbx_frame *k1, const orbx_tri_view *v1, const orbx_frame *const *k2s, const orbx_tri_view *v2s,
                                      int n2, const int32_t *pairs, int cap, const int *npairs, const float *scale_factors,
                                      const float *level_sigma2, int nlevels, float ratio_factor, uint8_t *status, float *x3d, int *n_new)
{
    const char *who = "orbx_frame_triangulate";
    if (!k1 || !v1 || !k2s || !v2s || !pairs || !npairs || !scale_factors || !level_sigma2 || !status || !x3d || !n_new || n2 < 1 || n2 > 64) {
        orbx_set_error("%s: invalid argument (no NULL argument, 1 <= n2 <= 64)", who);
        return ORBX_E_INVALID;
    }
    const orbx_frame *fr[65];
    TriHostKf h[65];
    fr[0] = k1;
    for (int i = 0; i < n2; i++) fr[1 + i] = k2s[i];
    for (int i = 0; i <= n2; i++) {
        const orbx_frame *f = fr[i];
        if (!f) { orbx_set_error("%s: a NULL frame", who); return ORBX_E_INVALID; }
        if (f->device != k1->device) { orbx_set_error("%s: the frames live on different devices", who); return ORBX_E_INVALID; }
        if ((f->has_stereo || f->from_extraction) && !f->depth_set) {
            orbx_set_error("%s: frame %d has stereo features or comes from an extraction, and no depth (orbx_frame_set_depth)", who, i);
            return ORBX_E_INVALID;
        }
        h[i].n = f->n; h[i].octave = f->h_oct.empty() ? nullptr : f->h_oct.data(); h[i].u_right = nullptr; h[i].has_depth = f->depth_set;
    }
    const TriArgs a = { n2, cap, nlevels, pairs, npairs, v1, v2s, scale_factors, level_sigma2, ratio_factor, status, x3d, n_new };
    size_t total;
    int rc = tri_check(who, a, h[0], h + 1, &total);
    if (rc) return rc;
    ProjCtx *c;
    if ((rc = orbx_ctx_get(g_proj, k1->device, &c))) return rc;
    return tri_run(who, c, a, k1->n, total, 0, [&](TriHead &H, uint8_t *, const uint8_t *, size_t) {
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

// ---------------------------------------------------------------- Sim3Solver's hypotheses (include/orbx.h: orbx_sim3_hypotheses)
// The kernel and its arithmetic are in orbx_sim3.hip; here are the refusals, the staging (the pose optimisation's: one blob up, one
// block down) and the delivery of the two calls.

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
    ProjCtx *c;
    int rc = orbx_ctx_get(g_proj, device, &c);
    if (rc) return rc;
    const size_t jobs_b = a16(sizeof(Sim3Job) * (size_t)njobs);
    size_t blob = jobs_b, out = 0;
    for (int j = 0; j < njobs; j++) {
        const size_t n = (size_t)jobs[j].n, nh = (size_t)jobs[j].n_hyp;
        blob += 2 * a16(12 * n) + 2 * a16(4 * n) + a16(12 * nh);
        out += a16(4 * nh) + a16(52 * nh) + a16(8 * nh * ((n + 63) / 64));
    }
    if ((rc = pose_reserve(c, blob, out))) return rc;
    uint8_t *h = c->h_blob;
    const uint8_t *d = c->d_blob;
    Sim3Job *hj = (Sim3Job *)h;
    size_t o = jobs_b, oo = 0;
    int first = 0;
    for (int j = 0; j < njobs; j++) {
        const orbx_sim3_job &in = jobs[j];
        const size_t n = (size_t)in.n, nh = (size_t)in.n_hyp;
        auto put = [&](const void *src, size_t bytes) { const size_t at = o; o += a16(bytes); memcpy(h + at, src, bytes); return d + at; };
        auto res = [&](size_t bytes) { const size_t at = oo; oo += a16(bytes); return c->d_work + at; };
        Sim3Job &J = hj[j];
        memset(&J, 0, sizeof J);
        J.n = in.n; J.n_hyp = in.n_hyp; J.fix_scale = in.fix_scale ? 1 : 0; J.first = first;
        first += in.n_hyp;
        J.X1 = (const float *)put(in.X1, 12 * n); J.X2 = (const float *)put(in.X2, 12 * n);
        J.max_err1 = (const float *)put(in.max_err1, 4 * n); J.max_err2 = (const float *)put(in.max_err2, 4 * n);
        J.samples = (const int32_t *)put(in.samples, 12 * nh);
        J.n_inliers = (int32_t *)res(4 * nh); J.srt = (float *)res(52 * nh); J.inlier_bits = (uint64_t *)res(8 * nh * ((n + 63) / 64));
        memcpy(J.K1, in.K1, sizeof J.K1); memcpy(J.K2, in.K2, sizeof J.K2);
    }
    ORBX_HIP(hipMemcpyAsync(c->d_blob, c->h_blob, blob, hipMemcpyHostToDevice, c->stream));
    orbx_sim3_launch((const Sim3Job *)c->d_blob, njobs, (int)total, c->stream);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(c->h_out, c->d_work, out, hipMemcpyDeviceToHost, c->stream));
    ORBX_HIP(hipStreamSynchronize(c->stream));
    const uint8_t *ho = (const uint8_t *)c->h_out;
    oo = 0;
    for (int j = 0; j < njobs; j++) {
        const orbx_sim3_job &in = jobs[j];
        const size_t nh = (size_t)in.n_hyp, wb = 8 * nh * (((size_t)in.n + 63) / 64);
        memcpy(in.n_inliers, ho + oo, 4 * nh); oo += a16(4 * nh);
        memcpy(in.srt, ho + oo, 52 * nh); oo += a16(52 * nh);
        memcpy(in.inlier_bits, ho + oo, wb); oo += a16(wb);
    }
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

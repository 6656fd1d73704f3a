// orbx_proj.hip — the projection-guided searches of ORB-SLAM2, seven in all, reference src/ORBmatcher.cc:
//   SearchByProjection(Frame&, const Frame&, th, bMono)                 :1396-1553   last frame
//   SearchByProjection(Frame&, const vector<MapPoint*>&, th)            :48-129      local map points
//   SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)   :1555-1685   relocalisation
//   SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)         :305-415     loop closing
//   Fuse x2 (search half) and each direction of SearchBySim3            :873-1164, :1218-1372   ("window best": independent points)
//   SearchBySim3                                                        :1166-1394
//   SearchForInitialization                                             :430-556
// with Frame::GetFeaturesInArea (src/Frame.cc:386-442) over the grid of Frame::AssignFeaturesToGrid.  The frame and map-point handles,
// the grid build, the frustum pass and the per-thread staging (CallCtx) are orbx_resident.h / orbx_resident.hip.
//
// In file order:
//   device   DevPoints, ProjParams (one parameter block describes every search)
//            a point's window and candidate test: point_window, cand_ok; the window walk both per-point kernels share: window_walk
//            k_proj_lists (candidate lists), k_proj_resolve (claim fixpoint + rotation filter), k_init_resolve (SearchForInitialization)
//            k_window_best (independent points against resident keyframes, many jobs per launch)
//   host     points_stage; proj_search (upload, grid, lists, resolve, download); points_check, proj_run; the parameter blocks params_*;
//            sim3_agree
//            the host-pointer entry points of the seven searches
//            the searches on a resident current frame; the searches on resident keyframes (orbx_frame_window_best_batch and its users)
//            orbx_frame_search_local_points (the map-point search on a resident table, k_frustum in front)
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
#include "orbx_resident.h"
#include <math.h>

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

// ---------------------------------------------------------------- host side

static size_t proj_tail_bytes(size_t nc, size_t np) { return a16(nc) + 6 * a16(4 * np) + a16(32 * np) + 2 * a16(np); }

// ---- the arrays of a point set into a staging blob at cursor b (sub-blocks in the order of DevPoints): u v level valid always, of
// the others those that `want` names.  A wanted array the caller left NULL reads 0 (has_obs: 1).  The DevPoints addresses them where
// the upload will put them; an array not wanted is NULL there.
enum { PT_AUX = 1, PT_ANGLE = 2, PT_VIEW_COS = 4, PT_DESC = 8, PT_HAS_OBS = 16, PT_ALL = 31 };

static DevPoints points_stage(BlobCursor &b, const orbx_proj_points *p, unsigned want)
{
    const size_t np = (size_t)p->n;
    DevPoints P;
    P.n = p->n;
    P.u = (const float *)b.put(p->u, 4 * np); P.v = (const float *)b.put(p->v, 4 * np);
    P.aux = want & PT_AUX ? (const float *)b.put(p->aux, 4 * np) : nullptr;
    P.level = (const int32_t *)b.put(p->level, 4 * np);
    P.angle = want & PT_ANGLE ? (const float *)b.put(p->angle, 4 * np) : nullptr;
    P.view_cos = want & PT_VIEW_COS ? (const float *)b.put(p->view_cos, 4 * np) : nullptr;
    P.desc = want & PT_DESC ? (const uint32_t *)b.put(p->desc, 32 * np) : nullptr;
    P.valid = b.put(p->valid, np);
    P.has_obs = want & PT_HAS_OBS ? b.put(p->has_obs, np, 1) : nullptr;
    return P;
}

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

// ---- the search proper: occupied + points staged behind `head` bytes of the blob (a host-pointer frame's arrays lie there already), one
// upload of the whole blob, the grid build when the frame is not resident (grid == NULL), lists, resolve, download.  F.occupied is set
// here (it points into the blob).  lp != NULL: the points are lp's (pts is NULL) and k_frustum runs in front of the lists.
static int proj_search(CallCtx *c, DevFrame F, size_t head, const int *grid_off, const int *grid_idx, const uint8_t *occupied,
                       const orbx_proj_points *pts, const float *sf, int nlevels, const ProjParams &pp_in, int32_t *match_cur,
                       int *nmatches, const float *inv_sigma2, int32_t *pt_choice, int32_t *pt_dist, const LocalPts *lp = nullptr)
{
    const size_t nc = (size_t)F.n, np = (size_t)(lp ? lp->n : pts->n);
    const size_t blob = head + (lp ? a16(nc) + a16(4 * np) + a16(np) : proj_tail_bytes(nc, np));
    int rc = call_reserve(c, blob, 0, 0);
    if (rc) return rc;
    BlobCursor b = { c->h_blob, c->d_blob, head };
    F.occupied = b.put(occupied, nc);   // NULL: no feature is occupied
    DevPoints P;
    const uint8_t *d_slots = nullptr, *d_flags = nullptr;
    if (lp) {
        d_slots = b.put(lp->slots, 4 * np); d_flags = b.put(lp->flags, np);
        memset(&P, 0, sizeof P);
        P.n = lp->n;            // its arrays: in the work area, below
    } else {
        P = points_stage(b, pts, PT_ALL);
    }
    if ((rc = call_upload(c, blob))) return rc;
    ProjParams pp = pp_in;
    for (int i = 0; i < ORBX_MAX_LEVELS; i++) {
        pp.sf[i] = i < nlevels ? sf[i] : 0.f;
        pp.inv_sigma2[i] = (inv_sigma2 && i < nlevels) ? inv_sigma2[i] : 0.f;
    }
    // work: cell_off[3073] | cell_idx[nc] | beg[np] | cnt[np] | pool_used | choice_a[np] | choice_b[np] | match[nc] | out_n |
    //       pt_choice[np] | pt_dist[np] | (lp: valid[np] u v aux level view_cos has_obs desc of the DevPoints k_frustum writes)
    BlobCursor w = { nullptr, nullptr, 0 };
    const size_t w_coff = w.take(4 * (PG_CELLS + 1)), w_cidx = w.take(4 * nc), w_beg = w.take(4 * np), w_cnt = w.take(4 * np), w_used = w.take(16),
                 w_ca = w.take(4 * np), w_cb = w.take(4 * np), w_match = w.take(4 * nc), w_n = w.take(16), w_pc = w.take(4 * np),
                 w_pd = w.take(4 * np);
    FrustumOut fo;
    memset(&fo, 0, sizeof fo);
    size_t w_valid = 0, w_lp[7] = { 0 };
    if (lp) {
        w_valid = w.take(np);
        for (int q = 0; q < 5; q++) w_lp[q] = w.take(4 * np);
        w_lp[5] = w.take(np); w_lp[6] = w.take(32 * np);
    }
    const size_t out = sizeof(int32_t) * (nc + 2 * np + 8) + (lp ? a16(np) : 0);
    if ((rc = call_reserve(c, 0, w.o, out))) return rc;
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
        orbx_frustum_launch(lp->m, (const int32_t *)d_slots, d_flags, lp->n, lp->A, fo, c->stream);
    }
    const int *d_coff = grid_off, *d_cidx = grid_idx;
    if (!grid_off) {   // a host-pointer frame: Frame::AssignFeaturesToGrid, once per call
        d_coff = (int *)(wk + w_coff); d_cidx = (int *)(wk + w_cidx);
        orbx_grid_build_launch(F, (int *)(wk + w_coff), (int *)(wk + w_cidx), c->stream);
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
    CallCtx *c;
    rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    const size_t head = frame_layout((size_t)cur->n).o_coff;
    rc = call_reserve(c, head + proj_tail_bytes((size_t)cur->n, (size_t)pts->n), 0, 0);
    if (rc) return rc;
    const DevFrame F = frame_stage(c, cur);   // the frame's arrays: the head of the blob
    return proj_search(c, F, head, nullptr, nullptr, cur->occupied, pts, sf, nlevels, pp_in, match_cur, nmatches, inv_sigma2,
                       pt_choice, pt_dist);
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

// the resident twin of proj_run: the same point validation; the frame's arrays and grid come from its block, nothing of it is staged
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
    CallCtx *c;
    rc = orbx_call_ctx(f->device, &c);
    if (rc) return rc;
    if ((rc = frame_order_before(f, c->stream))) return rc;
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
// read the handle, so LocalMapping and LoopClosing may search one keyframe at the same time; the staging is the calling thread's CallCtx.

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
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    const size_t o_pts = blob;
    for (int j = 0; j < njobs; j++)
        if (wg_first[j + 1] > wg_first[j]) { const size_t np = (size_t)jobs[j].pts->n; blob += 3 * a16(4 * np) + a16(np) + (jobs[j].chi2 ? a16(4 * np) : 0); }
    const size_t out = 2 * sizeof(int32_t) * total;
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    uint8_t *h = c->h_blob;
    const uint8_t *d = c->d_blob;
    WinJob *wj = reinterpret_cast<WinJob *>(h);
    memcpy(h + o_wg, wg_first.data(), sizeof(int) * ((size_t)njobs + 1));
    BlobCursor b = { c->h_blob, c->d_blob, o_pts };
    size_t off = 0;
    for (int j = 0; j < njobs; j++) {
        const orbx_window_job &jb = jobs[j];
        WinJob &W = wj[j];
        memset(&W, 0, sizeof W);
        if (wg_first[j + 1] == wg_first[j]) continue;   // no workgroup reads the record
        const orbx_frame *f = jb.kf;
        const orbx_proj_points *p = jb.pts;
        const size_t np = (size_t)p->n;
        W.P = points_stage(b, p, jb.chi2 ? PT_AUX : 0);
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
    }
    for (int j = 0; j < njobs; j++)   // a keyframe made from extraction buffers whose creation may still run (the handle is not written)
        if (wg_first[j + 1] > wg_first[j] && (rc = frame_order_before(jobs[j].kf, c->stream))) return rc;
    int32_t *d_idx = (int32_t *)c->d_work, *d_dist = d_idx + total;
    if ((rc = call_upload(c, blob))) return rc;
    hipLaunchKernelGGL(k_window_best, dim3(wg_first[njobs]), dim3(256), 0, c->stream, (const WinJob *)d, (const int *)(d + o_wg), njobs, d_idx, d_dist);
    if ((rc = call_fetch(c, out))) return rc;
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
    int rc = orbx_frustum_args("orbx_frame_search_local_points", m, slots, flags, n, false, pose, cam, view_cos_limit, log_scale_factor, nlevels, &lp.A);
    if (rc) return rc;
    for (int i = 0; i < cur->n; i++) match_cur[i] = -1;
    *nmatches = 0;
    if (n) memset(in_view, 0, (size_t)n);
    if (cur->n == 0 || n == 0) return ORBX_OK;
    lp.m = m; lp.slots = slots; lp.flags = flags; lp.n = n; lp.in_view = in_view;
    CallCtx *c;
    if ((rc = orbx_call_ctx(cur->device, &c))) return rc;
    if ((rc = frame_order_before(cur, c->stream))) return rc;
    if ((rc = mappoints_order_before(m, c->stream))) return rc;
    const uint8_t *d = cur->blk.d;
    rc = proj_search(c, frame_dev(cur), 0, (const int *)(d + cur->o_coff), (const int *)(d + cur->o_cidx), occupied, nullptr, scale_factors,
                     nlevels, params_map_points(th, nnratio), match_cur, nmatches, nullptr, nullptr, nullptr, &lp);
    if (!rc) cur->pending = false;
    return rc;
}

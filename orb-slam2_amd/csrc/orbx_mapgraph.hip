// orbx_mapgraph.hip — the resident observation graph (include/orbx.h: orbx_mapgraph): who observes what, in both views of the reference,
// edited in small batches and walked by three queries.
//   kernels: k_mg_scatter (every edit: word records, and the attribute bytes of a new keyframe), k_mg_vote (keyframeCounter of
//            Tracking::UpdateLocalKeyFrames, src/Tracking.cc:1515-1538, and KFcounter of KeyFrame::UpdateConnections, src/KeyFrame.cc:303-338),
//            k_mg_judge + k_mg_walk (LocalMapping::KeyFrameCulling, src/LocalMapping.cc:704-775, with the map-point part of
//            KeyFrame::SetBadFlag, src/KeyFrame.cc:505-507, and MapPoint::EraseObservation / SetBadFlag, src/MapPoint.cc:119-176, between
//            its iterations), k_mp_refresh (MapPoint::UpdateNormalAndDepth, src/MapPoint.cc:371-420, and
//            MapPoint::ComputeDistinctiveDescriptors, :266-340, from the rows, the resident keyframes and the map-point table)
//   host:    the handle, its mirror, the edits, the queries, orbx_mapgraph_refresh_points
//
// LAYOUT.  One device allocation: a word space (uint32) kf_n[max_keyframes] | match[max_keyframes][max_features] | hdr[max_points] |
// row[max_points][max_obs], then attr[max_keyframes][max_features] (bytes), then the staging of one edit upload.
//   kf_n   the keyframe's feature count, -1 = the slot is free
//   match  mvpMapPoints[i]: a point slot or -1
//   attr   octave (bits 0-4) | stereo (bit 6) | close (bit 7)
//   hdr    nObs (bits 0-11) | entries in the row (bits 12-20) | live (bit 24) | bad (bit 25)
//   row    mObservations: keyframe slot << 16 | feature index, the first `entries` words of the row, in no particular order
// The host keeps a MIRROR of the word space and of attr.  Every refusal (a full row, a keyframe that is already in a row and so adds
// nothing, a slot named twice) is decided on the mirror, before any device work; an edit is worked out on the mirror as a list of
// (word, value) records, and the device receives the final value of every word the edit touched: one upload, one scatter launch.  The
// queries never read the mirror: they run on the device's copy.  cull_keyframes changes the device's copy by itself, and the host then
// replays the culled keyframes on the mirror (erase_keyframe without an upload) and checks that both name the same bad points.
#include "orbx_resident.h"
#include "orbx_device.h"
#include <algorithm>
#include <mutex>

#define MG_HOLE 0xFFFFFFFFu
#define MG_NOBS(h) ((int)((h) & 0xFFFu))
#define MG_CNT(h) ((int)(((h) >> 12) & 0x1FFu))
#define MG_LIVE 0x01000000u
#define MG_BAD 0x02000000u
#define MG_HDR(nobs, cnt, flags) ((uint32_t)(nobs) | ((uint32_t)(cnt) << 12) | (flags))
#define MG_OCT 0x1Fu
#define MG_STEREO 0x40u
#define MG_CLOSE 0x80u
#define MG_STAGE_RECORDS 65536
#define MG_LDS_KEYFRAMES 8192   // k_mg_vote keeps its histogram in LDS up to this many keyframe slots (32 KiB), beyond it in HBM
#define MG_GROUP 8              // lanes that share one row: its entries are loaded together, MG_GROUP at a time

struct MgDev {
    uint32_t *w; uint8_t *attr;
    size_t a_match, a_hdr, a_row;   // word offsets; kf_n is at 0
    int max_kf, max_feat, max_points, max_obs;
    __host__ __device__ size_t match(int k, int i) const { return a_match + (size_t)k * max_feat + i; }
    __host__ __device__ size_t at(int k, int i) const { return (size_t)k * max_feat + i; }
    __host__ __device__ size_t hdr(int p) const { return a_hdr + p; }
    __host__ __device__ size_t row(int p, int e) const { return a_row + (size_t)p * max_obs + e; }
};

// ---------------------------------------------------------------- kernels

// an edit: nrec (word, value) records, every word named once; and, for a new keyframe, its attribute bytes with every match set to -1
__global__ __launch_bounds__(256) void k_mg_scatter(MgDev G, const uint2 *__restrict__ rec, int nrec, int init_kf, int init_n,
                                                    const uint8_t *__restrict__ init_attr)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < nrec) { const uint2 r = rec[t]; G.w[r.x] = r.y; }
    if (t < init_n) { G.attr[G.at(init_kf, t)] = init_attr[t]; G.w[G.match(init_kf, t)] = 0xFFFFFFFFu; }
}

// counts[observer]++ over the rows of the listed points that are live and not bad, `exclude` left out.  MG_GROUP lanes take one point
// and load MG_GROUP entries of its row at a time.  use_lds: a workgroup histogram of max_kf ints, flushed with integer atomics.
__global__ __launch_bounds__(256) void k_mg_vote(MgDev G, const int32_t *__restrict__ pts, int n, int exclude, int *__restrict__ counts, int use_lds)
{
    extern __shared__ int hist[];
    const int tid = threadIdx.x, sub = tid & (MG_GROUP - 1), grp = tid / MG_GROUP, per = 256 / MG_GROUP;
    if (use_lds) {
        for (int i = tid; i < G.max_kf; i += 256) hist[i] = 0;
        __syncthreads();
    }
    int *dst = use_lds ? hist : counts;
    for (int base = blockIdx.x * per; base < n; base += gridDim.x * per) {
        const int pi = base + grp;
        if (pi >= n) continue;
        const int p = pts[pi];
        if (p < 0 || p >= G.max_points) continue;
        const uint32_t h = G.w[G.hdr(p)];
        if (!(h & MG_LIVE) || (h & MG_BAD)) continue;
        const int cnt = MG_CNT(h);
        for (int e = sub; e < cnt; e += MG_GROUP) {
            const int kf = (int)(G.w[G.row(p, e)] >> 16);
            if (kf != exclude && kf < G.max_kf) atomicAdd(&dst[kf], 1);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int i = tid; i < G.max_kf; i += 256) { const int v = hist[i]; if (v) atomicAdd(&counts[i], v); }
    }
}

// Feature i of keyframe k as KeyFrameCulling sees it (src/LocalMapping.cc:726-766), by the MG_GROUP lanes of one group (sub = the lane's
// place in it; every lane of the wave must call).  counted: the feature adds to nMPs; red: to nRedundantObservations.
__device__ __forceinline__ void mg_judge(const MgDev &G, int k, int i, int nfeat, int mono, int sub, bool &counted, bool &red)
{
    counted = false;
    int c = 0;
    if (i < nfeat) {
        const int p = (int)G.w[G.match(k, i)];
        if (p >= 0) {
            const uint32_t h = G.w[G.hdr(p)];
            const uint32_t a = G.attr[G.at(k, i)];
            if ((h & MG_LIVE) && !(h & MG_BAD) && (mono || (a & MG_CLOSE))) {
                counted = true;
                if (MG_NOBS(h) > 3) {
                    const int cnt = MG_CNT(h), lim = (int)(a & MG_OCT) + 1;
                    for (int e = sub; e < cnt; e += MG_GROUP) {   // the row entry, then that keyframe's octave byte: a group's loads go out together
                        const uint32_t ent = G.w[G.row(p, e)];
                        const int k2 = (int)(ent >> 16), i2 = (int)(ent & 0xFFFFu);
                        if (k2 != k && k2 < G.max_kf && i2 < G.max_feat) c += (int)(G.attr[G.at(k2, i2)] & MG_OCT) <= lim;
                    }
                }
            }
        }
    }
    c += __shfl_xor(c, 1); c += __shfl_xor(c, 2); c += __shfl_xor(c, 4);
    red = counted && c >= 3;
}

// every (local keyframe, feature) on the graph as it stands: grid (feature chunks of 256 / MG_GROUP, n_local)
__global__ __launch_bounds__(256) void k_mg_judge(MgDev G, const int32_t *__restrict__ local, int mono, int *__restrict__ n_mps, int *__restrict__ n_red)
{
    const int j = blockIdx.y, k = local[j], nfeat = (int)G.w[k];
    const int i0 = blockIdx.x * (256 / MG_GROUP);
    if (i0 >= nfeat) return;
    const int tid = threadIdx.x, sub = tid & (MG_GROUP - 1);
    bool counted, red;
    mg_judge(G, k, i0 + tid / MG_GROUP, nfeat, mono, sub, counted, red);
    const int m = __popcll(__ballot(counted && sub == 0)), r = __popcll(__ballot(red && sub == 0));
    if ((tid & 63) == 0) { if (m) atomicAdd(&n_mps[j], m); if (r) atomicAdd(&n_red[j], r); }
}

// MapPoint::EraseObservation(k) on point p, by one thread.  Two features of k that hold the same point race for the entry: the
// compare-and-swap lets one of them through, as the second call of the reference finds no entry.
__device__ void mg_erase_obs(const MgDev &G, int p, int k, int *bad_list, int bad_cap, int *n_bad)
{
    uint32_t h = G.w[G.hdr(p)];
    int cnt = MG_CNT(h), pos = -1;
    uint32_t ent = 0;
    for (int e = 0; e < cnt; e++) { ent = G.w[G.row(p, e)]; if ((int)(ent >> 16) == k) { pos = e; break; } }
    if (pos < 0) return;
    if (atomicCAS(&G.w[G.row(p, pos)], ent, MG_HOLE) != ent) return;
    h = G.w[G.hdr(p)];
    cnt = MG_CNT(h);
    const int wgt = (G.attr[G.at(k, (int)(ent & 0xFFFFu))] & MG_STEREO) ? 2 : 1;
    int nobs = MG_NOBS(h) - wgt;
    if (nobs < 0) nobs = 0;
    const int last = cnt - 1;
    if (pos != last) G.w[G.row(p, pos)] = G.w[G.row(p, last)];
    cnt = last;
    if (nobs <= 2) {   // SetBadFlag: the row is cleared and every former observer loses the match at its index
        for (int e = 0; e < cnt; e++) {
            const uint32_t e2 = G.w[G.row(p, e)];
            const int k2 = (int)(e2 >> 16), i2 = (int)(e2 & 0xFFFFu);
            if (k2 < G.max_kf && i2 < G.max_feat) G.w[G.match(k2, i2)] = 0xFFFFFFFFu;
        }
        G.w[G.hdr(p)] = MG_HDR(nobs, 0, MG_LIVE | MG_BAD);
        const int s = atomicAdd(n_bad, 1);
        if (s < bad_cap) bad_list[s] = p;
    } else
        G.w[G.hdr(p)] = MG_HDR(nobs, cnt, MG_LIVE);
}

// The keyframes in order, one workgroup.  Until the first real cull the counts of k_mg_judge stand; behind one, every later keyframe is
// judged again on the graph as the cull left it.
__global__ __launch_bounds__(1024) void k_mg_walk(MgDev G, const int32_t *__restrict__ local, const int32_t *__restrict__ not_erase, int n_local,
                                                  int mono, int *n_mps, int *n_red, int *culled, int *bad_list, int bad_cap, int *n_bad)
{
    __shared__ int s_mps, s_red, s_dec;
    const int tid = threadIdx.x, sub = tid & (MG_GROUP - 1);
    bool dirty = false;   // the same in every thread
    for (int j = 0; j < n_local; j++) {
        const int k = local[j], nfeat = (int)G.w[k];
        if (dirty) {
            if (tid == 0) { s_mps = 0; s_red = 0; }
            __syncthreads();
            for (int i0 = 0; i0 < nfeat; i0 += 1024 / MG_GROUP) {
                bool counted, red;
                mg_judge(G, k, i0 + tid / MG_GROUP, nfeat, mono, sub, counted, red);
                const int m = __popcll(__ballot(counted && sub == 0)), r = __popcll(__ballot(red && sub == 0));
                if ((tid & 63) == 0) { if (m) atomicAdd(&s_mps, m); if (r) atomicAdd(&s_red, r); }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int mps = dirty ? s_mps : n_mps[j], red = dirty ? s_red : n_red[j];
            n_mps[j] = mps; n_red[j] = red;
            const int dec = (double)red > 0.9 * (double)mps ? (not_erase[j] ? 2 : 1) : 0;   // src/LocalMapping.cc:771
            culled[j] = dec; s_dec = dec;
        }
        __syncthreads();
        const int dec = s_dec;
        __syncthreads();
        if (dec == 1) {   // KeyFrame::SetBadFlag, src/KeyFrame.cc:505-507
            for (int i = tid; i < nfeat; i += 1024) {
                const int p = (int)G.w[G.match(k, i)];
                if (p >= 0 && p < G.max_points) mg_erase_obs(G, p, k, bad_list, bad_cap, n_bad);
            }
            if (tid == 0) G.w[k] = 0xFFFFFFFFu;
            __threadfence();   // this thread's writes out
            __syncthreads();
            __threadfence();   // and nothing stale read behind them
            dirty = true;
        }
    }
}

// ---- MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors (include/orbx.h: orbx_mapgraph_refresh_points states the arithmetic)

// a keyframe as the refresh sees it, indexed by slot: the camera centre, bad (bit 31) | features of the resident frame, its descriptors
struct RfKf { float cx, cy, cz; uint32_t bad_n; const uint32_t *desc; };
#define RF_BAD 0x80000000u

struct RfArgs {
    MgDev G;
    int n, what, cap, nkt, nlevels;          // cap: the longest row among the listed points (a multiple of 4): the LDS arrays are sized by it
    const int32_t *pts, *tslot, *ref;        // tslot: NULL without a table
    const float *pos, *sf;                   // pos: NULL = X Y Z from the table
    const RfKf *kft;                         // [nkt]
    float4 *tgeom; uint4 *tdesc;             // the table, or NULL
    uint8_t *status; float4 *geom; int32_t *best_kf, *best_idx; uint4 *desc;   // the output records, [n] each
};

static inline size_t rf_lds_bytes(int cap) { return (size_t)cap * 56 + (size_t)cap * cap * 2; }

// A wave per point, grid-stride.  The row is ranked by its entry word (keyframe slot << 16 | feature: a keyframe is in a row once, so
// this is the order of the keyframe slots) by counting in LDS; everything behind that runs in rank order, whatever the stored order was.
// GEOM: the lanes work out their entries' unit vectors, lane 0 adds them up in rank order (the order of the float sum is the contract).
// DESC: the entries of keyframes that are not bad are compacted in rank order with their descriptors in LDS; the Hamming matrix (u16),
// the row medians by bisection on the value and the wave minimum of median << 16 | rank are k_distinctive's.
// LDS: key[cap] sorted[cap] good[cap] | unit[cap][3] | dsc[cap][8] | dm[cap][cap] u16 = 56 cap + 2 cap^2 bytes, 142 KiB at cap = 256.
__global__ __launch_bounds__(64) void k_mp_refresh(RfArgs A)
{
    extern __shared__ __align__(16) unsigned char rf_smem[];
    const int cap = A.cap, lane = threadIdx.x;
    uint32_t *key = reinterpret_cast<uint32_t *>(rf_smem), *sorted = key + cap, *good = sorted + cap;
    float *unit = reinterpret_cast<float *>(good + cap);
    uint4 *dsc = reinterpret_cast<uint4 *>(unit + 3 * cap);
    uint16_t *dm = reinterpret_cast<uint16_t *>(dsc + 2 * cap);
    const MgDev &G = A.G;
    for (int i = blockIdx.x; i < A.n; i += gridDim.x) {
        __syncthreads();   // the previous point's LDS has been read
        const int p = A.pts[i];
        const uint32_t h = G.w[G.hdr(p)];
        const int cnt = min(MG_CNT(h), cap);
        if (!(h & MG_LIVE) || (h & MG_BAD) || cnt == 0) {   // the reference's early return
            if (lane == 0) A.status[i] = 0;
            continue;
        }
        for (int e = lane; e < cnt; e += 64) key[e] = G.w[G.row(p, e)];
        __syncthreads();
        for (int e = lane; e < cnt; e += 64) {
            const uint32_t k = key[e];
            int r = 0;
            for (int j = 0; j < cnt; j++) r += key[j] < k;
            sorted[r] = k;
        }
        __syncthreads();
        const long long ts = A.tslot ? A.tslot[i] : 0;
        unsigned st = 0;
        if (A.what & ORBX_REFRESH_GEOM) {
            float Px, Py, Pz;
            if (A.pos) { Px = A.pos[3 * (long long)i]; Py = A.pos[3 * (long long)i + 1]; Pz = A.pos[3 * (long long)i + 2]; }
            else { const float4 g0 = A.tgeom[2 * ts]; Px = g0.x; Py = g0.y; Pz = g0.z; }
            for (int r = lane; r < cnt; r += 64) {
                const int k = (int)(sorted[r] >> 16);
                float ux = 0.f, uy = 0.f, uz = 0.f;
                if (k < A.nkt) {
                    const RfKf K = A.kft[k];
                    const float dx = Px - K.cx, dy = Py - K.cy, dz = Pz - K.cz;
                    const double inv = 1.0 / __dsqrt_rn(((double)dx * dx + (double)dy * dy) + (double)dz * dz);
                    ux = (float)((double)dx * inv); uy = (float)((double)dy * inv); uz = (float)((double)dz * inv);
                }
                unit[3 * r] = ux; unit[3 * r + 1] = uy; unit[3 * r + 2] = uz;
            }
            __syncthreads();
            if (lane == 0) {
                float nx = 0.f, ny = 0.f, nz = 0.f;
                for (int r = 0; r < cnt; r++) { nx = nx + unit[3 * r]; ny = ny + unit[3 * r + 1]; nz = nz + unit[3 * r + 2]; }
                const double invn = 1.0 / (double)cnt;
                nx = (float)((double)nx * invn); ny = (float)((double)ny * invn); nz = (float)((double)nz * invn);
                const int ref = A.ref[i];
                int ri = 0;   // observations[pRefKF] default-inserts 0
                for (int r = 0; r < cnt; r++) if ((int)(sorted[r] >> 16) == ref) ri = (int)(sorted[r] & 0xFFFFu);
                float dmax = 0.f, dmin = 0.f;
                if (ref >= 0 && ref < A.nkt && ref < G.max_kf && ri < G.max_feat) {   // checked on the host
                    const RfKf K = A.kft[ref];
                    const float dx = Px - K.cx, dy = Py - K.cy, dz = Pz - K.cz;
                    const float dist = (float)__dsqrt_rn(((double)dx * dx + (double)dy * dy) + (double)dz * dz);
                    const int oct = min((int)(G.attr[G.at(ref, ri)] & MG_OCT), A.nlevels - 1);
                    dmax = dist * A.sf[oct];
                    dmin = dmax / A.sf[A.nlevels - 1];
                }
                const float4 g0 = make_float4(Px, Py, Pz, dmin), g1 = make_float4(nx, ny, nz, dmax);
                if (A.tgeom) { A.tgeom[2 * ts] = g0; A.tgeom[2 * ts + 1] = g1; }
                A.geom[2 * (long long)i] = g0; A.geom[2 * (long long)i + 1] = g1;
            }
            st |= ORBX_REFRESH_GEOM;
        }
        if (A.what & ORBX_REFRESH_DESC) {
            int nn = 0;
            for (int r0 = 0; r0 < cnt; r0 += 64) {   // the entries of keyframes that are not bad, compacted in rank order
                const int r = r0 + lane;
                bool take = false;
                uint32_t k = 0;
                const uint32_t *src = nullptr;
                if (r < cnt) {
                    k = sorted[r];
                    const int kf = (int)(k >> 16);
                    if (kf < A.nkt) {
                        const RfKf K = A.kft[kf];
                        take = !(K.bad_n & RF_BAD) && K.desc && (k & 0xFFFFu) < K.bad_n;   // the last two: checked on the host
                        src = K.desc;
                    }
                }
                const unsigned long long mask = __ballot(take);
                if (take) {
                    const int at = nn + __popcll(mask & ((1ull << lane) - 1ull));
                    const uint4 *s = reinterpret_cast<const uint4 *>(src + 8 * (size_t)(k & 0xFFFFu));
                    good[at] = k; dsc[2 * at] = s[0]; dsc[2 * at + 1] = s[1];
                }
                nn += __popcll(mask);
            }
            __syncthreads();
            if (nn > 0) {
                const uint32_t *dw = reinterpret_cast<const uint32_t *>(dsc);
                for (int a = lane; a < nn; a += 64) {
                    uint32_t da[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) da[q] = dw[8 * a + q];
                    for (int b = 0; b < nn; b++) dm[a * nn + b] = (uint16_t)hamming256(da, dw + 8 * b);
                }
                __syncthreads();
                const int km = (int)(0.5 * (nn - 1));
                unsigned best = 0xFFFFFFFFu;
                for (int a = lane; a < nn; a += 64) {
                    int lo = 0, hi = 256;   // the smallest v with #(d <= v) > km
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        int c = 0;
                        for (int b = 0; b < nn; b++) c += dm[a * nn + b] <= mid;
                        if (c > km) hi = mid; else lo = mid + 1;
                    }
                    const unsigned kk = ((unsigned)lo << 16) | (unsigned)a;
                    best = kk < best ? kk : best;
                }
                best = wave_min_u32(best);
                if (lane == 0) {
                    const int a = (int)(best & 0xFFFFu);
                    const uint32_t k = good[a];
                    const uint4 d0 = dsc[2 * a], d1 = dsc[2 * a + 1];
                    if (A.tdesc) { A.tdesc[2 * ts] = d0; A.tdesc[2 * ts + 1] = d1; }
                    A.desc[2 * (long long)i] = d0; A.desc[2 * (long long)i + 1] = d1;
                    A.best_kf[i] = (int32_t)(k >> 16); A.best_idx[i] = (int32_t)(k & 0xFFFFu);
                }
                st |= ORBX_REFRESH_DESC;
            }
        }
        if (lane == 0) A.status[i] = (uint8_t)st;
    }
}

// ---------------------------------------------------------------- the handle

struct MgUndo { size_t addr; uint32_t old; };

struct orbx_mapgraph {
    int device;
    MgDev G;                       // G.w / G.attr: the device's copy
    size_t words, feats;           // words of the word space; max_keyframes * max_features
    uint8_t *d_blob, *d_stage, *h_stage; size_t st_bytes, st_attr;   // st_attr: where the attribute bytes of a new keyframe lie in the staging
    std::vector<uint32_t> hw; std::vector<uint8_t> hattr;   // the mirror
    std::vector<MgUndo> undo;      // (word, old value) of the edit being worked out, in order
    std::vector<int32_t> refs;     // per keyframe slot: the row entries that name it (a slot is not given to a new keyframe while there are any)
    std::vector<std::pair<int, int>> undo_refs;
    std::vector<int32_t> bad;      // the points that went bad in it
    std::vector<uint64_t> keys;    // duplicate check of a batch
    std::vector<size_t> touched;
    std::vector<int32_t> kmap;     // refresh_points: per keyframe slot its place in the job's list, -1 between calls
    hipEvent_t ev; hipStream_t ev_stream; bool ev_set;
    std::mutex mu;
};

// ---- the edits on the mirror.  Every change of a word goes through mg_w, so a refusal half way rolls the mirror back.
static inline void mg_w(orbx_mapgraph *g, size_t addr, uint32_t val)
{
    g->undo.push_back({ addr, g->hw[addr] });
    g->hw[addr] = val;
}
static inline void mg_ref(orbx_mapgraph *g, int k, int delta)
{
    g->refs[k] += delta;
    g->undo_refs.push_back({ k, delta });
}
static void mg_rollback(orbx_mapgraph *g)
{
    for (size_t i = g->undo.size(); i-- > 0;) g->hw[g->undo[i].addr] = g->undo[i].old;
    for (const std::pair<int, int> &r : g->undo_refs) g->refs[r.first] -= r.second;
    g->undo.clear(); g->undo_refs.clear(); g->bad.clear();
}

// MapPoint::SetBadFlag, src/MapPoint.cc:159-176 (nObs stays as it is, as in the reference)
static void mg_set_bad(orbx_mapgraph *g, int p)
{
    const MgDev &G = g->G;
    const uint32_t h = g->hw[G.hdr(p)];
    for (int e = 0, cnt = MG_CNT(h); e < cnt; e++) {
        const uint32_t ent = g->hw[G.row(p, e)];
        mg_w(g, G.match((int)(ent >> 16), (int)(ent & 0xFFFFu)), 0xFFFFFFFFu);
        mg_ref(g, (int)(ent >> 16), -1);
    }
    mg_w(g, G.hdr(p), MG_HDR(MG_NOBS(h), 0, MG_LIVE | MG_BAD));
    g->bad.push_back(p);
}

// MapPoint::EraseObservation, src/MapPoint.cc:119-145.  The last entry of the row moves into the gap, on the device as here.
static void mg_erase_obs_host(orbx_mapgraph *g, int p, int k)
{
    const MgDev &G = g->G;
    const uint32_t h = g->hw[G.hdr(p)];
    const int cnt = MG_CNT(h);
    int pos = -1;
    for (int e = 0; e < cnt; e++) if ((int)(g->hw[G.row(p, e)] >> 16) == k) { pos = e; break; }
    if (pos < 0) return;
    const uint32_t ent = g->hw[G.row(p, pos)];
    int nobs = MG_NOBS(h) - ((g->hattr[G.at(k, (int)(ent & 0xFFFFu))] & MG_STEREO) ? 2 : 1);
    if (nobs < 0) nobs = 0;
    if (pos != cnt - 1) mg_w(g, G.row(p, pos), g->hw[G.row(p, cnt - 1)]);
    mg_w(g, G.hdr(p), MG_HDR(nobs, cnt - 1, MG_LIVE));
    mg_ref(g, k, -1);
    if (nobs <= 2) mg_set_bad(g, p);
}

// the map-point part of KeyFrame::SetBadFlag, src/KeyFrame.cc:505-507; then the slot is free
static void mg_erase_keyframe_host(orbx_mapgraph *g, int k)
{
    const MgDev &G = g->G;
    for (int i = 0, n = (int)g->hw[k]; i < n; i++) {
        const int p = (int)g->hw[G.match(k, i)];
        if (p >= 0) mg_erase_obs_host(g, p, k);
    }
    mg_w(g, (size_t)k, 0xFFFFFFFFu);
}

// a pair named twice in the batch that g->keys holds
static bool mg_twice(orbx_mapgraph *g)
{
    std::sort(g->keys.begin(), g->keys.end());
    return std::adjacent_find(g->keys.begin(), g->keys.end()) != g->keys.end();
}

// The edit worked out on the mirror goes to the device: the final value of every word it touched, MG_STAGE_RECORDS records to an upload
// (a keyframe's batch is one), and with the first of them the attribute bytes of a new keyframe.  One scatter launch per upload, on the
// calling thread's stream; the call does not wait for it.
static int mg_flush(orbx_mapgraph *g, int init_kf, int init_n)
{
    g->touched.clear();
    for (const MgUndo &u : g->undo) g->touched.push_back(u.addr);
    std::sort(g->touched.begin(), g->touched.end());
    g->touched.erase(std::unique(g->touched.begin(), g->touched.end()), g->touched.end());
    g->undo.clear(); g->undo_refs.clear(); g->bad.clear();
    if (g->touched.empty() && init_n <= 0) return ORBX_OK;
    CallCtx *c;
    int rc = orbx_call_ctx(g->device, &c);
    if (rc) return rc;
    const size_t n = g->touched.size();
    for (size_t first = 0; first == 0 || first < n; first += MG_STAGE_RECORDS) {
        const size_t k = n - first < MG_STAGE_RECORDS ? n - first : MG_STAGE_RECORDS;
        const int ni = first == 0 && init_n > 0 ? init_n : 0;
        if (g->ev_set) ORBX_HIP(hipEventSynchronize(g->ev));   // the previous upload has read the staging, and edits on other streams are done
        uint32_t *rec = (uint32_t *)g->h_stage;
        for (size_t i = 0; i < k; i++) { rec[2 * i] = (uint32_t)g->touched[first + i]; rec[2 * i + 1] = g->hw[g->touched[first + i]]; }
        if (ni) memcpy(g->h_stage + g->st_attr, &g->hattr[g->G.at(init_kf, 0)], (size_t)ni);
        if (k) ORBX_HIP(hipMemcpyAsync(g->d_stage, g->h_stage, 8 * k, hipMemcpyHostToDevice, c->stream));
        if (ni) ORBX_HIP(hipMemcpyAsync(g->d_stage + g->st_attr, g->h_stage + g->st_attr, (size_t)ni, hipMemcpyHostToDevice, c->stream));
        const int m = (int)k > ni ? (int)k : ni;
        hipLaunchKernelGGL(k_mg_scatter, dim3((m + 255) / 256), dim3(256), 0, c->stream, g->G, (const uint2 *)g->d_stage, (int)k, init_kf, ni,
                           (const uint8_t *)(g->d_stage + g->st_attr));
        ORBX_HIP(hipGetLastError());
        ORBX_HIP(hipEventRecord(g->ev, c->stream));
        g->ev_stream = c->stream; g->ev_set = true;
    }
    return ORBX_OK;
}

// stream s behind the graph's most recent edit (the caller holds g->mu)
static inline int mg_order_before(orbx_mapgraph *g, hipStream_t s)
{
    if (g->ev_set && g->ev_stream != s) ORBX_HIP(hipStreamWaitEvent(s, g->ev, 0));
    return ORBX_OK;
}

#define MG_REFUSE(code, ...) do { mg_rollback(g); orbx_set_error(__VA_ARGS__); return code; } while (0)

static inline bool mg_kf_live(const orbx_mapgraph *g, int k) { return k >= 0 && k < g->G.max_kf && (int32_t)g->hw[k] >= 0; }

// ---------------------------------------------------------------- the ABI

extern "C" int orbx_mapgraph_create(int device, int max_keyframes, int max_features, int max_points, int max_obs, orbx_mapgraph **out)
{
    if (!out || max_keyframes < 1 || max_keyframes > 65535 || max_features < 1 || max_features > 65535 || max_points < 1 ||
        max_points > (1 << 24) || max_obs < 4 || max_obs > 256) {
        orbx_set_error("orbx_mapgraph_create: invalid argument (max_keyframes and max_features in [1, 65535], max_points in [1, 2^24], max_obs in [4, 256])");
        return ORBX_E_INVALID;
    }
    *out = nullptr;
    const size_t feats = (size_t)max_keyframes * max_features;
    const size_t words = (size_t)max_keyframes + feats + (size_t)max_points * (1 + (size_t)max_obs);
    if (words > 0xFFFFFFFFull) {
        orbx_set_error("orbx_mapgraph_create: %zu words of graph, at most 2^32 - 1 (16 GiB) can be addressed", words);
        return ORBX_E_INVALID;
    }
    CallCtx *c;
    int rc = orbx_call_ctx(device, &c);
    if (rc) return rc;
    orbx_mapgraph *g = new orbx_mapgraph();
    g->device = device; g->words = words; g->feats = feats;
    g->st_attr = 8 * (size_t)MG_STAGE_RECORDS; g->st_bytes = g->st_attr + a16((size_t)max_features);
    g->d_blob = nullptr; g->h_stage = nullptr; g->ev = nullptr; g->ev_stream = nullptr; g->ev_set = false;
    const size_t o_attr = a16(4 * words), o_stage = o_attr + a16(feats), total = o_stage + g->st_bytes;
    const hipError_t e1 = hipMalloc((void **)&g->d_blob, total);
    const hipError_t e2 = e1 == hipSuccess ? hipHostMalloc((void **)&g->h_stage, g->st_bytes, hipHostMallocDefault) : e1;
    const hipError_t e3 = e2 == hipSuccess ? hipEventCreateWithFlags(&g->ev, hipEventDisableTiming) : e2;
    // kf_n = -1 (free), hdr = 0 (no point); match, row and attr are written before they are read
    const hipError_t e4 = e3 == hipSuccess ? hipMemset(g->d_blob, 0xFF, 4 * (size_t)max_keyframes) : e3;
    const hipError_t e5 = e4 == hipSuccess ? hipMemset(g->d_blob + 4 * ((size_t)max_keyframes + feats), 0, 4 * (size_t)max_points) : e4;
    if (e5 != hipSuccess) {
        orbx_set_error("orbx_mapgraph_create: HIP allocation of %zu bytes failed: %s", total, hipGetErrorString(e5));
        if (g->ev) hipEventDestroy(g->ev);
        if (g->h_stage) hipHostFree(g->h_stage);
        if (g->d_blob) hipFree(g->d_blob);
        delete g;
        return ORBX_E_HIP;
    }
    MgDev &G = g->G;
    G.w = (uint32_t *)g->d_blob; G.attr = g->d_blob + o_attr; g->d_stage = g->d_blob + o_stage;
    G.a_match = (size_t)max_keyframes; G.a_hdr = G.a_match + feats; G.a_row = G.a_hdr + (size_t)max_points;
    G.max_kf = max_keyframes; G.max_feat = max_features; G.max_points = max_points; G.max_obs = max_obs;
    g->hw.assign(words, 0u);
    std::fill(g->hw.begin(), g->hw.begin() + max_keyframes, 0xFFFFFFFFu);
    g->hattr.assign(feats, 0);
    g->refs.assign((size_t)max_keyframes, 0);
    g->kmap.assign((size_t)max_keyframes, -1);
    *out = g;
    return ORBX_OK;
}

extern "C" void orbx_mapgraph_destroy(orbx_mapgraph *g)
{
    if (!g) return;
    if (orbx_use_device(g->device) == hipSuccess) {
        if (g->ev_set) hipEventSynchronize(g->ev);
        hipEventDestroy(g->ev);
        hipHostFree(g->h_stage);
        hipFree(g->d_blob);
    }
    delete g;
}

extern "C" int orbx_mapgraph_clear(orbx_mapgraph *g)
{
    if (!g) { orbx_set_error("orbx_mapgraph_clear: null graph"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    CallCtx *c;
    int rc = orbx_call_ctx(g->device, &c);
    if (rc) return rc;
    if ((rc = mg_order_before(g, c->stream))) return rc;
    ORBX_HIP(hipMemsetAsync(g->G.w, 0xFF, 4 * (size_t)g->G.max_kf, c->stream));
    ORBX_HIP(hipMemsetAsync(g->G.w + g->G.a_hdr, 0, 4 * (size_t)g->G.max_points, c->stream));
    ORBX_HIP(hipEventRecord(g->ev, c->stream));
    g->ev_stream = c->stream; g->ev_set = true;
    std::fill(g->hw.begin(), g->hw.begin() + g->G.max_kf, 0xFFFFFFFFu);
    std::fill(g->hw.begin() + g->G.a_hdr, g->hw.begin() + g->G.a_row, 0u);
    std::fill(g->refs.begin(), g->refs.end(), 0);
    return ORBX_OK;
}

extern "C" int orbx_mapgraph_set_keyframe(orbx_mapgraph *g, int kf, int n, const uint8_t *octave, const uint8_t *stereo, const uint8_t *close)
{
    if (!g || n < 0 || (n && (!octave || !stereo || !close))) { orbx_set_error("orbx_mapgraph_set_keyframe: invalid argument (a graph, n >= 0 features, octave, stereo, close)"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    if (kf < 0) { orbx_set_error("orbx_mapgraph_set_keyframe: negative keyframe slot %d", kf); return ORBX_E_INVALID; }
    if (kf >= g->G.max_kf) { orbx_set_error("orbx_mapgraph_set_keyframe: keyframe slot %d, max_keyframes %d", kf, g->G.max_kf); return ORBX_E_CAPACITY; }
    if (n > g->G.max_feat) { orbx_set_error("orbx_mapgraph_set_keyframe: %d features, max_features %d", n, g->G.max_feat); return ORBX_E_CAPACITY; }
    if ((int32_t)g->hw[kf] >= 0) { orbx_set_error("orbx_mapgraph_set_keyframe: keyframe slot %d is in use", kf); return ORBX_E_INVALID; }
    if (g->refs[kf]) { orbx_set_error("orbx_mapgraph_set_keyframe: %d observations still name keyframe slot %d", g->refs[kf], kf); return ORBX_E_INVALID; }
    for (int i = 0; i < n; i++)
        if (octave[i] > MG_OCT) { orbx_set_error("orbx_mapgraph_set_keyframe: feature %d: octave %d, at most %d", i, octave[i], (int)MG_OCT); return ORBX_E_INVALID; }
    for (int i = 0; i < n; i++) {
        g->hattr[g->G.at(kf, i)] = (uint8_t)(octave[i] | (stereo[i] ? MG_STEREO : 0) | (close[i] ? MG_CLOSE : 0));
        g->hw[g->G.match(kf, i)] = 0xFFFFFFFFu;
    }
    mg_w(g, (size_t)kf, (uint32_t)n);
    return mg_flush(g, kf, n);
}

extern "C" int orbx_mapgraph_set_matches(orbx_mapgraph *g, int kf, const int32_t *idx, const int32_t *point, int n)
{
    if (!g || n < 0 || (n && (!idx || !point))) { orbx_set_error("orbx_mapgraph_set_matches: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    if (!mg_kf_live(g, kf)) { orbx_set_error("orbx_mapgraph_set_matches: keyframe slot %d is not in use", kf); return ORBX_E_INVALID; }
    const int nf = (int)g->hw[kf];
    g->keys.clear();
    for (int i = 0; i < n; i++) {
        if (idx[i] < 0 || idx[i] >= nf) { orbx_set_error("orbx_mapgraph_set_matches: entry %d: feature %d outside [0, %d)", i, idx[i], nf); return ORBX_E_INVALID; }
        if (point[i] < -1) { orbx_set_error("orbx_mapgraph_set_matches: entry %d: point slot %d", i, point[i]); return ORBX_E_INVALID; }
        if (point[i] >= g->G.max_points) { orbx_set_error("orbx_mapgraph_set_matches: entry %d: point slot %d, max_points %d", i, point[i], g->G.max_points); return ORBX_E_CAPACITY; }
        g->keys.push_back((uint64_t)idx[i]);
    }
    if (mg_twice(g)) { orbx_set_error("orbx_mapgraph_set_matches: a feature named twice"); return ORBX_E_INVALID; }
    for (int i = 0; i < n; i++) mg_w(g, g->G.match(kf, idx[i]), (uint32_t)point[i]);
    return mg_flush(g, 0, 0);
}

extern "C" int orbx_mapgraph_add_observations(orbx_mapgraph *g, const int32_t *point, const int32_t *kf, const int32_t *idx, int n)
{
    if (!g || n < 0 || (n && (!point || !kf || !idx))) { orbx_set_error("orbx_mapgraph_add_observations: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    const MgDev &G = g->G;
    g->keys.clear();
    for (int i = 0; i < n; i++) {
        if (point[i] < 0) { orbx_set_error("orbx_mapgraph_add_observations: entry %d: point slot %d", i, point[i]); return ORBX_E_INVALID; }
        if (point[i] >= G.max_points) { orbx_set_error("orbx_mapgraph_add_observations: entry %d: point slot %d, max_points %d", i, point[i], G.max_points); return ORBX_E_CAPACITY; }
        if (!mg_kf_live(g, kf[i])) { orbx_set_error("orbx_mapgraph_add_observations: entry %d: keyframe slot %d is not in use", i, kf[i]); return ORBX_E_INVALID; }
        if (idx[i] < 0 || idx[i] >= (int)g->hw[kf[i]]) { orbx_set_error("orbx_mapgraph_add_observations: entry %d: feature %d outside [0, %d)", i, idx[i], (int)g->hw[kf[i]]); return ORBX_E_INVALID; }
        g->keys.push_back((uint64_t)point[i] << 16 | (uint64_t)kf[i]);
    }
    if (mg_twice(g)) { orbx_set_error("orbx_mapgraph_add_observations: a (point, keyframe) pair named twice"); return ORBX_E_INVALID; }
    for (int i = 0; i < n; i++) {
        const int p = point[i];
        uint32_t h = g->hw[G.hdr(p)];
        if (h & MG_BAD) h = 0;   // the slot is used again: a new point
        int cnt = MG_CNT(h), e = 0;
        while (e < cnt && (int)(g->hw[G.row(p, e)] >> 16) != kf[i]) e++;
        if (e < cnt) continue;   // src/MapPoint.cc:109
        if (cnt == G.max_obs) MG_REFUSE(ORBX_E_CAPACITY, "orbx_mapgraph_add_observations: entry %d: point slot %d has max_obs = %d observations", i, p, G.max_obs);
        mg_w(g, G.row(p, cnt), (uint32_t)kf[i] << 16 | (uint32_t)idx[i]);
        mg_w(g, G.hdr(p), MG_HDR(MG_NOBS(h) + ((g->hattr[G.at(kf[i], idx[i])] & MG_STEREO) ? 2 : 1), cnt + 1, MG_LIVE));
        mg_ref(g, kf[i], +1);
    }
    return mg_flush(g, 0, 0);
}

extern "C" int orbx_mapgraph_erase_observations(orbx_mapgraph *g, const int32_t *point, const int32_t *kf, int n)
{
    if (!g || n < 0 || (n && (!point || !kf))) { orbx_set_error("orbx_mapgraph_erase_observations: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    g->keys.clear();
    for (int i = 0; i < n; i++) {
        if (point[i] < 0 || kf[i] < 0) { orbx_set_error("orbx_mapgraph_erase_observations: entry %d: point slot %d, keyframe slot %d", i, point[i], kf[i]); return ORBX_E_INVALID; }
        if (point[i] >= g->G.max_points || kf[i] >= g->G.max_kf) { orbx_set_error("orbx_mapgraph_erase_observations: entry %d: point slot %d of %d, keyframe slot %d of %d", i, point[i], g->G.max_points, kf[i], g->G.max_kf); return ORBX_E_CAPACITY; }
        g->keys.push_back((uint64_t)point[i] << 16 | (uint64_t)kf[i]);
    }
    if (mg_twice(g)) { orbx_set_error("orbx_mapgraph_erase_observations: a (point, keyframe) pair named twice"); return ORBX_E_INVALID; }
    for (int i = 0; i < n; i++) mg_erase_obs_host(g, point[i], kf[i]);
    return mg_flush(g, 0, 0);
}

extern "C" int orbx_mapgraph_erase_points(orbx_mapgraph *g, const int32_t *point, int n)
{
    if (!g || n < 0 || (n && !point)) { orbx_set_error("orbx_mapgraph_erase_points: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    g->keys.clear();
    for (int i = 0; i < n; i++) {
        if (point[i] < 0) { orbx_set_error("orbx_mapgraph_erase_points: entry %d: point slot %d", i, point[i]); return ORBX_E_INVALID; }
        if (point[i] >= g->G.max_points) { orbx_set_error("orbx_mapgraph_erase_points: entry %d: point slot %d, max_points %d", i, point[i], g->G.max_points); return ORBX_E_CAPACITY; }
        g->keys.push_back((uint64_t)point[i]);
    }
    if (mg_twice(g)) { orbx_set_error("orbx_mapgraph_erase_points: a point slot named twice"); return ORBX_E_INVALID; }
    for (int i = 0; i < n; i++) mg_set_bad(g, point[i]);
    return mg_flush(g, 0, 0);
}

extern "C" int orbx_mapgraph_erase_keyframe(orbx_mapgraph *g, int kf)
{
    if (!g) { orbx_set_error("orbx_mapgraph_erase_keyframe: null graph"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    if (!mg_kf_live(g, kf)) { orbx_set_error("orbx_mapgraph_erase_keyframe: keyframe slot %d is not in use", kf); return ORBX_E_INVALID; }
    mg_erase_keyframe_host(g, kf);
    return mg_flush(g, 0, 0);
}

extern "C" int orbx_mapgraph_keyframe_observations(orbx_mapgraph *g, int kf)
{
    if (!g || kf < 0 || kf >= g->G.max_kf) { orbx_set_error("orbx_mapgraph_keyframe_observations: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    return g->refs[kf];
}

// tests and debugging: from the device's copy
extern "C" int orbx_mapgraph_read_keyframe(orbx_mapgraph *g, int kf, int *n, int32_t *point, uint8_t *octave, uint8_t *stereo, uint8_t *close)
{
    if (!g || !n || kf < 0 || kf >= g->G.max_kf) { orbx_set_error("orbx_mapgraph_read_keyframe: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    ORBX_HIP(orbx_use_device(g->device));
    if (g->ev_set) ORBX_HIP(hipEventSynchronize(g->ev));
    int32_t nf;
    ORBX_HIP(hipMemcpy(&nf, g->G.w + kf, 4, hipMemcpyDeviceToHost));
    *n = nf;
    if (nf <= 0) return ORBX_OK;
    if (nf > g->G.max_feat) { orbx_set_error("orbx_mapgraph_read_keyframe: keyframe slot %d holds the count %d", kf, nf); return ORBX_E_HIP; }
    if (point) ORBX_HIP(hipMemcpy(point, g->G.w + g->G.match(kf, 0), 4 * (size_t)nf, hipMemcpyDeviceToHost));
    if (octave || stereo || close) {
        std::vector<uint8_t> a((size_t)nf);
        ORBX_HIP(hipMemcpy(a.data(), g->G.attr + g->G.at(kf, 0), (size_t)nf, hipMemcpyDeviceToHost));
        for (int i = 0; i < nf; i++) {
            if (octave) octave[i] = a[i] & MG_OCT;
            if (stereo) stereo[i] = (a[i] & MG_STEREO) != 0;
            if (close) close[i] = (a[i] & MG_CLOSE) != 0;
        }
    }
    return ORBX_OK;
}

extern "C" int orbx_mapgraph_read_points(orbx_mapgraph *g, int first, int n, int32_t *n_obs, uint8_t *flags, int32_t *n_entries, int32_t *kf, int32_t *idx)
{
    if (!g || !n_obs || !flags || !n_entries || first < 0 || n < 0 || first > g->G.max_points - n) { orbx_set_error("orbx_mapgraph_read_points: invalid argument"); return ORBX_E_INVALID; }
    if (n == 0) return ORBX_OK;
    std::lock_guard<std::mutex> lk(g->mu);
    ORBX_HIP(orbx_use_device(g->device));
    if (g->ev_set) ORBX_HIP(hipEventSynchronize(g->ev));
    const size_t mo = (size_t)g->G.max_obs;
    std::vector<uint32_t> h((size_t)n), r(kf || idx ? (size_t)n * mo : 0);
    ORBX_HIP(hipMemcpy(h.data(), g->G.w + g->G.hdr(first), 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (!r.empty()) ORBX_HIP(hipMemcpy(r.data(), g->G.w + g->G.row(first, 0), 4 * r.size(), hipMemcpyDeviceToHost));
    for (int p = 0; p < n; p++) {
        const int cnt = MG_CNT(h[p]);
        n_obs[p] = MG_NOBS(h[p]); flags[p] = (uint8_t)(((h[p] & MG_LIVE) ? 1 : 0) | ((h[p] & MG_BAD) ? 2 : 0)); n_entries[p] = cnt;
        if (cnt > g->G.max_obs) { orbx_set_error("orbx_mapgraph_read_points: point slot %d holds the count %d", first + p, cnt); return ORBX_E_HIP; }
        for (int e = 0; e < cnt && !r.empty(); e++) {
            if (kf) kf[p * mo + e] = (int32_t)(r[p * mo + e] >> 16);
            if (idx) idx[p * mo + e] = (int32_t)(r[p * mo + e] & 0xFFFFu);
        }
    }
    return ORBX_OK;
}

// ---- queries

// k_mg_vote over n point slots at d_pts (a device address) into the head of the work area, then the counts and the compact list
static int mg_vote_run(orbx_mapgraph *g, CallCtx *c, const int32_t *d_pts, int n, int exclude, int32_t *counts, int32_t *nz_slots, int *n_nz)
{
    const size_t out = 4 * (size_t)g->G.max_kf;
    ORBX_HIP(hipMemsetAsync(c->d_work, 0, out, c->stream));
    if (n > 0) {
        const int use_lds = g->G.max_kf <= MG_LDS_KEYFRAMES;
        const int per = 256 / MG_GROUP, blocks = std::min((n + per - 1) / per, 256);
        hipLaunchKernelGGL(k_mg_vote, dim3(blocks), dim3(256), use_lds ? 4 * (size_t)g->G.max_kf : 0, c->stream, g->G, d_pts, n, exclude,
                           (int *)c->d_work, use_lds);
    }
    int rc = call_fetch(c, out);
    if (rc) return rc;
    memcpy(counts, c->h_out, out);
    if (n_nz) {
        int m = 0;
        for (int k = 0; k < g->G.max_kf; k++) if (counts[k]) { if (nz_slots) nz_slots[m] = k; m++; }
        *n_nz = m;
    }
    return ORBX_OK;
}

extern "C" int orbx_mapgraph_vote(orbx_mapgraph *g, const int32_t *points, int n, int32_t *counts, int32_t *nz_slots, int *n_nz)
{
    if (!g || n < 0 || n > (1 << 20) || (n && !points) || !counts) { orbx_set_error("orbx_mapgraph_vote: invalid argument (a graph, n <= 2^20 point slots, counts)"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    for (int i = 0; i < n; i++)
        if (points[i] < 0 || points[i] >= g->G.max_points) { orbx_set_error("orbx_mapgraph_vote: entry %d: point slot %d outside [0, %d)", i, points[i], g->G.max_points); return ORBX_E_INVALID; }
    CallCtx *c;
    int rc = orbx_call_ctx(g->device, &c);
    if (rc) return rc;
    const size_t out = 4 * (size_t)g->G.max_kf;
    if ((rc = call_reserve(c, 4 * (size_t)n + 16, out, out))) return rc;
    if (n) memcpy(c->h_blob, points, 4 * (size_t)n);
    if ((rc = mg_order_before(g, c->stream))) return rc;
    if (n && (rc = call_upload(c, 4 * (size_t)n))) return rc;
    return mg_vote_run(g, c, (const int32_t *)c->d_blob, n, -1, counts, nz_slots, n_nz);
}

extern "C" int orbx_mapgraph_covisibility(orbx_mapgraph *g, int kf, int32_t *counts, int32_t *nz_slots, int *n_nz)
{
    if (!g || !counts) { orbx_set_error("orbx_mapgraph_covisibility: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    if (!mg_kf_live(g, kf)) { orbx_set_error("orbx_mapgraph_covisibility: keyframe slot %d is not in use", kf); return ORBX_E_INVALID; }
    CallCtx *c;
    int rc = orbx_call_ctx(g->device, &c);
    if (rc) return rc;
    const size_t out = 4 * (size_t)g->G.max_kf;
    if ((rc = call_reserve(c, 0, out, out))) return rc;
    if ((rc = mg_order_before(g, c->stream))) return rc;
    return mg_vote_run(g, c, (const int32_t *)(g->G.w + g->G.match(kf, 0)), (int)g->hw[kf], kf, counts, nz_slots, n_nz);
}

extern "C" int orbx_mapgraph_cull_keyframes(orbx_mapgraph *g, const int32_t *local, const uint8_t *not_erase, int n_local, int monocular,
                                            uint8_t *culled, int32_t *n_mps, int32_t *n_redundant, int32_t *bad_points, int cap, int *n_bad)
{
    if (!g || n_local < 0 || n_local > 65535 || cap < 0 || !n_bad || (cap && !bad_points) || (n_local && (!local || !not_erase || !culled))) {
        orbx_set_error("orbx_mapgraph_cull_keyframes: invalid argument (a graph, n_local <= 65535 keyframe slots, not_erase, culled, n_bad, bad_points[cap])");
        return ORBX_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(g->mu);
    g->keys.clear();
    size_t feats = 0;
    int widest = 0;
    for (int j = 0; j < n_local; j++) {
        if (!mg_kf_live(g, local[j])) { orbx_set_error("orbx_mapgraph_cull_keyframes: entry %d: keyframe slot %d is not in use", j, local[j]); return ORBX_E_INVALID; }
        g->keys.push_back((uint64_t)local[j]);
        feats += g->hw[local[j]];
        widest = std::max(widest, (int)g->hw[local[j]]);
    }
    if (mg_twice(g)) { orbx_set_error("orbx_mapgraph_cull_keyframes: a keyframe slot named twice"); return ORBX_E_INVALID; }
    *n_bad = 0;
    if (n_local == 0) return ORBX_OK;
    CallCtx *c;
    int rc = orbx_call_ctx(g->device, &c);
    if (rc) return rc;
    // up: local | not_erase   work and down: n_mps | n_red | culled | n_bad | bad_list[feats]: a keyframe makes at most one point bad per feature
    const size_t nl = (size_t)n_local, col = a16(4 * nl), blob = 2 * col, o_nbad = 3 * col, o_bad = o_nbad + 16, out = o_bad + a16(4 * feats);
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    memcpy(c->h_blob, local, 4 * nl);
    for (size_t j = 0; j < nl; j++) ((int32_t *)(c->h_blob + col))[j] = not_erase[j] ? 1 : 0;
    if ((rc = mg_order_before(g, c->stream))) return rc;
    if ((rc = call_upload(c, blob))) return rc;
    ORBX_HIP(hipMemsetAsync(c->d_work, 0, o_bad, c->stream));
    uint8_t *wk = c->d_work;
    const int32_t *d_local = (const int32_t *)c->d_blob, *d_ne = (const int32_t *)(c->d_blob + col);
    const int per = 256 / MG_GROUP;
    if (widest > 0)
        hipLaunchKernelGGL(k_mg_judge, dim3((widest + per - 1) / per, n_local), dim3(256), 0, c->stream, g->G, d_local, monocular ? 1 : 0,
                           (int *)wk, (int *)(wk + col));
    hipLaunchKernelGGL(k_mg_walk, dim3(1), dim3(1024), 0, c->stream, g->G, d_local, d_ne, n_local, monocular ? 1 : 0, (int *)wk, (int *)(wk + col),
                       (int *)(wk + 2 * col), (int *)(wk + o_bad), (int)feats, (int *)(wk + o_nbad));
    if ((rc = call_fetch(c, out))) return rc;
    const uint8_t *ho = (const uint8_t *)c->h_out;
    const int32_t *h_culled = (const int32_t *)(ho + 2 * col);
    const int dev_bad = *(const int32_t *)(ho + o_nbad);
    // the same culls on the mirror, in the same order; both sides must name the same bad points
    for (int j = 0; j < n_local; j++)
        if (h_culled[j] == 1) mg_erase_keyframe_host(g, local[j]);
    std::vector<int32_t> mine(g->bad), theirs((const int32_t *)(ho + o_bad), (const int32_t *)(ho + o_bad) + std::min((size_t)std::max(dev_bad, 0), feats));
    g->undo.clear(); g->undo_refs.clear(); g->bad.clear();
    std::sort(mine.begin(), mine.end()); std::sort(theirs.begin(), theirs.end());
    for (int j = 0; j < n_local; j++) culled[j] = (uint8_t)h_culled[j];
    if (n_mps) memcpy(n_mps, ho, 4 * nl);
    if (n_redundant) memcpy(n_redundant, ho + col, 4 * nl);
    if (mine != theirs) { orbx_set_error("orbx_mapgraph_cull_keyframes: the device names %d bad points, the host's mirror %zu others: the graph is inconsistent", dev_bad, mine.size()); return ORBX_E_HIP; }
    *n_bad = (int)theirs.size();
    if ((int)theirs.size() > cap) { orbx_set_error("orbx_mapgraph_cull_keyframes: %zu points went bad, cap %d", theirs.size(), cap); return ORBX_E_CAPACITY; }
    if (!theirs.empty()) memcpy(bad_points, theirs.data(), 4 * theirs.size());
    return ORBX_OK;
}

// ---- refresh: every refusal on the mirror and the table's host state, then one upload, one launch, one group of downloads

#define RF_REFUSE(code, ...) do { for (int q_ = 0; q_ < job->nk; q_++) { const int s_ = job->kf_slot[q_]; if (s_ >= 0 && s_ < g->G.max_kf) g->kmap[s_] = -1; } \
                                  orbx_set_error(__VA_ARGS__); return code; } while (0)

extern "C" int orbx_mapgraph_refresh_points(orbx_mapgraph *g, orbx_mappoints *m, const orbx_refresh_job *job, uint8_t *status, float *geom,
                                            int32_t *best_kf, int32_t *best_idx, uint8_t *desc, void *stream)
{
    static const char *who = "orbx_mapgraph_refresh_points";
    if (!g || !job) { orbx_set_error("%s: null graph or job", who); return ORBX_E_INVALID; }
    const int what = job->what, n = job->n, nk = job->nk;
    const bool do_geom = (what & ORBX_REFRESH_GEOM) != 0, do_desc = (what & ORBX_REFRESH_DESC) != 0;
    if (what < 1 || what > 3) { orbx_set_error("%s: what = %d, a non-empty OR of ORBX_REFRESH_GEOM and ORBX_REFRESH_DESC", who, what); return ORBX_E_INVALID; }
    if (n < 0 || n > (1 << 24) || nk < 0 || nk > 65535 || (n && !job->point) || (nk && (!job->kf_slot || !job->kf_centre || !job->kf_bad)) ||
        (n && do_geom && (!job->ref_kf || !job->scale_factors || job->nlevels < 1 || job->nlevels > 32)) || (n && do_geom && !job->pos && !m) ||
        (!m && job->table_slot)) {
        orbx_set_error("%s: invalid argument (n <= 2^24 points, nk <= 65535 keyframes with centre and bad; GEOM: ref_kf, scale_factors, 1 <= nlevels <= 32, pos or a table)", who);
        return ORBX_E_INVALID;
    }
    if (n == 0) return ORBX_OK;
    if (m && m->device != g->device) { orbx_set_error("%s: the graph is on device %d, the table on device %d", who, g->device, m->device); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    std::unique_lock<std::shared_timed_mutex> lm;
    if (m) lm = std::unique_lock<std::shared_timed_mutex>(m->mu);
    const MgDev &G = g->G;
    // the keyframes
    int nkt = 0;
    for (int q = 0; q < nk; q++) {
        const int s = job->kf_slot[q];
        if (s < 0 || s >= G.max_kf || g->kmap[s] >= 0) {
            for (int r = 0; r < q; r++) g->kmap[job->kf_slot[r]] = -1;
            if (s < 0) orbx_set_error("%s: keyframe %d: negative slot %d", who, q, s);
            else if (s >= G.max_kf) orbx_set_error("%s: keyframe %d: slot %d, max_keyframes %d", who, q, s, G.max_kf);
            else orbx_set_error("%s: keyframe slot %d listed twice", who, s);
            return s >= G.max_kf ? ORBX_E_CAPACITY : ORBX_E_INVALID;
        }
        g->kmap[s] = q;
        nkt = std::max(nkt, s + 1);
    }
    for (int q = 0; q < nk && do_desc; q++) {
        const orbx_frame *f = job->kf_frame ? job->kf_frame[q] : nullptr;
        if (f && f->device != g->device) RF_REFUSE(ORBX_E_INVALID, "%s: the graph is on device %d, the frame of keyframe slot %d on device %d", who, g->device, job->kf_slot[q], f->device);
    }
    // the points
    const int32_t *tsl = m ? (job->table_slot ? job->table_slot : job->point) : nullptr;
    g->keys.clear();
    for (int i = 0; i < n; i++) {
        const int p = job->point[i];
        if (p < 0) RF_REFUSE(ORBX_E_INVALID, "%s: entry %d: point slot %d", who, i, p);
        if (p >= G.max_points) RF_REFUSE(ORBX_E_CAPACITY, "%s: entry %d: point slot %d, max_points %d", who, i, p, G.max_points);
        g->keys.push_back((uint64_t)p);
        if (tsl && tsl[i] < 0) RF_REFUSE(ORBX_E_INVALID, "%s: entry %d: table slot %d", who, i, tsl[i]);
        if (tsl && tsl[i] >= m->capacity) RF_REFUSE(ORBX_E_CAPACITY, "%s: entry %d: table slot %d, capacity %d", who, i, tsl[i], m->capacity);
    }
    if (mg_twice(g)) RF_REFUSE(ORBX_E_INVALID, "%s: a point slot listed twice", who);
    if (m && job->table_slot) {
        g->keys.clear();
        for (int i = 0; i < n; i++) g->keys.push_back((uint64_t)tsl[i]);
        if (mg_twice(g)) RF_REFUSE(ORBX_E_INVALID, "%s: a table slot listed twice", who);
    }
    // the rows, on the mirror: what every point will report, and the longest row
    std::vector<uint8_t> expect((size_t)n, 0);
    int longest = 0;
    bool any = false;
    for (int i = 0; i < n; i++) {
        const int p = job->point[i];
        const uint32_t h = g->hw[G.hdr(p)];
        const int cnt = MG_CNT(h);
        if (!(h & MG_LIVE) || (h & MG_BAD) || cnt == 0) continue;
        longest = std::max(longest, cnt);
        int ref_idx = 0;
        bool takes = false;
        for (int e = 0; e < cnt; e++) {
            const uint32_t ent = g->hw[G.row(p, e)];
            const int k = (int)(ent >> 16), idx = (int)(ent & 0xFFFFu);
            const int q = k < G.max_kf ? g->kmap[k] : -1;
            if (q < 0) RF_REFUSE(ORBX_E_INVALID, "%s: entry %d: point slot %d is observed by keyframe slot %d, which is not listed", who, i, p, k);
            if (do_geom && k == job->ref_kf[i]) ref_idx = idx;
            if (do_desc && !job->kf_bad[q]) {
                const orbx_frame *f = job->kf_frame ? job->kf_frame[q] : nullptr;
                if (!f) RF_REFUSE(ORBX_E_INVALID, "%s: keyframe slot %d is not bad and has no resident frame", who, k);
                if (idx >= f->n) RF_REFUSE(ORBX_E_INVALID, "%s: point slot %d names feature %d of keyframe slot %d, whose frame has %d", who, p, idx, k, f->n);
                takes = true;
            }
        }
        if (do_geom) {
            const int ref = job->ref_kf[i];
            if (!mg_kf_live(g, ref) || g->kmap[ref] < 0) RF_REFUSE(ORBX_E_INVALID, "%s: entry %d: the reference keyframe slot %d is not listed or not in use", who, i, ref);
            if (ref_idx >= (int)g->hw[ref]) RF_REFUSE(ORBX_E_INVALID, "%s: entry %d: reference feature %d, keyframe slot %d has %d", who, i, ref_idx, ref, (int)g->hw[ref]);
            const int oct = (int)(g->hattr[G.at(ref, ref_idx)] & MG_OCT);
            if (oct >= job->nlevels) RF_REFUSE(ORBX_E_INVALID, "%s: entry %d: the reference feature's octave %d, nlevels %d", who, i, oct, job->nlevels);
            if (!job->pos && !(m->have[tsl[i]] & 1)) RF_REFUSE(ORBX_E_INVALID, "%s: entry %d: pos is NULL and table slot %d has never been given its geometry", who, i, tsl[i]);
            expect[i] |= ORBX_REFRESH_GEOM;
        }
        if (takes) expect[i] |= ORBX_REFRESH_DESC;
        any = true;
    }
    for (int q = 0; q < nk; q++) g->kmap[job->kf_slot[q]] = -1;   // every refusal is behind us
    CallCtx *c;
    int rc = orbx_call_ctx(g->device, &c);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t np = (size_t)n;
    const int cap = std::max(4, (longest + 3) & ~3);
    // up: pts | tslot | ref | pos | sf | kft     work and down: status | geom | best_kf | best_idx | desc
    BlobCursor up = { nullptr, nullptr, 0 };
    const size_t u_pts = up.take(4 * np), u_ts = up.take(job->table_slot ? 4 * np : 0), u_ref = up.take(do_geom ? 4 * np : 0),
                 u_pos = up.take(do_geom && job->pos ? 12 * np : 0), u_sf = up.take(do_geom ? 4 * (size_t)job->nlevels : 0),
                 u_kft = up.take(sizeof(RfKf) * (size_t)nkt), blob = up.o;
    const size_t o_st = 0, o_geom = a16(np), o_bk = o_geom + 32 * np, o_bi = o_bk + a16(4 * np), o_desc = o_bi + a16(4 * np), out = o_desc + 32 * np;
    if ((rc = call_reserve(c, blob, out, out))) return rc;
    uint8_t *hb = c->h_blob;
    memcpy(hb + u_pts, job->point, 4 * np);
    if (job->table_slot) memcpy(hb + u_ts, job->table_slot, 4 * np);
    if (do_geom) {
        memcpy(hb + u_ref, job->ref_kf, 4 * np);
        if (job->pos) memcpy(hb + u_pos, job->pos, 12 * np);
        memcpy(hb + u_sf, job->scale_factors, 4 * (size_t)job->nlevels);
    }
    RfKf *kft = (RfKf *)(hb + u_kft);
    memset(kft, 0, sizeof(RfKf) * (size_t)nkt);
    for (int s = 0; s < nkt; s++) kft[s].bad_n = RF_BAD;   // a slot that is not listed: named by no row that is worked on
    if ((rc = mg_order_before(g, st))) return rc;
    if (m && (rc = mappoints_order_before(m, st))) return rc;
    for (int q = 0; q < nk; q++) {
        RfKf &K = kft[job->kf_slot[q]];
        K.cx = job->kf_centre[3 * q]; K.cy = job->kf_centre[3 * q + 1]; K.cz = job->kf_centre[3 * q + 2];
        const orbx_frame *f = do_desc && job->kf_frame && !job->kf_bad[q] ? job->kf_frame[q] : nullptr;
        K.bad_n = f ? (uint32_t)f->n : RF_BAD;
        K.desc = f ? (const uint32_t *)(f->blk.d + f->o_desc) : nullptr;
        if (f && (rc = frame_order_before(f, st))) return rc;
    }
    if (any) {
        ORBX_HIP(hipMemcpyAsync(c->d_blob, c->h_blob, blob, hipMemcpyHostToDevice, st));
        RfArgs A;
        memset(&A, 0, sizeof A);
        A.G = G; A.n = n; A.what = what; A.cap = cap; A.nkt = nkt; A.nlevels = job->nlevels;
        const uint8_t *db = c->d_blob;
        uint8_t *wk = c->d_work;
        A.pts = (const int32_t *)(db + u_pts);
        A.tslot = m ? (const int32_t *)(db + (job->table_slot ? u_ts : u_pts)) : nullptr;
        A.ref = do_geom ? (const int32_t *)(db + u_ref) : nullptr;
        A.pos = do_geom && job->pos ? (const float *)(db + u_pos) : nullptr;
        A.sf = do_geom ? (const float *)(db + u_sf) : nullptr;
        A.kft = (const RfKf *)(db + u_kft);
        A.tgeom = m ? m->d_geom : nullptr; A.tdesc = m ? m->d_desc : nullptr;
        A.status = wk + o_st; A.geom = (float4 *)(wk + o_geom); A.best_kf = (int32_t *)(wk + o_bk); A.best_idx = (int32_t *)(wk + o_bi);
        A.desc = (uint4 *)(wk + o_desc);
        const size_t lds = rf_lds_bytes(cap);
        if (lds > 32768) ORBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mp_refresh), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_mp_refresh, dim3((unsigned)std::min(n, 4096)), dim3(64), lds, st, A);
        ORBX_HIP(hipGetLastError());
        if (m) {
            ORBX_HIP(hipEventRecord(m->ev, st));
            m->ev_stream = st; m->ev_set = true;
            for (int i = 0; i < n; i++) m->have[tsl[i]] |= expect[i];   // what has been enqueued is in the table for every later call
        }
        uint8_t *ho = (uint8_t *)c->h_out;
        ORBX_HIP(hipMemcpyAsync(ho + o_st, wk + o_st, np, hipMemcpyDeviceToHost, st));
        if (geom && do_geom) ORBX_HIP(hipMemcpyAsync(ho + o_geom, wk + o_geom, 32 * np, hipMemcpyDeviceToHost, st));
        if (best_kf && do_desc) ORBX_HIP(hipMemcpyAsync(ho + o_bk, wk + o_bk, 4 * np, hipMemcpyDeviceToHost, st));
        if (best_idx && do_desc) ORBX_HIP(hipMemcpyAsync(ho + o_bi, wk + o_bi, 4 * np, hipMemcpyDeviceToHost, st));
        if (desc && do_desc) ORBX_HIP(hipMemcpyAsync(ho + o_desc, wk + o_desc, 32 * np, hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < n; i++)
            if (ho[o_st + i] != expect[i]) { orbx_set_error("%s: entry %d: the device reports status %d, the host's mirror %d: the graph is inconsistent", who, i, ho[o_st + i], expect[i]); return ORBX_E_HIP; }
        for (int i = 0; i < n; i++) {   // a row whose bit is clear stays as the caller left it
            const size_t ii = (size_t)i;
            if ((expect[i] & ORBX_REFRESH_GEOM) && geom) memcpy(geom + 8 * ii, ho + o_geom + 32 * ii, 32);
            if (expect[i] & ORBX_REFRESH_DESC) {
                if (best_kf) best_kf[i] = ((const int32_t *)(ho + o_bk))[i];
                if (best_idx) best_idx[i] = ((const int32_t *)(ho + o_bi))[i];
                if (desc) memcpy(desc + 32 * ii, ho + o_desc + 32 * ii, 32);
            }
        }
    }
    if (status) memcpy(status, expect.data(), np);
    return ORBX_OK;
}

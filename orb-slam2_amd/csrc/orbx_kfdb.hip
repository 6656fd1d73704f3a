// orbx_kfdb.hip — KeyFrameDatabase on the device: the place-recognition query that starts Tracking::Relocalization
// (reference src/Tracking.cc:1650) and LoopClosing::DetectLoop (src/LoopClosing.cc:143-175): src/KeyFrameDatabase.cc:40-73 (add / erase /
// clear), :80-229 (DetectLoopCandidates), :234-349 (DetectRelocalizationCandidates), with L1Scoring::score
// (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).
//
// The keyframes' BowVectors live in HBM as a CSR arena (ascending uint32 word ids, double values).  No inverted file exists: the
// reference walks the query's words in ascending order and each word's posting list in insertion order, so a keyframe's place in
// lKFsSharingWords is its (smallest common word id, add sequence) -- a pure function of the data.  A query is
//   k_kfdb_count   per (query, keyframe): common words and the smallest common word id; per query the maximum (the 0.8 gate)
//   k_kfdb_score   per gated pair: the L1 score, terms formed in parallel and added in ascending word order into one double
//   k_kfdb_select  per query: covisibility accumulation, the 0.75 gate, first-occurrence de-duplication, the list in return order
//   k_kfdb_persist the relocalisation score each keyframe keeps between queries (mRelocScore, KeyFrameDatabase.cc:289 / :315)
// and the per-call forms are the batched form with a batch of one.
#include "orbx_device.h"
#include <limits.h>
#include <math.h>
#include <string.h>
#include <mutex>
#include <vector>

#define KFDB_QT 4096            // query words per LDS tile (longer queries take several passes)
#define KFDB_BM_BITS 16384      // hashed membership bitmap in front of the exact binary search
#define KFDB_NEIGH 10           // KeyFrame::GetBestCovisibilityKeyFrames(10)
#define KFDB_MAX_BATCH 1024

struct KfdbQuery {              // `batch` queries on the device: query b has min(n[b * nstride], cap) words at id / val + b * stride
    const uint32_t *id; const double *val; const int *n;
    long long stride; int nstride, cap;
};

struct orbx_kfdb {
    int device, nwords;
    std::mutex mu;
    hipStream_t stream;
    hipStream_t pending;        // caller stream of a batched query still in flight on the workspace (waited for by the next call) ...
    bool has_pending;           // ... when set: nullptr is a stream too (the legacy default stream of frames no transform has touched)
    // host mirror of the per-keyframe records (index = id = add sequence number)
    std::vector<long long> off; std::vector<int> len; std::vector<uint8_t> live;
    int nlive; long long used, live_words;
    // device
    uint32_t *d_ids; double *d_vals; long long arena_cap;
    long long *d_off; int *d_len; int *d_neigh; float *d_persist; int id_cap;   // d_len == 0: erased (or empty: shares no word either way)
    uint8_t *d_ws; size_t ws_cap;
    uint8_t *d_q; size_t q_cap;
    uint8_t *h_pin; size_t h_cap;
};

__device__ __forceinline__ int kfdb_nq(const KfdbQuery &Q, int q) { return max(0, min(Q.n[(long long)q * Q.nstride], Q.cap)); }
__device__ __forceinline__ int kfdb_min_common(int max_common) { return (int)((float)max_common * 0.8f); }     // KeyFrameDatabase.cc:145 / :273

// words [lo, lo + tn) of a query into LDS, with their hashed bitmap
__device__ __forceinline__ int kfdb_load_tile(const uint32_t *qid, const double *qval, int nq, int t, uint32_t *s_id, double *s_val, uint32_t *s_bm)
{
    const int lo = t * KFDB_QT, tn = max(0, min(KFDB_QT, nq - lo));
    __syncthreads();
    for (int i = threadIdx.x; i < KFDB_BM_BITS / 32; i += blockDim.x) s_bm[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < tn; i += blockDim.x) {
        const uint32_t w = qid[lo + i];
        s_id[i] = w;
        if (s_val) s_val[i] = qval[lo + i];
        const uint32_t h = w & (KFDB_BM_BITS - 1);
        atomicOr(&s_bm[h >> 5], 1u << (h & 31));
    }
    __syncthreads();
    return tn;
}

__device__ __forceinline__ int kfdb_find(const uint32_t *s_id, int tn, const uint32_t *s_bm, uint32_t w)
{
    const uint32_t h = w & (KFDB_BM_BITS - 1);
    if (!((s_bm[h >> 5] >> (h & 31)) & 1u)) return -1;
    int lo = 0, hi = tn;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_id[mid] < w) lo = mid + 1; else hi = mid; }
    return (lo < tn && s_id[lo] == w) ? lo : -1;
}

// grid (x, batch): a workgroup holds one tile of its query in LDS and its four waves take a keyframe each, streaming the keyframe's word
// ids once per tile.  This is the forward form of the inverted-file walk of :94-128 / :243-259: mnLoopWords / mnRelocWords is the size of the
// intersection, and the place in lKFsSharingWords follows from the smallest common word.  excl (loop query): keyframes of
// spConnectedKeyFrames share nothing (:120).
__global__ __launch_bounds__(256) void k_kfdb_count(const uint32_t *__restrict__ ids, const long long *__restrict__ off, const int *__restrict__ len,
                                                    int nids, KfdbQuery Q, const uint8_t *__restrict__ excl, int *__restrict__ words,
                                                    uint32_t *__restrict__ minw, unsigned long long *__restrict__ firstkey, int *__restrict__ maxw)
{
    __shared__ uint32_t s_id[KFDB_QT];
    __shared__ uint32_t s_bm[KFDB_BM_BITS / 32];
    const int q = blockIdx.y, nq = kfdb_nq(Q, q);
    const uint32_t *qid = Q.id + (long long)q * Q.stride;
    const int per = (nids + gridDim.x - 1) / gridDim.x, i0 = blockIdx.x * per, i1 = min(nids, i0 + per);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ntiles = max(1, (nq + KFDB_QT - 1) / KFDB_QT);
    for (int t = 0; t < ntiles; t++) {
        const int tn = kfdb_load_tile(qid, nullptr, nq, t, s_id, nullptr, s_bm);
        for (int id = i0 + wave; id < i1; id += 4) {
            const int L = (excl && excl[id]) ? 0 : len[id];
            const long long o = off[id];
            int c = 0; uint32_t mn = 0xFFFFFFFFu;
            if (tn > 0)
                for (int base = 0; base < L; base += 64) {
                    const int k = base + lane;
                    if (k < L) {
                        const uint32_t w = ids[o + k];
                        if (kfdb_find(s_id, tn, s_bm, w) >= 0) { c++; mn = min(mn, w); }
                    }
                }
            c = wave_sum(c); mn = wave_min_u32(mn);
            if (lane == 0) {
                const long long idx = (long long)q * nids + id;
                if (t) { c += words[idx]; mn = min(mn, minw[idx]); }
                words[idx] = c; minw[idx] = mn;
                if (t == ntiles - 1) {
                    firstkey[idx] = ~0ull;
                    if (c > 0) atomicMax(&maxw[q], c);
                }
            }
        }
    }
}

// L1Scoring::score(query, keyframe) (ScoringObject.cpp:23-68) for the pairs that pass the common-words gate (list == nullptr, :155 / :284)
// or for an explicit list of keyframes.  A wave takes a pair: 64 keyframe words at a time look themselves up in the query tile and form
// fabs(vi - wi) - fabs(vi) - fabs(wi); the terms of the matching lanes are then added in lane order, i.e. in ascending word order, into ONE
// double (uniform v_readlane broadcasts, as k_bow_build adds its L1 norm).  Tiles ascend in word id too, so the partial sum carried between
// tiles (sd) keeps the order.  si = (float)(-sum / 2.0) where the reference assigns to float; out_d keeps the double.
__global__ __launch_bounds__(256) void k_kfdb_score(const uint32_t *__restrict__ ids, const double *__restrict__ vals, const long long *__restrict__ off,
                                                    const int *__restrict__ len, int nids, KfdbQuery Q, const int *__restrict__ list, int nlist,
                                                    const int *__restrict__ words, const int *__restrict__ maxw, float *__restrict__ si,
                                                    double *__restrict__ sd, double *__restrict__ out_d)
{
    __shared__ uint32_t s_id[KFDB_QT];
    __shared__ double s_val[KFDB_QT];
    __shared__ uint32_t s_bm[KFDB_BM_BITS / 32];
    const int q = blockIdx.y, nq = kfdb_nq(Q, q);
    const uint32_t *qid = Q.id + (long long)q * Q.stride;
    const double *qval = Q.val + (long long)q * Q.stride;
    const int nitems = list ? nlist : nids;
    const int min_common = list ? 0 : kfdb_min_common(maxw[q]);
    const int per = (nitems + gridDim.x - 1) / gridDim.x, i0 = blockIdx.x * per, i1 = min(nitems, i0 + per);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int pass = 0;
    for (int it = i0 + (int)threadIdx.x; it < i1; it += 256) pass |= list ? 1 : (words[(long long)q * nids + it] > min_common);
    if (!__syncthreads_or(pass)) return;
    const int ntiles = max(1, (nq + KFDB_QT - 1) / KFDB_QT);
    for (int t = 0; t < ntiles; t++) {
        const int tn = kfdb_load_tile(qid, qval, nq, t, s_id, s_val, s_bm);
        for (int it = i0 + wave; it < i1; it += 4) {
            const int id = list ? list[it] : it;
            if (!list && !(words[(long long)q * nids + it] > min_common)) continue;
            const long long slot = (long long)q * nitems + it;
            double acc = t ? sd[slot] : 0.0;
            const int L = len[id];
            const long long o = off[id];
            if (tn > 0)
                for (int base = 0; base < L; base += 64) {
                    const int k = base + lane;
                    int j = -1;
                    double term = 0.0;
                    if (k < L) {
                        j = kfdb_find(s_id, tn, s_bm, ids[o + k]);
                        if (j >= 0) { const double vi = s_val[j], wi = vals[o + k]; term = fabs(vi - wi) - fabs(vi) - fabs(wi); }
                    }
                    unsigned long long m = __ballot(j >= 0);
                    const int t_lo = __double2loint(term), t_hi = __double2hiint(term);
                    while (m) {
                        const int b = __builtin_ctzll(m);
                        m &= m - 1;
                        acc += __hiloint2double(__builtin_amdgcn_readlane(t_hi, b), __builtin_amdgcn_readlane(t_lo, b));
                    }
                }
            if (lane == 0) {
                if (t < ntiles - 1) sd[slot] = acc;
                else {
                    const double s = -acc / 2.0;
                    if (list) out_d[it] = s; else si[slot] = (float)s;
                }
            }
        }
    }
}

// mRelocScore of neighbour n as query q reads it (:312-315): this query's score if it scored n, else the score of the last earlier query of
// the batch that did, else what the handle kept from before the batch
__device__ __forceinline__ float kfdb_reloc_score(int q, int n, int nids, const int *words, const float *si, const float *persist, const int *s_minc)
{
    for (int p = q; p >= 0; p--)
        if (words[(long long)p * nids + n] > s_minc[p]) return si[(long long)p * nids + n];
    return persist[n];
}

// one workgroup per query: :178-228 (loop = 1) / :297-346 (loop = 0) in fp32.  The order of lAccScoreAndMatch enters the result only through
// the de-duplication (the first group that names a keyframe places it), so no list is sorted: every retained group posts its key
// (smallest common word, id) to its best keyframe with atomicMin, and the posted keyframes are ranked by that key (a counting rank: cnt * cnt
// loads for a list of cnt keyframes -- a handful in place recognition, about 2 per query on the place scenes; quadratic only in the LIST).
__global__ __launch_bounds__(256) void k_kfdb_select(int nids, const int *__restrict__ len, const int *__restrict__ neigh, const float *__restrict__ persist,
                                                     const int *__restrict__ words, const uint32_t *__restrict__ minw, const float *__restrict__ si,
                                                     float *__restrict__ accv, int *__restrict__ bestv, int *__restrict__ list,
                                                     unsigned long long *__restrict__ firstkey, const int *__restrict__ maxw, int loop, float min_score,
                                                     int *__restrict__ cand, int cap, int *__restrict__ ncand)
{
    __shared__ int s_minc[KFDB_MAX_BATCH];
    __shared__ float s_red[256];
    __shared__ int s_cnt;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (maxw[q] == 0) { if (tid == 0) ncand[q] = 0; return; }     // lKFsSharingWords.empty() (:131 / :261)
    for (int p = tid; p <= q; p += 256) s_minc[p] = kfdb_min_common(maxw[p]);
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const int min_common = s_minc[q];
    const long long qo = (long long)q * nids;
    float best_acc = loop ? min_score : 0.0f;                        // :171 / :298
    for (int id = tid; id < nids; id += 256) {
        int best = -1;
        float acc = 0.0f;
        if (words[qo + id] > min_common && (!loop || si[qo + id] >= min_score)) {     // lScoreAndMatch (:162-163 / :290)
            float best_score = si[qo + id];
            acc = best_score; best = id;
            for (int k = 0; k < KFDB_NEIGH; k++) {
                const int n = neigh[(long long)id * KFDB_NEIGH + k];
                if (n < 0 || n >= nids || len[n] == 0) continue;     // unknown or erased: the reference's lists never hold it
                float s2;
                if (loop) {                                          // :189: queried by this keyframe AND past the gate
                    if (!(words[qo + n] > min_common)) continue;
                    s2 = si[qo + n];
                } else {                                             // :312: shares a word; the score may be a stale one
                    if (!(words[qo + n] > 0)) continue;
                    s2 = kfdb_reloc_score(q, n, nids, words, si, persist, s_minc);
                }
                acc += s2;
                if (s2 > best_score) { best = n; best_score = s2; }
            }
            if (acc > best_acc) best_acc = acc;
        }
        accv[qo + id] = acc; bestv[qo + id] = best;
    }
    s_red[tid] = best_acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s && s_red[tid + s] > s_red[tid]) s_red[tid] = s_red[tid + s];
        __syncthreads();
    }
    const float min_retain = 0.75f * s_red[0];                       // :207 / :330
    for (int id = tid; id < nids; id += 256) {
        const int best = bestv[qo + id];
        if (best >= 0 && accv[qo + id] > min_retain)
            atomicMin(&firstkey[qo + best], ((unsigned long long)minw[qo + id] << 32) | (unsigned)id);
    }
    __threadfence_block();
    __syncthreads();
    for (int id = tid; id < nids; id += 256)
        if (__hip_atomic_load(&firstkey[qo + id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ull) list[qo + atomicAdd(&s_cnt, 1)] = id;
    __threadfence_block();
    __syncthreads();
    const int cnt = s_cnt;
    for (int c = tid; c < cnt; c += 256) {
        const int id = list[qo + c];
        const unsigned long long key = __hip_atomic_load(&firstkey[qo + id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int rank = 0;
        for (int j = 0; j < cnt; j++)
            rank += __hip_atomic_load(&firstkey[qo + list[qo + j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key;
        if (rank < cap) cand[(long long)q * cap + rank] = id;
    }
    if (tid == 0) ncand[q] = cnt;
}

// after a batch of relocalisation queries: every keyframe keeps the score of the last query that scored it (:289)
__global__ __launch_bounds__(256) void k_kfdb_persist(int nids, int batch, const int *__restrict__ words, const float *__restrict__ si,
                                                      const int *__restrict__ maxw, float *__restrict__ persist)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= nids) return;
    for (int p = batch - 1; p >= 0; p--)
        if (words[(long long)p * nids + id] > kfdb_min_common(maxw[p])) { persist[id] = si[(long long)p * nids + id]; return; }
}

// arena growth: live keyframes move to their new offsets, erased ones are dropped (one workgroup per keyframe)
__global__ __launch_bounds__(256) void k_kfdb_compact(const uint32_t *__restrict__ ids, const double *__restrict__ vals, const long long *__restrict__ off,
                                                      const long long *__restrict__ noff, const int *__restrict__ len,
                                                      uint32_t *__restrict__ nids_, double *__restrict__ nvals)
{
    const int id = blockIdx.x, L = len[id];
    const long long o = off[id], n = noff[id];
    for (int i = threadIdx.x; i < L; i += 256) { nids_[n + i] = ids[o + i]; nvals[n + i] = vals[o + i]; }
}

// ---------------------------------------------------------------- host side

static int kfdb_enter(orbx_kfdb *db)
{
    ORBX_HIP(orbx_use_device(db->device));
    if (db->has_pending) { ORBX_HIP(hipStreamSynchronize(db->pending)); db->has_pending = false; db->pending = nullptr; }
    return ORBX_OK;
}

static int kfdb_grow_ids(orbx_kfdb *db, int need)
{
    if (need <= db->id_cap) return ORBX_OK;
    int cap = db->id_cap ? db->id_cap : 1024;
    while (cap < need) cap *= 2;
    long long *n_off = nullptr; int *n_len = nullptr, *n_neigh = nullptr; float *n_persist = nullptr;
    const size_t n = db->off.size();
    hipError_t e = hipMalloc((void **)&n_off, sizeof(long long) * cap);
    if (e == hipSuccess) e = hipMalloc((void **)&n_len, sizeof(int) * cap);
    if (e == hipSuccess) e = hipMalloc((void **)&n_neigh, sizeof(int) * KFDB_NEIGH * (size_t)cap);
    if (e == hipSuccess) e = hipMalloc((void **)&n_persist, sizeof(float) * cap);
    if (e == hipSuccess) e = hipMemset(n_off, 0, sizeof(long long) * cap);
    if (e == hipSuccess) e = hipMemset(n_len, 0, sizeof(int) * cap);
    if (e == hipSuccess) e = hipMemset(n_neigh, 0xFF, sizeof(int) * KFDB_NEIGH * (size_t)cap);
    if (e == hipSuccess) e = hipMemset(n_persist, 0, sizeof(float) * cap);
    if (n) {
        if (e == hipSuccess) e = hipMemcpy(n_off, db->d_off, sizeof(long long) * n, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(n_len, db->d_len, sizeof(int) * n, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(n_neigh, db->d_neigh, sizeof(int) * KFDB_NEIGH * n, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(n_persist, db->d_persist, sizeof(float) * n, hipMemcpyDeviceToDevice);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {                   // the handle keeps its old arrays; nothing of the attempt stays allocated
        void *fresh[] = { n_off, n_len, n_neigh, n_persist };
        for (void *p : fresh) if (p) hipFree(p);
        orbx_set_error("orbx_kfdb: growing the per-keyframe arrays to %d failed: %s", cap, hipGetErrorString(e));
        return ORBX_E_HIP;
    }
    void *old[] = { db->d_off, db->d_len, db->d_neigh, db->d_persist };
    for (void *p : old) if (p) hipFree(p);
    db->d_off = n_off; db->d_len = n_len; db->d_neigh = n_neigh; db->d_persist = n_persist; db->id_cap = cap;
    return ORBX_OK;
}

// room for `n` more words behind `used`; growing also reclaims the storage of erased keyframes
static int kfdb_grow_arena(orbx_kfdb *db, int n)
{
    if (db->used + n <= db->arena_cap) return ORBX_OK;
    long long cap = 2 * (db->live_words + n);
    if (cap < (1 << 16)) cap = 1 << 16;
    uint32_t *n_ids = nullptr; double *n_vals = nullptr;
    const int nids = (int)db->off.size();
    long long used = 0;
    long long *d_noff = nullptr;
    std::vector<long long> noff(nids);
    for (int i = 0; i < nids; i++) { noff[i] = used; if (db->live[i]) used += db->len[i]; }
    hipError_t e = hipMalloc((void **)&n_ids, sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMalloc((void **)&n_vals, sizeof(double) * cap);
    if (nids) {
        if (e == hipSuccess) e = hipMalloc((void **)&d_noff, sizeof(long long) * nids);
        if (e == hipSuccess) e = hipMemcpy(d_noff, noff.data(), sizeof(long long) * nids, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_kfdb_compact, dim3(nids), dim3(256), 0, db->stream, db->d_ids, db->d_vals, db->d_off, d_noff, db->d_len, n_ids, n_vals);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
        // (the old arena and its offsets stay valid until the new offsets have landed: they go up last)
        if (e == hipSuccess) e = hipMemcpy(db->d_off, noff.data(), sizeof(long long) * nids, hipMemcpyHostToDevice);
    }
    if (d_noff) hipFree(d_noff);
    if (e != hipSuccess) {
        if (n_ids) hipFree(n_ids);
        if (n_vals) hipFree(n_vals);
        orbx_set_error("orbx_kfdb: growing the arena to %lld words failed: %s", cap, hipGetErrorString(e));
        return ORBX_E_HIP;
    }
    if (nids) db->off = noff;
    if (db->d_ids) hipFree(db->d_ids);
    if (db->d_vals) hipFree(db->d_vals);
    db->d_ids = n_ids; db->d_vals = n_vals; db->arena_cap = cap; db->used = used;
    return ORBX_OK;
}

static int kfdb_ws(orbx_kfdb *db, size_t bytes) { return bytes > db->ws_cap ? ensure(&db->d_ws, &db->ws_cap, 2 * bytes) : ORBX_OK; }
static int kfdb_pin(orbx_kfdb *db, size_t bytes) { return bytes > db->h_cap ? ensure_pinned(&db->h_pin, &db->h_cap, 2 * bytes) : ORBX_OK; }

static int kfdb_check_vector(const char *who, int nwords, const uint32_t *id, const double *val, int n)
{
    if (n < 0 || (n && (!id || !val))) { orbx_set_error("%s: invalid BowVector (n = %d or null arrays)", who, n); return ORBX_E_INVALID; }
    for (int i = 0; i < n; i++) {
        if (id[i] >= (uint32_t)nwords) { orbx_set_error("%s: invalid word id %u at %d (the vocabulary has %d words)", who, id[i], i, nwords); return ORBX_E_INVALID; }
        if (i && id[i] <= id[i - 1]) { orbx_set_error("%s: invalid BowVector, word ids not ascending at %d", who, i); return ORBX_E_INVALID; }
        if (!std::isfinite(val[i])) { orbx_set_error("%s: invalid BowVector, value %d is not finite", who, i); return ORBX_E_INVALID; }
    }
    return ORBX_OK;
}

extern "C" int orbx_kfdb_create(int device, int nwords, orbx_kfdb **out)
{
    if (!out || nwords < 1) { orbx_set_error("orbx_kfdb_create: invalid argument"); return ORBX_E_INVALID; }
    *out = nullptr;
    if (int rc = orbx_check_device(device)) return rc;
    ORBX_HIP(hipSetDevice(device));
    orbx_kfdb *db = new orbx_kfdb();
    db->device = device; db->nwords = nwords; db->stream = nullptr; db->pending = nullptr; db->has_pending = false;
    db->nlive = 0; db->used = 0; db->live_words = 0;
    db->d_ids = nullptr; db->d_vals = nullptr; db->arena_cap = 0;
    db->d_off = nullptr; db->d_len = nullptr; db->d_neigh = nullptr; db->d_persist = nullptr; db->id_cap = 0;
    db->d_ws = nullptr; db->ws_cap = 0; db->d_q = nullptr; db->q_cap = 0; db->h_pin = nullptr; db->h_cap = 0;
    if (hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess) { orbx_set_error("orbx_kfdb_create: no stream"); delete db; return ORBX_E_HIP; }
    *out = db;
    return ORBX_OK;
}

extern "C" void orbx_kfdb_destroy(orbx_kfdb *db)
{
    if (!db) return;
    hipSetDevice(db->device);
    if (db->has_pending) hipStreamSynchronize(db->pending);
    if (db->stream) { hipStreamSynchronize(db->stream); hipStreamDestroy(db->stream); }
    void *ptrs[] = { db->d_ids, db->d_vals, db->d_off, db->d_len, db->d_neigh, db->d_persist, db->d_ws, db->d_q };
    for (void *p : ptrs) if (p) hipFree(p);
    if (db->h_pin) hipHostFree(db->h_pin);
    delete db;
}

extern "C" int orbx_kfdb_size(orbx_kfdb *db)
{
    if (!db) { orbx_set_error("null keyframe database"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> g(db->mu);
    return db->nlive;
}

extern "C" int orbx_kfdb_next_id(orbx_kfdb *db)
{
    if (!db) { orbx_set_error("null keyframe database"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> g(db->mu);
    return (int)db->off.size();
}

extern "C" int orbx_kfdb_clear(orbx_kfdb *db)
{
    if (!db) { orbx_set_error("null keyframe database"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> g(db->mu);
    if (int rc = kfdb_enter(db)) return rc;
    const size_t n = db->off.size();
    if (n) {
        ORBX_HIP(hipMemset(db->d_len, 0, sizeof(int) * n));
        ORBX_HIP(hipMemset(db->d_neigh, 0xFF, sizeof(int) * KFDB_NEIGH * n));
        ORBX_HIP(hipMemset(db->d_persist, 0, sizeof(float) * n));
        ORBX_HIP(hipDeviceSynchronize());
    }
    db->off.clear(); db->len.clear(); db->live.clear();
    db->nlive = 0; db->used = 0; db->live_words = 0;
    return ORBX_OK;
}

// the new keyframe's record, once its words are in the arena at db->used
static int kfdb_commit(orbx_kfdb *db, int n, int *id)
{
    const int k = (int)db->off.size();
    const long long o = db->used;
    ORBX_HIP(hipMemcpy(db->d_off + k, &o, sizeof o, hipMemcpyHostToDevice));
    ORBX_HIP(hipMemcpy(db->d_len + k, &n, sizeof n, hipMemcpyHostToDevice));
    db->off.push_back(o); db->len.push_back(n); db->live.push_back(1);
    db->used += n; db->live_words += n; db->nlive++;
    if (id) *id = k;
    return ORBX_OK;
}

extern "C" int orbx_kfdb_add(orbx_kfdb *db, const uint32_t *bow_id, const double *bow_val, int nbow, int *id)
{
    if (!db) { orbx_set_error("null keyframe database"); return ORBX_E_INVALID; }
    if (int rc = kfdb_check_vector("orbx_kfdb_add", db->nwords, bow_id, bow_val, nbow)) return rc;
    std::lock_guard<std::mutex> g(db->mu);
    if (int rc = kfdb_enter(db)) return rc;
    if (int rc = kfdb_grow_ids(db, (int)db->off.size() + 1)) return rc;
    if (int rc = kfdb_grow_arena(db, nbow)) return rc;
    if (nbow) {
        ORBX_HIP(hipMemcpy(db->d_ids + db->used, bow_id, sizeof(uint32_t) * nbow, hipMemcpyHostToDevice));
        ORBX_HIP(hipMemcpy(db->d_vals + db->used, bow_val, sizeof(double) * nbow, hipMemcpyHostToDevice));
    }
    return kfdb_commit(db, nbow, id);
}

extern "C" int orbx_kfdb_add_from_frames(orbx_kfdb *db, orbx_bow_frames *f, int index, void *stream, int *id)
{
    if (!db || !f || index < 0 || index >= f->batch || f->device != db->device) { orbx_set_error("orbx_kfdb_add_from_frames: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> g(db->mu);
    if (int rc = kfdb_enter(db)) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : f->last_stream;
    int n = 0;
    ORBX_HIP(hipMemcpyAsync(&n, f->counts + 2 * (size_t)index, sizeof n, hipMemcpyDeviceToHost, s));    // the count alone comes to the host (arena bookkeeping)
    ORBX_HIP(hipStreamSynchronize(s));
    n = n < 0 ? 0 : (n > f->cap ? f->cap : n);
    if (int rc = kfdb_grow_ids(db, (int)db->off.size() + 1)) return rc;
    if (int rc = kfdb_grow_arena(db, n)) return rc;
    if (n) {
        ORBX_HIP(hipMemcpyAsync(db->d_ids + db->used, f->bow_id + (size_t)index * f->cap, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, s));
        ORBX_HIP(hipMemcpyAsync(db->d_vals + db->used, f->bow_val + (size_t)index * f->cap, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
        ORBX_HIP(hipStreamSynchronize(s));
    }
    return kfdb_commit(db, n, id);
}

// a BowVector computed elsewhere into slot `index` of an orbx_bow_frames (the FeatureVector of the slot is left alone): the query / add forms
// that take frames then serve a host-side vector too
extern "C" int orbx_bow_frames_set_bow(orbx_bow_frames *f, int index, const uint32_t *bow_id, const double *bow_val, int nbow, void *stream)
{
    if (!f || index < 0 || index >= f->batch || nbow < 0 || nbow > f->cap || (nbow && (!bow_id || !bow_val))) {
        orbx_set_error("orbx_bow_frames_set_bow: invalid argument (nbow <= cap)");
        return ORBX_E_INVALID;
    }
    for (int i = 0; i < nbow; i++) {
        if (i && bow_id[i] <= bow_id[i - 1]) { orbx_set_error("orbx_bow_frames_set_bow: invalid BowVector, word ids not ascending at %d", i); return ORBX_E_INVALID; }
        if (!std::isfinite(bow_val[i])) { orbx_set_error("orbx_bow_frames_set_bow: invalid BowVector, value %d is not finite", i); return ORBX_E_INVALID; }
    }
    ORBX_HIP(orbx_use_device(f->device));
    hipStream_t s = stream ? (hipStream_t)stream : f->last_stream;
    if (nbow) {
        ORBX_HIP(hipMemcpyAsync(f->bow_id + (size_t)index * f->cap, bow_id, sizeof(uint32_t) * nbow, hipMemcpyHostToDevice, s));
        ORBX_HIP(hipMemcpyAsync(f->bow_val + (size_t)index * f->cap, bow_val, sizeof(double) * nbow, hipMemcpyHostToDevice, s));
    }
    ORBX_HIP(hipMemcpyAsync(f->counts + 2 * (size_t)index, &nbow, sizeof nbow, hipMemcpyHostToDevice, s));
    ORBX_HIP(hipStreamSynchronize(s));
    if (stream) f->last_stream = s;
    return ORBX_OK;
}

static bool kfdb_is_live(const orbx_kfdb *db, int id) { return id >= 0 && id < (int)db->live.size() && db->live[id]; }

extern "C" int orbx_kfdb_erase(orbx_kfdb *db, int id)
{
    if (!db) { orbx_set_error("null keyframe database"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> g(db->mu);
    if (!kfdb_is_live(db, id)) { orbx_set_error("orbx_kfdb_erase: invalid id %d (unknown or already erased)", id); return ORBX_E_INVALID; }
    if (int rc = kfdb_enter(db)) return rc;
    const int zero = 0;
    ORBX_HIP(hipMemcpy(db->d_len + id, &zero, sizeof zero, hipMemcpyHostToDevice));
    db->live[id] = 0; db->nlive--; db->live_words -= db->len[id];
    return ORBX_OK;
}

extern "C" int orbx_kfdb_set_covisibility(orbx_kfdb *db, int id, const int32_t *neigh_ids, int n)
{
    if (!db || n < 0 || n > KFDB_NEIGH || (n && !neigh_ids)) { orbx_set_error("orbx_kfdb_set_covisibility: invalid argument (at most %d neighbours)", KFDB_NEIGH); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> g(db->mu);
    if (!kfdb_is_live(db, id)) { orbx_set_error("orbx_kfdb_set_covisibility: invalid id %d (unknown or erased)", id); return ORBX_E_INVALID; }
    if (int rc = kfdb_enter(db)) return rc;
    int32_t row[KFDB_NEIGH];
    for (int k = 0; k < KFDB_NEIGH; k++) row[k] = k < n ? neigh_ids[k] : -1;
    ORBX_HIP(hipMemcpy(db->d_neigh + (size_t)id * KFDB_NEIGH, row, sizeof row, hipMemcpyHostToDevice));
    return ORBX_OK;
}

extern "C" int orbx_kfdb_reloc_scores(orbx_kfdb *db, float *scores, int n)
{
    if (!db || n < 0 || (n && !scores)) { orbx_set_error("orbx_kfdb_reloc_scores: invalid argument"); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> g(db->mu);
    if (int rc = kfdb_enter(db)) return rc;
    const int m = n < (int)db->off.size() ? n : (int)db->off.size();
    if (m) ORBX_HIP(hipMemcpy(scores, db->d_persist, sizeof(float) * m, hipMemcpyDeviceToHost));
    for (int i = m; i < n; i++) scores[i] = 0.0f;
    return ORBX_OK;
}

// a query vector for the kernels: uploaded from the host, or in place in an orbx_bow_frames (whose transform is waited for)
static int kfdb_query(orbx_kfdb *db, const char *who, const uint32_t *qid, const double *qval, int nq, orbx_bow_frames *f, int index, KfdbQuery *Q)
{
    if (f) {
        if (index < 0 || index >= f->batch || f->device != db->device) { orbx_set_error("%s: invalid frame index %d", who, index); return ORBX_E_INVALID; }
        if (f->last_stream != db->stream) ORBX_HIP(hipStreamSynchronize(f->last_stream));
        Q->id = f->bow_id + (size_t)index * f->cap; Q->val = f->bow_val + (size_t)index * f->cap; Q->n = f->counts + 2 * (size_t)index;
        Q->stride = f->cap; Q->nstride = 2; Q->cap = f->cap;
        return ORBX_OK;
    }
    if (int rc = kfdb_check_vector(who, db->nwords, qid, qval, nq)) return rc;
    const size_t o_val = a16(4 * (size_t)nq + 16), total = o_val + 8 * (size_t)nq + 16;
    if (total > db->q_cap) if (int rc = ensure(&db->d_q, &db->q_cap, 2 * total)) return rc;
    if (int rc = kfdb_pin(db, total)) return rc;
    // [n | ids ...][vals ...] through the pinned block: one upload
    memcpy(db->h_pin, &nq, sizeof nq);
    if (nq) { memcpy(db->h_pin + 16, qid, 4 * (size_t)nq); memcpy(db->h_pin + o_val, qval, 8 * (size_t)nq); }
    ORBX_HIP(hipMemcpyAsync(db->d_q, db->h_pin, total, hipMemcpyHostToDevice, db->stream));
    ORBX_HIP(hipStreamSynchronize(db->stream));      // the pinned block is reused for the results
    Q->n = (const int *)db->d_q; Q->id = (const uint32_t *)(db->d_q + 16); Q->val = (const double *)(db->d_q + o_val);
    Q->stride = 0; Q->nstride = 0; Q->cap = INT_MAX;
    return ORBX_OK;
}

struct KfdbWs {
    int *words; uint32_t *minw; float *si, *accv; int *bestv, *list; unsigned long long *firstkey; double *sd;
    int *maxw, *ncand, *cand; uint8_t *excl;
    size_t total;
};

static KfdbWs kfdb_carve(uint8_t *base, size_t batch, size_t nids, size_t cap)
{
    KfdbWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { uint8_t *r = base + o; o += a16(bytes); return r; };
    const size_t m = batch * nids;
    w.maxw = (int *)take(4 * batch); w.ncand = (int *)take(4 * batch);
    w.firstkey = (unsigned long long *)take(8 * m); w.sd = (double *)take(8 * m);
    w.words = (int *)take(4 * m); w.minw = (uint32_t *)take(4 * m); w.si = (float *)take(4 * m); w.accv = (float *)take(4 * m);
    w.bestv = (int *)take(4 * m); w.list = (int *)take(4 * m);
    w.cand = (int *)take(4 * batch * cap); w.excl = take(nids);
    w.total = o;
    return w;
}

// a wave per keyframe up to 8192 keyframes (a keyframe's words are a chain of dependent 64-word steps: parallelism comes from the number of waves)
static int kfdb_grid(int items) { const int g = (items + 3) / 4; return g < 1 ? 1 : (g > 2048 ? 2048 : g); }

// the launch chain of `batch` queries on stream s; loop = 1 takes batch == 1
static int kfdb_launch(orbx_kfdb *db, const KfdbQuery &Q, int batch, const KfdbWs &w, int loop, float min_score, int *d_cand, int cap, int *d_ncand, hipStream_t s)
{
    const int nids = (int)db->off.size();
    ORBX_HIP(hipMemsetAsync(w.maxw, 0, 4 * (size_t)batch, s));
    hipLaunchKernelGGL(k_kfdb_count, dim3(kfdb_grid(nids), batch), dim3(256), 0, s, db->d_ids, db->d_off, db->d_len, nids, Q,
                       loop ? w.excl : nullptr, w.words, w.minw, w.firstkey, w.maxw);
    hipLaunchKernelGGL(k_kfdb_score, dim3(kfdb_grid(nids), batch), dim3(256), 0, s, db->d_ids, db->d_vals, db->d_off, db->d_len, nids, Q,
                       nullptr, 0, w.words, w.maxw, w.si, w.sd, nullptr);
    hipLaunchKernelGGL(k_kfdb_select, dim3(batch), dim3(256), 0, s, nids, db->d_len, db->d_neigh, db->d_persist, w.words, w.minw, w.si, w.accv,
                       w.bestv, w.list, w.firstkey, w.maxw, loop, min_score, d_cand, cap, d_ncand);
    if (!loop)
        hipLaunchKernelGGL(k_kfdb_persist, dim3((nids + 255) / 256), dim3(256), 0, s, nids, batch, w.words, w.si, w.maxw, db->d_persist);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

static int kfdb_detect(orbx_kfdb *db, const char *who, const uint32_t *qid, const double *qval, int nq, orbx_bow_frames *f, int index, int loop,
                       const int32_t *connected, int nconnected, float min_score, int32_t *cand, int cap, int *ncand, int32_t *words_out, float *score_out)
{
    if (!db || !ncand || cap < 0 || (cap && !cand) || nconnected < 0 || (nconnected && !connected)) { orbx_set_error("%s: invalid argument", who); return ORBX_E_INVALID; }
    *ncand = 0;
    std::lock_guard<std::mutex> g(db->mu);
    if (int rc = kfdb_enter(db)) return rc;
    const int nids = (int)db->off.size();
    KfdbQuery Q;
    if (int rc = kfdb_query(db, who, qid, qval, nq, f, index, &Q)) return rc;
    if (words_out) memset(words_out, 0, sizeof(int32_t) * nids);
    if (score_out) memset(score_out, 0, sizeof(float) * nids);
    if (db->nlive == 0 || (!f && nq == 0)) return ORBX_OK;          // empty database / empty query: nothing is touched
    const int dcap = cap < nids ? cap : nids;
    KfdbWs w = kfdb_carve(nullptr, 1, nids, dcap);
    if (int rc = kfdb_ws(db, w.total)) return rc;
    w = kfdb_carve(db->d_ws, 1, nids, dcap);
    // results: [maxw ncand | cand | words | si]
    const size_t o_cand = 16, o_words = o_cand + a16(4 * (size_t)dcap), o_si = o_words + a16(4 * (size_t)nids), total = o_si + a16(4 * (size_t)nids);
    if (int rc = kfdb_pin(db, total > (size_t)nids ? total : (size_t)nids)) return rc;
    if (loop) {
        memset(db->h_pin, 0, nids);
        for (int i = 0; i < nconnected; i++) if (connected[i] >= 0 && connected[i] < nids) db->h_pin[connected[i]] = 1;
        ORBX_HIP(hipMemcpyAsync(w.excl, db->h_pin, nids, hipMemcpyHostToDevice, db->stream));
        ORBX_HIP(hipStreamSynchronize(db->stream));
    }
    if (int rc = kfdb_launch(db, Q, 1, w, loop, min_score, w.cand, dcap, w.ncand, db->stream)) return rc;
    uint8_t *h = db->h_pin;
    ORBX_HIP(hipMemcpyAsync(h, w.maxw, 4, hipMemcpyDeviceToHost, db->stream));
    ORBX_HIP(hipMemcpyAsync(h + 4, w.ncand, 4, hipMemcpyDeviceToHost, db->stream));
    if (dcap) ORBX_HIP(hipMemcpyAsync(h + o_cand, w.cand, 4 * (size_t)dcap, hipMemcpyDeviceToHost, db->stream));
    if (words_out || score_out) ORBX_HIP(hipMemcpyAsync(h + o_words, w.words, 4 * (size_t)nids, hipMemcpyDeviceToHost, db->stream));
    if (score_out) ORBX_HIP(hipMemcpyAsync(h + o_si, w.si, 4 * (size_t)nids, hipMemcpyDeviceToHost, db->stream));
    ORBX_HIP(hipStreamSynchronize(db->stream));
    const int maxw = ((const int *)h)[0], nc = ((const int *)h)[1];
    *ncand = nc;
    const int32_t *hw = (const int32_t *)(h + o_words);
    if (words_out) memcpy(words_out, hw, 4 * (size_t)nids);
    if (score_out) {
        const int min_common = (int)((float)maxw * 0.8f);
        const float *hs = (const float *)(h + o_si);
        for (int i = 0; i < nids; i++) score_out[i] = hw[i] > min_common ? hs[i] : 0.0f;
    }
    if (nc > cap) { orbx_set_error("%s: %d candidates, capacity %d", who, nc, cap); return ORBX_E_CAPACITY; }
    if (nc) memcpy(cand, h + o_cand, 4 * (size_t)nc);
    return ORBX_OK;
}

extern "C" int orbx_kfdb_detect_relocalization(orbx_kfdb *db, const uint32_t *bow_id, const double *bow_val, int nbow, int32_t *cand, int cap,
                                               int *ncand, int32_t *words_out, float *score_out)
{
    return kfdb_detect(db, "orbx_kfdb_detect_relocalization", bow_id, bow_val, nbow, nullptr, 0, 0, nullptr, 0, 0.0f, cand, cap, ncand, words_out, score_out);
}

extern "C" int orbx_kfdb_detect_relocalization_frame(orbx_kfdb *db, orbx_bow_frames *f, int index, int32_t *cand, int cap, int *ncand,
                                                     int32_t *words_out, float *score_out)
{
    if (!f) { orbx_set_error("orbx_kfdb_detect_relocalization_frame: invalid argument"); return ORBX_E_INVALID; }
    return kfdb_detect(db, "orbx_kfdb_detect_relocalization_frame", nullptr, nullptr, 0, f, index, 0, nullptr, 0, 0.0f, cand, cap, ncand, words_out, score_out);
}

extern "C" int orbx_kfdb_detect_loop(orbx_kfdb *db, const uint32_t *bow_id, const double *bow_val, int nbow, const int32_t *connected_ids, int nconnected,
                                     float min_score, int32_t *cand, int cap, int *ncand, int32_t *words_out, float *score_out)
{
    return kfdb_detect(db, "orbx_kfdb_detect_loop", bow_id, bow_val, nbow, nullptr, 0, 1, connected_ids, nconnected, min_score, cand, cap, ncand, words_out, score_out);
}

extern "C" int orbx_kfdb_detect_loop_frame(orbx_kfdb *db, orbx_bow_frames *f, int index, const int32_t *connected_ids, int nconnected, float min_score,
                                           int32_t *cand, int cap, int *ncand, int32_t *words_out, float *score_out)
{
    if (!f) { orbx_set_error("orbx_kfdb_detect_loop_frame: invalid argument"); return ORBX_E_INVALID; }
    return kfdb_detect(db, "orbx_kfdb_detect_loop_frame", nullptr, nullptr, 0, f, index, 1, connected_ids, nconnected, min_score, cand, cap, ncand, words_out, score_out);
}

static int kfdb_score(orbx_kfdb *db, const char *who, const uint32_t *qid, const double *qval, int nq, orbx_bow_frames *f, int index,
                      const int32_t *ids, int n, double *scores)
{
    if (!db || n < 0 || (n && (!ids || !scores))) { orbx_set_error("%s: invalid argument", who); return ORBX_E_INVALID; }
    std::lock_guard<std::mutex> g(db->mu);
    for (int i = 0; i < n; i++)
        if (!kfdb_is_live(db, ids[i])) { orbx_set_error("%s: invalid id %d at %d (unknown or erased)", who, ids[i], i); return ORBX_E_INVALID; }
    if (int rc = kfdb_enter(db)) return rc;
    KfdbQuery Q;
    if (int rc = kfdb_query(db, who, qid, qval, nq, f, index, &Q)) return rc;
    if (n == 0) return ORBX_OK;
    const size_t o_sd = a16(4 * (size_t)n), o_out = o_sd + a16(8 * (size_t)n), total = o_out + a16(8 * (size_t)n);
    if (int rc = kfdb_ws(db, total)) return rc;
    if (int rc = kfdb_pin(db, total)) return rc;
    memcpy(db->h_pin, ids, 4 * (size_t)n);
    ORBX_HIP(hipMemcpyAsync(db->d_ws, db->h_pin, 4 * (size_t)n, hipMemcpyHostToDevice, db->stream));
    hipLaunchKernelGGL(k_kfdb_score, dim3(kfdb_grid(n), 1), dim3(256), 0, db->stream, db->d_ids, db->d_vals, db->d_off, db->d_len, (int)db->off.size(), Q,
                       (const int *)db->d_ws, n, nullptr, nullptr, nullptr, (double *)(db->d_ws + o_sd), (double *)(db->d_ws + o_out));
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(db->h_pin + o_out, db->d_ws + o_out, 8 * (size_t)n, hipMemcpyDeviceToHost, db->stream));
    ORBX_HIP(hipStreamSynchronize(db->stream));
    memcpy(scores, db->h_pin + o_out, 8 * (size_t)n);
    return ORBX_OK;
}

extern "C" int orbx_kfdb_score(orbx_kfdb *db, const uint32_t *bow_id, const double *bow_val, int nbow, const int32_t *ids, int n, double *scores)
{
    return kfdb_score(db, "orbx_kfdb_score", bow_id, bow_val, nbow, nullptr, 0, ids, n, scores);
}

extern "C" int orbx_kfdb_score_frame(orbx_kfdb *db, orbx_bow_frames *f, int index, const int32_t *ids, int n, double *scores)
{
    if (!f) { orbx_set_error("orbx_kfdb_score_frame: invalid argument"); return ORBX_E_INVALID; }
    return kfdb_score(db, "orbx_kfdb_score_frame", nullptr, nullptr, 0, f, index, ids, n, scores);
}

extern "C" int orbx_kfdb_detect_relocalization_batch_device(orbx_kfdb *db, orbx_bow_frames *f, int batch, void *d_cand, int cap, void *d_ncand, void *stream)
{
    if (!db || !f || batch < 1 || batch > f->batch || batch > KFDB_MAX_BATCH || cap < 1 || !d_cand || !d_ncand || f->device != db->device) {
        orbx_set_error("orbx_kfdb_detect_relocalization_batch_device: invalid argument (batch <= %d)", KFDB_MAX_BATCH);
        return ORBX_E_INVALID;
    }
    std::lock_guard<std::mutex> g(db->mu);
    hipStream_t s = stream ? (hipStream_t)stream : f->last_stream;
    if (db->has_pending && db->pending == s) db->has_pending = false;    // the same stream orders the two batches itself
    if (int rc = kfdb_enter(db)) return rc;
    if (f->last_stream != s) ORBX_HIP(hipStreamSynchronize(f->last_stream));
    const int nids = (int)db->off.size();
    if (db->nlive == 0) { ORBX_HIP(hipMemsetAsync(d_ncand, 0, 4 * (size_t)batch, s)); return ORBX_OK; }
    KfdbWs w = kfdb_carve(nullptr, batch, nids, 0);
    if (int rc = kfdb_ws(db, w.total)) return rc;
    w = kfdb_carve(db->d_ws, batch, nids, 0);
    KfdbQuery Q;
    Q.id = f->bow_id; Q.val = f->bow_val; Q.n = f->counts; Q.stride = f->cap; Q.nstride = 2; Q.cap = f->cap;
    if (int rc = kfdb_launch(db, Q, batch, w, 0, 0.0f, (int *)d_cand, cap, (int *)d_ncand, s)) return rc;
    db->pending = s; db->has_pending = true;
    return ORBX_OK;
}

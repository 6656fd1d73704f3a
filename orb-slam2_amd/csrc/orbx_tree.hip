// orbx_tree.hip — the extractor's quadtree cull (ORBextractor::DistributeOctTree, reference src/ORBextractor.cc:617-915): k_tree, its LDS
// budget (orbx_tree_plan / orbx_tree_commit) and the choice of workgroup width and table memory (orbx_tree_launch).
// File map of the extractor: orbx_extract.hip.
#include "orbx_device.h"

#include <algorithm>

#ifdef ORBX_DIAG
__device__ unsigned long long g_tree_stamp[4096 * 8]; // diagnostic build only: summed phase cycles of the level-0 workgroups of k_tree (slot 6 = phase-2 sweeps, 7 = workgroups)
#define TSTAMP(k) do { if (blockIdx.y == 0) STAMP_TO(g_tree_stamp, k); } while (0)
// timeline of the level-0 tree of image 0: (tag, m, cycles since the previous entry)
__device__ unsigned g_tree_tl[256][4];
#define TLOG(tag, mval) do { if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && _tl_n < 256) { const unsigned long long _t = __builtin_amdgcn_s_memtime(); \
    g_tree_tl[_tl_n][0] = (tag); g_tree_tl[_tl_n][1] = (unsigned)(mval); g_tree_tl[_tl_n][2] = (unsigned)(_t - _tl_prev); g_tree_tl[_tl_n][3] = 1; _tl_n++; _tl_prev = _t; } } while (0)
#else
#define TLOG(tag, mval) do { } while (0)
#define TSTAMP(k) do { } while (0)
#endif

// ================================================================ K3: quadtree cull (E4)
// ORBextractor::DistributeOctTree (src/ORBextractor.cc:617-915) as a label-propagation problem:
// every point carries the id (= list position) of its leaf; a sweep counts the four children of
// every splitting node with LDS atomics, scans to get the new list positions and relabels the
// points.  Order algebra (validated against the sequential oracle by tests/quadtree_model.py):
//   new list = reverse(children of split nodes in processing order, n1..n4) ++ unsplit nodes;
//   phase 1 processes all nodes with >1 point in list order; phase 2 processes them sorted by
//   (count desc, list position asc) and stops after the split that reaches N leaves.
// One 256-thread workgroup per (level, image).
extern __shared__ __align__(16) unsigned char tree_smem[];

// NT threads per workgroup: 256 for batches (many (level, image) workgroups co-resident per CU), 1024 when a launch has
// fewer workgroups than the chip has CUs (a single frame: the longest workgroup's latency chain IS the kernel time)
// TAB_LDS: node tables in LDS (every ORB-SLAM2 configuration) -- a compile-time fact, so that their accesses are ds_ instructions
// and LDS atomics; behind a pointer chosen at run time they were FLAT instructions (300 per wave through the vector-memory path).
template <int NT, bool TAB_LDS>
__device__ __forceinline__ void tree_body(const Geom *__restrict__ g, const int *__restrict__ cell_cnt,
                                              const uint32_t *__restrict__ cand, uint32_t *__restrict__ g_pts,
                                              uint16_t *__restrict__ g_nid, int *__restrict__ lvl_cnt,
                                              uint32_t *__restrict__ lvl_kp, int lds_pts_cap, int *__restrict__ err_flag,
                                              unsigned char *__restrict__ g_tab, long long g_tab_stride, const uint32_t *__restrict__ cand_prim, int reg_pts);

#ifndef ORBX_TREE_WPE
#define ORBX_TREE_WPE 6     // waves per SIMD the 256-thread form is compiled for (= workgroups per CU): 79 VGPRs, no spills; the LDS (25 KB per
                            // workgroup with the overflow array) holds six anyway (7: 72 VGPRs + 20 bytes of scratch, 0.094 against 0.091 ms)
#endif
// (the 1024-thread form has four waves per SIMD by construction: with the 256-thread form's register cap it spilled)
template <int NT, bool TAB_LDS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(NT == 1024 ? 4 : ORBX_TREE_WPE, NT == 1024 ? 4 : ORBX_TREE_WPE))) void k_tree(const Geom *__restrict__ g, const int *__restrict__ cell_cnt,
                                              const uint32_t *__restrict__ cand, uint32_t *__restrict__ g_pts,
                                              uint16_t *__restrict__ g_nid, int *__restrict__ lvl_cnt,
                                              uint32_t *__restrict__ lvl_kp, int lds_pts_cap, int *__restrict__ err_flag,
                                              unsigned char *__restrict__ g_tab, long long g_tab_stride, const uint32_t *__restrict__ cand_prim, int reg_pts)
{
#ifdef ORBX_DIAG_TREE_TWICE     // experiment: the whole tree a second time on the same input (idempotent) -- the second pass runs from a warm instruction cache
    for (int rep = 0; rep < 2; rep++) {
        if (rep) __syncthreads();
        tree_body<NT, TAB_LDS>(g, cell_cnt, cand, g_pts, g_nid, lvl_cnt, lvl_kp, lds_pts_cap, err_flag, g_tab, g_tab_stride, cand_prim, reg_pts);
    }
#else
    tree_body<NT, TAB_LDS>(g, cell_cnt, cand, g_pts, g_nid, lvl_cnt, lvl_kp, lds_pts_cap, err_flag, g_tab, g_tab_stride, cand_prim, reg_pts);
#endif
}

template <int NT, bool TAB_LDS>
__device__ __forceinline__ void tree_body(const Geom *__restrict__ g, const int *__restrict__ cell_cnt,
                                              const uint32_t *__restrict__ cand, uint32_t *__restrict__ g_pts,
                                              uint16_t *__restrict__ g_nid, int *__restrict__ lvl_cnt,
                                              uint32_t *__restrict__ lvl_kp, int lds_pts_cap, int *__restrict__ err_flag,
                                              unsigned char *__restrict__ g_tab, long long g_tab_stride, const uint32_t *__restrict__ cand_prim, int reg_pts)
{
    constexpr int NB = ORBX_NODE_BITS, NMASK = (1 << NB) - 1;
    // points per thread in the register form: 12 on 256 threads (3072 per level); the 1024-thread form of single frames takes 4 (4096: a
    // textured 1241 x 376 level 0 has ~3300 candidates, and a level beyond the register capacity walks its points in the HBM scratch)
    constexpr int REG_PTS = NT == 1024 ? ORBX_TREE_REG_PTS_BIG : ORBX_TREE_REG_PTS;
    constexpr int RP = REG_PTS / NT;
    // x = image, y = level: workgroups are dealt to the 8 XCDs by linear id % 8, so every XCD gets the same mix of
    // levels (x = level would put all level-0 trees, the longest barrier chains, on one XCD), heaviest level first
    const int l = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const LevelGeom &L = g->lv[l];
    const int cap = g->max_node_cap; // multiple of 4
    // node tables (76 B per leaf): in LDS when they fit beside the points (every ORB-SLAM2 configuration: <= ~1900 leaves per
    // level), else in this workgroup's slice of an HBM workspace (any nfeatures the reference accepts up to the 14-bit node
    // id: __syncthreads orders the workgroup's own global stores and loads, the same code runs on either memory)
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    const size_t tab_bytes = (size_t)cap * 76;
    unsigned char *tab;
    if constexpr (TAB_LDS) tab = tree_smem; else tab = g_tab + (size_t)wg * (size_t)g_tab_stride;
    int *cnt = reinterpret_cast<int *>(tab);
    int *cnt_n = cnt + cap;
    uint2 *box = reinterpret_cast<uint2 *>(cnt_n + cap);
    uint2 *box_n = box + cap;
    int *cc = reinterpret_cast<int *>(box_n + cap); // [4*cap] child counts, then child positions (16-byte aligned)
    int *cc_n = cc + 4 * cap;                       // the next table's child counts
    int *a1 = cc_n + 4 * cap;                       // processing rank of split nodes
    int *a2 = a1 + cap;                             // children per processed node -> S offsets
    int *a3 = a2 + cap;                             // unsplit flags -> ranks
    int *a4 = a3 + cap;                             // phase-2 gains
    int *ncarr = a4 + cap;                          // non-empty children per node (0 = not split)
    // [max_cells_level + 4], always LDS; in the register form it sits behind the staging area the gather uses (which aliases the
    // node tables: they are not live yet)
    int *cellpref = !TAB_LDS ? reinterpret_cast<int *>(tree_smem)
                             : reinterpret_cast<int *>(tree_smem + (reg_pts && tab_bytes < (size_t)REG_PTS * 4 ? (size_t)REG_PTS * 4 : tab_bytes));
    uint32_t *lpts = reinterpret_cast<uint32_t *>(cellpref + ((g->max_cells_level + 4) & ~3));
    uint16_t *lnid = reinterpret_cast<uint16_t *>(lpts + lds_pts_cap);
    __shared__ int s_w[2 * (NT / 64)];  // wave totals of the block scans; the one-barrier sweeps alternate between the halves
    __shared__ int s_acc;
    __shared__ int s_acc2[2];           // n_to_expand of the one-barrier sweeps, alternating (the idle one is zeroed a sweep ahead)

    int *out_cnt = lvl_cnt + (long long)b * ORBX_MAX_LEVELS + l;
#ifdef ORBX_DIAG
    unsigned long long _t_prev = __builtin_amdgcn_s_memtime();
    unsigned long long _tl_prev = _t_prev; int _tl_n = 0;
#endif
    // ---- gather this level's candidates (cell-row-major, in-cell row-major)
    const int *ccnt = cell_cnt + (long long)b * g->total_cells + L.cell_base;
    // Single-frame form (1024 threads, one cell per thread): the cell's dense candidate record is requested together with its count --
    // its address does not depend on the counts -- so the gather is one global round trip, not two (the tree's time is a chain of such steps)
    constexpr bool PREFETCH = NT == 1024;
    const bool pre = PREFETCH && L.n_cells <= NT;
    uint4 pq0 = make_uint4(0, 0, 0, 0), pq1 = pq0, pq2 = pq0, pq3 = pq0;
    if (pre && tid < L.n_cells) {
        const uint4 *pr = reinterpret_cast<const uint4 *>(cand_prim + ((long long)b * g->total_cells + L.cell_base + tid) * ORBX_CAND_PRIM);
        pq0 = pr[0]; pq1 = pr[1]; pq2 = pr[2]; pq3 = pr[3];
    }
    for (int c = tid; c < L.n_cells; c += NT) cellpref[c] = ccnt[c];
    __syncthreads();
    const int n = lds_excl_scan_nt<NT>(cellpref, L.n_cells, s_w);
    if (n == 0) {
        if (tid == 0) *out_cnt = 0;
        return;
    }
    // Points never move (a point keeps the list position of its leaf as a label), and every pass over them is
    // `for (i = tid; i < n; i += NT)`: with n <= ORBX_TREE_REG_PTS thread tid simply KEEPS its points i = tid + NT * k and their
    // labels in registers -- no LDS for them at all (they were half of the workgroup's LDS, and LDS is what limits the
    // (level, image) workgroups per CU: 4 -> 8), and no LDS round trip per point and sweep.  Bigger levels fall back to arrays
    // (LDS up to lds_pts_cap, else the HBM scratch).
    // (register form with an overflow: a level with up to lds_pts_cap more candidates than the registers hold keeps the excess in a small
    // LDS array -- every textured 1241 x 376 level 0 has 3100-4000 candidates, and a level beyond the capacity walks ALL its points in the
    // HBM scratch)
    const bool in_regs = reg_pts && n <= REG_PTS + lds_pts_cap;
    const int n_over = in_regs && n > REG_PTS ? n - REG_PTS : 0;
    // Which points a thread keeps is free (a point's list index i travels with it); neighbouring LANES take points NT / 64 apart, not
    // neighbours: the list is cell-row-major, neighbours fall into the same quadtree node, and 64 lanes adding to one node's LDS
    // counter serialise (the relabel + classify passes of the first sweeps, 16-64 counters for ~3000 points, were 11 k of 72 k cycles)
    const int pbase = (tid & 63) * (NT / 64) + (tid >> 6);
    uint32_t rp[RP];
    unsigned rn[RP];
#pragma unroll
    for (int k = 0; k < RP; k++) { rp[k] = 0; rn[k] = 0; }
    uint32_t *pts;
    uint16_t *nid;
    if (in_regs) { pts = reinterpret_cast<uint32_t *>(tree_smem); nid = nullptr; }   // staging for the gather only
    else if (n <= lds_pts_cap) { pts = lpts; nid = lnid; }
    else {
        pts = g_pts + (long long)b * g->cand_total + L.cand_off;
        nid = g_nid + (long long)b * g->cand_total + L.cand_off;
    }
    {   // one thread per cell: the copies of different cells are independent loads in flight together
        const uint32_t *src = cand + (long long)b * g->cand_total + L.cand_off;
        for (int c = tid; c < L.n_cells; c += NT) {
            const int beg = cellpref[c], end = c + 1 < L.n_cells ? cellpref[c + 1] : n;
            const uint32_t *s = src + (long long)c * L.cand_cap;
            // the cell's dense 64-byte record as four independent 16-byte loads (an element-wise loop was a chain of dependent
            // load -> store round trips, as long as the fullest cell); only the rare entries beyond it walk the slot block
            const uint4 *pr = reinterpret_cast<const uint4 *>(cand_prim + ((long long)b * g->total_cells + L.cell_base + c) * ORBX_CAND_PRIM);
            const int cn = end - beg;
            if (cn > 0) {
                static_assert(ORBX_CAND_PRIM == 16, "four uint4 per record");
                uint4 q0, q1, q2, q3;
                if (pre) { q0 = pq0; q1 = pq1; q2 = pq2; q3 = pq3; } else { q0 = pr[0]; q1 = pr[1]; q2 = pr[2]; q3 = pr[3]; }
                const uint32_t v[16] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w };
                if (in_regs && end > REG_PTS) {     // (part of) the cell lies beyond the register capacity: those points go to the overflow array
#pragma unroll
                    for (int e = 0; e < 16; e++) if (e < cn) { const int i = beg + e; if (i < REG_PTS) pts[i] = v[e]; else lpts[i - REG_PTS] = v[e]; }
                    for (int e = 16; e < cn; e++) { const int i = beg + e; if (i < REG_PTS) pts[i] = s[e]; else lpts[i - REG_PTS] = s[e]; }
                } else {
#pragma unroll
                    for (int e = 0; e < 16; e++) if (e < cn) pts[beg + e] = v[e];
                    for (int e = 16; e < cn; e++) pts[beg + e] = s[e];
                }
            }
        }
    }
    if (in_regs) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RP; k++) { const int i = pbase + NT * k; if (i < n) rp[k] = reinterpret_cast<const uint32_t *>(tree_smem)[i]; }
        __syncthreads();        // the staging area becomes the node tables
    }
    // one pass over the points: BODY sees the index i, the packed point p and its label nd (read / write)
    // (the empty asm hides the point's value from loop-invariant code motion: LLVM otherwise extracts x and y of all the thread's points
    // once, keeps those 2 x RP values alive across the sweep loop and spills -- 40 spill stores / 64 reloads in the 256-thread form)
#define FOR_POINTS(...) do { \
        if (in_regs) { \
            _Pragma("unroll") for (int k_ = 0; k_ < RP; k_++) { \
                const int i = pbase + NT * k_; \
                if (i < n) { uint32_t p = rp[k_]; asm volatile("" : "+v"(p)); unsigned nd = rn[k_]; __VA_ARGS__; rn[k_] = nd; } \
            } \
            for (int j_ = tid; j_ < n_over; j_ += NT) { \
                const int i = REG_PTS + j_; (void)i; const uint32_t p = lpts[j_]; (void)p; unsigned nd = lnid[j_]; __VA_ARGS__; lnid[j_] = (uint16_t)nd; \
            } \
        } else { \
            for (int i = tid; i < n; i += NT) { const uint32_t p = pts[i]; (void)p; unsigned nd = nid[i]; __VA_ARGS__; nid[i] = (uint16_t)nd; } \
        } } while (0)
    TSTAMP(0);  // cell counts, prefix, gather
    TLOG(0, n);
    // ---- roots (src/ORBextractor.cc:627-705)
    const int N = L.quota;
    int m;
    // With a handful of roots (3 for a 1241 x 376 level) every point of the level would hit one of 3 LDS addresses: same-address LDS
    // atomics serialise lane by lane, and this pass and the first classification were 27 % of a level-0 tree (36 k cycles).  A thread
    // owns at most 15 points per pass, so it counts them in 4-bit fields of one 64-bit register; the fields are summed over the wave
    // on the DPP path and lane 0 adds each total once: T atomics per wave instead of one per point.
    // points a thread sees per pass, at most (the 4-bit count fields below must hold them)
    const int ppt = in_regs ? (min(n, REG_PTS) + NT - 1) / NT + (n_over + NT - 1) / NT : (n + NT - 1) / NT;
    const bool few_pts_per_thread = ppt <= 15;
    const bool seven_pts_per_thread = ppt <= 7;   // (the 1024-thread form: a thread holds at most 4 + 1 points)
    auto add_packed = [&](unsigned long long acc, int T, int *dst) {
        if (seven_pts_per_thread) {
            // all sixteen fields summed over the wave TOGETHER, widening as the partial sums grow: a field is at most 7, so two lanes'
            // sum still fits its nibble (one DPP step on the packed words), a 16-lane row's fits a byte (three steps on four words of
            // byte fields), the wave's a 16-bit field (the two cross-row steps on eight words).  Lane t then picks field t's total and
            // ONE LDS atomic instruction adds them all (sixteen separate wave sums + atomics were 4 k of a level-0 tree's 60 k cycles)
            unsigned lo = (unsigned)acc, hi = (unsigned)(acc >> 32);
            lo += (unsigned)ORBX_DPP((int)lo, 0, 0x111, 0xf, 0xf); hi += (unsigned)ORBX_DPP((int)hi, 0, 0x111, 0xf, 0xf);
            unsigned w[4] = { lo & 0x0F0F0F0Fu, (lo >> 4) & 0x0F0F0F0Fu, hi & 0x0F0F0F0Fu, (hi >> 4) & 0x0F0F0F0Fu };   // fields 0 2 4 6 | 1 3 5 7 | 8 10 12 14 | 9 11 13 15
            unsigned x[8];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                w[q] += (unsigned)ORBX_DPP((int)w[q], 0, 0x112, 0xf, 0xf);
                w[q] += (unsigned)ORBX_DPP((int)w[q], 0, 0x114, 0xf, 0xe);
                w[q] += (unsigned)ORBX_DPP((int)w[q], 0, 0x118, 0xf, 0xc);
                x[2 * q] = w[q] & 0x00FF00FFu; x[2 * q + 1] = (w[q] >> 8) & 0x00FF00FFu;      // bytes 0 2 | 1 3 of the word
            }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                x[q] += (unsigned)ORBX_DPP((int)x[q], 0, 0x142, 0xa, 0xf);
                x[q] += (unsigned)ORBX_DPP((int)x[q], 0, 0x143, 0xc, 0xf);
                x[q] = (unsigned)__builtin_amdgcn_readlane((int)x[q], 63);
            }
            // field t: word q = 2 * (t >> 3) + (t & 1), byte bi = (t & 7) >> 1 of it -> x[2 q + (bi & 1)], 16-bit slot bi >> 1
            const int t = tid & 63, q = 2 * ((t >> 3) & 1) + (t & 1), bi = (t & 7) >> 1, xi = 2 * q + (bi & 1);
            unsigned sel = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) sel = xi == j ? x[j] : sel;
            const int val = (int)((sel >> (16 * (bi >> 1))) & 0xFFFFu);
            if (t < T && val) atomicAdd(&dst[t], val);
            return;
        }
        for (int t = 0; t < T; t++) {                                   // T <= 16, wave-uniform
            const int s = wave_sum((int)((acc >> (4 * t)) & 15ull));
            if ((tid & 63) == 0 && s) atomicAdd(&dst[t], s);
        }
    };
    // ---- sweeps.  Invariant at the top of the loop: cc[0..4m) holds the child counts of the current
    // table (cnt/box) and every point label is (node id | child << NB).
    auto classify = [&](int id, uint32_t p, const int *cn, const uint2 *bx_tab, int *cct) -> int {
        int c = 0;
        if (cn[id] > 1) {
            const uint2 bx = bx_tab[id];
            const int x0 = bx.x & 0xFFFF, x1 = bx.x >> 16, y0 = bx.y & 0xFFFF, y1 = bx.y >> 16;
            const int x = p & 0xFFF, y = (p >> 12) & 0xFFF;
            const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1; // ceil(d/2), DivideNode :553-554
            c = (x >= x0 + hx ? 1 : 0) + (y >= y0 + hy ? 2 : 0);
            atomicAdd(&cct[id * 4 + c], 1);
        }
        return c;
    };
    // (1024-thread form only: with 256 threads, twelve points each, the extra arithmetic per point costs more than the barriers it saves:
    // 0.126 against 0.116 ms per 512-image launch)
    if (NT == 1024 && L.n_ini <= 4 && few_pts_per_thread) {
        // Up to four roots (every usual aspect ratio: 3 for 1241 x 376, 1 for 640 x 480): counting them, dropping the empty ones and
        // the first classification are two barrier-to-barrier steps.  The root counts go to a scratch array that every thread then
        // reads whole, so the id of a root (= non-empty roots before it) and the table size need no scan, and a root's box is
        // arithmetic on its index, so the first classification does not wait for the table entries other threads write.
        if (tid < 16) { a3[tid] = 0; cc[tid] = 0; }
        __syncthreads();
        TLOG(2, 0);
        {
            unsigned long long acc = 0;
            FOR_POINTS({
                int r = (int)((float)(p & 0xFFF) / L.hx);
                r = r < 0 ? 0 : r >= L.n_ini ? L.n_ini - 1 : r;
                acc += 1ull << (4 * r);
                nd = (unsigned)r;
            });
            TLOG(3, 0);
            add_packed(acc, L.n_ini, a3);
            TLOG(4, 0);
        }
        __syncthreads();
        TLOG(5, 0);
        const int4 rc = *reinterpret_cast<const int4 *>(a3);          // counts of roots 0..3 (zero beyond n_ini)
        const unsigned nz = (rc.x > 0 ? 1u : 0u) | (rc.y > 0 ? 2u : 0u) | (rc.z > 0 ? 4u : 0u) | (rc.w > 0 ? 8u : 0u);
        m = __popc(nz);
        if (tid < L.n_ini && ((nz >> tid) & 1u)) {
            const int id = __popc(nz & ((1u << tid) - 1u));
            const unsigned x0 = (unsigned)(int)(L.hx * (float)tid), x1 = (unsigned)(int)(L.hx * (float)(tid + 1));
            box[id] = make_uint2(x0 | (x1 << 16), 0u | ((unsigned)L.tree_h << 16));
            cnt[id] = tid == 0 ? rc.x : tid == 1 ? rc.y : tid == 2 ? rc.z : rc.w;
        }
        unsigned long long acc = 0;
        FOR_POINTS({
            const int r = (int)nd, id = __popc(nz & ((1u << r) - 1u));
            const int rcnt = r == 0 ? rc.x : r == 1 ? rc.y : r == 2 ? rc.z : rc.w;
            int c = 0;
            if (rcnt > 1) {
                const int x0 = (int)(L.hx * (float)r), x1 = (int)(L.hx * (float)(r + 1)), y0 = 0, y1 = L.tree_h;
                const int x = p & 0xFFF, y = (p >> 12) & 0xFFF;
                const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;
                c = (x >= x0 + hx ? 1 : 0) + (y >= y0 + hy ? 2 : 0);
                acc += 1ull << (4 * (id * 4 + c));
            }
            nd = (unsigned)(id | (c << NB));
        });
        TLOG(6, 0);
        add_packed(acc, 4 * m, cc);
        TLOG(7, 0);
    } else {
        for (int k = tid; k < L.n_ini; k += NT) cc[k] = 0;
        __syncthreads();
        if (L.n_ini <= 16 && few_pts_per_thread) {
            unsigned long long acc = 0;
            FOR_POINTS({
                int r = (int)((float)(p & 0xFFF) / L.hx);
                r = r < 0 ? 0 : r >= L.n_ini ? L.n_ini - 1 : r;
                acc += 1ull << (4 * r);
                nd = (unsigned)r;
            });
            add_packed(acc, L.n_ini, cc);
        } else {
            FOR_POINTS({
                int r = (int)((float)(p & 0xFFF) / L.hx);
                r = r < 0 ? 0 : r >= L.n_ini ? L.n_ini - 1 : r;
                atomicAdd(&cc[r], 1);
                nd = (unsigned)r;
            });
        }
        __syncthreads();
        for (int k = tid; k < L.n_ini; k += NT) a1[k] = cc[k] > 0;
        __syncthreads();
        m = lds_excl_scan_nt<NT>(a1, L.n_ini, s_w);
        for (int k = tid; k < L.n_ini; k += NT)
            if (cc[k] > 0) {
                const int id = a1[k];
                const unsigned x0 = (unsigned)(int)(L.hx * (float)k), x1 = (unsigned)(int)(L.hx * (float)(k + 1));
                box[id] = make_uint2(x0 | (x1 << 16), 0u | ((unsigned)L.tree_h << 16));
                cnt[id] = cc[k];
            }
        FOR_POINTS({ nd = (unsigned)a1[nd]; });
        __syncthreads();

        for (int k = tid; k < 4 * m; k += NT) cc[k] = 0;
        __syncthreads();
        if (4 * m <= 16 && few_pts_per_thread) {       // the same for the first classification: at most 16 (root, child) counters
            unsigned long long acc = 0;
            FOR_POINTS({
                const int id = (int)nd;
                int c = 0;
                if (cnt[id] > 1) {
                    const uint2 bx = box[id];
                    const int x0 = bx.x & 0xFFFF, x1 = bx.x >> 16, y0 = bx.y & 0xFFFF, y1 = bx.y >> 16;
                    const int x = p & 0xFFF, y = (p >> 12) & 0xFFF;
                    const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;
                    c = (x >= x0 + hx ? 1 : 0) + (y >= y0 + hy ? 2 : 0);
                    acc += 1ull << (4 * (id * 4 + c));
                }
                nd = (unsigned)(id | (c << NB));
            });
            add_packed(acc, 4 * m, cc);
        } else {
            FOR_POINTS({ const int id = (int)nd; nd = (unsigned)(id | (classify(id, p, cnt, box, cc) << NB)); });
        }

    }
    bool phase2 = false;
    if (tid < 2) s_acc2[tid] = 0;
    TSTAMP(1);  // roots + first classification
    TLOG(1, m);
    for (int sweep = 0;; sweep++) {
        const int prev = m;
        __syncthreads();
        TLOG(10, m);
        int nsplit = 0, S, U;
        // Phase-1 sweep of a table that fits one node per thread (every ORB-SLAM2 setting on 1024 threads, the small levels on 256):
        // node k stays with thread k from its child counts to its children's table entries, so the split flags, the packed scan input
        // and the scan result never go through LDS, and the sweep needs three workgroup barriers instead of six (a level-0 tree of a
        // single frame is a chain of ~50 barrier-to-barrier steps of ~0.4 us each: that chain, not the work, is its 35 us).
        const bool one_per_thread = NT == 1024 && !phase2 && m <= NT;   // (neutral at 256 threads, and its live values push that form into register spills)
        int my_nc = 0, my_run = 0;
        if (one_per_thread) {
            const int par = sweep & 1;
            int v = 0;
            if (tid < m) {
                const int sp = cnt[tid] > 1;
                my_nc = sp ? (cc[4 * tid] > 0) + (cc[4 * tid + 1] > 0) + (cc[4 * tid + 2] > 0) + (cc[4 * tid + 3] > 0) : 0;
                v = sp ? my_nc : (1 << 16);
            }
            const int inc = wave_incl_scan(v);
            if ((tid & 63) == 63) s_w[par * (NT / 64) + (tid >> 6)] = inc;
            __syncthreads();
            int base = 0, tot = 0;
#pragma unroll
            for (int i = 0; i < NT / 64; i++) { const int t = s_w[par * (NT / 64) + i]; if (i < (tid >> 6)) base += t; tot += t; }
            my_run = base + inc - v;
            S = tot & 0xFFFF; U = tot >> 16;
        } else
        if (!phase2) {
            // processing order == list order: one packed scan gives both the children offset of every split
            // node (low 16 bits) and the rank of every unsplit node (high 16 bits)
            for (int k = tid; k < m; k += NT) {
                const int sp = cnt[k] > 1;
                const int ncv = sp ? (cc[4 * k] > 0) + (cc[4 * k + 1] > 0) + (cc[4 * k + 2] > 0) + (cc[4 * k + 3] > 0) : 0;
                ncarr[k] = ncv;
                a2[k] = sp ? ncv : (1 << 16);
            }
            if (tid == 0) s_acc = 0;
            __syncthreads();
            const int tot = lds_excl_scan_nt<NT>(a2, m, s_w);
            S = tot & 0xFFFF; U = tot >> 16;
        } else if (m <= 64) {
            // Phase 2 on a table of at most 64 nodes (1000-feature settings reach it at m = 64; it is the last sweep of nearly every
            // tree): ONE wave orders the nodes, lane = node, everything in registers and DPP -- rank by (count desc, list position
            // asc), gains in rank order, how many splits reach N, children offsets, unsplit ranks -- and publishes the tables the
            // apply step reads.  The workgroup form below takes sixteen barrier-to-barrier steps for the same thing (18.8 k of a
            // level-0 tree's 72 k cycles).
            // (the 64 x 64 comparisons of the ranks are dealt to the workgroup's waves first, 64 / waves "other nodes" each -- in one
            // wave they were a 64-step dependent loop --, summed with one LDS atomic per lane and wave)
            if (NT != 1024) {       // (256 threads: the two extra barriers cost more than the shorter loop saves: 0.137 against 0.119 ms per 512-image launch)
                if (tid < 64) {
                    const int k = tid, ck = k < m ? cnt[k] : 0;
                    int r = 0;
                    for (int k2 = 0; k2 < m; k2++) { const int c2 = __builtin_amdgcn_readlane(ck, k2); r += (c2 > ck) || (c2 == ck && k2 < k); }
                    a1[k] = r;
                }
            } else {
                constexpr int NWV = NT / 64, PER = (64 + NWV - 1) / NWV;
                const int k = tid & 63, wv_ = tid >> 6;
                if (tid < 64) a1[tid] = 0;
                __syncthreads();
                const int ck = k < m ? cnt[k] : 0;
                int part = 0;
#pragma unroll
                for (int j = 0; j < PER; j++) {
                    const int k2 = wv_ * PER + j;
                    if (k2 < m) {                               // wave-uniform
                        const int c2 = __builtin_amdgcn_readlane(ck, k2 & 63);
                        part += (c2 > ck) || (c2 == ck && k2 < k);
                    }
                }
                if (part && ck > 1) atomicAdd(&a1[k], part);
                __syncthreads();
            }
            if (tid < 64) {
                const int k = tid;
                const int ck = k < m ? cnt[k] : 0;
                const bool cand = ck > 1;
                const int ncv = cand ? (cc[4 * k] > 0) + (cc[4 * k + 1] > 0) + (cc[4 * k + 2] > 0) + (cc[4 * k + 3] > 0) : 0;
                const int r = a1[k];
                const int ncand = __popcll(__ballot(cand));
                if (cand) a4[r] = ncv - 1;                      // gains in processing (rank) order
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int g_r = k < ncand ? a4[k] : 0;          // lane = rank from here
                const int px = wave_incl_scan(g_r) - g_r;
                const int less = __popcll(__ballot(k < ncand && prev + px + g_r < N));
                nsplit = min(ncand, less + 1);
                const int nc_r = k < nsplit ? g_r + 1 : 0;      // children of the node of rank k, if it splits
                const int inc = wave_incl_scan(nc_r);
                if (k < nsplit) a2[k] = inc - nc_r;
                const int s_tot = __builtin_amdgcn_readlane(inc, 63);
                const bool sp = cand && r < nsplit;             // lane = node again
                const int uns = k < m && !sp ? 1 : 0;
                const int uinc = wave_incl_scan(uns);
                if (k < m) { ncarr[k] = sp ? ncv : 0; a1[k] = cand ? r : -1; a3[k] = uinc - uns; }
                if (k == 0) { s_w[0] = s_tot; s_w[1] = __builtin_amdgcn_readlane(uinc, 63); }
            }
            __syncthreads();
            S = s_w[0]; U = s_w[1];
            // (s_w[0..1] are next written by a block scan or by this branch, both behind the barrier at the end of the apply step)
        } else {
            // processing order: count desc, list position asc (src/ORBextractor.cc:832-834 with the
            // address tie-break defined as "created later first" == nearer the list front)
            if (tid == 0) s_acc = 0;
            __syncthreads();
            int ncand_local = 0;
            for (int k = tid; k < m; k += NT) {
                const int ck = cnt[k];
                int r = -1, ncv = 0;
                if (ck > 1) {
                    // rank = nodes that come before this one: four counts per LDS read, the reads independent of each other (one count
                    // per dependent read made this loop 15 k of a level-0 tree's 72 k cycles)
                    r = 0;
                    const int m4 = m & ~3;
                    for (int k2 = 0; k2 < m4; k2 += 4) {
                        const int4 c4 = *reinterpret_cast<const int4 *>(cnt + k2);
                        r += ((c4.x > ck) || (c4.x == ck && k2 < k)) + ((c4.y > ck) || (c4.y == ck && k2 + 1 < k)) +
                             ((c4.z > ck) || (c4.z == ck && k2 + 2 < k)) + ((c4.w > ck) || (c4.w == ck && k2 + 3 < k));
                    }
                    for (int k2 = m4; k2 < m; k2++) {
                        const int c2 = cnt[k2];
                        r += (c2 > ck) || (c2 == ck && k2 < k);
                    }
                    ncv = (cc[4 * k] > 0) + (cc[4 * k + 1] > 0) + (cc[4 * k + 2] > 0) + (cc[4 * k + 3] > 0);
                    ncand_local++;
                }
                a1[k] = r;
                ncarr[k] = ncv;
            }
            if (ncand_local) atomicAdd(&s_acc, ncand_local);
            __syncthreads();
            const int ncand = s_acc;
            for (int k = tid; k < m; k += NT)
                if (a1[k] >= 0) { a2[a1[k]] = ncarr[k] - 1; a4[a1[k]] = ncarr[k] - 1; }
            __syncthreads();
            if (tid == 0) s_acc = 0;
            lds_excl_scan_nt<NT>(a2, ncand, s_w);
            int less = 0;
            for (int r = tid; r < ncand; r += NT) less += (prev + a2[r] + a4[r] < N);
            if (less) atomicAdd(&s_acc, less);
            __syncthreads();
            nsplit = min(ncand, s_acc + 1);
            __syncthreads();
            for (int k = tid; k < m; k += NT) {
                const bool sp = a1[k] >= 0 && a1[k] < nsplit;
                if (!sp) ncarr[k] = 0;
                a3[k] = !sp;
            }
            if (tid == 0) s_acc = 0;
            __syncthreads();
            for (int k = tid; k < m; k += NT)
                if (ncarr[k] > 0) a2[a1[k]] = ncarr[k];
            __syncthreads();
            S = lds_excl_scan_nt<NT>(a2, nsplit, s_w);
            U = lds_excl_scan_nt<NT>(a3, m, s_w);
        }
        if (S + U > cap) { // cannot happen (SURVEY.md A.4 bound); never write out of bounds
            if (tid == 0) { atomicExch(err_flag, 1); *out_cnt = 0; }
            return;
        }
        TSTAMP(2);  // order / scans of the sweep
        TLOG(phase2 ? 12 : 11, S + U);
#ifdef ORBX_DIAG
        if (phase2 && blockIdx.y == 0 && tid == 0) atomicAdd(&g_tree_stamp[((blockIdx.x * 131 + blockIdx.y) & 4095) * 8 + 6], 1ull);
#endif
        // ---- apply: build the next table, turn cc into child positions, zero the next table's counters
        int expand_local = 0;
        for (int k = tid; k < m; k += NT) {
            if ((one_per_thread ? my_nc : ncarr[k]) > 0) {
                const uint2 bx = box[k];
                const int x0 = bx.x & 0xFFFF, x1 = bx.x >> 16, y0 = bx.y & 0xFFFF, y1 = bx.y >> 16;
                const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;
                int pos = S - 1 - (one_per_thread ? (my_run & 0xFFFF) : phase2 ? a2[a1[k]] : (a2[k] & 0xFFFF));
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int q = cc[4 * k + c];
                    if (q > 0) {
                        const unsigned cx0 = (c & 1) ? x0 + hx : x0, cx1 = (c & 1) ? x1 : x0 + hx;
                        const unsigned cy0 = (c & 2) ? y0 + hy : y0, cy1 = (c & 2) ? y1 : y0 + hy;
                        box_n[pos] = make_uint2(cx0 | (cx1 << 16), cy0 | (cy1 << 16));
                        cnt_n[pos] = q;
                        reinterpret_cast<int4 *>(cc_n)[pos] = make_int4(0, 0, 0, 0);
                        expand_local += q > 1;
                        cc[4 * k + c] = pos;
                        pos--;
                    }
                }
            } else {
                const int pos = S + (one_per_thread ? (my_run >> 16) : phase2 ? a3[k] : (a2[k] >> 16));
                box_n[pos] = box[k];
                cnt_n[pos] = cnt[k];
                reinterpret_cast<int4 *>(cc_n)[pos] = make_int4(0, 0, 0, 0);
                cc[4 * k] = cc[4 * k + 1] = cc[4 * k + 2] = cc[4 * k + 3] = pos;
            }
        }
        if (expand_local) atomicAdd(one_per_thread ? &s_acc2[sweep & 1] : &s_acc, expand_local);
        __syncthreads();
        m = S + U;
        const int n_to_expand = one_per_thread ? s_acc2[sweep & 1] : s_acc;
        if (tid == 0) s_acc2[(sweep & 1) ^ 1] = 0;    // the other accumulator: next used after the next sweep's barriers
        const bool done = m >= N || m == prev;                     // :803-806, :883-884
        if (!phase2 && !done && m + 3 * n_to_expand > N) phase2 = true; // :814
        if (done) {
            // final relabel fused with "one keypoint per leaf: max response, first in list order wins ties" (:895-912): the next
            // table's counters (cc_n) were zeroed by the apply step above for every leaf, so they serve as the per-leaf maxima
            // without a clearing pass and its barrier
            unsigned *bestn = reinterpret_cast<unsigned *>(cc_n);
            FOR_POINTS({
                const int v = (int)nd;
                nd = (unsigned)cc[(v & NMASK) * 4 + (v >> NB)];
                atomicMax(&bestn[nd], ((p >> 24) << 24) | (0xFFFFFFu - (unsigned)i));
            });
            __syncthreads();
            break;
        }
        TSTAMP(3);  // apply
        TLOG(13, m);
        // ---- relabel fused with the next sweep's classification (one pass over the points)
        FOR_POINTS({
            const int v = (int)nd;
            const int id = cc[(v & NMASK) * 4 + (v >> NB)];
            nd = (unsigned)(id | (classify(id, p, cnt_n, box_n, cc_n) << NB));
        });
        { int *t = cnt; cnt = cnt_n; cnt_n = t; }
        { uint2 *t = box; box = box_n; box_n = t; }
        { int *t = cc; cc = cc_n; cc_n = t; }
        TSTAMP(4);  // relabel + classify
        TLOG(14, m);
    }

    // ---- one keypoint per leaf: max response, first in list order wins ties (:895-912)
    const unsigned *best = reinterpret_cast<const unsigned *>(cc_n);
    uint32_t *okp = lvl_kp + (long long)b * g->kp_total + L.kp_off;
    if (in_regs) {      // the winner of a leaf is written by the thread that holds it
        FOR_POINTS({
            const int k = (int)(nd & NMASK);
            if ((best[k] & 0xFFFFFFu) == 0xFFFFFFu - (unsigned)i && k < L.kp_cap) {
                const unsigned x = (p & 0xFFF) + ORBX_MIN_BORDER, y = ((p >> 12) & 0xFFF) + ORBX_MIN_BORDER;
                okp[k] = x | (y << 12) | (p & 0xFF000000u);
            }
        });
    } else {
        for (int k = tid; k < m; k += NT) {
            const uint32_t p = pts[0xFFFFFFu - (best[k] & 0xFFFFFFu)];
            const unsigned x = (p & 0xFFF) + ORBX_MIN_BORDER, y = ((p >> 12) & 0xFFF) + ORBX_MIN_BORDER;
            if (k < L.kp_cap) okp[k] = x | (y << 12) | (p & 0xFF000000u);
        }
    }
#undef FOR_POINTS
    TSTAMP(5);  // final relabel, best per leaf, output
    TLOG(20, m);
#ifdef ORBX_DIAG
    if (blockIdx.y == 0 && tid == 0) atomicAdd(&g_tree_stamp[((blockIdx.x * 131 + blockIdx.y) & 4095) * 8 + 7], 1ull);
#endif
    if (tid == 0) *out_cnt = min(m, L.kp_cap);
}

#ifdef ORBX_DIAG
extern "C" int orbx_diag_tree_timeline(unsigned *out /*[256][4]*/)
{
    ORBX_HIP(hipDeviceSynchronize());
    ORBX_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tree_tl), sizeof(unsigned) * 1024));
    static unsigned z[1024];
    ORBX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_tree_tl), z, sizeof z));
    return ORBX_OK;
}

extern "C" int orbx_diag_tree_stamps(unsigned long long *out, int reset) { return orbx_diag_stamp_sums(HIP_SYMBOL(g_tree_stamp), out, reset); }
#endif

// ================================================================ host side

static const size_t kTreeLdsLimit = 150 * 1024;
static size_t tree_tab_bytes(const Geom &G) { return (size_t)G.max_node_cap * (4 + 4 + 8 + 8 + 16 + 16 + 4 * 5); }
static size_t tree_fixed_lds(const Geom &G) { return (size_t)((G.max_cells_level + 4) & ~3) * 4 + 64; }
// the node tables (76 B per leaf) go to LDS when they fit there together with the cell prefix array and at least 3072 points
static bool tree_tab_in_lds(const Geom &G) { return tree_tab_bytes(G) + tree_fixed_lds(G) + (size_t)3072 * 6 <= kTreeLdsLimit; }
static size_t tree_lds_bytes(const Geom &G, int lds_pts_cap)
{
    return (tree_tab_in_lds(G) ? tree_tab_bytes(G) : 0) + tree_fixed_lds(G) + (size_t)lds_pts_cap * 6;
}
// LDS point capacity of k_tree: about a level's typical candidate count, bounded so that several (level, image)
// workgroups fit one CU; levels with more candidates keep their points in the HBM scratch
static int lds_pts_cap(const Geom &G)
{
    int c = (G.lv[0].w * G.lv[0].h / 160 + 1023) & ~1023; // P_0/160: measured best at 512 images per launch (1241x376: 3072)
    c = c < 3072 ? 3072 : c > 12288 ? 12288 : c;
    while (c > 3072 && tree_lds_bytes(G, c) > kTreeLdsLimit) c -= 1024;
    return c;
}

// Register form of k_tree (points and labels in VGPRs, see the kernel): for image sizes whose levels normally hold at most
// ORBX_TREE_REG_PTS candidates (the same P_0/160 rule) and node tables that fit the LDS; bigger levels of such an image go to the
// HBM scratch.  The workgroup's LDS is then the node tables (which double as the gather's staging area) + the cell prefix array.
static bool tree_reg_mode(const Geom &G) { return tree_tab_in_lds(G) && lds_pts_cap(G) <= ORBX_TREE_REG_PTS; }
// (register form: the capacity of the overflow array -- points beyond the register capacity of a level; 6 bytes each)
static int tree_launch_pts_cap(const Geom &G) { return tree_reg_mode(G) ? ORBX_TREE_OVER_PTS : lds_pts_cap(G); }
static size_t tree_launch_lds(const Geom &G)
{
    if (!tree_reg_mode(G)) return tree_lds_bytes(G, lds_pts_cap(G));
    return std::max(tree_tab_bytes(G), (size_t)ORBX_TREE_REG_PTS_BIG * 4) + tree_fixed_lds(G) + (size_t)ORBX_TREE_OVER_PTS * 6;   // (the 1024-thread form stages 4096 points)
}

// The quadtree's step of orbx_prepare_geometry, before anything is allocated: refuses a geometry whose per-level cells do not fit the LDS.
// *hbm_tab_bytes: node-table bytes one (level, image) workgroup keeps in the HBM workspace (d_tree_tab); 0 when the tables fit the LDS.
int orbx_tree_plan(const Geom &G, size_t *hbm_tab_bytes)
{
    if (tree_launch_lds(G) > kTreeLdsLimit) {
        orbx_set_error("internal: %d FAST cells per level do not fit the quadtree kernel's LDS", G.max_cells_level);
        return ORBX_E_INVALID;
    }
    *hbm_tab_bytes = tree_tab_in_lds(G) ? 0 : tree_tab_bytes(G);
    return ORBX_OK;
}

// ... and its last step, on the handle's device: the dynamic LDS the four instances are launched with for this geometry
int orbx_tree_commit(const Geom &G)
{
    const void *kt[4] = { reinterpret_cast<const void *>(k_tree<256, true>), reinterpret_cast<const void *>(k_tree<256, false>),
                          reinterpret_cast<const void *>(k_tree<1024, true>), reinterpret_cast<const void *>(k_tree<1024, false>) };
    for (const void *f : kt) ORBX_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tree_launch_lds(G)));
    return ORBX_OK;
}

void orbx_tree_launch(orbx_extractor *e, int batch, hipStream_t s)
{
    const Geom &G = e->geom;
    int32_t *forms = e->last_forms;     // orbx_debug_launch_forms
    // 256 threads for batches (many (level, image) workgroups co-resident per CU); launches of few workgroups: 1024 threads
    // each shorten the per-workgroup chain (a single stereo frame: 51 -> 19 us)
    // (up to 512 workgroups -- 64 images of 8 levels: 16 frames 78 -> 85.5 k frames/s, 32 frames 106.5 -> 109 k; 1024 workgroups: slower)
    const bool big = batch * G.nlevels <= 512, lds = tree_tab_in_lds(G);
    void (*kern)(const Geom *, const int *, const uint32_t *, uint32_t *, uint16_t *, int *, uint32_t *, int, int *, unsigned char *, long long,
                 const uint32_t *, int) =
        big ? (lds ? k_tree<1024, true> : k_tree<1024, false>) : (lds ? k_tree<256, true> : k_tree<256, false>);
    forms[3] = big ? 1024 : 256; forms[4] = lds; forms[5] = tree_reg_mode(G);
    hipLaunchKernelGGL(kern, dim3(batch, G.nlevels), dim3(big ? 1024 : 256), tree_launch_lds(G), s, e->d_geom,
                       e->d_cell_cnt, e->d_cand, e->d_tree_pts, e->d_tree_nid, e->d_lvl_cnt, e->d_lvl_kp, tree_launch_pts_cap(G), orbx_err_flag(e),
                       lds ? nullptr : e->d_tree_tab, (long long)align_up(tree_tab_bytes(G), 256), e->d_cand_prim, tree_reg_mode(G) ? 1 : 0);
}

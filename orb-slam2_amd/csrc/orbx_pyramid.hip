// orbx_pyramid.hip — the extractor's image pyramid (ORBextractor::ComputePyramid, reference src/ORBextractor.cc:1341-1370): the resize kernels,
// their host tables (orbx_pyramid_plan) and the choice between one launch per level and grouped launches (orbx_pyramid_launch).
// File map of the extractor: orbx_extract.hip.
#include "orbx_device.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

// ================================================================ K1: pyramid level (E2)
// cv::resize INTER_LINEAR 8UC1 from level l-1 to level l.  Coefficient tables are
// computed on the host with the reference's float/double arithmetic; the kernel is pure integer.
// A one-wave workgroup produces a 256 x RS_TH (8) output tile, lane = four adjacent output columns, all rows:
//  * the source rectangle (<= 311 x 12) goes to LDS with direct loads (global_load_lds_dwordx4: three whole source rows per
//    instruction, any byte alignment, no VGPR round trip, no address arithmetic per element); 3840 bytes of LDS per wave =
//    the CU's maximum of 32 waves (the kernel is latency bound: 16-row tiles, 21 waves per CU, were 3 % slower);
//  * the loop runs over SOURCE rows (fully unrolled: every LDS offset is an immediate): the horizontal interpolation
//    of a source row is computed once and serves the (up to two) output rows it belongs to -- at scale 1.2 that is
//    1.33 instead of 2 horizontal passes per output row; an output row is emitted as soon as its lower source row
//    is done.  Which output row that is comes from the tile row's host record and depends only on the tile (every lane has the
//    same rows): scalar control flow -- a few hundred scalar instructions per tile whatever its width, which is why a lane
//    takes four columns (with two the kernel was bound by the scalar unit, not by the vector ALUs).
// One-wave workgroups need no barrier partners and drift apart in time, so loads of one tile overlap arithmetic of
// another on the same CU (a 16-wave workgroup walking all levels of an image with barriers between them was no faster).
#define RS_PX 4      // output columns per lane
#define RS_TW (64 * RS_PX)
#ifndef RS_TH_LOG2
#define RS_TH_LOG2 3
#endif
#define RS_TH (1 << RS_TH_LOG2)
#define RS_NT 64     // threads per workgroup: one wave
#define RS_PITCH 320 // LDS bytes per staged source row (>= 1.2 * RS_TW + 2 + 3): twenty 16-byte pieces, three rows per direct load
#define RS_ROWS (RS_TH == 16 ? 22 : 12)   // source rows of a tile at scale 1.2: ceil(1.2 * RS_TH) + 2

// Launch constants by value, and everything a tile needs to start its loads in ONE record per tile row / tile column (host
// tables): the wave's first dependent fetch is already the last one before the direct loads (it used to walk kernel arguments
// -> geometry -> coefficient tables -> emit table, holding its LDS all the while).
struct ResizeArgs {
    int d_w, d_pitch, s_w, s_pitch, s_level0;
    int tab_x, tab_tx, tab_ty;          // int16 units into the table buffer
    long long d_off, s_off;             // byte offsets of the two levels inside one image's pyramid block
};
#define RS_TY_REC (4 + 4 * RS_ROWS)     // tile-row record, int16 units: (first source row, source rows, 0, 0), then RS_ROWS x (e, b0, b1, 0)

__global__ __launch_bounds__(RS_NT) void k_resize(const ResizeArgs A, PyrRef pr,
                                                uint8_t *__restrict__ pyr_w, const int16_t *__restrict__ tabs)
{
    __shared__ __align__(16) uint8_t src_t[RS_ROWS * RS_PITCH];
    // image-fastest grid: consecutive workgroups (dealt round-robin over the XCDs) take the same tile of different images, so what is in
    // flight on the chip at any time is spread over every image of the batch (1.4 MB apart) instead of packed into a few -- measured 2-3 %
    // faster than tile-fastest, like every attempt to keep neighbouring tiles on one XCD was slower
    const int b = blockIdx.x, lane = threadIdx.x, tile_x = blockIdx.y, tile_y = blockIdx.z;
    const int x_t = tile_x * RS_TW;
    const int spitch = A.s_level0 ? pr.img0_pitch : A.s_pitch;
    const uint8_t *src = A.s_level0 ? pr.img0 + (long long)b * pr.img0_stride : pr.pyr + (long long)b * pr.pyr_stride + A.s_off;
    uint8_t *dst = pyr_w + (long long)b * pr.pyr_stride + A.d_off;
    const int16_t *tx = tabs + A.tab_x;
    const int16_t *ry = tabs + A.tab_ty + tile_y * RS_TY_REC, *rx = tabs + A.tab_tx + 4 * tile_x;
    const int sy_min = __builtin_amdgcn_readfirstlane((int)ry[0]), nrows = __builtin_amdgcn_readfirstlane((int)ry[1]);
    const int sx_min = __builtin_amdgcn_readfirstlane((int)rx[0]), nfull = __builtin_amdgcn_readfirstlane((int)rx[1]),
              tail = __builtin_amdgcn_readfirstlane((int)rx[2]);
    // Per SOURCE row of the tile (wave-uniform scalars): which output row is complete once this source row has been
    // interpolated, and its vertical weights: (y | skip << 12 | same << 13 | two << 14, b0, b1, 0), or e = -1 for none;
    // rows of other tiles are already filtered out by the host
    short4 qs[RS_ROWS];
#pragma unroll
    for (int k = 0; k < RS_ROWS; k++) qs[k] = *reinterpret_cast<const short4 *>(ry + 4 + 4 * k);
    // the lane's output columns: source offsets and the 11-bit weights (requested before the tile loads: independent of them)
    const int x4 = x_t + RS_PX * lane;
    short4 qx[RS_PX];
#pragma unroll
    for (int i = 0; i < RS_PX; i++) qx[i] = *reinterpret_cast<const short4 *>(tx + 4 * min(x4 + i, A.d_w - 1)); // (ofs, a0, a1, 0)
    {
        // 16-byte pieces that lie wholly inside the source row are fetched by direct loads (global_load_lds_dwordx4: 1 KB per wave
        // instruction, any byte alignment): lane = (row lane / 20, piece lane % 20) of three whole rows per load -- the LDS pitch
        // of 320 bytes is exactly twenty pieces.  The < 16 bytes a right-edge tile still needs behind the last whole piece are
        // fetched as bytes (a piece there could reach past the caller's last image row).
        const uint8_t *s0 = src + (long long)sy_min * spitch + sx_min;
        const int lr = lane / 20, lc = lane - lr * 20;
        if (lr < 3 && lc < nfull)
            for (int r = 0; r < nrows; r += 3)
                if (r + lr < nrows)
                    __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t *>(s0 + (long long)(r + lr) * spitch + 16 * lc),
                                                     reinterpret_cast<uint32_t *>(src_t + r * RS_PITCH), 16, 0, 0);
        if (tail)
            for (int i = lane; i < nrows * tail; i += RS_NT) {
                const int r = i / tail, c = 16 * nfull + (i - r * tail);
                src_t[r * RS_PITCH + c] = s0[(long long)r * spitch + c];
            }
    }
    int o0[RS_PX], o1[RS_PX], a0[RS_PX], a1[RS_PX];
#pragma unroll
    for (int i = 0; i < RS_PX; i++) {
        const int sx0 = qx[i].x;
        o0[i] = sx0 - sx_min;
        o1[i] = min(sx0 + 1, A.s_w - 1) - sx_min;
        a0[i] = qx[i].y;
        a1[i] = qx[i].z;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the direct loads have landed in LDS
    __syncthreads();
    const int d_w = A.d_w, d_pitch = A.d_pitch;
    int hp[RS_PX], hc[RS_PX];                   // (t >> 4) of source rows k - 1 and k
#pragma unroll
    for (int i = 0; i < RS_PX; i++) hp[i] = hc[i] = 0;
    uint8_t *dcol = dst + x4;
    // the weights are non-negative and each pair sums to 2048 (+-1 by rounding), so v stays inside [0, 255]:
    // ((2049 * (255 * 2049 >> 4)) >> 16) + 2 >> 2 == 255 -- cv::resize's saturate_cast never fires for INTER_LINEAR
    // (b * h) >> 16 as the high half of (b << 16) * h: one multiply, no shift (b <= 2049, h < 2^15: the product stays below 2^42)
#define EMIT(Y, B0, B1, HA) do { \
        const unsigned w0_ = (unsigned)(B0) << 16, w1_ = (unsigned)(B1) << 16; \
        uint32_t out_ = 0; \
        _Pragma("unroll") for (int i = 0; i < RS_PX; i++) out_ |= ((__umulhi(w0_, (unsigned)(HA)[i]) + __umulhi(w1_, (unsigned)hc[i]) + 2u) >> 2) << (8 * i); \
        if (x4 < d_w) *reinterpret_cast<uint32_t *>(dcol + (long long)(Y) * d_pitch) = out_; } while (0)
#pragma unroll
    for (int k = 0; k < RS_ROWS; k++) {         // fully unrolled: every LDS offset below is an immediate
        if (k < nrows) {                        // wave-uniform
#pragma unroll
            for (int i = 0; i < RS_PX; i++) {
                hp[i] = hc[i];
                hc[i] = (src_t[k * RS_PITCH + o0[i]] * a0[i] + src_t[k * RS_PITCH + o1[i]] * a1[i]) >> 4;
            }
            const int e = __builtin_amdgcn_readfirstlane((int)qs[k].x);
            if (e >= 0) {
                const int y = e & 0xFFF;
                if (!(e & 0x1000)) {
                    const int b0 = __builtin_amdgcn_readfirstlane((int)qs[k].y), b1 = __builtin_amdgcn_readfirstlane((int)qs[k].z);
                    if (e & 0x2000) EMIT(y, b0, b1, hc);                // bottom clamp: both source rows are this one
                    else EMIT(y, b0, b1, hp);
                }
                // two output rows end on the clamped last source row when consecutive levels have equal heights: the second one
                // is y + 1 with both rows = this one and the clamp weights (2048, 0)
                if (e & 0x4000) EMIT(y + 1, 2048, 0, hc);
            }
        }
    }
#undef EMIT
}

// Fallback for scale factors whose source rectangle does not fit the LDS tile of k_resize
// (ORB-SLAM2 always uses 1.2): same arithmetic straight from global memory, 4 pixels per thread.
__global__ __launch_bounds__(256) void k_resize_direct(const Geom *__restrict__ g, int l, PyrRef pr,
                                                       uint8_t *__restrict__ pyr_w, const int16_t *__restrict__ tabs)
{
    const LevelGeom &D = g->lv[l];
    const LevelGeom &S = g->lv[l - 1];
    const int b = blockIdx.z;
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= D.h || x4 >= D.pitch) return;
    int spitch;
    const uint8_t *src = orbx_level_ptr(pr, S, l - 1, b, &spitch);
    uint8_t *dst = pyr_w + (long long)b * pr.pyr_stride + D.pyr_off;
    if (D.resize_lds == 2) { // exact 2x in both directions: cv::resize switches INTER_LINEAR to the 2x2 area average
        const uint8_t *r0 = src + (long long)(2 * y) * spitch, *r1 = r0 + spitch;
        uint32_t out = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = x4 + i;
            if (x < D.w) out |= (uint32_t)((r0[2 * x] + r0[2 * x + 1] + r1[2 * x] + r1[2 * x + 1] + 2) >> 2) << (8 * i);
        }
        *reinterpret_cast<uint32_t *>(dst + (long long)y * D.pitch + x4) = out;
        return;
    }
    const int16_t *tx = tabs + D.tab_x, *ty = tabs + D.tab_y;
    const int sy0 = ty[4 * y], b0 = ty[4 * y + 1], b1 = ty[4 * y + 2];
    const int sy1 = sy0 + 1 < S.h ? sy0 + 1 : S.h - 1;
    const uint8_t *r0 = src + (long long)sy0 * spitch, *r1 = src + (long long)sy1 * spitch;
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int x = x4 + i;
        if (x < D.w) {
            const int sx0 = tx[4 * x], a0 = tx[4 * x + 1], a1 = tx[4 * x + 2];
            const int sx1 = sx0 + 1 < S.w ? sx0 + 1 : S.w - 1;
            const int t0 = r0[sx0] * a0 + r0[sx1] * a1;
            const int t1 = r1[sx0] * a0 + r1[sx1] * a1;
            int v = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
            v = v < 0 ? 0 : v > 255 ? 255 : v;
            out |= (uint32_t)v << (8 * i);
        }
    }
    *reinterpret_cast<uint32_t *>(dst + (long long)y * D.pitch + x4) = out;
}

// ---------------------------------------------------------------- K1g: several pyramid levels per launch (small launches)
// A single frame's pyramid is seven dependent launches of a few microseconds of work each: its time is the launch chain (7 x 5 us), not
// the pixels.  k_pyr_group shortens the chain: a workgroup owns one tile of the LAST level of a group of consecutive levels and computes,
// level by level through two LDS buffers, every pixel of the earlier levels that tile depends on (host tables: per tile column / row and
// level the region [lo, hi) and the part [lo, own_hi) it also writes to the pyramid -- the regions of neighbouring tiles overlap by the
// interpolation halo, the owned parts tile each level exactly).  The halo pixels are computed twice (1.4 x the pixels for five levels on
// 32 x 16 tiles), which is why batches keep k_resize; the arithmetic per pixel is k_resize's, from the same coefficient tables.
#define ORBX_PYR_GROUP_MAX 7
#define PG_TW 32
#define PG_TH 16
#define PG_NT 512
#define PG_LDS_LIMIT (64 * 1024)
struct PyrGroupLevel { int w, h, pitch, tab_x, tab_y, pad; long long pyr_off; };
struct PyrGroupArgs {
    int n, s_level0, s_w, s_h, s_pitch, tab_cx, tab_cy, lds_b;
    long long s_off;
    PyrGroupLevel lv[ORBX_PYR_GROUP_MAX];
};
#define PG_CX_REC 8     // int16 units per (tile column, step): lo, hi, own_hi, dwords per source row (step 0), magic of the dwords / 4-pixel groups per row (lo, hi), 0, 0
#define PG_CY_REC 4     // per (tile row, step): lo, hi, own_hi, 0

extern __shared__ __align__(16) uint8_t pg_smem[];

__global__ __launch_bounds__(PG_NT) void k_pyr_group(const PyrGroupArgs A, PyrRef pr, uint8_t *__restrict__ pyr_w, const int16_t *__restrict__ tabs)
{
    const int b = blockIdx.z, tid = threadIdx.x;
    const int16_t *cx = tabs + A.tab_cx + (int)blockIdx.x * PG_CX_REC * (A.n + 1);
    const int16_t *cy = tabs + A.tab_cy + (int)blockIdx.y * PG_CY_REC * (A.n + 1);
    const int spitch = A.s_level0 ? pr.img0_pitch : A.s_pitch;
    const uint8_t *src = A.s_level0 ? pr.img0 + (long long)b * pr.img0_stride : pr.pyr + (long long)b * pr.pyr_stride + A.s_off;
    uint8_t *cur = pg_smem, *nxt = pg_smem + A.lds_b;
    int ox = cx[0], oy = cy[0], cp;             // origin and pitch of the region in `cur`
    {
        const int rows = cy[1] - oy, ndw = cx[3];
        const unsigned magic = (unsigned)(uint16_t)cx[4] | ((unsigned)(uint16_t)cx[5] << 16);
        cp = 4 * ndw;
        if ((((uintptr_t)src | (unsigned)spitch) & 3) == 0) {       // ox is a multiple of 4: whole aligned dwords, never past the row's pitch
            for (int i = tid; i < rows * ndw; i += PG_NT) {
                const int r = ndw == 1 ? i : (int)__umulhi((unsigned)i, magic), c = i - r * ndw;   // (2^32 / 1 has no 32-bit magic)
                reinterpret_cast<uint32_t *>(cur)[i] = *reinterpret_cast<const uint32_t *>(src + (long long)(oy + r) * spitch + ox + 4 * c);
            }
        } else {                                                     // a caller's level-0 image at an odd address or pitch: bytes inside the row only
            const int wb = min(cp, A.s_w - ox);
            for (int i = tid; i < rows * cp; i += PG_NT) {
                const int r = i / cp, c = i - r * cp;
                if (c < wb) cur[i] = src[(long long)(oy + r) * spitch + ox + c];
            }
        }
    }
    __syncthreads();
    int s_w = A.s_w, s_h = A.s_h;
    for (int k = 1; k <= A.n; k++) {
        const PyrGroupLevel &L = A.lv[k - 1];
        const int16_t *qx_ = cx + PG_CX_REC * k, *qy_ = cy + PG_CY_REC * k;
        const int lx = qx_[0], hx = qx_[1], own_x = qx_[2], ly = qy_[0], hy = qy_[1], own_y = qy_[2];
        const unsigned magic = (unsigned)(uint16_t)qx_[4] | ((unsigned)(uint16_t)qx_[5] << 16);
        const int rw = hx - lx, rh = hy - ly, dp = (rw + 3) & ~3;
        const int16_t *tx = tabs + L.tab_x, *ty = tabs + L.tab_y;
        uint8_t *dst = pyr_w + (long long)b * pr.pyr_stride + L.pyr_off;
        const bool keep = k < A.n;               // the last level of the group is only written out
        // a thread takes four adjacent pixels of a row: one row record, the four column records as two 16-byte loads, one packed
        // LDS store (the region's rows are dword aligned in `nxt`) and one dword store to the pyramid
        const int ng = (rw + 3) >> 2;
        for (int i = tid; i < ng * rh; i += PG_NT) {
            const int yy = ng == 1 ? i : (int)__umulhi((unsigned)i, magic), xx = 4 * (i - yy * ng);
            const int x = lx + xx, y = ly + yy;
            const short4 qy = *reinterpret_cast<const short4 *>(ty + 4 * y);
            const int sy0 = qy.x, sy1 = min(sy0 + 1, s_h - 1);
            const uint8_t *r0 = cur + (sy0 - oy) * cp - ox, *r1 = cur + (sy1 - oy) * cp - ox;
            short4 qx[4];
            if (xx + 3 < rw) {           // the four records are contiguous (8 bytes each, 8-byte aligned)
                const uint2 *tp = reinterpret_cast<const uint2 *>(tx + 4 * x);
                const uint2 t0_ = tp[0], t1_ = tp[1], t2_ = tp[2], t3_ = tp[3];
                qx[0] = *reinterpret_cast<const short4 *>(&t0_); qx[1] = *reinterpret_cast<const short4 *>(&t1_);
                qx[2] = *reinterpret_cast<const short4 *>(&t2_); qx[3] = *reinterpret_cast<const short4 *>(&t3_);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) qx[j] = *reinterpret_cast<const short4 *>(tx + 4 * min(x + j, hx - 1));
            }
            uint32_t out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int sx0 = qx[j].x, sx1 = min(sx0 + 1, s_w - 1);
                const int t0 = r0[sx0] * qx[j].y + r0[sx1] * qx[j].z;
                const int t1 = r1[sx0] * qx[j].y + r1[sx1] * qx[j].z;
                const int v = (((qy.y * (t0 >> 4)) >> 16) + ((qy.z * (t1 >> 4)) >> 16) + 2) >> 2;   // in [0, 255], see k_resize
                out |= (uint32_t)v << (8 * j);
            }
            if (keep) *reinterpret_cast<uint32_t *>(nxt + yy * dp + xx) = out;
            if (y < own_y) {
                uint8_t *d = dst + (long long)y * L.pitch + x;
                if (x + 3 < own_x) *reinterpret_cast<uint32_t *>(d) = out;      // (any byte alignment: global memory takes unaligned dwords)
                else
#pragma unroll
                    for (int j = 0; j < 4; j++) if (x + j < own_x) d[j] = (uint8_t)(out >> (8 * j));
            }
        }
        __syncthreads();
        { uint8_t *t = cur; cur = nxt; nxt = t; }
        ox = lx; oy = ly; cp = dp; s_w = L.w; s_h = L.h;
    }
}

// ================================================================ host side

// cv::resize coefficient tables, reference call site src/ORBextractor.cc:1366
// Stored interleaved, one (ofs, c0, c1, 0) quad of int16 per destination index: one 8-byte load per index on the device.
static void linear_tables(int ssize, int dsize, int16_t *quads)
{
    const double inv_scale = (double)dsize / ssize;
    const double scale = 1. / inv_scale;
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floor((double)f);
        f -= s;
        if (s < 0) { f = 0; s = 0; }
        if (s >= ssize - 1) { f = 0; s = ssize - 1; }
        int v0 = orbx_cv_round((1.f - f) * 2048), v1 = orbx_cv_round(f * 2048);
        quads[4 * d] = (int16_t)s;
        quads[4 * d + 1] = (int16_t)(v0 < -32768 ? -32768 : v0 > 32767 ? 32767 : v0);
        quads[4 * d + 2] = (int16_t)(v1 < -32768 ? -32768 : v1 > 32767 ? 32767 : v1);
        quads[4 * d + 3] = 0;
    }
}

// Host tables of k_pyr_group: for every group, per tile column (row) of its last level and per step k = 0 (the source level) .. n
// the region [lo, hi) the workgroup holds and the part [lo, own_hi) it writes out.  Appends to `tabs`; returns false when a region does
// not fit the LDS (the geometry then keeps per-level launches).
static bool build_pyr_groups(orbx_extractor *e, const Geom &G, std::vector<int16_t> &tabs)
{
    e->n_pyr_groups = 0;
    int sizes[ORBX_MAX_LEVELS], nsizes = 0;
    {
        const char *env = getenv("ORBX_PYR_GROUPS");        // experiments: "2,5" = levels 1-2, then 3-7; "0" = per-level launches only
        const char *p = env && *env ? env : "2,5";
        while (*p && nsizes < ORBX_MAX_LEVELS) {
            const int v = atoi(p);
            if (v < 1) return false;
            sizes[nsizes++] = std::min(v, ORBX_PYR_GROUP_MAX);
            while (*p && *p != ',') p++;
            if (*p == ',') p++;
        }
        if (!nsizes) return false;
    }
    for (int l = 1; l < G.nlevels; l++) if (G.lv[l].resize_lds == 2) return false;     // exact 2x levels are area averages
    int first = 1, gi = 0;
    while (first < G.nlevels) {
        const int n = std::min(sizes[std::min(gi, nsizes - 1)], G.nlevels - first);
        orbx_extractor::PyrGroup &P = e->pyr_groups[gi];
        P.first = first; P.n = n;
        size_t lds[2] = { 0, 0 };
        std::vector<int> ext_axis[2];
        for (int axis = 0; axis < 2; axis++) {
            const int T = axis ? PG_TH : PG_TW;
            auto dim = [&](int lvl) { return axis ? G.lv[lvl].h : G.lv[lvl].w; };
            const int last = first + n - 1, tiles = (dim(last) + T - 1) / T, rec = axis ? PG_CY_REC : PG_CX_REC;
            std::vector<int> lo((size_t)(n + 1) * tiles), hi(lo.size()), own(lo.size());
            for (int t = 0; t < tiles; t++) { lo[(size_t)n * tiles + t] = t * T; hi[(size_t)n * tiles + t] = own[(size_t)n * tiles + t] = std::min(t * T + T, dim(last)); }
            for (int k = n - 1; k >= 0; k--) {
                const int lvl = first - 1 + k, D = dim(lvl);                    // the level of step k; step k + 1 reads it through its table
                const int16_t *tb = &tabs[axis ? G.lv[lvl + 1].tab_y : G.lv[lvl + 1].tab_x];
                std::vector<int> nlo(tiles), nhi(tiles);
                for (int t = 0; t < tiles; t++) {
                    nlo[t] = tb[4 * lo[(size_t)(k + 1) * tiles + t]];
                    nhi[t] = std::min(tb[4 * (hi[(size_t)(k + 1) * tiles + t] - 1)] + 1, D - 1) + 1;
                    if (nlo[t] < 0 || nhi[t] <= nlo[t] || (t && nlo[t] < nlo[t - 1])) return false;   // not a monotone down-scaling table
                }
                for (int t = 0; t < tiles; t++) {
                    size_t i = (size_t)k * tiles + t;
                    if (k == 0) { lo[i] = nlo[t] & ~3; hi[i] = nhi[t]; own[i] = nhi[t]; }
                    else {
                        lo[i] = t ? nlo[t] : 0;
                        own[i] = t + 1 < tiles ? nlo[t + 1] : D;
                        hi[i] = std::max(nhi[t], own[i]);
                    }
                }
            }
            // records + the LDS need of the even / odd steps
            const int off = (int)tabs.size();
            (axis ? P.tab_cy : P.tab_cx) = off;
            tabs.resize(tabs.size() + (size_t)tiles * rec * (n + 1), 0);
            std::vector<int> ext(n + 1, 0);                                    // largest extent of a step over the tiles (x: LDS pitch, y: rows)
            for (int t = 0; t < tiles; t++)
                for (int k = 0; k <= n; k++) {
                    const size_t i = (size_t)k * tiles + t;
                    int16_t *r = &tabs[off + ((size_t)t * (n + 1) + k) * rec];
                    if (hi[i] > 32767) return false;
                    r[0] = (int16_t)lo[i]; r[1] = (int16_t)hi[i]; r[2] = (int16_t)own[i];
                    int extent = hi[i] - lo[i];
                    if (!axis) {
                        int div;
                        if (k == 0) {
                            const int pitch_lim = lo[i] + (((dim(first - 1) - lo[i]) + 3) & ~3);      // align4(w) as seen from lo: never past the pitch
                            const int ndw = (std::min(lo[i] + ((hi[i] - lo[i] + 3) & ~3), pitch_lim) - lo[i]) / 4;
                            r[3] = (int16_t)ndw; div = ndw; extent = 4 * ndw;
                        } else { div = (extent + 3) >> 2; extent = (extent + 3) & ~3; }     // groups of four pixels per row
                        const unsigned magic = (unsigned)((0x100000000ull + (unsigned)div - 1) / (unsigned)div);
                        r[4] = (int16_t)(magic & 0xFFFF); r[5] = (int16_t)(magic >> 16);
                    }
                    ext[k] = std::max(ext[k], extent);
                }
            if (!axis) P.tiles_x = tiles; else P.tiles_y = tiles;
            ext_axis[axis] = ext;
        }
        for (int k = 0; k < n; k++) lds[k & 1] = std::max(lds[k & 1], (size_t)ext_axis[0][k] * ext_axis[1][k]);   // pitch x rows; step n is not kept
        P.lds_b = (int)align_up(lds[0], 16);
        P.lds_bytes = P.lds_b + (int)align_up(lds[1], 16);
        if (P.lds_bytes > PG_LDS_LIMIT) return false;
        first += n; gi++;
    }
    e->n_pyr_groups = gi;
    return true;
}

// The pyramid's step of orbx_prepare_geometry: lays out the tables of every level >= 1 (LevelGeom::tab_*, int16 units of `tabs`), fills
// them, decides each level's kernel (resize_lds) and appends the k_pyr_group tables (e->pyr_groups).
void orbx_pyramid_plan(orbx_extractor *e, Geom &G, std::vector<int16_t> &tabs)
{
    size_t tab_units = 0;
    for (int l = 1; l < e->nlevels; l++) {
        LevelGeom &L = G.lv[l];
        L.tab_x = (int)tab_units; tab_units += 4 * (size_t)L.w;   // int16 units, multiples of 4: 8-byte aligned quads
        L.tab_y = (int)tab_units; tab_units += 4 * (size_t)L.h;
        // k_resize's per-tile records: one per tile row (first source row, count, emit entries), one per tile column
        L.tab_ty = (int)tab_units; tab_units += (size_t)RS_TY_REC * ((L.h + RS_TH - 1) / RS_TH);
        L.tab_tx = (int)tab_units; tab_units += 4 * (size_t)((L.w + RS_TW - 1) / RS_TW);
    }
    // resize tables
    tabs.assign(tab_units, 0);
    std::vector<char> emit_ok(e->nlevels, 1);
    std::vector<std::vector<int16_t>> emit(e->nlevels);
    for (int l = 1; l < e->nlevels; l++) {
        LevelGeom &L = G.lv[l];
        const LevelGeom &S = G.lv[l - 1];
        linear_tables(S.w, L.w, &tabs[L.tab_x]);
        linear_tables(S.h, L.h, &tabs[L.tab_y]);
        // emit table of k_resize: source row sy -> the output row y whose LOWER source row min(sy0 + 1, S.h - 1) is sy:
        // (y | same << 13 | two << 14, b0, b1, 0), y = -1 for none
        emit[l].assign(4 * (size_t)S.h, 0);
        int16_t *ts = emit[l].data();
        const int16_t *ty = &tabs[L.tab_y];
        for (int sy = 0; sy < S.h; sy++) ts[4 * sy] = -1;
        for (int y = 0; y < L.h; y++) {
            const int sy0 = ty[4 * y], rb = sy0 + 1 < S.h - 1 ? sy0 + 1 : S.h - 1, same = sy0 == rb;
            if (ts[4 * rb] < 0) {
                ts[4 * rb] = (int16_t)(y | (same ? 0x2000 : 0)); ts[4 * rb + 1] = ty[4 * y + 1]; ts[4 * rb + 2] = ty[4 * y + 2];
            } else if (same && (ts[4 * rb] & 0xFFF) == y - 1 && !(ts[4 * rb] & 0x6000) && ty[4 * y + 1] == 2048 && ty[4 * y + 2] == 0) {
                ts[4 * rb] |= 0x4000;       // second row on the clamped last source row
            } else emit_ok[l] = 0;          // not a down-scaling table: such a level takes k_resize_direct
        }
    }
    for (int l = 1; l < e->nlevels; l++) { // does every output tile's source rectangle fit k_resize's LDS tile?
        LevelGeom &L = G.lv[l];
        const LevelGeom &S = G.lv[l - 1];
        const int16_t *tx = &tabs[L.tab_x], *ty = &tabs[L.tab_y];
        bool ok = true;
        for (int x0 = 0; x0 < L.w && ok; x0 += RS_TW) {
            const int xl = (x0 + RS_TW < L.w ? x0 + RS_TW : L.w) - 1;
            const int smax = tx[4 * xl] + 1 < S.w - 1 ? tx[4 * xl] + 1 : S.w - 1;
            if (((smax - tx[4 * x0]) / 4 + 1) * 4 > RS_PITCH) ok = false;
        }
        for (int y0 = 0; y0 < L.h && ok; y0 += RS_TH) {
            const int yl = (y0 + RS_TH < L.h ? y0 + RS_TH : L.h) - 1;
            const int smax = ty[4 * yl] + 1 < S.h - 1 ? ty[4 * yl] + 1 : S.h - 1;
            if (smax - ty[4 * y0] + 1 > RS_ROWS) ok = false;
        }
        L.resize_lds = (S.w == 2 * L.w && S.h == 2 * L.h) ? 2 : (ok && emit_ok[l] && L.h < 4096) ? 1 : 0;   // 2: area-average kernel path (k_resize_direct)
        if (L.resize_lds != 1) continue;
        // per-tile records (see k_resize): everything a tile needs before its loads, in one fetch
        for (int by = 0, y0 = 0; y0 < L.h; by++, y0 += RS_TH) {
            int16_t *r = &tabs[L.tab_ty + (size_t)by * RS_TY_REC];
            const int yl = (y0 + RS_TH < L.h ? y0 + RS_TH : L.h) - 1;
            const int sy_min = ty[4 * y0], sy_max = ty[4 * yl] + 1 < S.h - 1 ? ty[4 * yl] + 1 : S.h - 1, nrows = sy_max - sy_min + 1;
            r[0] = (int16_t)sy_min; r[1] = (int16_t)nrows; r[2] = r[3] = 0;
            for (int k = 0; k < RS_ROWS; k++) {
                int16_t *q = r + 4 + 4 * k;
                q[0] = -1; q[1] = q[2] = q[3] = 0;
                if (k >= nrows) continue;
                const int16_t *t = &emit[l][4 * (size_t)(sy_min + k)];
                if (t[0] < 0) continue;
                const int y = t[0] & 0xFFF, in1 = y >= y0 && y <= yl, in2 = (t[0] & 0x4000) && y + 1 >= y0 && y + 1 <= yl;
                if (!in1 && !in2) continue;
                q[0] = (int16_t)(y | (t[0] & 0x2000) | (in1 ? 0 : 0x1000) | (in2 ? 0x4000 : 0)); q[1] = t[1]; q[2] = t[2];
            }
        }
        for (int bx = 0, x0 = 0; x0 < L.w; bx++, x0 += RS_TW) {
            int16_t *r = &tabs[L.tab_tx + 4 * (size_t)bx];
            const int xl = (x0 + RS_TW < L.w ? x0 + RS_TW : L.w) - 1;
            const int sx_min = tx[4 * x0], sx_max = tx[4 * xl] + 1 < S.w - 1 ? tx[4 * xl] + 1 : S.w - 1, need = sx_max - sx_min + 1;
            const int nfull = std::min((need + 15) >> 4, (S.w - sx_min) >> 4), tail = std::max(need - 16 * nfull, 0);
            r[0] = (int16_t)sx_min; r[1] = (int16_t)nfull; r[2] = (int16_t)tail; r[3] = 0;
        }
    }
    if (!build_pyr_groups(e, G, tabs)) e->n_pyr_groups = 0;
}

void orbx_pyramid_launch(orbx_extractor *e, const PyrRef &pr, int batch, hipStream_t s)
{
    const Geom &G = e->geom;
    // Pyramid: launches of a frame or two build it in two grouped launches; mid-sized launches keep one launch per level for the big levels
    // (1, 2) and take the small ones (3 .. 7, latency-bound even for dozens of images) in one grouped launch; batches: one launch per level
    const int regime = e->n_pyr_groups > 0 && batch <= e->pyr_group_max_images ? 2
                     : e->n_pyr_groups > 1 && batch <= e->pyr_group_mid_images ? 1 : 0;
    auto launch_level = [&](int l) {
        const LevelGeom &L = G.lv[l];
        orbx_prof_begin(e, ORBX_STAGE_RESIZE, s);
        if (L.resize_lds == 1)
        {
            const LevelGeom &S = G.lv[l - 1];
            ResizeArgs ra;
            ra.d_w = L.w; ra.d_pitch = L.pitch; ra.s_w = S.w; ra.s_pitch = S.pitch; ra.s_level0 = l == 1;
            ra.tab_x = L.tab_x; ra.tab_tx = L.tab_tx; ra.tab_ty = L.tab_ty; ra.d_off = L.pyr_off; ra.s_off = S.pyr_off;
            hipLaunchKernelGGL(k_resize, dim3(batch, (L.w + RS_TW - 1) / RS_TW, (L.h + RS_TH - 1) / RS_TH), dim3(RS_NT), 0, s, ra, pr, e->d_pyr, e->d_tabs);
        }
        else
            hipLaunchKernelGGL(k_resize_direct, dim3((L.pitch / 4 + 63) / 64, (L.h + 3) / 4, batch), dim3(256), 0, s,
                               e->d_geom, l, pr, e->d_pyr, e->d_tabs);
        orbx_prof_end(e, s);
    };
    auto launch_group = [&](int gi) {
        const orbx_extractor::PyrGroup &P = e->pyr_groups[gi];
        const LevelGeom &S = G.lv[P.first - 1];
        PyrGroupArgs ga;
        memset(&ga, 0, sizeof ga);
        ga.n = P.n; ga.s_level0 = P.first == 1; ga.s_w = S.w; ga.s_h = S.h; ga.s_pitch = S.pitch; ga.s_off = S.pyr_off;
        ga.tab_cx = P.tab_cx; ga.tab_cy = P.tab_cy; ga.lds_b = P.lds_b;
        for (int k = 0; k < P.n; k++) {
            const LevelGeom &L = G.lv[P.first + k];
            ga.lv[k].w = L.w; ga.lv[k].h = L.h; ga.lv[k].pitch = L.pitch; ga.lv[k].tab_x = L.tab_x; ga.lv[k].tab_y = L.tab_y; ga.lv[k].pyr_off = L.pyr_off;
        }
        orbx_prof_begin(e, ORBX_STAGE_RESIZE, s);
        hipLaunchKernelGGL(k_pyr_group, dim3(P.tiles_x, P.tiles_y, batch), dim3(PG_NT), (size_t)P.lds_bytes, s, ga, pr, e->d_pyr, e->d_tabs);
        orbx_prof_end(e, s);
    };
    e->last_forms[0] = regime;          // orbx_debug_launch_forms
    if (regime == 0) for (int l = 1; l < G.nlevels; l++) launch_level(l);
    else
        for (int gi = 0; gi < e->n_pyr_groups; gi++) {
            if (regime == 2 || gi >= 1) launch_group(gi);
            else for (int l = e->pyr_groups[gi].first; l < e->pyr_groups[gi].first + e->pyr_groups[gi].n; l++) launch_level(l);
        }
}

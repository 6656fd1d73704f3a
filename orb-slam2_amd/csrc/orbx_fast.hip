// orbx_fast.hip — the extractor's FAST stage (the cell loop of ORBextractor::ComputeKeyPointsOctTree, reference src/ORBextractor.cc:953-1009):
// k_fast (a wave or several per cell) and k_fast2 (a wave per pair of cells), their LDS carves and per-cell / per-pair records
// (orbx_fast_plan) and the choice of waves per cell, grid order and pair form (orbx_fast_launch).  File map of the extractor: orbx_extract.hip.
#include "orbx_device.h"

#include <stdlib.h>
#include <string.h>
#include <algorithm>

// ================================================================ K2: FAST per cell (E3)
// cornerScore<16> without a threshold: with x_k the 16 ring pixels, A = max over the 16 arcs of 9
// contiguous ring pixels of min(v - x) = v - min_arcs(max_arc x) and B = max_arcs(min_arc x) - v.
// A pixel is a FAST-9 corner at threshold t iff max(A,B) > t and its OpenCV score is then
// max(A,B)-1 independent of t, so one score map at minThFAST serves both passes of
// src/ORBextractor.cc:988-995.  The sliding 9-window max/min over the circular ring is a doubling
// 3x3 composition of three-input min/max (v_min3_i32 / v_max3_i32).
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 pk(unsigned lo, unsigned hi)
{
    const unsigned v = lo | (hi << 16);
    return __builtin_bit_cast(u16x2, v);
}

template <int P>
__device__ __forceinline__ int fast_score_full(const uint8_t *t, int th)
{
    const int v = t[0];
    int x[16];
    x[0] = t[3 * P];      x[1] = t[3 * P + 1];  x[2] = t[2 * P + 2];   x[3] = t[P + 3];
    x[4] = t[3];          x[5] = t[-P + 3];     x[6] = t[-2 * P + 2];  x[7] = t[-3 * P + 1];
    x[8] = t[-3 * P];     x[9] = t[-3 * P - 1]; x[10] = t[-2 * P - 2]; x[11] = t[-P - 3];
    x[12] = t[-3];        x[13] = t[P - 3];     x[14] = t[2 * P - 2];  x[15] = t[3 * P - 1];
    // window 9 = 3 x 3 with three-input min/max (v_min3_i32 / v_max3_i32)
    int lo3[16], hi3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        lo3[k] = min(min(x[k], x[(k + 1) & 15]), x[(k + 2) & 15]);
        hi3[k] = max(max(x[k], x[(k + 1) & 15]), x[(k + 2) & 15]);
    }
    int lo9[16], hi9[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        lo9[k] = min(min(lo3[k], lo3[(k + 3) & 15]), lo3[(k + 6) & 15]);
        hi9[k] = max(max(hi3[k], hi3[(k + 3) & 15]), hi3[(k + 6) & 15]);
    }
    int a[6], bq[6];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        a[k] = max(max(lo9[3 * k], lo9[3 * k + 1]), lo9[3 * k + 2]);
        bq[k] = min(min(hi9[3 * k], hi9[3 * k + 1]), hi9[3 * k + 2]);
    }
    const int max_of_min = max(max(max(a[0], a[1]), a[2]), max(max(a[3], a[4]), lo9[15]));
    const int min_of_max = min(min(min(bq[0], bq[1]), bq[2]), min(min(bq[3], bq[4]), hi9[15]));
    const int s = max(v - min_of_max, max_of_min - v);
    return s > th ? s - 1 : 0;
}

// The same score for TWO pixels per lane (round 4).  gfx950 has packed three-input f16 minimum / maximum (v_pk_minimum3_f16 / v_pk_maximum3_f16)
// at the issue cost of v_min3_u32 (4.4 cycles per wave-instruction, tools/ubench/pk3_cost.hip) -- two three-input comparisons per instruction.
// An 8-bit pixel x travels as the half-precision bit pattern 0x4000 + x: a positive NORMAL number (2 + x / 512) whose order is the order of
// x, so the float minimum / maximum of patterns IS the integer minimum / maximum of pixels (all 2^24 triples x both halves checked on the
// device by the microbenchmark; no denormal mode, NaN or signed zero can be involved).  The low halves carry candidate a, the high halves
// candidate b of the lane: the arc network below is the one of fast_score_full, instruction for instruction, on 128 candidates at a time.
__device__ __forceinline__ unsigned pk_min3(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned pk_max3(unsigned a, unsigned b, unsigned c)
{
    unsigned r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// FAST_PK_BIAS: 0x40004000 makes every pattern a NORMAL half (0x4000 + x) at the price of one v_or_b32 per ring pixel; with 0 the patterns are the
// half-precision SUBNORMALS 0x0000 .. 0x00FF, whose order is also the order of x and which v_pk_minimum3_f16 / v_pk_maximum3_f16 compare exactly as
// long as the wave's float mode keeps f16 denormals (MODE.FP_DENORM[3:2] = 3: LLVM's default for every AMDGPU kernel; k_fast sets it itself on
// entry so that the result cannot depend on a build flag).  Both forms checked over all 2^24 triples by tools/ubench/pk3_cost.hip; 0.743 -> 0.718 ms.
#ifndef FAST_PK_BIAS
#define FAST_PK_BIAS 0u
#endif
template <int P>
__device__ __forceinline__ void fast_score_pair(const uint8_t *ta, const uint8_t *tb, int th, int *sa, int *sb)
{
    constexpr int off[16] = { 3 * P, 3 * P + 1, 2 * P + 2, P + 3, 3, -P + 3, -2 * P + 2, -3 * P + 1,
                              -3 * P, -3 * P - 1, -2 * P - 2, -P - 3, -3, P - 3, 2 * P - 2, 3 * P - 1 };
    // (the packing costs a v_perm_b32 + a v_or_b32 per ring pixel.  ds_read_u8_d16 / _d16_hi would pack in the load, but on an SRAM-ECC part
    // -- gfx950:sramecc+ -- a d16 load clobbers the other half of its register: tried from inline assembly, wrong results, and not faster)
    unsigned x[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        u16x2 v2;
        v2.x = ta[off[k]]; v2.y = tb[off[k]];
        x[k] = __builtin_bit_cast(unsigned, v2) | FAST_PK_BIAS;
    }
    unsigned lo3[16], hi3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        lo3[k] = pk_min3(x[k], x[(k + 1) & 15], x[(k + 2) & 15]);
        hi3[k] = pk_max3(x[k], x[(k + 1) & 15], x[(k + 2) & 15]);
    }
    unsigned lo9[16], hi9[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        lo9[k] = pk_min3(lo3[k], lo3[(k + 3) & 15], lo3[(k + 6) & 15]);
        hi9[k] = pk_max3(hi3[k], hi3[(k + 3) & 15], hi3[(k + 6) & 15]);
    }
    unsigned a[5], bq[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        a[k] = pk_max3(lo9[3 * k], lo9[3 * k + 1], lo9[3 * k + 2]);
        bq[k] = pk_min3(hi9[3 * k], hi9[3 * k + 1], hi9[3 * k + 2]);
    }
    const unsigned mom = pk_max3(pk_max3(a[0], a[1], a[2]), pk_max3(a[3], a[4], lo9[15]), lo9[15]);     // max over arcs of the arc minimum, both halves
    const unsigned mox = pk_min3(pk_min3(bq[0], bq[1], bq[2]), pk_min3(bq[3], bq[4], hi9[15]), hi9[15]); // min over arcs of the arc maximum
    const int va = ta[0], vb = tb[0];
    const int s_a = max(va - (int)(mox & 0xFFu), (int)(mom & 0xFFu) - va);
    const int s_b = max(vb - (int)((mox >> 16) & 0xFFu), (int)((mom >> 16) & 0xFFu) - vb);
    *sa = s_a > th ? s_a - 1 : 0;
    *sb = s_b > th ? s_b - 1 : 0;
}

// One wave (64-thread workgroup) per (cell, image) -- no workgroup barriers, many independent cells in flight per CU.
// The kernel is VALU-issue bound, and on gfx950 only a few wave64 opcodes issue at the full rate (add / sub / and / or /
// xor / lshr / mov and the 16-bit VOP2 forms: ~2.5 cycles per wave-instruction; min / max / min3 / perm / alignbyte /
// packed-16 / mul / cmp / cndmask / mbcnt / DPP / SDWA: ~4.3, tools/ubench/op_cost.hip), so every phase is written for few
// instruction-cycles per pixel:
//  1. the cell (+3 px halo) goes to LDS with direct loads (global_load_lds_dword: no VGPR round trip, no ds_write; one
//     instruction = RPL whole tile rows), all in flight at once, while the wave zeroes its score tile and bitmaps;
//  2. pretest on 4 horizontally adjacent pixels per lane in byte-parallel (SWAR) form with full-rate ops only: on values
//     halved to 7 bits a borrow-free per-byte subtract leaves "x7 <= c7 - s7" in bit 7 of every byte.  Halving makes the test
//     CONSERVATIVE (never a false negative; floor((c-s)/2) <= c7 - s7), which is all a pretest needs: a FAST-9 corner has two
//     adjacent compass pixels (of N, E, S, W at distance 3) darker than c - t or brighter than c + t.  The four flag bits are
//     OR-ed into a per-row candidate bitmap in LDS (ds_or_b32): no ballots, no per-iteration prefix sums;
//  3. lane = row: the row bitmaps are unrolled into the dense ordered candidate list (one wave prefix sum per cell);
//  4. threshold-free cornerScore (v_min3 / v_max3 arc network) on dense lanes -> score tile;
//  5. strict in-cell 3x3 maximum per listed pixel -> survivor bitmap; lane = row again: ordered emission.
// Threshold schedule of src/ORBextractor.cc:988-995 as it stands: the whole sequence runs at iniThFAST; only a cell that
// keeps nothing (no corner, or only tied maxima) runs again at minThFAST.  Scores do not depend on the threshold and the
// iniThFAST pretest passes ~40 % fewer pixels to the score network than a minThFAST one, which nearly every textured cell
// used to pay for.  Candidate = x | y<<12 | score<<24, (x,y) relative to (16,16).
extern __shared__ __align__(16) unsigned char fast_smem[];
#ifndef FAST_XG
#define FAST_XG 2
#endif
// Launch constants of k_fast by value (kernel-argument segment): fetching them through the Geom pointer was one more level in
// the chain of dependent scalar loads every wave starts with (arguments -> geometry -> cell record -> tile).
struct FastArgs {
    int total_cells;
    int lds_sc, lds_list, lds_bm;   // LDS carve: score tile, candidate list, candidate bitmap (the survivor bitmap follows it)
    int bm_rows;                    // bitmap rows (u64 each): tallest detect area plus the row overrun of the last pretest iteration
    int ini_th, min_th;
    int list_cap;                   // entries of the candidate list (used by the several-waves-per-cell form; one wave: ORBX_FAST_LIST_CAP)
    int lane_tab_off;               // byte offset of the lane table behind the cell records (orbx_fast_plan)
    long long cand_total;
};

// Lane geometry of k_fast's pretest and list phases from the host.  Everything a lane derives from its number and the cell's detect shape
// (dw, dh) -- its pretest row and group, pixel mask and bitmap slot, its list segment -- is the same for every cell of that shape, and a
// geometry has a handful of shapes (interior, last column, last row, corner of each level: under 32 at 1241 x 376, for ~640 k waves per
// launch).  The host tabulates it: one 16-byte entry per (shape class, lane), the class rides above the level number in CellRec::level.  A wave
// requests its entry before the tile loads and reads it behind the same wait, so the fetch costs no round trip of its own.
//   x  pixel mask of the lane's pretest group (0: the lane idles)
//   y  bits 0-15 tile byte offset of the group's centre dword in the first pretest iteration, bits 16-31 byte offset of its bitmap word
//   z  bits 0-15 list segment as the entries carry it (row << 6 | first bit), bit 16 the segment's row exists, bits 24-28 shift of the
//      group's nibble inside its bitmap word
//   w  0
// (The tile-load geometry, lane / DWR and lane % DWR, stays in the kernel: the loads it addresses are what covers the fetch.)
// The wave-uniform part (rows per pretest iteration, half-row segments) stays on the scalar unit, which has time to spare.
// One pure function of (P, dw, dh, lane) serves the plan and orbx_debug_fast_lane_table; uni[0] = rpi, uni[1] = half_mode.
#define FAST_MAX_CLASSES 2048       // the class shares CellRec::level (a short) with the level number: level in bits 0-3, class in bits 4-14
static_assert(ORBX_MAX_LEVELS <= 16, "CellRec::level: four bits of level number");
static void fast_lane_entry(int P, int dw, int dh, int lane, uint32_t out[4], int uni[2])
{
    const int gpr = (dw + 3) >> 2;
    const unsigned magic = 0xFFFFFFFFu / (unsigned)gpr + 1u;
    const int lq = gpr == 1 ? lane : (int)(((unsigned long long)(unsigned)lane * magic) >> 32);
    const int rpi = std::min(gpr == 1 ? 64 : (int)((64ull * magic) >> 32), 8);
    const int lr = std::min(lq, rpi), gq = lane - lq * gpr;
    const int nvalid = std::max(1, std::min(4, dw - 4 * gq));
    const unsigned vmask = lr < rpi ? (0x80808080u >> (8 * (4 - nvalid))) : 0u;
    const int bm_sh = 4 * (gq & 7);
    const bool half_mode = dh <= 32 && dw <= 32;
    const int brow = half_mode ? lane >> 1 : lane;
    const unsigned bsh = half_mode ? 16u * (lane & 1) : 0u;
    const unsigned pc_off = (unsigned)((lr + 3) * P + 4 * (1 + gq)), pb_off = 4u * (unsigned)(lr * 2 + (gq >> 3));
    out[0] = vmask;
    out[1] = pc_off | (pb_off << 16);
    out[2] = ((unsigned)brow << 6) | bsh | (brow < dh ? 0x10000u : 0u) | ((unsigned)bm_sh << 24);
    out[3] = 0;
    uni[0] = rpi; uni[1] = half_mode ? 1 : 0;
}

// debug: the lane table of one detect shape, out[64][4], and the wave-uniform pair uni[2] = (rpi, half_mode); needs no device
extern "C" int orbx_debug_fast_lane_table(int tile_pitch, int dw, int dh, uint32_t *out, int32_t *uni)
{
    if ((tile_pitch != 48 && tile_pitch != ORBX_TILE_PITCH) || dw < 1 || dh < 1 || dw > (tile_pitch == 48 ? 38 : 59) || dh > 64 || !out || !uni) {
        orbx_set_error("orbx_debug_fast_lane_table: invalid argument"); return ORBX_E_INVALID;
    }
    int u[2] = { 0, 0 };
    for (int lane = 0; lane < 64; lane++) fast_lane_entry(tile_pitch, dw, dh, lane, out + 4 * lane, u);
    uni[0] = u[0]; uni[1] = u[1];
    return ORBX_OK;
}

#ifdef ORBX_DIAG
__device__ unsigned long long g_fast_stamp[4096 * 8]; // diagnostic build only: summed phase cycles of k_fast, 4096 slots
__device__ uint2 g_span_0[SPAN_SLOTS];                // SPAN_END(0): slot 0 of orbx_diag_spans
#ifdef ORBX_DIAG_SPANS_ONLY     // (see STAMP_TO, orbx_device.h) every wave of k_fast logs the end of its phases in its own slot
__device__ unsigned g_fast_phase[16384][8];
#define STAMP(k) do { (void)_t_prev; if (threadIdx.x == 0) { \
    const unsigned _id = blockIdx.x + gridDim.x * blockIdx.y; if (_id < 16384) g_fast_phase[_id][k] = (unsigned)__builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define STAMP(k) STAMP_TO(g_fast_stamp, k)
#endif
#else
#define STAMP(k) do { } while (0)
#endif

// P / SP = LDS pitches of the pixel tile and the score tile: (48, 40) when every cell of the pyramid is at most 38 px wide
// (one direct load = 5 tile rows of 12 dwords, 60 lanes), else (80, 64) (3 rows of 20 dwords).  Both tile pitches put rows
// r and r + 8 (and no closer pair) on the same LDS banks: candidates line up along vertical image edges, and with a
// 64-byte pitch (rows r, r + 2 on the same banks) the byte reads of the score network ran 3.4x the bank-conflict cycles.
// NW = waves per cell: 1 for batches (above).  A launch of a frame or two leaves most of the chip idle and lasts as long as its
// fullest cell (a cell with 5x the candidates of the median one ran 15.6 us against 5.3 us: the score and maximum loops walk the
// candidate list 64 at a time): there NW waves share the cell -- tile rows, pretest rows and list entries are dealt round-robin to
// the waves, the bitmaps and tiles are the workgroup's, list and emission stay with wave 0.  Same results by construction: every
// phase writes disjoint bytes or ORs bits, and the phases are separated by the barriers the one-wave form already has.
template <int P, int SP, int NW, bool IMG_FAST = false>
__global__ __launch_bounds__(64 * NW) void k_fast(const FastArgs fa, const CellRec *__restrict__ cells, PyrRef pr,
                                             int *__restrict__ cell_cnt, uint32_t *__restrict__ cand, uint32_t *__restrict__ cand_prim)
{
    constexpr int DWR = P / 4;      // dwords per tile row = lanes per row of one direct load
    constexpr int RPL = 64 / DWR;   // whole tile rows per direct load (lanes >= RPL * DWR stay idle)
    // The kernel is VALU-issue bound and sensitive to where its code lies: shifted by an ODD number of dwords (its 8-byte instructions
    // then straddle 8-byte fetch units) it runs 2.5 % slower, any even shift is the same (tools/ab_fast_only.py on -DORBX_FAST_PAD=1..15
    // builds).  A one-instruction change near the top of the kernel had moved it by 4 bytes: when this kernel changes, compare both parities.
#ifdef ORBX_FAST_PAD    // experiment: shift the kernel's code by ORBX_FAST_PAD dwords (s_nop 0)
    asm volatile(".fill %0, 4, 0xBF800000" :: "n"(ORBX_FAST_PAD));
#endif
    if (FAST_PK_BIAS == 0u)
        __builtin_amdgcn_s_setreg((1 << 11) | (6 << 6) | 1, 3);      // hwreg(HW_REG_MODE, 6, 2) = 3: f16 / f64 denormals kept (fast_score_pair compares subnormal patterns)
    uint8_t *tile = fast_smem;
    uint8_t *sc = fast_smem + fa.lds_sc;
    uint16_t *list = reinterpret_cast<uint16_t *>(fast_smem + fa.lds_list);
    uint32_t *bm = reinterpret_cast<uint32_t *>(fast_smem + fa.lds_bm); // candidate bitmap, then survivor bitmap: u64 per row
    uint32_t *sv = bm + 2 * fa.bm_rows;
    const int ini_th = fa.ini_th, min_th = fa.min_th;
    // IMG_FAST (one wave per cell, batches): grid (image, cell) -- image-fastest, see k_resize: consecutive workgroups take the same cell of
    // different images (0.789 -> 0.778 ms per 512 images); else grid (cell, image): a frame or two, or more cells than grid.y can hold
    const int b = IMG_FAST ? blockIdx.x : blockIdx.y;
    const int lane = NW == 1 ? (int)threadIdx.x : (int)(threadIdx.x & 63), wv = NW == 1 ? 0 : (int)(threadIdx.x >> 6), tid = threadIdx.x;
    // Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8, speed only): remap so that FAST_XG
    // horizontally adjacent cells land on the same XCD (their halos share cache lines in that XCD's L2) while each
    // XCD's work stays spread over the whole image (contiguous runs per XCD were measured slower).
    int cell;
    {
        const int bx = IMG_FAST ? blockIdx.y : blockIdx.x;
        const int grp = bx / (8 * FAST_XG), r = bx - grp * (8 * FAST_XG);
        cell = grp * (8 * FAST_XG) + (r & 7) * FAST_XG + (r >> 3);
        if (cell >= fa.total_cells) return;
    }
#ifdef ORBX_DIAG
    unsigned long long _t_prev = __builtin_amdgcn_s_memtime();
#endif
    SPAN_BEGIN();
    // the 40-byte record as ten dwords (scalar loads; 16-bit fields fetched by themselves become vector loads on gfx950)
    CellRec rec;
    int cls;
    {
        const uint32_t *cw = reinterpret_cast<const uint32_t *>(cells + cell);
        uint32_t w[10];
#pragma unroll
        for (int i = 0; i < 10; i++) w[i] = cw[i];
        rec.level = (short)(w[0] & 0xF); rec.skip = (short)(w[0] >> 16);
        cls = (int)((w[0] >> 4) & 0x7FF);       // shape class of the cell: its block of the lane table
        rec.ini_x = (short)(w[1] & 0xFFFF); rec.ini_y = (short)(w[1] >> 16);
        rec.tw = (short)(w[2] & 0xFFFF); rec.th = (short)(w[2] >> 16);
        rec.pitch = (int)w[3]; rec.cand_cap = (int)w[4]; rec.gpr_magic = w[5];
        rec.pyr_off = (long long)(((unsigned long long)w[7] << 32) | w[6]);
        rec.cand_slot = (long long)(((unsigned long long)w[9] << 32) | w[8]);
    }
    int *my_cnt = cell_cnt + (long long)b * fa.total_cells + cell;
    if (rec.skip) { // src/ORBextractor.cc:961-976 skip rules, evaluated on the host
        if (lane == 0) *my_cnt = 0;
        return;
    }
#ifndef ORBX_FAST_LANE_INLINE
    // the lane's pretest / list geometry (fast_lane_entry), requested ahead of the tile loads and first read behind their wait
    const uint4 lg = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(cells) + fa.lane_tab_off)[cls * 64 + lane];
#endif
    const int ini_x = rec.ini_x, ini_y = rec.ini_y, tw = rec.tw, th = rec.th, dw = tw - 6, dh = th - 6;
    const int pitch = rec.level == 0 ? pr.img0_pitch : rec.pitch;
    const uint8_t *img = rec.level == 0 ? pr.img0 + (long long)b * pr.img0_stride
                                        : pr.pyr + (long long)b * pr.pyr_stride + rec.pyr_off;
    // ---- 1. tile: the fetch starts one byte left of the cell (gfx950 global and LDS-direct loads need no alignment), so the
    // first detectable pixel always sits at tile column 4: every pretest group of four pixels is a whole LDS dword whatever
    // the cell's position or the caller's pitch.  Lane = (row lane / DWR, dword lane % DWR) of RPL whole rows per load; the data
    // lands at tile + RPL * P * k + 4 * lane, i.e. row-major with pitch P.
    constexpr int xo = 1; // tile column of image column ini_x
    {
        const int lr0 = lane / DWR, lc = lane - lr0 * DWR;
        const int ndw = (tw + xo + 3) >> 2;             // dwords per row that hold cell pixels (<= 17)
        // scalar row base + one 32-bit lane offset (lds_load_sbase: the load's saddr form): the row groups advance on the scalar unit,
        // no 64-bit vector add per load
        const uint8_t *base = img + (long long)ini_y * pitch + (ini_x - xo);
        const unsigned voff = (unsigned)(lr0 * pitch + 4 * lc);
        const int full = th / RPL;
        if (lc < ndw && lr0 < RPL) {
            const int wvu = NW == 1 ? 0 : __builtin_amdgcn_readfirstlane(wv);   // (wave-uniform, but not provably so from threadIdx.x >> 6)
            base += (long long)wvu * RPL * pitch;
            for (int k = wvu; k < full; k += NW, base += (long long)NW * RPL * pitch)
                lds_load_sbase<4>(base, voff, tile + RPL * P * k);
            // the last, partial group of rows never reads below the cell (after the loop `base` stands at this wave's next group:
            // the partial group is `full`, taken by the wave whose turn it is)
            if ((NW == 1 || full % NW == wvu) && full * RPL + lr0 < th)
                lds_load_sbase<4>(base, voff, tile + RPL * P * full);
        }
    }
    {   // meanwhile: zero score tile (1-px zero rim included) and both bitmaps
        uint4 *z = reinterpret_cast<uint4 *>(sc);
        for (int i = tid; i < ((dh + 2) * SP + 15) / 16; i += 64 * NW) z[i] = make_uint4(0, 0, 0, 0);
        uint4 *zb = reinterpret_cast<uint4 *>(bm);
        for (int i = tid; i < fa.bm_rows; i += 64 * NW) zb[i] = make_uint4(0, 0, 0, 0);   // 2 bitmaps x 8 bytes per row
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the direct loads have landed in LDS
    __syncthreads();
    STAMP(0);
    const uint8_t *t0 = tile + 3 * P + xo + 3;           // detectable pixel (0, 0)
    // pretest geometry: tile dwords 1 .. gpr of a row hold the detectable pixels (tile columns 4 .. dw + 3); one iteration =
    // rpi whole rows, lane = (row lr, group gq); lanes beyond rpi * gpr idle with an empty pixel mask
    const int gpr = (dw + 3) >> 2;
    // floor(i / gpr) by multiply-high with the host's magic number (an integer division costs ~30 instructions here)
    const int rpi = min(gpr == 1 ? 64 : (int)__umulhi(64u, rec.gpr_magic), 8);   // (the last column's cells can be narrow: keep the row overrun <= 8)
    // Bitmap rows are walked with one lane per SEGMENT: a whole row (64 bits, low word then high word), or -- when the detect
    // area is at most 32 x 32, most cells of a 30-px grid -- half a 32-bit row word: the bit loops below run as long as the
    // fullest segment, and half rows are half as full
    const bool half_mode = dh <= 32 && dw <= 32;
#ifdef ORBX_FAST_LANE_INLINE   // the lane's geometry computed by every wave (the form before the host table; fast_lane_entry restates it)
    const int lq = gpr == 1 ? lane : (int)__umulhi((unsigned)lane, rec.gpr_magic);
    const int lr = min(lq, rpi), gq = lane - lq * gpr;
    const int nvalid = max(1, min(4, dw - 4 * gq));      // only the last group of a row can be partial
    const unsigned vmask = lr < rpi ? (0x80808080u >> (8 * (4 - nvalid))) : 0u;
    const int bm_sh = 4 * (gq & 7);
    const int pc_off = (lr + 3) * P + 4 * (1 + gq), pb_off = 4 * (lr * 2 + (gq >> 3));
    const int brow = half_mode ? lane >> 1 : lane;
    const unsigned bsh = half_mode ? 16u * (lane & 1) : 0u;
    const bool row_ok = brow < dh;
    (void)cls;
#else
    const unsigned vmask = lg.x;
    const int pc_off = (int)(lg.y & 0xFFFFu), pb_off = (int)(lg.y >> 16);
    const int bm_sh = (int)(lg.z >> 24);
    const int brow = (int)((lg.z & 0xFFFFu) >> 6);
    const unsigned bsh = lg.z & 63u;
    const bool row_ok = (lg.z & 0x10000u) != 0;
#endif
    uint32_t *slot = cand + (long long)b * fa.cand_total + rec.cand_slot;
    uint32_t *prim = cand_prim + ((long long)b * fa.total_cells + cell) * ORBX_CAND_PRIM;   // the first 16 candidates: dense, 64 B per cell
    int th_cur = ini_th, nsurv = 0;
    int emitted = 0;            // one wave, one round: maxima written straight from the corner list (see below)
    bool direct = false;
    for (int pass = 0; pass < 2; pass++) {
        // ---- 2. SWAR pretest.  With s = t + 1 and x7 = x >> 1 per byte: x < c - t  ==>  x7 <= c7 - s7 (dark) and
        // x > c + t  ==>  (127 - x7) <= (127 - c7) - s7 (bright).  R = (c7 | 0x80) - s7 cannot borrow across bytes; its bit 7
        // says c7 >= s7 (else no x can pass) and its low 7 bits are c7 - s7; (R | 0x80) - x7 then has bit 7 set iff
        // x7 <= c7 - s7.  The bright side is the same on complemented values, folded into an add: KB + x7 with
        // KB = (RB | 0x80) - 0x7f.  Corner candidates: (N | S) & (E | W) on either side.
        {
            const unsigned s7 = (unsigned)((th_cur + 1) >> 1) * 0x01010101u;
            const uint8_t *pc = tile + pc_off + wv * rpi * P;
            uint32_t *pb = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(bm) + pb_off) + wv * rpi * 2;
            for (int r0 = wv * rpi; r0 < dh; r0 += NW * rpi, pc += NW * rpi * P, pb += NW * rpi * 2) {
                const uint32_t *rc = reinterpret_cast<const uint32_t *>(pc);
                const unsigned C = rc[0], Wd = rc[-1], Ed = rc[1], N = rc[3 * DWR], S = rc[-3 * DWR];
                const unsigned Wv = __builtin_amdgcn_alignbyte(C, Wd, 1), Ev = __builtin_amdgcn_alignbyte(Ed, C, 3);
                const unsigned c7 = (C >> 1) & 0x7f7f7f7fu, n7 = (N >> 1) & 0x7f7f7f7fu, u7 = (S >> 1) & 0x7f7f7f7fu,
                               e7 = (Ev >> 1) & 0x7f7f7f7fu, w7 = (Wv >> 1) & 0x7f7f7f7fu;
                const unsigned R = (c7 | 0x80808080u) - s7, RD = R | 0x80808080u;
                const unsigned RB = ((c7 ^ 0x7f7f7f7fu) | 0x80808080u) - s7, KB = (RB | 0x80808080u) - 0x7f7f7f7fu;
                const unsigned dark = ((RD - n7) | (RD - u7)) & ((RD - e7) | (RD - w7)) & R;
                const unsigned bright = ((KB + n7) | (KB + u7)) & ((KB + e7) | (KB + w7)) & RB;
                const unsigned any = (dark | bright) & vmask;
                // bits 7, 15, 23, 31 -> one nibble: the multiplier routes bit 8k of (any >> 7) to bit 24 + k, no carries
                const unsigned nib = (((any >> 7) * 0x01020408u) >> 24) << bm_sh;
                if (nib) atomicOr(pb, nib);   // rows >= dh of the last iteration land in bitmap rows that are never read
            }
        }
        __syncthreads();
        STAMP(1);
        // ---- 3. bitmap -> ordered list of (py << 6 | px): lane = segment, exclusive prefix of the segment populations.  The list holds
        // ORBX_FAST_LIST_CAP entries (LDS is what limits the waves per CU, and a textured cell lists ~130 of its ~1000 pixels);
        // a cell with more candidates takes them in rounds of that many: all scores first, then the maxima
        unsigned c_lo = 0, c_hi = 0;
        if (row_ok) { const uint2 m = *reinterpret_cast<const uint2 *>(bm + 2 * brow); c_lo = half_mode ? (m.x >> bsh) & 0xFFFFu : m.x; c_hi = half_mode ? 0u : m.y; }
        const int c_cnt = __popc(c_lo) + __popc(c_hi);
        const int c_incl = wave_incl_scan(c_cnt);
        const int nlist = __builtin_amdgcn_readlane(c_incl, 63);
        const unsigned rowbits = ((unsigned)brow << 6) | bsh;
        // ---- 4. full score on the compacted pixels (dense lanes); entries ascend in (py, px)
        // With `compact` the entries that turned out to be corners (3 % of the pixels, against the 13 % the pretest lists) are
        // packed to the front of the list in place (a write never passes the reads of its own or a later iteration): the
        // maximum search below then takes one iteration where the full list took two or three.  Returns their number.
        auto score_entries = [&](int n, bool compact) -> int {
            int n2 = 0;
            if (NW == 1) {
                // one wave: 128 entries per iteration, two per lane (fast_score_pair); lane L takes entries i0 + L and i0 + 64 + L, so the
                // corners of the first 64 precede those of the second 64 in the compacted list as they did in the list
                for (int i0 = 0; i0 < n; i0 += 128) {
                    const int ia = i0 + lane, ib = ia + 64;
                    const bool in_a = ia < n, in_b = ib < n;
                    const int ea = list[in_a ? ia : i0], eb = list[in_b ? ib : i0];      // (entry i0 always exists: a lane without an entry recomputes it and drops the result)
                    const int pya = ea >> 6, pxa = ea & 63, pyb = eb >> 6, pxb = eb & 63;
                    int sa, sb;
                    fast_score_pair<P>(t0 + pya * P + pxa, t0 + pyb * P + pxb, th_cur, &sa, &sb);
                    if (!in_a) sa = 0;
                    if (!in_b) sb = 0;
                    if (in_a) sc[(pya + 1) * SP + pxa + 1] = (uint8_t)sa;
                    if (in_b) sc[(pyb + 1) * SP + pxb + 1] = (uint8_t)sb;
                    if (compact) {
                        const unsigned long long ma = __ballot(sa > 0), mb = __ballot(sb > 0);
                        const int na = __popcll(ma);
                        if (sa > 0) list[n2 + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ma >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ma, 0u))] = (uint16_t)ea;
                        if (sb > 0) list[n2 + na + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mb, 0u))] = (uint16_t)eb;
                        n2 += na + __popcll(mb);
                    }
                }
                return compact ? n2 : n;
            }
            // several waves per cell: wave w takes the entries [128 (w + NW k), 128 (w + NW k) + 128), two per lane as above; no compaction (the
            // maximum search walks the whole list: entries that are no corners have score 0)
            for (int i0 = 128 * wv; i0 < n; i0 += 128 * NW) {
                const int ia = i0 + lane, ib = ia + 64;
                const bool in_a = ia < n, in_b = ib < n;
                const int ea = list[in_a ? ia : i0], eb = list[in_b ? ib : i0];
                const int pya = ea >> 6, pxa = ea & 63, pyb = eb >> 6, pxb = eb & 63;
                int sa, sb;
                fast_score_pair<P>(t0 + pya * P + pxa, t0 + pyb * P + pxb, th_cur, &sa, &sb);
                if (in_a) sc[(pya + 1) * SP + pxa + 1] = (uint8_t)sa;
                if (in_b) sc[(pyb + 1) * SP + pxb + 1] = (uint8_t)sb;
            }
            return n;
        };
        // ---- 5. strict 3x3 maximum of the listed pixels (only they can score > 0) -> survivor bitmap
        auto mark_maxima = [&](int n) {
            for (int i0 = 64 * wv; i0 < n; i0 += 64 * NW) {
                const int i = i0 + lane;
                if (i < n) {          // lanes without an entry issue no LDS traffic at all (an LDS atomic costs per active lane, also one that ORs a zero)
                    const int e = list[i], py = e >> 6, px = e & 63;
                    const uint8_t *c = sc + (py + 1) * SP + px + 1;
                    const int s = c[0];
                    const int nb = max(max(max((int)c[-1], (int)c[1]), max((int)c[-SP - 1], (int)c[-SP])),
                                       max(max((int)c[-SP + 1], (int)c[SP - 1]), max((int)c[SP], (int)c[SP + 1])));
                    if (s > nb) atomicOr(sv + 2 * py + (px >> 5), 1u << (px & 31));   // s > nb >= 0 implies a corner at th_cur
                }
            }
        };
        const int list_cap = NW == 1 ? ORBX_FAST_LIST_CAP : fa.list_cap;     // several waves: a whole cell, always one round
        if (nlist <= list_cap) {
            if (NW == 1) {
                unsigned lo = c_lo, hi = c_hi;
                uint16_t *lp = list + (c_incl - c_cnt);
                while (lo) { *lp++ = (uint16_t)(rowbits | (unsigned)__builtin_ctz(lo)); lo &= lo - 1; }
                while (hi) { *lp++ = (uint16_t)(rowbits | 32u | (unsigned)__builtin_ctz(hi)); hi &= hi - 1; }
            } else {
                // every wave has the same segments and offsets: wave w unrolls bits [16 w / NW * ..) of each 16-bit quarter -- the bit
                // walk is as long as the fullest piece, and a piece is 1 / NW of what one wave walked
                constexpr int PIECE = 64 / 4;                        // a 64-bit row in four 16-bit quarters, each cut in NW pieces
                const unsigned long long rowm = (unsigned long long)c_lo | ((unsigned long long)c_hi << 32);
                uint16_t *lp0 = list + (c_incl - c_cnt);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int b0 = q * PIECE + (PIECE * wv) / NW, b1 = q * PIECE + (PIECE * (wv + 1)) / NW;
                    const unsigned long long below0 = (1ull << b0) - 1ull, below1 = b1 >= 64 ? ~0ull : (1ull << b1) - 1ull;   // b0 < 64 always
                    unsigned long long m = rowm & below1 & ~below0;
                    uint16_t *lp = lp0 + __popcll(rowm & below0);
                    while (m) { *lp++ = (uint16_t)(rowbits | (unsigned)__builtin_ctzll(m)); m &= m - 1; }
                }
            }
            __syncthreads();
            STAMP(5);
            const int ncorner = score_entries(nlist, true);
            STAMP(6);
            __syncthreads();
            STAMP(2);
            if (NW == 1) {
                // one wave, one round (nearly every cell): the compacted corner list is already in the cell's row-major order, so the strict
                // maxima among them are EMITTED as they are found -- a ballot and a rank per 64 corners -- instead of going through the
                // survivor bitmap, a second prefix sum over its segments and a bit walk per segment (~55 of a cell's 730 vector instructions)
                int run = 0;
                const int X0e = ini_x + 3 - ORBX_MIN_BORDER, Y0e = ini_y + 3 - ORBX_MIN_BORDER;
                for (int i0 = 0; i0 < ncorner; i0 += 64) {
                    const int i = i0 + lane;
                    bool is_max = false;
                    uint32_t recw = 0;
                    if (i < ncorner) {
                        const int e = list[i], py = e >> 6, px = e & 63;
                        const uint8_t *c = sc + (py + 1) * SP + px + 1;
                        const int s = c[0];
                        const int nb = max(max(max((int)c[-1], (int)c[1]), max((int)c[-SP - 1], (int)c[-SP])),
                                           max(max((int)c[-SP + 1], (int)c[SP - 1]), max((int)c[SP], (int)c[SP + 1])));
                        is_max = s > nb;                 // s > nb >= 0 implies a corner at th_cur
                        recw = (uint32_t)(X0e + px) | ((uint32_t)(Y0e + py) << 12) | ((uint32_t)s << 24);
                    }
                    const unsigned long long m = __ballot(is_max);
                    const int o = run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                    if (is_max && o < rec.cand_cap) (o < ORBX_CAND_PRIM ? prim : slot)[o] = recw;
                    run += __popcll(m);
                }
                emitted = run;
                direct = true;
            } else {
                mark_maxima(ncorner);
                __syncthreads();
            }
        } else {
            auto list_round = [&](int base) {   // the candidates of rank base .. base + CAP - 1
                if (wv != 0) return;
                unsigned lo = c_lo, hi = c_hi;
                int r = c_incl - c_cnt - base;
                while (lo) { if ((unsigned)r < (unsigned)list_cap) list[r] = (uint16_t)(rowbits | (unsigned)__builtin_ctz(lo)); r++; lo &= lo - 1; }
                while (hi) { if ((unsigned)r < (unsigned)list_cap) list[r] = (uint16_t)(rowbits | 32u | (unsigned)__builtin_ctz(hi)); r++; hi &= hi - 1; }
            };
            for (int base = 0; base < nlist; base += list_cap) {
                list_round(base);
                __syncthreads();
                score_entries(min(list_cap, nlist - base), false);
                __syncthreads();
            }
            STAMP(2);
            for (int base = 0; base < nlist; base += list_cap) {
                list_round(base);
                __syncthreads();
                mark_maxima(min(list_cap, nlist - base));
                __syncthreads();
            }
        }
        STAMP(3);
        if (direct) {   // (wave-uniform) the maxima of this pass are already in the cell's slots
            if (emitted != 0 || th_cur == min_th) break;
            th_cur = min_th;
            direct = false;
            continue;
        }
        {
            unsigned lo = 0, hi = 0;
            if (row_ok) { const uint2 m = *reinterpret_cast<const uint2 *>(sv + 2 * brow); lo = half_mode ? (m.x >> bsh) & 0xFFFFu : m.x; hi = half_mode ? 0u : m.y; }
            nsurv = __popc(lo) + __popc(hi);
        }
        // the cell falls back to minThFAST only if iniThFAST kept nothing (:991-995); pretest, scores and bitmaps of the
        // second pass are supersets of the first, so nothing has to be cleared
        if (__builtin_amdgcn_readfirstlane(__any(nsurv != 0)) || th_cur == min_th) break;
        th_cur = min_th;
    }
    if (direct) {
        if (lane == 0) *my_cnt = min(emitted, rec.cand_cap);
    } else
    // ---- ordered (row-major) emission into the cell's candidate slots: lane = bitmap segment (row, or half a row)
    if (wv == 0) {
        unsigned lo = 0, hi = 0;
        if (row_ok) { const uint2 m = *reinterpret_cast<const uint2 *>(sv + 2 * brow); lo = half_mode ? (m.x >> bsh) & 0xFFFFu : m.x; hi = half_mode ? 0u : m.y; }
        const int incl = wave_incl_scan(nsurv);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        int o = incl - nsurv;
        const int Y = ini_y + 3 + brow - ORBX_MIN_BORDER, X0 = ini_x + 3 - ORBX_MIN_BORDER + (int)bsh;
        const uint8_t *srow = sc + (brow + 1) * SP + 1 + bsh;
        while (lo) {
            const int px = __builtin_ctz(lo);
            lo &= lo - 1;
            if (o < rec.cand_cap) (o < ORBX_CAND_PRIM ? prim : slot)[o] = (uint32_t)(X0 + px) | ((uint32_t)Y << 12) | ((uint32_t)srow[px] << 24);
            o++;
        }
        while (hi) {
            const int px = 32 + __builtin_ctz(hi);
            hi &= hi - 1;
            if (o < rec.cand_cap) (o < ORBX_CAND_PRIM ? prim : slot)[o] = (uint32_t)(X0 + px) | ((uint32_t)Y << 12) | ((uint32_t)srow[px] << 24);
            o++;
        }
        if (lane == 0) *my_cnt = min(total, rec.cand_cap);
    }
    STAMP(4);
    SPAN_END(0);
#ifdef ORBX_DIAG
    if (lane == 0) atomicAdd(&g_fast_stamp[((blockIdx.x * 131 + blockIdx.y) & 4095) * 8 + 7], 1ull);
#endif
}

// ---------------------------------------------------------------- K2p: FAST on PAIRS of horizontally adjacent cells (batches)
// One wave takes two cells of a cell row, A and its right neighbour B (the last cell of a row with an odd number of columns goes
// alone).  What one cell per wave pays per cell -- record fetch and decode, tile load and zeroing, the pretest prologue, a prefix sum
// and a bit walk for the list, one for the emission -- is paid once per pair, the score / maximum iterations (64 candidates each)
// run on ONE concatenated candidate list (a 31 x 32 cell lists ~127 pretest candidates: two or three iterations, the last two-thirds
// empty; a pair lists ~254: four or five), and the 3-px halo between A and B is fetched once (72 bytes per tile row for 62 owned
// pixels instead of 2 x 40 for 2 x 31).
// Bit space: everything after the tile load is indexed by (row, bit), bit = tile column - 4.  The tile fetch starts xo = 1 + off bytes
// left of cell A with off = 32 - dwA, so A's detectable pixels are bits [off, 32) and B's are bits [32, 32 + dwB): the A | B boundary
// is a 32-bit word boundary of every bitmap row and a dword boundary of every pretest group, and "which cell" is bit 5 of a bit index.
// (A cell that goes alone sits at bits [0, dwA).)  Per-cell semantics of src/ORBextractor.cc:953-1009 are kept exactly:
//  * non-maximum suppression is per cell (cv::FAST sees one cell at a time: scores outside it count as 0): the score tile has a
//    zero column between the two cells (score column = bit + 1 + (bit >> 5)), so a maximum never looks into the other cell;
//  * the minThFAST fallback is per cell: a second pass lists only the segments of the cell(s) that kept nothing;
//  * each cell's survivors go to its own candidate slots in its own row-major order: the emission scans a packed (A | B << 16) count.
// Bitmap segments: 32-bit halves of a row (lane = row, half; the half is the cell) when the detect area has at most 32 rows, else
// whole 64-bit rows (lane = row; low word = A, high word = B).
#ifndef FAST2_P
#define FAST2_P 72      // tile pitch: 1 + 32 - dwA + 3 + dwA + dwB + 3 <= 71 bytes
#endif
#ifndef FAST2_LIST_CAP
#define FAST2_LIST_CAP 1024 // candidates listed per round: a pair lists ~350 on a textured frame, and the rounds of a fuller list walk it twice without compaction
#endif
#ifndef FAST2_SP
#define FAST2_SP 68     // score pitch: rim + 32 + gap + 32 + rim = 67 bytes; 17 dwords: rows r and r + 32 share banks
#endif
struct PairRec {
    short level, ncells;         // ncells: cells whose count this wave writes (1 or 2); dwa == 0: all of them skipped
    short ini_x, ini_y;          // cell A's rectangle origin (incl. the 3-px halo), level coordinates
    short dwa, dwb;              // detect widths of A and B (0: skipped / absent; dwb != 0 implies dwa == the level's cell width)
    int cell;                    // index of cell A in the image's cell arrays (B = cell + 1)
    int pitch, cand_cap;
    unsigned gpr_magic;          // multiply-high division by gpr = pretest groups per row = (bits used + 3) >> 2
    int th;                      // tile rows (detect rows + 6)
    long long pyr_off, cand_slot;
};
static_assert(sizeof(PairRec) == 48, "PairRec layout");

template <int P, int SP>
__global__ __launch_bounds__(64) void k_fast2(const FastArgs fa, const PairRec *__restrict__ pairs, int total_pairs, PyrRef pr,
                                              int *__restrict__ cell_cnt, uint32_t *__restrict__ cand, uint32_t *__restrict__ cand_prim)
{
    constexpr int DWR = P / 4;      // dwords per tile row
    constexpr int RPL = 64 / DWR;   // whole tile rows per direct load
#ifdef ORBX_FAST_PAD
    asm volatile(".fill %0, 4, 0xBF800000" :: "n"(ORBX_FAST_PAD));
#endif
    uint8_t *tile = fast_smem;
    uint8_t *sc = fast_smem + fa.lds_sc;
    uint16_t *list = reinterpret_cast<uint16_t *>(fast_smem + fa.lds_list);
    uint32_t *bm = reinterpret_cast<uint32_t *>(fast_smem + fa.lds_bm); // candidate bitmap, then survivor bitmap: u64 per row
    uint32_t *sv = bm + 2 * fa.bm_rows;
    const int ini_th = fa.ini_th, min_th = fa.min_th;
    const int b = blockIdx.y, lane = threadIdx.x;
    int pi;
    {   // FAST_XG neighbouring pairs of a cell row on the same XCD (see k_fast)
        const int bx = blockIdx.x, grp = bx / (8 * FAST_XG), r = bx - grp * (8 * FAST_XG);
        pi = grp * (8 * FAST_XG) + (r & 7) * FAST_XG + (r >> 3);
        if (pi >= total_pairs) return;
    }
#ifdef ORBX_DIAG
    unsigned long long _t_prev = __builtin_amdgcn_s_memtime();
#endif
    SPAN_BEGIN();
    int level, ncells, ini_x, ini_y, dwa, dwb, cell0, rpitch, cand_cap, th;
    unsigned gpr_magic;
    long long pyr_off, cand_slot;
    {
        const uint32_t *cw = reinterpret_cast<const uint32_t *>(pairs + pi);
        uint32_t w[12];
#pragma unroll
        for (int i = 0; i < 12; i++) w[i] = cw[i];
        level = (short)(w[0] & 0xFFFF); ncells = (short)(w[0] >> 16);
        ini_x = (short)(w[1] & 0xFFFF); ini_y = (short)(w[1] >> 16);
        dwa = (short)(w[2] & 0xFFFF); dwb = (short)(w[2] >> 16);
        cell0 = (int)w[3]; rpitch = (int)w[4]; cand_cap = (int)w[5]; gpr_magic = w[6]; th = (int)w[7];
        pyr_off = (long long)(((unsigned long long)w[9] << 32) | w[8]);
        cand_slot = (long long)(((unsigned long long)w[11] << 32) | w[10]);
    }
    int *my_cnt = cell_cnt + (long long)b * fa.total_cells + cell0;
    if (dwa == 0) { // src/ORBextractor.cc:961-976 skip rules, evaluated on the host (a skipped A has no B to its right that is not skipped)
        if (lane < ncells) my_cnt[lane] = 0;
        return;
    }
    const int off = dwb ? 32 - dwa : 0, xo = 1 + off;   // bit of A's first detectable pixel; bytes fetched left of cell A
    const int nbits = off + dwa + dwb;                  // bits [off, nbits) are detectable pixels
    const int tw = dwa + dwb + 6, dh = th - 6;
    const int pitch = level == 0 ? pr.img0_pitch : rpitch;
    const uint8_t *img = level == 0 ? pr.img0 + (long long)b * pr.img0_stride : pr.pyr + (long long)b * pr.pyr_stride + pyr_off;
    // ---- 1. tile (cell A, cell B and the halo around both) -> LDS by direct loads, RPL whole rows per instruction
    {
        const int lr0 = lane / DWR, lc = lane - lr0 * DWR;
        const int ndw = (tw + xo + 3) >> 2;             // dwords per row that hold tile pixels (<= 18)
        const uint8_t *base = img + (long long)ini_y * pitch + (ini_x - xo);
        const unsigned voff = (unsigned)(lr0 * pitch + 4 * lc);
        const int full = th / RPL;
        if (lc < ndw && lr0 < RPL) {
            for (int k = 0; k < full; k++, base += (long long)RPL * pitch)
                lds_load_sbase<4>(base, voff, tile + RPL * P * k);
            if (full * RPL + lr0 < th)      // the last, partial group of rows never reads below the cells
                lds_load_sbase<4>(base, voff, tile + RPL * P * full);
        }
    }
    {   // meanwhile: zero score tile (rim and the column between the cells included) and both bitmaps
        uint4 *z = reinterpret_cast<uint4 *>(sc);
        for (int i = lane; i < ((dh + 2) * SP + 15) / 16; i += 64) z[i] = make_uint4(0, 0, 0, 0);
        uint4 *zb = reinterpret_cast<uint4 *>(bm);
        for (int i = lane; i < fa.bm_rows; i += 64) zb[i] = make_uint4(0, 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    STAMP(0);
    const uint8_t *t0 = tile + 3 * P + 4;               // detect row 0, bit 0
    // pretest geometry: tile dwords 1 .. gpr of a row hold bits 0 .. 4 gpr - 1; one iteration = rpi whole rows
    const int gpr = (nbits + 3) >> 2;
    const int lq = gpr == 1 ? lane : (int)__umulhi((unsigned)lane, gpr_magic);
    const int rpi = min(gpr == 1 ? 64 : (int)__umulhi(64u, gpr_magic), 8);
    const int lr = min(lq, rpi), gq = lane - lq * gpr;
    unsigned vmask = 0;
    {   // bytes of this lane's group whose bit is a detectable pixel: bits [max(off, 4 gq), min(nbits, 4 gq + 4))
        const int lo = min(max(off - 4 * gq, 0), 4), hi = min(max(nbits - 4 * gq, 0), 4);
        if (lr < rpi && hi > lo) vmask = (0x80808080u >> (8 * (4 - hi))) & (0x80808080u << (8 * lo));
    }
    const int bm_sh = 4 * (gq & 7);
    uint32_t *slot = cand + (long long)b * fa.cand_total + cand_slot;
    uint32_t *prim = cand_prim + ((long long)b * fa.total_cells + cell0) * ORBX_CAND_PRIM;
    const bool half_mode = dh <= 32;
    const int brow = half_mode ? lane >> 1 : lane;
    const int half = half_mode ? lane & 1 : 0;
    const unsigned bsh = 32u * (unsigned)half;
    int th_cur = ini_th;
    unsigned s_lo = 0, s_hi = 0;                        // this lane's survivor bits
    bool need_a = true, need_b = dwb != 0;              // cells listed by the current pass
    for (int pass = 0; pass < 2; pass++) {
        // ---- 2. SWAR pretest (see k_fast): both cells, 4 adjacent bits per lane
        {
            const unsigned s7 = (unsigned)((th_cur + 1) >> 1) * 0x01010101u;
            const uint8_t *pc = tile + (lr + 3) * P + 4 * (1 + gq);
            uint32_t *pb = bm + lr * 2 + (gq >> 3);
            for (int r0 = 0; r0 < dh; r0 += rpi, pc += rpi * P, pb += rpi * 2) {
                const uint32_t *rc = reinterpret_cast<const uint32_t *>(pc);
                const unsigned C = rc[0], Wd = rc[-1], Ed = rc[1], N = rc[3 * DWR], S = rc[-3 * DWR];
                const unsigned Wv = __builtin_amdgcn_alignbyte(C, Wd, 1), Ev = __builtin_amdgcn_alignbyte(Ed, C, 3);
                const unsigned c7 = (C >> 1) & 0x7f7f7f7fu, n7 = (N >> 1) & 0x7f7f7f7fu, u7 = (S >> 1) & 0x7f7f7f7fu,
                               e7 = (Ev >> 1) & 0x7f7f7f7fu, w7 = (Wv >> 1) & 0x7f7f7f7fu;
                const unsigned R = (c7 | 0x80808080u) - s7, RD = R | 0x80808080u;
                const unsigned RB = ((c7 ^ 0x7f7f7f7fu) | 0x80808080u) - s7, KB = (RB | 0x80808080u) - 0x7f7f7f7fu;
                const unsigned dark = ((RD - n7) | (RD - u7)) & ((RD - e7) | (RD - w7)) & R;
                const unsigned bright = ((KB + n7) | (KB + u7)) & ((KB + e7) | (KB + w7)) & RB;
                const unsigned any = (dark | bright) & vmask;
                const unsigned nib = (((any >> 7) * 0x01020408u) >> 24) << bm_sh;
                if (nib) atomicOr(pb, nib);   // rows >= dh of the last iteration land in bitmap rows that are never read
            }
        }
        __syncthreads();
        STAMP(1);
        // ---- 3. bitmap -> ordered list of (row << 6 | bit): lane = segment; only the cells this pass is for
        unsigned c_lo = 0, c_hi = 0;
        if (brow < dh) {
            const uint2 m = *reinterpret_cast<const uint2 *>(bm + 2 * brow);
            if (half_mode) c_lo = half ? (need_b ? m.y : 0u) : (need_a ? m.x : 0u);
            else { c_lo = need_a ? m.x : 0u; c_hi = need_b ? m.y : 0u; }
        }
        const int c_cnt = __popc(c_lo) + __popc(c_hi);
        const int c_incl = wave_incl_scan(c_cnt);
        const int nlist = __builtin_amdgcn_readlane(c_incl, 63);
        const unsigned rowbits = ((unsigned)brow << 6) | bsh;
        // ---- 4. full score of the listed pixels; corners packed to the front of the list in place (order kept)
        auto score_entries = [&](int n, bool compact) -> int {
            int n2 = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                int e = 0, s = 0;
                if (i < n) {
                    e = list[i];
                    const int py = e >> 6, bx = e & 63;
                    s = fast_score_full<P>(t0 + py * P + bx, th_cur);
                    sc[(py + 1) * SP + bx + 1 + (bx >> 5)] = (uint8_t)s;
                }
                if (compact) {
                    const unsigned long long m = __ballot(s > 0);
                    if (s > 0) list[n2 + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = (uint16_t)e;
                    n2 += __popcll(m);
                }
            }
            return compact ? n2 : n;
        };
        // ---- 5. strict 3x3 maximum inside the pixel's own cell -> survivor bitmap
        auto mark_maxima = [&](int n) {
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                if (i < n) {
                    const int e = list[i], py = e >> 6, bx = e & 63;
                    const uint8_t *c = sc + (py + 1) * SP + bx + 1 + (bx >> 5);
                    const int s = c[0];
                    const int nb = max(max(max((int)c[-1], (int)c[1]), max((int)c[-SP - 1], (int)c[-SP])),
                                       max(max((int)c[-SP + 1], (int)c[SP - 1]), max((int)c[SP], (int)c[SP + 1])));
                    if (s > nb) atomicOr(sv + 2 * py + (bx >> 5), 1u << (bx & 31));
                }
            }
        };
        constexpr int list_cap = FAST2_LIST_CAP;
        if (nlist <= list_cap) {
            unsigned lo = c_lo, hi = c_hi;
            uint16_t *lp = list + (c_incl - c_cnt);
            while (lo) { *lp++ = (uint16_t)(rowbits | (unsigned)__builtin_ctz(lo)); lo &= lo - 1; }
            while (hi) { *lp++ = (uint16_t)(rowbits | 32u | (unsigned)__builtin_ctz(hi)); hi &= hi - 1; }
            __syncthreads();
            STAMP(5);
            const int ncorner = score_entries(nlist, true);
            STAMP(6);
            __syncthreads();
            STAMP(2);
            mark_maxima(ncorner);
            __syncthreads();
        } else {
            auto list_round = [&](int base) {   // the candidates of rank base .. base + CAP - 1
                unsigned lo = c_lo, hi = c_hi;
                int r = c_incl - c_cnt - base;
                while (lo) { if ((unsigned)r < (unsigned)list_cap) list[r] = (uint16_t)(rowbits | (unsigned)__builtin_ctz(lo)); r++; lo &= lo - 1; }
                while (hi) { if ((unsigned)r < (unsigned)list_cap) list[r] = (uint16_t)(rowbits | 32u | (unsigned)__builtin_ctz(hi)); r++; hi &= hi - 1; }
            };
            for (int base = 0; base < nlist; base += list_cap) {
                list_round(base);
                __syncthreads();
                score_entries(min(list_cap, nlist - base), false);
                __syncthreads();
            }
            STAMP(2);
            for (int base = 0; base < nlist; base += list_cap) {
                list_round(base);
                __syncthreads();
                mark_maxima(min(list_cap, nlist - base));
                __syncthreads();
            }
        }
        STAMP(3);
        s_lo = 0; s_hi = 0;
        if (brow < dh) { const uint2 m = *reinterpret_cast<const uint2 *>(sv + 2 * brow); s_lo = half_mode ? (half ? m.y : m.x) : m.x; s_hi = half_mode ? 0u : m.y; }
        // a cell falls back to minThFAST only if iniThFAST kept nothing IN THAT CELL (:991-995); the second pass lists only such cells.
        // Pretest bits, scores and survivors of the second pass are supersets of the first: nothing has to be cleared
        if (th_cur == min_th) break;
        const bool any_a = __any(half_mode ? (half == 0 && s_lo != 0) : s_lo != 0);
        const bool any_b = __any(half_mode ? (half == 1 && s_lo != 0) : s_hi != 0);
        need_a = !any_a; need_b = dwb != 0 && !any_b;
        if (!(need_a || need_b)) break;
        th_cur = min_th;
    }
    // ---- ordered (row-major per cell) emission into each cell's candidate slots: lane = bitmap segment
    {
        const int n_lo = __popc(s_lo), n_hi = __popc(s_hi);
        const int v = half_mode ? n_lo << (16 * half) : n_lo | (n_hi << 16);
        const int incl = wave_incl_scan(v);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        const int excl = incl - v;
        const int Y = ini_y + 3 + brow - ORBX_MIN_BORDER, X0 = ini_x + 3 - ORBX_MIN_BORDER - off;     // x of bit 0
        const uint8_t *srow = sc + (brow + 1) * SP + 1;
        {   // low word: cell A (whole-row segments) or this lane's cell (half-row segments)
            int o = half_mode ? (excl >> (16 * half)) & 0xFFFF : excl & 0xFFFF;
            uint32_t *pm = prim + (half ? ORBX_CAND_PRIM : 0), *sl = slot + (half ? cand_cap : 0);
            unsigned lo = s_lo;
            while (lo) {
                const int bx = (int)bsh + __builtin_ctz(lo);
                lo &= lo - 1;
                if (o < cand_cap) (o < ORBX_CAND_PRIM ? pm : sl)[o] = (uint32_t)(X0 + bx) | ((uint32_t)Y << 12) | ((uint32_t)srow[bx + (bx >> 5)] << 24);
                o++;
            }
        }
        if (!half_mode) {   // high word: cell B
            int o = excl >> 16;
            uint32_t *pm = prim + ORBX_CAND_PRIM, *sl = slot + cand_cap;
            unsigned hi = s_hi;
            while (hi) {
                const int bx = 32 + __builtin_ctz(hi);
                hi &= hi - 1;
                if (o < cand_cap) (o < ORBX_CAND_PRIM ? pm : sl)[o] = (uint32_t)(X0 + bx) | ((uint32_t)Y << 12) | ((uint32_t)srow[bx + 1] << 24);
                o++;
            }
        }
        if (lane == 0) my_cnt[0] = min(total & 0xFFFF, cand_cap);
        if (lane == 1 && ncells == 2) my_cnt[1] = min(total >> 16, cand_cap);
    }
    STAMP(4);
    SPAN_END(0);
#ifdef ORBX_DIAG
    if (lane == 0) atomicAdd(&g_fast_stamp[((blockIdx.x * 131 + blockIdx.y) & 4095) * 8 + 7], 1ull);
#endif
}

#ifdef ORBX_DIAG
#ifdef ORBX_DIAG_SPANS_ONLY
extern "C" int orbx_diag_fast_phases(unsigned *out /*[16384][8]*/)
{
    ORBX_HIP(hipDeviceSynchronize());
    ORBX_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fast_phase), sizeof(unsigned) * 16384 * 8));
    return ORBX_OK;
}
#endif

extern "C" int orbx_diag_fast_stamps(unsigned long long *out, int reset) { return orbx_diag_stamp_sums(HIP_SYMBOL(g_fast_stamp), out, reset); }
int orbx_fast_diag_spans(unsigned *out, int reset) { return orbx_diag_span_read(HIP_SYMBOL(g_span_0), out, reset); }
#endif

// ================================================================ host side

// The FAST step of orbx_prepare_geometry: the LDS carves of both kernels (Geom::fast_* / fast2_*), the cell records and -- where the
// geometry allows the pair form -- the pair records as bytes (PairRec is this file's), empty otherwise.
void orbx_fast_plan(const orbx_extractor *e, Geom &G, std::vector<CellRec> &cells_out, std::vector<uint8_t> &pair_bytes)
{
    {   // LDS carve of k_fast, sized by the largest cell over the levels
        int max_th = 0, max_dh = 0, max_npx = 0;
        for (int l = 0; l < e->nlevels; l++) {
            const LevelGeom &L = G.lv[l];
            if (L.h_cell + 6 > max_th) max_th = L.h_cell + 6;
            if (L.h_cell > max_dh) max_dh = L.h_cell;
            if (L.w_cell * L.h_cell > max_npx) max_npx = L.w_cell * L.h_cell;
        }
        int max_w_cell = 0;
        for (int l = 0; l < e->nlevels; l++) if (G.lv[l].w_cell > max_w_cell) max_w_cell = G.lv[l].w_cell;
        // tile row = 1 + w_cell + 6 pixels rounded up to dwords <= 48 bytes; score row = w_cell + 2 <= 40
        G.fast_small = (((max_w_cell + 7 + 3) & ~3) <= 48 && max_w_cell + 2 <= 40) ? 1 : 0;
        const int tp = G.fast_small ? 48 : ORBX_TILE_PITCH, sp = G.fast_small ? 40 : ORBX_SCORE_PITCH;
        // tile rows: the cell, the whole rows of the last direct load, and the row overrun of the last pretest iteration
        // (up to 7 rows of at least 8 groups) plus its S neighbour three rows further down
        // (row dh - 1 + 8 of the pretest reads its S neighbour at tile row th + 7)
        // The overrun rows are only ever READ (their flags land in bitmap rows nobody looks at), so they need no storage of their
        // own: they alias whatever follows the tile (score tile and list, always more than 8 rows' worth).
        G.fast_lds_sc = (int)align_up((size_t)max_th * tp + 8, 16);
        G.fast_lds_list = G.fast_lds_sc + (int)align_up((size_t)(max_dh + 2) * sp, 16);
        G.fast_lds_bm = G.fast_lds_list + (int)align_up((size_t)std::min(max_npx, ORBX_FAST_LIST_CAP) * 2 + 16, 16);
        G.fast_bm_rows = (max_dh + 9 + 1) & ~1;          // even: the two bitmaps are zeroed as one run of 16-byte stores
        G.fast_lds_bytes = G.fast_lds_bm + 2 * G.fast_bm_rows * 8;
        // several waves per cell (small launches: LDS is no limit there): the list holds every pixel of the largest cell -- one round always
        G.fast_list_cap_big = std::max(max_npx, ORBX_FAST_LIST_CAP);
        G.fast_lds_bm_big = G.fast_lds_list + (int)align_up((size_t)G.fast_list_cap_big * 2 + 16, 16);
        G.fast_lds_bytes_big = G.fast_lds_bm_big + 2 * G.fast_bm_rows * 8;
    }
    std::vector<CellRec> cells(G.total_cells);
    for (int l = 0; l < e->nlevels; l++) {
        const LevelGeom &L = G.lv[l];
        const int max_bx = L.w - ORBX_MIN_BORDER, max_by = L.h - ORBX_MIN_BORDER;
        for (int ci = 0; ci < L.n_cells; ci++) {
            CellRec &c = cells[L.cell_base + ci];
            const int row = ci / L.n_cols, col = ci % L.n_cols;
            const int ini_y = ORBX_MIN_BORDER + row * L.h_cell, ini_x = ORBX_MIN_BORDER + col * L.w_cell; // :957-971
            const int max_y = ini_y + L.h_cell + 6 < max_by ? ini_y + L.h_cell + 6 : max_by;
            const int max_x = ini_x + L.w_cell + 6 < max_bx ? ini_x + L.w_cell + 6 : max_bx;
            c.level = (short)l;
            c.ini_x = (short)ini_x; c.ini_y = (short)ini_y; c.tw = (short)(max_x - ini_x); c.th = (short)(max_y - ini_y);
            // src/ORBextractor.cc:961-976 skip rules (note the asymmetric 3 / 6)
            c.skip = (ini_y >= max_by - 3 || ini_x >= max_bx - 6 || c.tw - 6 <= 0 || c.th - 6 <= 0) ? 1 : 0;
            c.pitch = L.pitch; c.cand_cap = L.cand_cap; c.pyr_off = L.pyr_off;
            { const int gpr = (c.tw - 6 + 3) >> 2; c.gpr_magic = gpr > 0 ? 0xFFFFFFFFu / (unsigned)gpr + 1u : 0u; }
            c.cand_slot = L.cand_off + (long long)ci * L.cand_cap;
        }
    }
    // k_fast2: pairs of horizontally adjacent cells (batches).  Usable when every cell's detect area fits 32 bits x 64 rows.
    std::vector<PairRec> pairs;
    {
        bool ok = true;
        for (int l = 0; l < e->nlevels; l++) if (G.lv[l].w_cell > 32 || G.lv[l].h_cell > 56) ok = false;
        G.fast2_ok = ok ? 1 : 0;
        G.total_pairs = 0;
        if (ok) {
            // two groups of levels, each a launch with its own LDS carve: detect areas of at most 32 rows (the 30-px grid's usual cells), then the
            // taller ones (a level whose cell rows do not divide evenly: up to 40 rows at 1241x376) -- sized together, the tall tiles cost every
            // wave of the launch a sixth of its occupancy
            for (int grp = 0; grp < 2; grp++) {
                int max_th = 0, max_dh = 0;
                G.fast2_first[grp] = (int)pairs.size();
                for (int l = 0; l < e->nlevels; l++) {
                    const LevelGeom &L = G.lv[l];
                    if ((L.h_cell <= 32 ? 0 : 1) != grp) continue;
                    max_th = std::max(max_th, L.h_cell + 6); max_dh = std::max(max_dh, L.h_cell);
                    for (int row = 0; row < L.n_rows; row++)
                        for (int col = 0; col < L.n_cols; col += 2) {
                            const CellRec &a = cells[L.cell_base + row * L.n_cols + col];
                            const bool has_b = col + 1 < L.n_cols;
                            PairRec q;
                            memset(&q, 0, sizeof q);
                            q.level = (short)l; q.ncells = has_b ? 2 : 1;
                            q.ini_x = a.ini_x; q.ini_y = a.ini_y; q.th = a.th;
                            q.dwa = a.skip ? 0 : (short)(a.tw - 6);
                            q.dwb = 0;
                            if (has_b && !a.skip) {
                                const CellRec &bc = cells[L.cell_base + row * L.n_cols + col + 1];
                                if (!bc.skip) {
                                    q.dwb = (short)(bc.tw - 6);
                                    // B starts one cell width right of A, on the same rows: the pair's tile is one rectangle
                                    if (bc.ini_x != a.ini_x + L.w_cell || bc.ini_y != a.ini_y || bc.th != a.th || a.tw != L.w_cell + 6) ok = false;
                                }
                            }
                            if (q.dwa > 32 || q.dwb > 32 || q.dwa < 0 || q.dwb < 0 || (q.dwb && q.dwa != L.w_cell)) ok = false;
                            const int off = q.dwb ? 32 - q.dwa : 0;
                            if (a.ini_x - (1 + off) < 0) ok = false;                   // the fetch starts 1 + off bytes left of cell A
                            const int nbits = off + q.dwa + q.dwb, gpr = (nbits + 3) >> 2;
                            q.gpr_magic = gpr > 0 ? 0xFFFFFFFFu / (unsigned)gpr + 1u : 0u;
                            q.cell = L.cell_base + row * L.n_cols + col;
                            q.pitch = L.pitch; q.cand_cap = L.cand_cap; q.pyr_off = L.pyr_off; q.cand_slot = a.cand_slot;
                            pairs.push_back(q);
                        }
                }
                G.fast2_count[grp] = (int)pairs.size() - G.fast2_first[grp];
                // LDS carve (pitches FAST2_P / FAST2_SP): tile | score tile | candidate list | candidate + survivor bitmaps; the pretest's
                // overrun rows alias what follows the tile (see k_fast)
                G.fast2_lds_sc[grp] = (int)align_up((size_t)max_th * FAST2_P + 8, 16);
                G.fast2_lds_list[grp] = G.fast2_lds_sc[grp] + (int)align_up((size_t)(max_dh + 2) * FAST2_SP, 16);
                G.fast2_lds_bm[grp] = G.fast2_lds_list[grp] + (int)align_up((size_t)FAST2_LIST_CAP * 2 + 16, 16);
                G.fast2_bm_rows[grp] = (max_dh + 9 + 1) & ~1;
                G.fast2_lds_bytes[grp] = G.fast2_lds_bm[grp] + 2 * G.fast2_bm_rows[grp] * 8;
            }
            if (!ok) { G.fast2_ok = 0; pairs.clear(); }
            G.total_pairs = (int)pairs.size();
        }
    }
    // Shape classes and the lane table of k_fast (fast_lane_entry): one class per distinct detect shape (dw, dh), its id above the level number
    // in CellRec::level; the table follows the records in the same upload, 16-byte aligned (G.fast_lane_tab_off bytes behind the first record)
    {
        const int P = G.fast_small ? 48 : ORBX_TILE_PITCH;
        std::vector<std::pair<int, int>> shapes;
        for (int l = 0; l < e->nlevels; l++)
            for (int ci = 0; ci < G.lv[l].n_cells; ci++) {
                CellRec &c = cells[G.lv[l].cell_base + ci];
                if (c.skip) continue;               // (a skipped cell keeps class 0 and never reads the table)
                const std::pair<int, int> sh(c.tw - 6, c.th - 6);
                size_t k = std::find(shapes.begin(), shapes.end(), sh) - shapes.begin();
                if (k == shapes.size()) shapes.push_back(sh);
                c.level = (short)(l | ((int)k << 4));   // (k < FAST_MAX_CLASSES: dw <= 59 and dh <= 64 per level, ORBX_MAX_LEVELS levels, in practice four shapes per level)
            }
        const size_t tab_off = align_up((size_t)G.total_cells * sizeof(CellRec), 16), tab_bytes = shapes.size() * 64 * 16;
        G.fast_lane_tab_off = (int)tab_off;
        cells.resize((tab_off + tab_bytes + sizeof(CellRec) - 1) / sizeof(CellRec));   // whole records: the upload copies cells.size() of them
        uint32_t *tab = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(cells.data()) + tab_off);
        int uni[2];
        for (size_t k = 0; k < shapes.size(); k++)
            for (int lane = 0; lane < 64; lane++) fast_lane_entry(P, shapes[k].first, shapes[k].second, lane, tab + (k * 64 + lane) * 4, uni);
    }
    std::vector<uint8_t> pb(pairs.size() * sizeof(PairRec));
    if (!pairs.empty()) memcpy(pb.data(), pairs.data(), pb.size());
    cells_out.swap(cells); pair_bytes.swap(pb);
}

// debug: the cell records of the handle's current geometry as the plan builds them, eight ints per cell: level, skip, ini_x, ini_y, tw, th,
// level pitch, shape class.  Returns the number of cells (also when cap is smaller: nothing is written then), 0 before the first extraction.
extern "C" int orbx_debug_fast_cells(const orbx_extractor *e, int32_t *out, int cap)
{
    if (!e || cap < 0 || (cap > 0 && !out)) { orbx_set_error("orbx_debug_fast_cells: invalid argument"); return ORBX_E_INVALID; }
    if (e->geom.w == 0) return 0;
    Geom G = e->geom;
    std::vector<CellRec> cells;
    std::vector<uint8_t> pairs;
    orbx_fast_plan(e, G, cells, pairs);
    if (cap < G.total_cells) return G.total_cells;
    for (int i = 0; i < G.total_cells; i++) {
        const CellRec &c = cells[i];
        const int32_t v[8] = { c.level & 0xF, c.skip, c.ini_x, c.ini_y, c.tw, c.th, c.pitch, (c.level >> 4) & 0x7FF };
        memcpy(out + 8 * i, v, sizeof v);
    }
    return G.total_cells;
}

void orbx_fast_launch(orbx_extractor *e, const PyrRef &pr, int batch, hipStream_t s)
{
    const Geom &G = e->geom;
    int32_t *forms = e->last_forms;     // orbx_debug_launch_forms
    e->last_fast_form = 1;
    forms[1] = 1; forms[2] = 0;         // waves per cell; grid order 0 = (cell, image), 1 = image-major (k_fast<48, 40, 1, true>)
    {
        FastArgs fa;
        fa.total_cells = G.total_cells; fa.lds_sc = G.fast_lds_sc; fa.lds_list = G.fast_lds_list; fa.lds_bm = G.fast_lds_bm;
        fa.bm_rows = G.fast_bm_rows; fa.ini_th = e->ini_th; fa.min_th = e->min_th; fa.cand_total = G.cand_total; fa.list_cap = ORBX_FAST_LIST_CAP;
        fa.lane_tab_off = G.fast_lane_tab_off;
        const dim3 grid((G.total_cells + 8 * FAST_XG - 1) / (8 * FAST_XG) * (8 * FAST_XG), batch);
        if (G.fast_small)
        {
            // a frame or two: several waves per cell (the launch lasts as long as its fullest cell); batches: one
            const long long waves1 = (long long)G.total_cells * batch;
            const int nw = e->fast_waves ? e->fast_waves : waves1 * 4 <= 16384 ? 4 : waves1 * 2 <= 16384 ? 2 : 1;    // (tools/sweep_small.sh: one frame 4, two frames 2, more 1)
            int lds_bytes = G.fast_lds_bytes;
            if (nw > 1) { fa.list_cap = G.fast_list_cap_big; fa.lds_bm = G.fast_lds_bm_big; lds_bytes = G.fast_lds_bytes_big; }
            forms[1] = nw; forms[2] = nw == 1 && grid.x <= 65535;
            // one wave per PAIR of horizontally adjacent cells (k_fast2): opt-in experiment form (ORBX_FAST_PAIR=1)
            if (G.fast2_ok && e->fast_pair == 1) {
                e->last_fast_form = 2;
                forms[1] = 0; forms[2] = 0;
                fa.list_cap = FAST2_LIST_CAP;
                for (int grp = 0; grp < 2; grp++) {
                    if (!G.fast2_count[grp]) continue;
                    fa.lds_sc = G.fast2_lds_sc[grp]; fa.lds_list = G.fast2_lds_list[grp]; fa.lds_bm = G.fast2_lds_bm[grp]; fa.bm_rows = G.fast2_bm_rows[grp];
                    const dim3 grid2((G.fast2_count[grp] + 8 * FAST_XG - 1) / (8 * FAST_XG) * (8 * FAST_XG), batch);
                    hipLaunchKernelGGL((k_fast2<FAST2_P, FAST2_SP>), grid2, dim3(64), G.fast2_lds_bytes[grp], s, fa, (const PairRec *)e->d_pairs + G.fast2_first[grp],
                                       G.fast2_count[grp], pr, e->d_cell_cnt, e->d_cand, e->d_cand_prim);
                }
            } else
#define LAUNCH_FAST(NW_) hipLaunchKernelGGL((k_fast<48, 40, NW_>), grid, dim3(64 * NW_), lds_bytes, s, fa, e->d_cells, pr, e->d_cell_cnt, e->d_cand, e->d_cand_prim)
            if (nw == 4) LAUNCH_FAST(4); else if (nw == 3) LAUNCH_FAST(3); else if (nw == 2) LAUNCH_FAST(2);
            else if (grid.x <= 65535) hipLaunchKernelGGL((k_fast<48, 40, 1, true>), dim3(batch, grid.x), dim3(64), lds_bytes, s, fa, e->d_cells, pr, e->d_cell_cnt, e->d_cand, e->d_cand_prim);
            else LAUNCH_FAST(1);
#undef LAUNCH_FAST
        }
        else
            hipLaunchKernelGGL((k_fast<ORBX_TILE_PITCH, ORBX_SCORE_PITCH, 1>), grid, dim3(64), G.fast_lds_bytes, s, fa, e->d_cells, pr, e->d_cell_cnt,
                               e->d_cand, e->d_cand_prim);     // (cells wider than 38 px: scale factors far from 1.2; kept on the (cell, image) grid)
    }
}

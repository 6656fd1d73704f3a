// orbx_desc.hip — the extractor's descriptor stage (IC_Angle, the 7x7 GaussianBlur and computeOrbDescriptor, reference
// src/ORBextractor.cc:83-157, :1311-1334): k_desc with the stereo row table it builds on the side, its constant tables and Gaussian taps,
// and the launch (orbx_desc_launch).  File map of the extractor: orbx_extract.hip.
#include "orbx_device.h"
#include "orb_pattern.inc"

#include <limits.h>
#include <stddef.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

// k_desc's constant tables as ONE symbol: the wave forms one base address (one s_getpc_b64) and reaches every table as base + lane offset +
// immediate; a symbol per table cost an s_getpc_b64 / s_add_u32 / s_addc_u32 triple per table and load
struct DescTab {
    uint32_t pat4[256];         // x0 | y0<<8 | x1<<16 | y1<<24, signed bytes (src/ORBextractor.cc:160-418, data)
    uint4 omask[64];            // IC_Angle: per lane (row, half) the byte mask of its 16-pixel window inside the circular patch
    uint4 rowB[2][3][64];       // row pass on the matrix cores: per tap profile and column tile the lane's B fragment (orbx_desc_rowpass_matrix)
};
__constant__ DescTab c_desc;
static_assert(offsetof(DescTab, omask) + sizeof(uint4[64]) <= 4096 && sizeof(uint4[3][64]) <= 4096, "every table load is base + lane offset + a 12-bit immediate");

#ifdef ORBX_DIAG
__device__ unsigned long long g_desc_stamp[4096 * 8]; // diagnostic build only: summed phase cycles of k_desc, 4096 slots
__device__ uint2 g_span_1[SPAN_SLOTS];                // SPAN_END(1): slot 1 of orbx_diag_spans
#define DSTAMP(k) STAMP_TO(g_desc_stamp, k)
#else
#define DSTAMP(k) do { } while (0)
#endif

// ================================================================ K4: orientation + blur + rBRIEF (E5-E8)
// One wave per keypoint.  The 43x43 unblurred patch is staged in LDS with BORDER_REFLECT_101 at
// the image edge (the reference blurs a clone of the level, src/ORBextractor.cc:1312-1314), the
// intensity centroid is taken on it (IC_Angle, :83-111), the 7x7 sigma=2 fixed-point Gaussian is
// applied to the patch only (never materialising the blurred level; its row pass on the whole patch, its
// column pass only at the 512 steered sample positions), and the 256 pairs are compared with one ballot
// per 64 pairs (computeOrbDescriptor, :116-157).
// The row pass is the exact integer banded product R[43 x 37] = Raw[43 x 43] . G[43 x 37].  MF = true (the default) computes it on the
// matrix cores: nine v_mfma_i32_16x16x64_i8 (three row tiles x three column tiles, one K step of 64 >= 43 each) on the pixels biased to
// signed bytes (p - 128, one XOR per dword) against the constant banded tap matrix, with 128 * sum(g) as the accumulator's start, so that
// the int32 result is sum(g * p) itself.  MF = false keeps the row pass on the vector ALUs (v_dot4_u32_u8 against shifted tap words);
// ORBX_DESC_VALU_ROWPASS=1, read when the extractor is created, selects it.  Both forms write the same u16 values and share everything else.
// Launch constants of k_desc by value (kernel-argument segment, scalar loads that depend on nothing): the level of a slot is
// found by comparing against kp_off[] in registers, and only then one dependent fetch (the level's record) remains before the
// patch address is known.  Fetching them through the Geom pointer was a chain of dependent scalar loads at the start of every
// wave, during which the wave already holds its LDS.
// The start of a wave is two scalar round trips:
//   1. the head of DescArgs, everything up to kp_off[]: adjacent fields, fetched as wide loads that depend on nothing;
//   2. everything that depends on (b, slot, l), requested in one batch: the level's record lv[l] (one 32-byte load), the image's
//      row of level counts, the slot's packed keypoint, and the PyrRef fields.
// The compiler sinks scalar loads to their first use, behind branches and behind other waits (it makes six to eight dependent rounds of
// these two): DESC_PIN names the values of a round as inputs of one empty asm statement, which puts all their loads in front of one wait.
// Measured (profiles/r18_desc_start.txt): the rounds themselves are worth 0.5 % of the kernel at most; what the start
// gained over its predecessor (2.7 %) came with its shorter scalar instruction stream and its registers.
struct DescLevel { int w, h, pitch, kp_off; long long pyr_off; float scale; int patch_size; };     // 32 bytes
struct DescArgs {
    int kp_total, nimg, cap, rt_on;   // per-image staging slots; images of the launch; output capacity per image; 1: slot "-1" is the row-table wave
    unsigned xg;                      // image columns of the grid: min(8, images) -- blockIdx.x = xg * slot + image column
    int rowb_off;                     // matrix-core row pass: byte offset of the tap profile's rowB table in c_desc
    int acc0;                         // ... and 128 * sum(g), where its accumulators start
    unsigned gauss;                   // taps g0 | g1 << 8 | g2 << 16 | g3 << 24 of the handle's 7-tap kernel (symmetric; orbx_gaussian_taps)
    const int *lvl_cnt;               // [image][ORBX_MAX_LEVELS] keypoints kept per level, zero beyond nlevels
    const uint32_t *lvl_kp;           // [image][kp_total] packed keypoints
    int kp_off[ORBX_MAX_LEVELS];      // first staging slot of level i; INT_MAX for i >= nlevels
    DescLevel lv[ORBX_MAX_LEVELS];
};
static_assert(offsetof(DescArgs, kp_off) == 48 && sizeof(DescLevel) == 32, "the head of DescArgs is three 16-byte loads in front of kp_off[]");
#ifdef ORBX_DESC_NO_PIN     // A/B timing: the same start with its loads left where the compiler puts them
#define DESC_PIN(...) do { } while (0)
#else
#define DESC_PIN(...) asm volatile("" :: __VA_ARGS__)
#endif

// NL = 8 or ORBX_MAX_LEVELS: the level search and the count sums below are unrolled over NL levels (ORB-SLAM2 uses 8)
// The row table of Frame::ComputeStereoMatches (vRowIndices, src/Frame.cc:584-604) as a by-product of the extraction: it depends only
// on the keypoints' rows, octaves and columns, which the quadtree has already fixed, so ONE extra wave per image builds it inside the
// k_desc launch while the other waves compute descriptors (a launch of its own, k_stereo_prep, was 10 us of a single frame's 124 us
// chain).  orbx_stereo_match_batch_device uses it when its caller says so (ORBX_ROWTAB_OF_EXTRACTION: the keypoint buffer still holds what this extraction wrote); any other caller
// of the stereo matcher still gets k_stereo_prep.  Layout (see orbx_stereo.hip): CSR by the keypoint's centre row, row_off[rows + 1],
// one entry (iR | octave << 16, x, minr | maxr << 16, 0) per keypoint.
struct RowTabArgs { int *row_off; uint4 *entries; int ent_cap, rows, on, pad; };
#define ORBX_ROWTAB_MAX_ROWS 600    // a 256-byte level table + two int arrays of rows + 4 entries in k_desc's 5096 bytes of LDS

template <int NL>
__device__ __forceinline__ void desc_rowtab(const DescArgs &da, const int *__restrict__ lc, const uint32_t *__restrict__ kp_img, int cap,
                                            const RowTabArgs &rt, int b, int *cnt, int *cur, int4 *lvtab)
{
    // The wave is alone on its critical path (it must not outlast the descriptor waves of its launch, ~12 us for a single frame), so
    // everything is arranged for few dependent steps: all staging slots are fetched at once (CH per lane, in registers for both
    // passes), the per-level constants come from one LDS read per slot instead of an 8-way select, one LDS atomic per keypoint and pass.
    const int lane = threadIdx.x, rows = rt.rows;
    constexpr int CH = 24;              // 1536 staging slots per trip: every ORB-SLAM2 setting up to ~1400 features in one
    uint32_t pk[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) { const int s = 64 * k + lane; pk[k] = s < da.kp_total ? kp_img[s] : 0u; }
    for (int i = lane; i < rows; i += 64) { cnt[i] = 0; cur[i] = 0; }
    if (lane < NL) {                    // per level: keypoints kept, output index of its first one (= counts of the lower levels), first slot, scale
        int off = 0, c = 0, ko = 0;
        float sc = 1.0f;
#pragma unroll
        for (int i = 0; i < NL; i++) {      // (static indices into the kernel-argument struct: a lane-indexed access would go through scratch)
            const int ci = lc[i];
            if (i < lane) off += ci;
            if (i == lane) { c = ci; ko = da.lv[i].kp_off; sc = da.lv[i].scale; }
        }
        lvtab[lane] = make_int4(c, off, ko, __float_as_int(sc));
    }
    __syncthreads();                    // a one-wave workgroup: orders the LDS passes
    // A slot of level l, position j is output index off[l] + j; x, y = (float)x_l * scale_l, band radius 2 * scale_l (:588-596):
    // exactly the floats k_desc writes into the keypoint record and k_stereo_prep reads back from it.
#define FOR_KEYPOINTS(RELOAD, ...) do { \
        for (int base_ = 0; base_ < da.kp_total; base_ += 64 * CH) { \
            if ((RELOAD) || base_) { \
                _Pragma("unroll") for (int k_ = 0; k_ < CH; k_++) { const int s_ = base_ + 64 * k_ + lane; pk[k_] = s_ < da.kp_total ? kp_img[s_] : 0u; } \
            } \
            _Pragma("unroll") for (int k_ = 0; k_ < CH; k_++) { \
                const int s_ = base_ + 64 * k_ + lane; \
                if (base_ + 64 * k_ < da.kp_total) {    /* wave-uniform */ \
                    int l_ = 0; \
                    _Pragma("unroll") for (int i_ = 1; i_ < NL; i_++) l_ += s_ >= da.kp_off[i_]; \
                    const int4 lv_ = lvtab[l_]; \
                    const float sc_ = __int_as_float(lv_.w); \
                    const int j_ = s_ - lv_.z, ir = lv_.y + j_; \
                    if (s_ < da.kp_total && j_ < lv_.x && ir < cap && ir < rt.ent_cap) { \
                        const uint32_t p_ = pk[k_]; \
                        float fx = (float)(int)(p_ & 0xFFF), fy = (float)(int)((p_ >> 12) & 0xFFF); \
                        if (l_ != 0) { fx *= sc_; fy *= sc_; } \
                        const int crow = min(max((int)floorf(fy), 0), rows - 1); \
                        const int oct = l_; (void)fx; (void)oct; (void)ir; (void)sc_; \
                        __VA_ARGS__; \
                    } \
                } \
            } \
        } } while (0)
    FOR_KEYPOINTS(false, { atomicAdd(&cnt[crow], 1); });
    __syncthreads();
    int carry = 0;
    int *ro = rt.row_off + (long long)b * (rows + 1);
    for (int base = 0; base < rows; base += 64) {       // exclusive scan of the row counts by the wave
        const int i = base + lane, v = i < rows ? cnt[i] : 0;
        const int inc = wave_incl_scan(v);
        if (i < rows) { cnt[i] = carry + inc - v; ro[i] = carry + inc - v; }
        carry += __builtin_amdgcn_readlane(inc, 63);
    }
    if (lane == 0) ro[rows] = carry;
    __syncthreads();
    uint4 *en = rt.entries + (long long)b * rt.ent_cap;
    FOR_KEYPOINTS(da.kp_total > 64 * CH, {
        const float r_ = 2.0f * sc_;
        const int maxr = min((int)ceilf(fy + r_), rows - 1), minr = max((int)floorf(fy - r_), 0);
        en[cnt[crow] + atomicAdd(&cur[crow], 1)] = make_uint4((unsigned)ir | ((unsigned)oct << 16), __float_as_uint(fx),
                                                              (unsigned)minr | ((unsigned)maxr << 16), 0u);
    });
#undef FOR_KEYPOINTS
}

template <int NL, bool MF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(64))) void k_desc(const DescArgs da, PyrRef pr, orbx_keypoint *__restrict__ out_kps,
                                             uint8_t *__restrict__ out_desc, int *__restrict__ out_n, const RowTabArgs rt,
                                             const int *__restrict__ err_flag, int *__restrict__ flag_out)
{
    // LDS pitches: raw bytes (11 dwords per row), row-pass u16 (column-major, 43 rows per column, 37 columns).  1908 + 3188 bytes
    // round to 5120 = 160 KB / 32: the CU holds its maximum of 32 waves (the kernel is latency bound: with 5600 bytes, 29 waves
    // per CU, it ran 3 % slower; every KB more costs 7 %)
    // Matrix-core form: 12 dwords per raw row (every A fragment is an aligned 16-byte read; bytes 44..47 of a row are never staged and
    // only ever meet zero taps) and 44 rows per hb column (a lane's four vertically adjacent results are one aligned 8-byte store).
    // The fragment reads of the third row tile run to row 47 + 16 bytes = byte 2320.  The raw patch is dead once the fragments
    // are in registers, so hb (37 * 88 = 3256 bytes) lies OVER it: 2320 + 3256 would not fit the 5120.  The array keeps the vector form's
    // size (the row-table wave needs it).
    constexpr int RP = MF ? 48 : 44, HR = MF ? 44 : 43;
    constexpr int RAW_BYTES = 43 * 44 + 16;              // 1908 (vector form)
    constexpr int SMEM_BYTES = RAW_BYTES + (37 * 43 + 3) * 2;    // 5096
    __shared__ __align__(16) uint8_t desc_smem[SMEM_BYTES];
    uint8_t *raw = desc_smem;
    uint16_t *hb = reinterpret_cast<uint16_t *>(desc_smem + (MF ? 0 : RAW_BYTES));   // vector form: + the zero-tap row "43" of the last column, read as part of a dword
    static_assert(RAW_BYTES % 4 == 0 && sizeof(desc_smem) >= 16 * ORBX_MAX_LEVELS + 2 * (ORBX_ROWTAB_MAX_ROWS + 4) * sizeof(int), "row table workspace");
    static_assert(!MF || (47 * RP + 64 <= SMEM_BYTES && 37 * HR * 2 <= SMEM_BYTES && RP % 16 == 0 && (HR * 2) % 8 == 0), "matrix-core row pass: fragment reads and hb inside the array, aligned");
    // Workgroups are dealt round-robin over the 8 XCDs (linear id % 8, speed only): XCD x walks the images x, x + 8, x + 16, ...
    // one after the other, so the patches its waves fetch at any time come from one or two images (1.4 MB of pyramid each)
    // instead of from every image in flight on the chip: the per-XCD L2 (4 MB) then holds them
    const int lane = threadIdx.x;
    // grid = (8 * kp_total, ceil(images / 8)): blockIdx.x = 8 * slot + XCD, blockIdx.y = group of eight images; the linear
    // workgroup id (dispatch order) then has the XCD in its low three bits and the slot running fastest within an XCD
    // (with the row table on, slot "-1" -- the first workgroups dispatched -- is the table wave of each image)
    // A launch of fewer than eight images (a single stereo frame: two) has no empty XCD columns in its grid: blockIdx.x = xg * slot +
    // image, xg = min(8, images) -- dispatching the 6 800 empty workgroups of an 8-wide grid took longer than the 2 000 waves that
    // had work (their starts spread over 6.5 us).
    // ---- round 1: the head of the kernel arguments (three 16-byte loads and kp_off[], nothing depends on anything)
#ifdef ORBX_DIAG
    unsigned long long _t_prev = __builtin_amdgcn_s_memtime();
#endif
    SPAN_BEGIN();
    const unsigned xg = da.xg;
    const int cap = da.cap;
    if constexpr (NL == 8)
        DESC_PIN("s"(da.kp_total), "s"(da.nimg), "s"(da.rt_on), "s"(xg), "s"(da.rowb_off), "s"(da.lvl_cnt), "s"(da.lvl_kp), "s"(da.kp_off[1]), "s"(da.kp_off[2]), "s"(da.kp_off[3]),
                 "s"(da.kp_off[4]), "s"(da.kp_off[5]), "s"(da.kp_off[6]), "s"(da.kp_off[7]));
    else
        DESC_PIN("s"(da.kp_total), "s"(da.nimg), "s"(da.rt_on), "s"(xg), "s"(da.rowb_off), "s"(da.lvl_cnt), "s"(da.lvl_kp), "s"(da.kp_off[1]), "s"(da.kp_off[2]), "s"(da.kp_off[3]),
                 "s"(da.kp_off[4]), "s"(da.kp_off[5]), "s"(da.kp_off[6]), "s"(da.kp_off[7]), "s"(da.kp_off[8]), "s"(da.kp_off[9]), "s"(da.kp_off[10]),
                 "s"(da.kp_off[11]), "s"(da.kp_off[12]), "s"(da.kp_off[13]), "s"(da.kp_off[14]), "s"(da.kp_off[15]));
    unsigned sx = blockIdx.x >> 3;
    if (xg != 8) sx = blockIdx.x / xg;      // (fewer than eight images: the division stays behind its condition)
    const int slot = (int)sx - da.rt_on, b = (int)(blockIdx.y * 8u + (blockIdx.x - sx * xg));
    if (b >= da.nimg) return;
    // 32-bit byte offsets of the image's rows (scalar loads take base + a zero-extended 32-bit register): image * max(kp_total,
    // ORBX_MAX_LEVELS) <= 2^30 for every image of a handle's largest batch, orbx_prepare_geometry refuses anything larger
    const unsigned cnt_byte = (unsigned)b * (unsigned)(ORBX_MAX_LEVELS * sizeof(int)), kp_byte = ((unsigned)b * (unsigned)da.kp_total) * 4u;
    if (slot < 0) {
        desc_rowtab<NL>(da, reinterpret_cast<const int *>(reinterpret_cast<const uint8_t *>(da.lvl_cnt) + cnt_byte),
                        reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(da.lvl_kp) + kp_byte), cap, rt, b,
                        reinterpret_cast<int *>(desc_smem) + 4 * ORBX_MAX_LEVELS, reinterpret_cast<int *>(desc_smem) + 4 * ORBX_MAX_LEVELS + ((rt.rows + 4) & ~3),
                        reinterpret_cast<int4 *>(desc_smem));
        return;
    }
    // level of the slot: kp_off[] ascends (INT_MAX beyond nlevels), one scalar compare and select per level
    int l = 0;
    asm("" : "+s"(l));      // (opaque: a select between the constants 0 and 1 is formed on the vector unit and read back)
#pragma unroll
    for (int i = 1; i < NL; i++) l = slot >= da.kp_off[i] ? i : l;
    // ---- round 2, one batch: the level's record, the image's row of level counts (zero beyond nlevels), the slot's packed keypoint (slots
    // past the level's count hold stale data that is never used) and the pyramid's addresses
    // (k_desc only reads the counts and the staging slots: loads through constant-address-space pointers, which the compiler may issue on
    // the scalar unit; through the plain pointers of DescArgs it made them vector loads and read the values back lane by lane)
    const DescLevel L = da.lv[l];
    typedef const __attribute__((address_space(4))) uint8_t *cptr_t;
    typedef const __attribute__((address_space(4))) uint32_t *cptr32_t;
    const cptr_t lc = reinterpret_cast<cptr_t>(reinterpret_cast<unsigned long long>(da.lvl_cnt)) + cnt_byte;
    int cn[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) cn[i] = (int)*reinterpret_cast<cptr32_t>(lc + 4 * i);
    const uint32_t p = *reinterpret_cast<cptr32_t>(reinterpret_cast<cptr_t>(reinterpret_cast<unsigned long long>(da.lvl_kp)) + (kp_byte + 4u * (unsigned)slot));
    const PyrRef P = pr;
    // the lane's constant data (lane-indexed = vector loads) is requested here, with the wave's second round trip, not in the phases that
    // use it, where each table would cost a round trip of its own: four pattern words, the orientation mask, the B fragments of the
    // three column tiles (matrix-core form).  One base for all of them (opaque to the compiler, which otherwise forms every table's address
    // from the program counter again).
    unsigned long long tb_ = reinterpret_cast<unsigned long long>(&c_desc);
    asm volatile("" : "+s"(tb_));
    typedef const __attribute__((address_space(1))) uint8_t *gptr_t;
    const gptr_t tb = reinterpret_cast<gptr_t>(tb_);
    uint32_t pat4[4];
#pragma unroll
    for (int jj = 0; jj < 4; jj++) pat4[jj] = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(tb + offsetof(DescTab, pat4) + 256 * jj + 4 * lane);
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4 *gptr4_t;
    auto load16 = [](gptr_t a) { const u32x4 t = *reinterpret_cast<gptr4_t>(a); return make_uint4(t.x, t.y, t.z, t.w); };
    const uint4 omask = load16(tb + offsetof(DescTab, omask) + 16 * lane);
    uint4 rowB[3] = {};     // (matrix-core form) the lane's B fragments of the three column tiles
    if constexpr (MF) {
        const gptr_t tbB = tb + (unsigned)da.rowb_off;
#pragma unroll
        for (int nt = 0; nt < 3; nt++) rowB[nt] = load16(tbB + 1024 * nt + 16 * lane);
    }
    if constexpr (NL == 8)
        DESC_PIN("s"(L.w), "s"(L.h), "s"(L.pitch), "s"(L.kp_off), "s"(L.pyr_off), "s"(L.scale), "s"(L.patch_size), "s"(p),
                 "s"(P.img0), "s"(P.img0_stride), "s"(P.img0_pitch), "s"(P.pyr), "s"(P.pyr_stride),
                 "s"(cn[0]), "s"(cn[1]), "s"(cn[2]), "s"(cn[3]), "s"(cn[4]), "s"(cn[5]), "s"(cn[6]), "s"(cn[7]));
    else
        DESC_PIN("s"(L.w), "s"(L.h), "s"(L.pitch), "s"(L.kp_off), "s"(L.pyr_off), "s"(L.scale), "s"(L.patch_size), "s"(p),
                 "s"(P.img0), "s"(P.img0_stride), "s"(P.img0_pitch), "s"(P.pyr), "s"(P.pyr_stride),
                 "s"(cn[0]), "s"(cn[1]), "s"(cn[2]), "s"(cn[3]), "s"(cn[4]), "s"(cn[5]), "s"(cn[6]), "s"(cn[7]),
                 "s"(cn[8]), "s"(cn[9]), "s"(cn[10]), "s"(cn[11]), "s"(cn[12]), "s"(cn[13]), "s"(cn[14]), "s"(cn[15]));
    // prefix sums of the counts; the level's own count and the counts below it are S[l + 1] - S[l] and S[l], both selected from registers
    // by the bits of l (a select tree: NL - 1 selects each, against a compare, a select and an add per level and a second fetch of lc[l])
    int S[NL + 1];
    S[0] = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) S[i + 1] = S[i] + cn[i];
    if (slot == 0 && lane == 0) {
        out_n[b] = S[NL] < cap ? S[NL] : cap;
        if (flag_out && b == 0) *flag_out = *err_flag;     // (pipelined frames: the quadtree's error flag rides in the frame's result block)
    }
    int lo_[NL], hi_[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) { lo_[i] = S[i]; hi_[i] = S[i + 1]; }
#pragma unroll
    for (int w = NL / 2, bit = 0; w >= 1; w >>= 1, bit++) {
        const bool odd = (l >> bit) & 1;
#pragma unroll
        for (int k = 0; k < w; k++) { lo_[k] = odd ? lo_[2 * k + 1] : lo_[2 * k]; hi_[k] = odd ? hi_[2 * k + 1] : hi_[2 * k]; }
    }
    const int off = lo_[0];
    const int j = slot - L.kp_off;
    if (j >= hi_[0] - off) return;
    const int idx = off + j;
    if (idx >= cap) return;
    const int x = p & 0xFFF, y = (p >> 12) & 0xFFF, resp = p >> 24;
    const int pitch = l == 0 ? P.img0_pitch : L.pitch;
    // (the pyramid block of one image is below 4 GB, orbx_prepare_geometry: image * stride is one 32 x 32 -> 64 bit product)
    const uint8_t *img = l == 0 ? P.img0 + (long long)b * P.img0_stride : P.pyr + (unsigned long long)(unsigned)b * (unsigned)P.pyr_stride + L.pyr_off;
#ifdef ORBX_DIAG
    asm volatile("" :: "v"(x), "s"(pitch));
    DSTAMP(5); // prologue: both scalar rounds, level search, count prefix, patch address
#endif
    // ---- stage the 43x43 patch at LDS column 0 of every row (unaligned dword loads: the window phase is a constant,
    // so the realignment shifts below are immediates and the row pass reads three dwords per item instead of four)
    constexpr int xo = 0;
    const int x0a = x - 21;
    if (x >= 21 && x + 21 < L.w && y >= 21 && y + 21 < L.h && x0a + 44 <= pitch) {
        const uint8_t *src = img + (long long)(y - 21) * pitch + x0a;
        // nine direct loads (global_load_lds_dword: any byte alignment, no VGPR round trip, no ds_write), all in flight together.
        // Lane = (row lane/11, dword lane%11) of a 5-row band (55 lanes), band k covers rows 5k..5k+4 and lands at raw + 220 k + 4 lane:
        // row-major with the 44-byte pitch.  (Matrix-core form: 12 dwords per row, 60 lanes, 240 bytes per band; the twelfth dword of a
        // row is not loaded -- it only meets zero taps, and loading it would push keypoints near the right edge of the pitch to the slow path.)
        // scalar band base + one 32-bit lane offset: the bands advance on the scalar unit (a 64-bit vector multiply-add per load otherwise)
        constexpr int DW = RP / 4;
        const int lr = lane / DW, lc = lane - lr * DW;
        const unsigned voff = (unsigned)(lr * pitch + 4 * lc);
        if (lane < 5 * DW && lc < 11) {
#pragma unroll
            for (int k = 0; k < 8; k++, src += 5 * (long long)pitch)
                __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t *>(src + voff), reinterpret_cast<uint32_t *>(raw + 5 * RP * k), 4, 0, 0);
            if (lr < 3)   // rows 40..42
                __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t *>(src + voff), reinterpret_cast<uint32_t *>(raw + 5 * RP * 8), 4, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else { // image edge (BORDER_REFLECT_101 of the cloned level, :1312-1314)
        // lane = patch column (its reflected source column computed once), rows walked on the scalar unit, sixteen byte loads in
        // flight (three round trips for the 43 rows): ~2 vector instructions per row (an element-wise walk with a division and two
        // reflections per byte cost more than the whole rest of the keypoint, for the ~6 % of the keypoints that lie within 21 px of an
        // image edge).  Every load is scalar row base + the column as an unsigned 32-bit lane offset: written as img[ry * pitch + cx] the
        // compiler adds the column to the image base first and forms every row's address with a 64-bit vector multiply-add.
#ifdef ORBX_DESC_EDGE_VADDR     // A/B timing: that form, eight loads in flight
        const int cx = reflect101(x - 21 + min(lane, 42), L.w);
        if (lane < 43) {
#pragma unroll 8
            for (int r = 0; r < 43; r++) {
                const int ry = reflect101(y - 21 + r, L.h);
                raw[r * RP + lane] = img[(long long)ry * pitch + cx];
            }
        }
#else
        const unsigned cx = (unsigned)reflect101(x - 21 + min(lane, 42), L.w);
        if (lane < 43) {
            constexpr int G = 16;
#pragma unroll 1
            for (int r0 = 0; r0 < 43; r0 += G) {
                uint8_t v[G];
#pragma unroll
                for (int k = 0; k < G; k++) {
                    const int ry = reflect101(y - 21 + min(r0 + k, 42), L.h);      // (rows past the patch: row 42 again, not stored)
                    unsigned long long rowp = reinterpret_cast<unsigned long long>(img + (long long)ry * pitch);
                    asm("" : "+s"(rowp));   // (opaque: keeps the row base on the scalar unit)
                    v[k] = reinterpret_cast<const __attribute__((address_space(1))) uint8_t *>(rowp)[cx];
                }
#pragma unroll
                for (int k = 0; k < G; k++)
                    if (r0 + k < 43) raw[(r0 + k) * RP + lane] = v[k];
            }
        }
#endif
    }
    DSTAMP(6); // patch loads issued and consumed (the last LDS stores may still be in flight)
    __syncthreads();
    DSTAMP(0);
    // ---- IC_Angle: lane = (row v+15, half); integer moments, order-independent
    int m10 = 0, m01 = 0;
    if (lane < 62) {
        // lane = (row v, half): its 16-pixel window (left half u = -16..-1, right half u = 0..15) is five aligned LDS
        // dwords realigned with v_alignbyte and masked to the circular patch (mask fetched with the first round trip);
        // sum(I) by v_sad_u8 against 0 and sum(k*I), k = 0..15, by v_dot4_u32_u8 against constant weights
        const int v = (lane >> 1) - 15, half = lane & 1;
        const int off = xo + (half ? 21 : 5);     // byte offset of the window in the staged row
        const uint32_t *d = reinterpret_cast<const uint32_t *>(raw + (21 + v) * RP) + (off >> 2);
        const unsigned D0 = d[0], D1 = d[1], D2 = d[2], D3 = d[3], D4 = d[4];
        const int sh = off & 3;
        const unsigned W0 = __builtin_amdgcn_alignbyte(D1, D0, sh) & omask.x, W1 = __builtin_amdgcn_alignbyte(D2, D1, sh) & omask.y,
                       W2 = __builtin_amdgcn_alignbyte(D3, D2, sh) & omask.z, W3 = __builtin_amdgcn_alignbyte(D4, D3, sh) & omask.w;
        const unsigned rs = __builtin_amdgcn_sad_u8(W0, 0u, __builtin_amdgcn_sad_u8(W1, 0u, __builtin_amdgcn_sad_u8(W2, 0u, __builtin_amdgcn_sad_u8(W3, 0u, 0u))));
        const unsigned pk = __builtin_amdgcn_udot4(W0, 0x03020100u, __builtin_amdgcn_udot4(W1, 0x07060504u,
                            __builtin_amdgcn_udot4(W2, 0x0B0A0908u, __builtin_amdgcn_udot4(W3, 0x0F0E0D0Cu, 0u, false), false), false), false);
        m10 = (int)pk - (half ? 0 : 16 * (int)rs);   // u = k - 16 in the left half
        m01 = v * (int)rs;
    }
    m10 = wave_sum(m10);
    m01 = wave_sum(m01);
    const float angle = dev_fast_atan2((float)m01, (float)m10);
    DSTAMP(1);
    // the steering sine / cosine (a long dependent fp64 chain) is computed here, where it can overlap the LDS traffic of the blur
    const float factor_pi = (float)(3.14159265358979323846 / 180.f);
    float sn, cs;
    dev_sincos(angle * factor_pi, &sn, &cs);
    const unsigned g0 = da.gauss & 0xFFu, g1 = (da.gauss >> 8) & 0xFFu, g2 = (da.gauss >> 16) & 0xFFu, g3 = da.gauss >> 24;   // symmetric: g4 = g2, g5 = g1, g6 = g0
    if constexpr (MF) {
        // ---- row pass on the matrix cores.  Row tile mt, column tile nt: D[16 x 16] = A_mt[16 x 64] . B_nt[64 x 16] + acc0.
        // A fragment: lane = (row l % 16 of the tile, K block l / 16) holds 16 consecutive bytes of its raw row (one aligned ds_read_b128),
        // biased to signed.  Byte j of K block q is column 16 q + j in both A and B, so the product does not depend on the order in which
        // the instruction walks K.  Columns 43..63 (the next raw row's first bytes for q = 3, never-staged bytes 44..47) and rows 43..47
        // (beyond the patch, inside the array) are arbitrary bytes: the former meet zero taps, the latter's results are padding or dropped.
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        const int r16 = lane & 15, q = lane >> 4;
        const uint4 *ap = reinterpret_cast<const uint4 *>(raw + r16 * RP + 16 * q);
        i32x4 A[3];
#pragma unroll
        for (int mt = 0; mt < 3; mt++) {
            const uint4 t = ap[mt * RP];     // 16 rows of RP bytes, in uint4s
            A[mt] = i32x4{ (int)(t.x ^ 0x80808080u), (int)(t.y ^ 0x80808080u), (int)(t.z ^ 0x80808080u), (int)(t.w ^ 0x80808080u) };
        }
        // hb overlays the raw patch: every fragment is in registers before the first result is written (one wave per workgroup)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // D layout: lane = (column l % 16 of the tile, rows 4 (l / 16) .. + 3): four vertically adjacent u16 of one hb column, one
        // aligned 8-byte store.  Rows >= 44 and columns >= 37 are not written (row 43 is the padding row that only meets the zero tap)
        const i32x4 C0 = { da.acc0, da.acc0, da.acc0, da.acc0 };
        uint8_t *wp = reinterpret_cast<uint8_t *>(hb) + r16 * (HR * 2) + q * 8;
#pragma unroll
        for (int mt = 0; mt < 3; mt++) {
#pragma unroll
            for (int nt = 0; nt < 3; nt++) {
                const i32x4 Bf = { (int)rowB[nt].x, (int)rowB[nt].y, (int)rowB[nt].z, (int)rowB[nt].w };
                const i32x4 D = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[mt], Bf, C0, 0, 0, 0);
                if ((mt < 2 || q < 3) && (nt < 2 || r16 < 5))     // results of real rows are <= 65535
                    *reinterpret_cast<uint2 *>(wp + nt * 16 * (HR * 2) + mt * 32) = make_uint2(__builtin_amdgcn_perm((unsigned)D.y, (unsigned)D.x, 0x05040100u), __builtin_amdgcn_perm((unsigned)D.w, (unsigned)D.z, 0x05040100u));   // low halves: D.x | D.y << 16
            }
        }
    } else {
    // ---- row pass on the vector ALUs: 4 outputs per item from 3 aligned dwords.  Output k needs bytes k .. k + 6: instead of shifting the data
    // (v_alignbyte) the TAPS are shifted -- ten constant tap words, v_dot4_u32_u8 against each dword an output touches
    const unsigned TA0 = g0 | g1 << 8 | g2 << 16 | g3 << 24, TB0 = g2 | g1 << 8 | g0 << 16;
    const unsigned TA1 = g0 << 8 | g1 << 16 | g2 << 24, TB1 = g3 | g2 << 8 | g1 << 16 | g0 << 24;
    const unsigned TA2 = g0 << 16 | g1 << 24, TB2 = g2 | g3 << 8 | g2 << 16 | g1 << 24, TC2 = g0;
    const unsigned TA3 = g0 << 24, TB3 = g1 | g2 << 8 | g3 << 16 | g2 << 24, TC3 = g1 | g0 << 8;
    // lane = (row r_lo = lane / 10 of a band of six rows, group gq = lane % 10), eight bands: every LDS address of the pass is
    // the lane's base plus an immediate (no per-item index arithmetic); the last band holds row 42 only
    if (lane < 60) {
        const int r_lo = lane / 10, gq = lane - r_lo * 10;
        const uint32_t *d0 = reinterpret_cast<const uint32_t *>(raw + r_lo * RP) + gq;
        uint16_t *w0 = hb + (4 * gq) * HR + r_lo;   // column-major: the column pass reads vertically adjacent values as packed pairs
#pragma unroll
        for (int it = 0; it < 8; it++) {
            if (it < 7 || r_lo == 0) {
                const uint32_t *d = d0 + it * 6 * (RP / 4);
                const unsigned W0 = d[0], W1 = d[1], W2 = d[2]; // the 10 bytes an item needs (4 outputs + 6 taps) start dword-aligned
                unsigned o[4];
                o[0] = __builtin_amdgcn_udot4(W0, TA0, __builtin_amdgcn_udot4(W1, TB0, 0u, false), false);
                o[1] = __builtin_amdgcn_udot4(W0, TA1, __builtin_amdgcn_udot4(W1, TB1, 0u, false), false);
                o[2] = __builtin_amdgcn_udot4(W0, TA2, __builtin_amdgcn_udot4(W1, TB2, __builtin_amdgcn_udot4(W2, TC2, 0u, false), false), false);
                o[3] = __builtin_amdgcn_udot4(W0, TA3, __builtin_amdgcn_udot4(W1, TB3, __builtin_amdgcn_udot4(W2, TC3, 0u, false), false), false);
                w0[6 * it] = (uint16_t)o[0];
                if (gq < 9) {   // the tenth group only owns column 36
#pragma unroll
                    for (int k = 1; k < 4; k++) w0[k * HR + 6 * it] = (uint16_t)o[k];
                }
            }
        }
    }
    }
    __syncthreads();
    DSTAMP(2);
    // ---- column pass ONLY at the 512 sampled positions (8 per lane) instead of on all 37 x 37: the seven row-pass values of
    // a sample are contiguous in its column (column-major hb), fetched as four aligned dwords and realigned by the row parity
    // with one v_alignbit each (shift in a register; one misaligned ds_read_b128 instead returns the right bytes on gfx950 but ran
    // the kernel 36 % slower); an output is four v_dot2_u32_u16 against the packed symmetric taps (g0,g1)(g2,g3)(g2,g1)(g0,0)
    // with the rounding constant as the first accumulator.  Row 43 is padding: it only ever meets the zero tap.
    typedef unsigned short u16x2v __attribute__((ext_vector_type(2)));
    const u16x2v G01 = __builtin_bit_cast(u16x2v, g0 | (g1 << 16)), G23 = __builtin_bit_cast(u16x2v, g2 | (g3 << 16)),
                 G21 = __builtin_bit_cast(u16x2v, g2 | (g1 << 16)), G0 = __builtin_bit_cast(u16x2v, g0);
    // Rounding: cvRound(v) = round-half-even = the low bits of v + 1.5 * 2^23 (|v| < 2^22; one packed add for both coordinates,
    // no v_rndne / v_cvt).  With rb = bits(row + M), qb = bits(col + M): 44 * (low 24 bits of qb) + rb is the u16 index of
    // (18 + col, 18 + row) in hb plus a constant.
    const float MAGIC = 12582912.f;   // 0x4B400000
    auto blurred = [&](unsigned rb, unsigned qb) -> unsigned {
        const unsigned i16 = __umul24(qb, (unsigned)HR) + rb - (0x400000u * HR + 0x4B400000u) + 18u * (HR + 1);
        const unsigned ba = i16 << 1, sh = ba << 3;   // v_alignbit / v_lshrrev use the low 5 bits of the shift: 16 * (row parity)
        const uint32_t *d = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(hb) + (ba & ~3u));
        const unsigned D0 = d[0], D1 = d[1], D2 = d[2], D3 = d[3];
        unsigned acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2v, __builtin_amdgcn_alignbit(D1, D0, sh)), G01, 1u << 15, false); // sums stay below 2^25
        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2v, __builtin_amdgcn_alignbit(D2, D1, sh)), G23, acc, false);
        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2v, __builtin_amdgcn_alignbit(D3, D2, sh)), G21, acc, false);
        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2v, D3 >> (sh & 31u)), G0, acc, false);
        const unsigned v = acc >> 16;
        return v > 255u ? 255u : v;
    };
    const float a = cs, bb = sn;
    unsigned long long words[4];
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
        const uint32_t pw = pat4[jj];
        const float x0 = (float)(signed char)(pw & 0xFF), y0 = (float)(signed char)((pw >> 8) & 0xFF),
                    x1 = (float)(signed char)((pw >> 16) & 0xFF), y1 = (float)(signed char)(pw >> 24);
        // (x*b + y*a, x*a - y*b) as two packed fp32 multiplies and one packed add (v_pk_mul_f32 / v_pk_add_f32 round each
        // component like the scalar forms; y*(-b) == -(y*b) exactly, so the subtraction is unchanged)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 BA = { bb, a }, AnB = { a, -bb }, MM = { MAGIC, MAGIC };
        const f32x2 R0 = (f32x2{ x0, x0 } * BA + f32x2{ y0, y0 } * AnB) + MM, R1 = (f32x2{ x1, x1 } * BA + f32x2{ y1, y1 } * AnB) + MM;
        const unsigned t0 = blurred(__float_as_uint(R0.x), __float_as_uint(R0.y)), t1 = blurred(__float_as_uint(R1.x), __float_as_uint(R1.y));
        words[jj] = __ballot(t0 < t1);
    }
    if (lane == 0) {
        unsigned long long *d = reinterpret_cast<unsigned long long *>(out_desc + ((long long)b * cap + idx) * 32);
        d[0] = words[0]; d[1] = words[1]; d[2] = words[2]; d[3] = words[3];
        orbx_keypoint kp;
        kp.x = (float)x; kp.y = (float)y;
        if (l != 0) { kp.x *= L.scale; kp.y *= L.scale; } // :1326-1334
        kp.size = (float)L.patch_size;
        kp.angle = angle;
        kp.response = (float)resp;
        kp.octave = l;
        kp.class_id = -1;
        out_kps[(long long)b * cap + idx] = kp;
    }
    DSTAMP(4);
    SPAN_END(1);
#ifdef ORBX_DIAG
    if (lane == 0) atomicAdd(&g_desc_stamp[((blockIdx.x * 131 + blockIdx.y) & 4095) * 8 + 7], 1ull);
#endif
}

#ifdef ORBX_DIAG
extern "C" int orbx_diag_desc_stamps(unsigned long long *out, int reset) { return orbx_diag_stamp_sums(HIP_SYMBOL(g_desc_stamp), out, reset); }
int orbx_desc_diag_spans(unsigned *out, int reset) { return orbx_diag_span_read(HIP_SYMBOL(g_span_1), out, reset); }
#endif

// ================================================================ host side

int orbx_desc_upload_constants(orbx_extractor *e)
{
    uint32_t pat[256];
    for (int i = 0; i < 256; i++)
        pat[i] = (uint32_t)(uint8_t)ORB_PAT_X0[i] | ((uint32_t)(uint8_t)ORB_PAT_Y0[i] << 8) | ((uint32_t)(uint8_t)ORB_PAT_X1[i] << 16) |
                 ((uint32_t)(uint8_t)ORB_PAT_Y1[i] << 24);
    ORBX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_desc), pat, sizeof pat, offsetof(DescTab, pat4)));
    {   // the banded tap matrices of the matrix-core row pass, one per tap profile (a launch names its profile's table: DescArgs::rowb_off)
        uint8_t rb[2][3 * 64 * 16];
        int acc0;
        for (int prof = 0; prof < 2; prof++) { const int rc = orbx_desc_rowpass_matrix(prof, rb[prof], &acc0); if (rc) return rc; }
        static_assert(sizeof rb == sizeof(DescTab::rowB), "one table of three column tiles per tap profile");
        ORBX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_desc), rb, sizeof rb, offsetof(DescTab, rowB)));
    }
    {   // k_desc's orientation lanes: lane = (row v = lane/2 - 15, half = lane & 1); the left half covers u = -16..-1 and
        // keeps u >= -umax[|v|], the right half covers u = 0..15 and keeps u <= umax[|v|] (src/ORBextractor.cc:91-108)
        uint8_t m[64][16];
        memset(m, 0, sizeof m);
        for (int lane = 0; lane < 62; lane++) {
            const int v = (lane >> 1) - 15, d = e->umax[v < 0 ? -v : v];
            for (int k = 0; k < 16; k++) {
                const int u = (lane & 1) ? k : k - 16;
                m[lane][k] = (u >= -d && u <= d) ? 0xFF : 0;
            }
        }
        ORBX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_desc), m, sizeof m, offsetof(DescTab, omask)));
    }
    return ORBX_OK;
}

// The 7-tap sigma = 2 kernel of cv::GaussianBlur(.., Size(7, 7), 2, 2, BORDER_REFLECT_101) on 8-bit images (src/ORBextractor.cc:1311)
// as the 8-bit fixed-point integers the OpenCV generation named by `profile` filters with.  Both generations run the same
// arithmetic around the taps -- exact integer row pass, column pass (sum + 2^15) >> 16 -- so the table IS the profile:
//   ORBX_CV_PROFILE_3_2   (OpenCV <= 3.4.1): cvRound(k * 256) of the float kernel, not renormalised: 18 34 49 55 49 34 18 (sum 257)
//   ORBX_CV_PROFILE_3_4_2 (OpenCV >= 3.4.2 / 4.x, the bit-exact fixed-point path): rounded from the outside in with the
//                          rounding error carried along, centre = 256 - the rest: 18 34 48 56 48 34 18 (sum 256)
// (both restated from memory of OpenCV -- parity unpinned).
extern "C" int orbx_gaussian_taps(int profile, int taps[7])
{
    if (!taps || (profile != ORBX_CV_PROFILE_3_2 && profile != ORBX_CV_PROFILE_3_4_2)) { orbx_set_error("orbx_gaussian_taps: unknown profile %d", profile); return ORBX_E_INVALID; }
    const double scale2x = -0.5 / (2.0 * 2.0);
    if (profile == ORBX_CV_PROFILE_3_2) {
        float cf[7]; double sum = 0;
        for (int i = 0; i < 7; i++) { const double x = i - 3.0; cf[i] = (float)exp(scale2x * x * x); sum += cf[i]; }
        sum = 1. / sum;
        for (int i = 0; i < 7; i++) { cf[i] = (float)(cf[i] * sum); taps[i] = (int)lrint((double)cf[i] * 256.0); }
    } else {
        double k[7], sum = 0, err = 0;
        for (int i = 0; i < 7; i++) { const double x = i - 3.0; k[i] = exp(scale2x * x * x); sum += k[i]; }
        int rest = 0;
        for (int i = 0; i < 3; i++) {
            const double adj = k[i] / sum * 256.0 + err;
            const int v = (int)lrint(adj);
            err = adj - v;
            taps[i] = taps[6 - i] = v;
            rest += 2 * v;
        }
        taps[3] = 256 - rest;
    }
    return ORBX_OK;
}

// The constant operand of k_desc's matrix-core row pass for a tap profile: R[43 x 37] = Raw[43 x 43] . G with G[k][c] = g[k - c] for
// 0 <= k - c <= 6, else 0, cut into three column tiles of 16 and laid out as the B fragments of v_mfma_i32_16x16x64_i8: byte j of lane l
// of tile nt is G[16 (l / 16) + j][16 nt + l % 16], zero for k >= 43 and c >= 37.  *acc0 = 128 * sum(g): the kernel feeds p - 128.
extern "C" int orbx_desc_rowpass_matrix(int profile, uint8_t *out, int *acc0)
{
    int taps[7];
    const int rc = orbx_gaussian_taps(profile, taps);
    if (rc) return rc;
    if (!out || !acc0) { orbx_set_error("orbx_desc_rowpass_matrix: null argument"); return ORBX_E_INVALID; }
    int sum = 0;
    for (int i = 0; i < 7; i++) sum += taps[i];
    *acc0 = 128 * sum;
    for (int nt = 0; nt < 3; nt++)
        for (int l = 0; l < 64; l++)
            for (int j = 0; j < 16; j++) {
                const int k = 16 * (l / 16) + j, c = 16 * nt + l % 16, d = k - c;
                out[(nt * 64 + l) * 16 + j] = (uint8_t)(k < 43 && c < 37 && d >= 0 && d <= 6 ? taps[d] : 0);
            }
    return ORBX_OK;
}

extern "C" int orbx_extractor_set_cv_profile(orbx_extractor *e, int profile)
{
    if (!e) { orbx_set_error("null extractor"); return ORBX_E_INVALID; }
    int taps[7];
    const int rc = orbx_gaussian_taps(profile, taps);
    if (rc) return rc;
    for (int i = 0; i < 4; i++) e->gauss[i] = taps[i];   // launch constants of k_desc: later launches use them, earlier ones keep theirs
    e->cv_profile = profile;
    return ORBX_OK;
}

// k_desc's step of orbx_prepare_geometry: does the stereo row table ride along with this geometry's extractions (desc_rowtab)?
bool orbx_desc_rowtab_plan(const Geom &G) { return G.lv[0].h <= ORBX_ROWTAB_MAX_ROWS && !getenv("ORBX_NO_ROWTAB"); }

void orbx_desc_launch(orbx_extractor *e, const PyrRef &pr, int batch, void *d_kps, void *d_desc, void *d_n_out, int cap, hipStream_t s)
{
    const Geom &G = e->geom;
    DescArgs da;
    memset(&da, 0, sizeof da);
    da.kp_total = G.kp_total; da.nimg = batch; da.cap = cap; da.xg = batch < 8 ? batch : 8;
    da.lvl_cnt = e->d_lvl_cnt; da.lvl_kp = e->d_lvl_kp;
    da.gauss = (unsigned)e->gauss[0] | (unsigned)e->gauss[1] << 8 | (unsigned)e->gauss[2] << 16 | (unsigned)e->gauss[3] << 24;
    da.rowb_off = (int)(offsetof(DescTab, rowB) + (e->cv_profile == ORBX_CV_PROFILE_3_4_2) * sizeof(uint4[3][64])); da.acc0 = 128 * (2 * (e->gauss[0] + e->gauss[1] + e->gauss[2]) + e->gauss[3]);
    for (int i = 0; i < ORBX_MAX_LEVELS; i++) {
        da.kp_off[i] = i < G.nlevels ? G.lv[i].kp_off : INT_MAX;
        if (i < G.nlevels) {
            const LevelGeom &L = G.lv[i];
            da.lv[i].w = L.w; da.lv[i].h = L.h; da.lv[i].pitch = L.pitch; da.lv[i].kp_off = L.kp_off; da.lv[i].pyr_off = L.pyr_off;
            da.lv[i].scale = L.scale; da.lv[i].patch_size = L.patch_size;
        }
    }
    RowTabArgs rt;
    memset(&rt, 0, sizeof rt);
    e->rt_kps = nullptr;
    if (e->d_rt_off && cap < 65536) {          // the stereo row table rides along (see desc_rowtab)
        rt.row_off = e->d_rt_off; rt.entries = (uint4 *)e->d_rt_entries; rt.ent_cap = e->rt_ent_cap; rt.rows = G.lv[0].h; rt.on = 1;
        e->rt_kps = d_kps; e->rt_cap = cap; e->rt_batch = batch;
    }
    da.rt_on = rt.on;
    e->last_forms[6] = G.nlevels <= 8 ? 8 : ORBX_MAX_LEVELS;    // orbx_debug_launch_forms
    e->last_forms[9] = e->desc_valu_rowpass ? 1 : 2;
    const auto kern = e->desc_valu_rowpass ? (G.nlevels <= 8 ? k_desc<8, false> : k_desc<ORBX_MAX_LEVELS, false>)
                                           : (G.nlevels <= 8 ? k_desc<8, true> : k_desc<ORBX_MAX_LEVELS, true>);
    hipLaunchKernelGGL(kern, dim3(da.xg * (G.kp_total + rt.on), (batch + 7) / 8), dim3(64), 0, s, da, pr,
                       (orbx_keypoint *)d_kps, (uint8_t *)d_desc, (int *)d_n_out, rt, (const int *)orbx_err_flag(e), e->flag_out);
}

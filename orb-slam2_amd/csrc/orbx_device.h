// orbx_device.h — wave64 / workgroup helpers and the exact-arithmetic device primitives.
#pragma once
#include "orbx_internal.h"

#define WAVE 64

// ---- arrays that take part in a RELAXED PUBLISH PROTOCOL (k_stereo's folded median cut, k_match's last-arriver finalisation).
// Producers on any XCD write their results as relaxed agent-scope atomic stores (gfx942 / gfx950: `global_store ... sc1`, a write-through
// that leaves no dirty line in the producer's L2), wait for the acknowledgements (`publish_drain`: s_waitcnt vmcnt(0)) and only then bump a
// relaxed agent-scope arrival counter; the workgroup whose bump completes the count reads the array with relaxed agent-scope atomic loads
// (sc1: served from the memory side, never from a stale line of its own XCD's L2).  That replaces a release fence per producer
// (`__threadfence()` = buffer_wbl2: 17-27 us of a 2000-item launch, profiles/r03_match_stamps.txt) and is correct ONLY while EVERY access to
// such an array inside the launch is an agent-scope atomic: one plain load may hit a stale L2 line, one plain store may sit dirty in an L2 the
// consumer never sees.  `Published<T>` therefore has no operator[] and hands out no pointer: a plain access of these arrays does not
// compile.  A launch whose consumer is a LATER launch (kernel boundaries write back and invalidate) may use `plain_across_launches()`.
// The reasoning is about this memory system, so the build is refused for any other target.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "liborbx relies on gfx950 cache semantics (sc1 write-through stores in the relaxed publish protocols): build with --offload-arch=gfx950 only"
#endif
template <typename T>
class Published {
    T *p_;
public:
    Published() = default;
    __host__ __device__ explicit Published(T *p) : p_(p) {}
    __device__ __forceinline__ void put(long long i, T v) const { __hip_atomic_store(p_ + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ T get(long long i) const { return __hip_atomic_load(p_ + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __host__ __device__ __forceinline__ Published at(long long off) const { return Published(p_ + off); }
    // only for a launch that does not run the protocol (its results are consumed by a later launch)
    __device__ __forceinline__ T *plain_across_launches() const { return p_; }
};
// a producer's stores have been acknowledged by the memory side: what it publishes next (the arrival bump) is ordered behind them
__device__ __forceinline__ void publish_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// the arrival bump itself; returns the number of producers that had arrived before this one
__device__ __forceinline__ int publish_arrive(int *counter) { return __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// forward declaration of the DPP helper macro used below
#define ORBX_DPP(v, identity, ctrl, row_mask, bank_mask) \
    __builtin_amdgcn_update_dpp((int)(identity), (int)(v), ctrl, row_mask, bank_mask, false)

// inclusive wave64 prefix sum on the DPP path: Kogge-Stone inside each 16-lane row (row_shr 1, 2, 4, 8), then the
// row totals ripple with row_bcast:15 (into rows 1 and 3) and row_bcast:31 (into rows 2 and 3)
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += ORBX_DPP(v, 0, 0x111, 0xf, 0xf);
    v += ORBX_DPP(v, 0, 0x112, 0xf, 0xf);
    v += ORBX_DPP(v, 0, 0x114, 0xf, 0xf);
    v += ORBX_DPP(v, 0, 0x118, 0xf, 0xf);
    v += ORBX_DPP(v, 0, 0x142, 0xa, 0xf);
    v += ORBX_DPP(v, 0, 0x143, 0xc, 0xf);
    return v;
}

// inclusive wave64 prefix OR, same network
__device__ __forceinline__ unsigned wave_incl_scan_or(unsigned v)
{
    v |= (unsigned)ORBX_DPP(v, 0, 0x111, 0xf, 0xf);
    v |= (unsigned)ORBX_DPP(v, 0, 0x112, 0xf, 0xf);
    v |= (unsigned)ORBX_DPP(v, 0, 0x114, 0xf, 0xf);
    v |= (unsigned)ORBX_DPP(v, 0, 0x118, 0xf, 0xf);
    v |= (unsigned)ORBX_DPP(v, 0, 0x142, 0xa, 0xf);
    v |= (unsigned)ORBX_DPP(v, 0, 0x143, 0xc, 0xf);
    return v;
}

// Wave64 reductions on the DPP data path (row_shr 1/2/4/8 inside each 16-lane row, then row_bcast 15 / 31
// across rows; the total lands in lane 63 and is broadcast with v_readlane): 6 VALU + DPP steps instead of the six
// dependent ds_bpermute round trips that __shfl_xor lowers to.  Lanes without a source read `identity`.

__device__ __forceinline__ int wave_sum(int v)
{
    v += ORBX_DPP(v, 0, 0x111, 0xf, 0xf); // row_shr:1
    v += ORBX_DPP(v, 0, 0x112, 0xf, 0xf); // row_shr:2
    v += ORBX_DPP(v, 0, 0x114, 0xf, 0xe); // row_shr:4
    v += ORBX_DPP(v, 0, 0x118, 0xf, 0xc); // row_shr:8
    v += ORBX_DPP(v, 0, 0x142, 0xa, 0xf); // row_bcast:15
    v += ORBX_DPP(v, 0, 0x143, 0xc, 0xf); // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    const unsigned id = 0xFFFFFFFFu;
    v = min(v, (unsigned)ORBX_DPP(v, id, 0x111, 0xf, 0xf));
    v = min(v, (unsigned)ORBX_DPP(v, id, 0x112, 0xf, 0xf));
    v = min(v, (unsigned)ORBX_DPP(v, id, 0x114, 0xf, 0xe));
    v = min(v, (unsigned)ORBX_DPP(v, id, 0x118, 0xf, 0xc));
    v = min(v, (unsigned)ORBX_DPP(v, id, 0x142, 0xa, 0xf));
    v = min(v, (unsigned)ORBX_DPP(v, id, 0x143, 0xc, 0xf));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// reductions inside each 16-lane row (a quarter wave), result in every lane of the row: butterfly of row rotations
__device__ __forceinline__ unsigned row16_min_u32(unsigned v)
{
    v = min(v, (unsigned)ORBX_DPP(v, v, 0x128, 0xf, 0xf)); // row_ror:8
    v = min(v, (unsigned)ORBX_DPP(v, v, 0x124, 0xf, 0xf)); // row_ror:4
    v = min(v, (unsigned)ORBX_DPP(v, v, 0x122, 0xf, 0xf)); // row_ror:2
    v = min(v, (unsigned)ORBX_DPP(v, v, 0x121, 0xf, 0xf)); // row_ror:1
    return v;
}
__device__ __forceinline__ unsigned row16_or_u32(unsigned v)
{
    v |= (unsigned)ORBX_DPP(v, v, 0x128, 0xf, 0xf);
    v |= (unsigned)ORBX_DPP(v, v, 0x124, 0xf, 0xf);
    v |= (unsigned)ORBX_DPP(v, v, 0x122, 0xf, 0xf);
    v |= (unsigned)ORBX_DPP(v, v, 0x121, 0xf, 0xf);
    return v;
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
    v = max(v, (unsigned)ORBX_DPP(v, 0, 0x111, 0xf, 0xf));
    v = max(v, (unsigned)ORBX_DPP(v, 0, 0x112, 0xf, 0xf));
    v = max(v, (unsigned)ORBX_DPP(v, 0, 0x114, 0xf, 0xe));
    v = max(v, (unsigned)ORBX_DPP(v, 0, 0x118, 0xf, 0xc));
    v = max(v, (unsigned)ORBX_DPP(v, 0, 0x142, 0xa, 0xf));
    v = max(v, (unsigned)ORBX_DPP(v, 0, 0x143, 0xc, 0xf));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// ---- LDS-direct load (global_load_lds_dword / _dwordx4) addressed as a wave-uniform 64-bit base plus a 32-bit lane offset: lane i's
// BYTES bytes at sbase + voff land at lds_dst + BYTES * i.  __builtin_amdgcn_global_load_lds only takes a flat per-lane pointer, for which the
// compiler forms sbase + voff with a 64-bit vector add (v_lshl_add_u64) in front of EVERY load, also when the caller advances the base on
// the scalar unit; the instruction's own `saddr` form takes the SGPR pair and the 32-bit VGPR as they are.  M0 (the LDS destination) is set
// inside the statement and put back, the compiler may keep a value of its own there.  The compiler does not count these loads: the caller
// waits with an explicit s_waitcnt vmcnt(0) before the data is read (every site had that wait already).  sbase and lds_dst must be
// wave-uniform and computed on the scalar unit (a base fresh from v_readfirstlane would need wait states in front of the load).
// Used by the tile loads of k_fast / k_fast2, where it measured (k_fast is bound by vector issue, and the compiler also held the zeroing
// of the score tile behind the builtin's loads).  k_desc's patch loads and k_resize's row groups (the dwordx4 form) measured 0.5 % slower
// with it -- neither is bound by vector issue, and the four scalar instructions around each load lengthen the wave -- and keep the
// builtin ("Where the next percent is").  -DORBX_LDS_LOAD_FLAT: the builtin form here too, for A/B timing.
template <int BYTES>
__device__ __forceinline__ void lds_load_sbase(const uint8_t *sbase, unsigned voff, const void *lds_dst)
{
    static_assert(BYTES == 4 || BYTES == 16, "global_load_lds_dword / global_load_lds_dwordx4");
#ifdef ORBX_LDS_LOAD_FLAT
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t *>(sbase + voff),
                                     reinterpret_cast<uint32_t *>(const_cast<void *>(lds_dst)), BYTES, 0, 0);
#elif defined(__HIP_DEVICE_COMPILE__)
    const unsigned lds = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)lds_dst;
    unsigned keep;
    if constexpr (BYTES == 4)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds) : "memory");
#endif
}

// exclusive scan of one value per thread over an NT-thread workgroup (NT = 256 or 1024); s_w = NT / 64 ints of LDS
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int *total, int *s_w)
{
    int t_ = threadIdx.x;
    asm volatile("" : "+v"(t_));        // (opaque: &s_w[wv] is not kept in a register between calls -- in k_bow2 it went to scratch)
    const int lane = t_ & (WAVE - 1), wv = t_ >> 6;
    const int inc = wave_incl_scan(v);
    if (lane == WAVE - 1) s_w[wv] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / WAVE; i++) { const int t = s_w[i]; if (i < wv) base += t; tot += t; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}
__device__ __forceinline__ int block_excl_scan256(int v, int *total, int *s_w) { return block_excl_scan<256>(v, total, s_w); }

// in-place exclusive scan of an LDS array a[0..m) by an NT-thread workgroup; returns the total.
// Callers must __syncthreads() before (inputs complete); outputs are visible on return.
template <int NT>
__device__ __forceinline__ int lds_excl_scan_nt(int *a, int m, int *s_w)
{
    const int per = (m + NT - 1) / NT;
    const int beg = threadIdx.x * per;
    const int end = beg + per < m ? beg + per : m;
    int s = 0;
    for (int i = beg; i < end; i++) s += a[i];
    int tot;
    int run = block_excl_scan<NT>(s, &tot, s_w);
    for (int i = beg; i < end; i++) { int t = a[i]; a[i] = run; run += t; }
    __syncthreads();
    return tot;
}
__device__ __forceinline__ int lds_excl_scan(int *a, int m, int *s_w) { return lds_excl_scan_nt<256>(a, m, s_w); }

// floor(i / d) for 0 <= i < 2^16, 1 <= d < 2^16 by multiply-high (d == 1 would overflow the magic)
struct FastDiv {
    unsigned magic; bool one;
    __device__ __forceinline__ explicit FastDiv(int d) : magic(0xFFFFFFFFu / (unsigned)d + 1u), one(d == 1) {}
    __device__ __forceinline__ int div(int i) const { return one ? i : (int)__umulhi((unsigned)i, magic); }
};

__device__ __forceinline__ int reflect101(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

// cv::fastAtan2 (OpenCV 3.x polynomial): fp32, one rounding per operation
// (the translation unit is compiled with -ffp-contract=off).
__device__ __forceinline__ float dev_fast_atan2(float y, float x)
{
    const float p1 = 0.9997878412794807f * (float)(180 / 3.14159265358979323846);
    const float p3 = -0.3258083974640975f * (float)(180 / 3.14159265358979323846);
    const float p5 = 0.1555786518463281f * (float)(180 / 3.14159265358979323846);
    const float p7 = -0.04432655554792128f * (float)(180 / 3.14159265358979323846);
    const float eps = (float)2.2204460492503131e-16;
    // one division and one polynomial for both octant cases: min / (max + eps) is the quotient either branch of the
    // reference forms (ax >= ay: ay / (ax + eps), else ax / (ay + eps)); same operations on the same values
    const float ax = fabsf(x), ay = fabsf(y);
    const bool steep = !(ax >= ay);
    const float c = (steep ? ax : ay) / ((steep ? ay : ax) + eps), c2 = c * c;
    const float pl = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    float a = steep ? 90.f - pl : pl;
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// Deterministic sin/cos: fp64 Cody-Waite reduction by pi/2 + fixed minimax polynomials on
// [-pi/4, pi/4], explicit operation order, rounded once to fp32 (SURVEY.md A.6 build rule: the
// reference's libm cosf/sinf, src/ORBextractor.cc:123, is not reproducible across hosts).
__device__ __forceinline__ void dev_sincos(float angle_rad, float *s_out, float *c_out)
{
    const double INV_PIO2 = 6.36619772367581382433e-01;
    const double PIO2_HI = 1.57079632673412561417e+00;
    const double PIO2_LO = 6.07710050650619224932e-11;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    double x = (double)angle_rad;
    double k = rint(x * INV_PIO2);
    double r = (x - k * PIO2_HI) - k * PIO2_LO;
    double z = r * r;
    double ps = S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))));
    double sn = r + (r * z) * ps;
    double pc = C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))));
    double cs = (1.0 - 0.5 * z) + (z * z) * pc;
    int q = (int)((long long)k & 3);
    double s, c;
    if (q == 0) { s = sn; c = cs; }
    else if (q == 1) { s = cs; c = -sn; }
    else if (q == 2) { s = -sn; c = -cs; }
    else { s = -cs; c = sn; }
    *s_out = (float)s;
    *c_out = (float)c;
}

// cvRound on a float that is known to be small: round-half-to-even
__device__ __forceinline__ int dev_cv_round(float v) { return (int)rintf(v); }

// descriptor idx of a [.][32]-byte array (16-byte aligned) as eight words: two 16-byte loads
__device__ __forceinline__ void load_desc(const uint32_t *d, long long idx, uint32_t *out)
{
    const uint4 *s = reinterpret_cast<const uint4 *>(d + idx * 8);
    const uint4 v0 = s[0], v1 = s[1];
    out[0] = v0.x; out[1] = v0.y; out[2] = v0.z; out[3] = v0.w;
    out[4] = v1.x; out[5] = v1.y; out[6] = v1.z; out[7] = v1.w;
}

__device__ __forceinline__ int hamming256(const uint32_t *a, const uint32_t *b)
{
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d += __popc(a[i] ^ b[i]);
    return d;
}

// rotation bin of src/ORBmatcher.cc:253-258 (factor = 1/30 with HISTO_LENGTH = 30: upstream quirk kept)
__device__ __forceinline__ int rot_bin(float a1, float a2)
{
    const float factor = 1.0f / 30;
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == 30) bin = 0;
    return (unsigned)bin < 30 ? bin : 0; // the reference asserts the range; NaN / huge angles must not index out of the histogram
}

// ComputeThreeMaxima (src/ORBmatcher.cc:1687-1728) on the 30 per-bin counts, as the reference scans them: strict comparisons, so among
// equal counts the lowest bin ranks first; a bin the 0.1f tests drop (or that never was) reads -1.  One thread.
__device__ __forceinline__ void three_maxima(const int *hist, int *i1, int *i2, int *i3)
{
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < 30; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    *i1 = ind1; *i2 = ind2; *i3 = ind3;   // written once: the scan itself stays in registers
}

// ---- Frame::UndistortKeyPoints (src/Frame.cc:470-515) on one point: cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK).  Shared by
// k_undistort (orbx_frame.hip) and the resident-frame ingest (orbx_resident.hip) so that both give the same bits (-ffp-contract=off in both).
struct UndistortParams { double fx, fy, ifx, ify, cx, cy, k[5]; };

static inline UndistortParams orbx_undistort_params(float fx, float fy, float cx, float cy, const float *dist_coef, int ndist)
{
    UndistortParams p;
    p.fx = fx; p.fy = fy; p.ifx = 1. / p.fx; p.ify = 1. / p.fy; p.cx = cx; p.cy = cy;
    for (int i = 0; i < 5; i++) p.k[i] = i < ndist ? (double)dist_coef[i] : 0.0;
    return p;
}

__device__ __forceinline__ float2 dev_undistort(float2 s, const UndistortParams &p)
{
    double x = ((double)s.x - p.cx) * p.ifx, y = ((double)s.y - p.cy) * p.ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1 + ((p.k[4] * r2 + p.k[1]) * r2 + p.k[0]) * r2);
        const double dx = 2 * p.k[2] * x * y + p.k[3] * (r2 + 2 * x * x);
        const double dy = p.k[2] * (r2 + 2 * y * y) + 2 * p.k[3] * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    float2 o;
    o.x = (float)(p.fx * x + p.cx);
    o.y = (float)(p.fy * y + p.cy);
    return o;
}

// ---- Frame::ComputeStereoFromRGBD (src/Frame.cc:754-774) after Tracking::GrabImageRGBD's depth conversion (src/Tracking.cc:232-233): k_rgbd_depth
// (orbx_frame.hip) behind orbx_extract_rgbd, the pipelined RGB-D form (both orbx_hostapi.hip) and orbx_rgbd_depth_batch_device.
struct RgbdArgs {
    UndistortParams up; int undistort;   // undistort: dist_coef[0] != 0 (src/Frame.cc:472-476)
    int depth_type, apply_scale; float scale, bf;
    int w, h; long long depth_img_stride, depth_pitch;   // bytes
    const uint8_t *depth;                // device (or mapped pinned host) address of image 0
    const orbx_keypoint *kps; const int *n; int cap;      // [batch][cap] keypoints, [batch] counts
    float2 *xy_un; float *u_right, *z;   // [batch][cap]; xy_un may be null
};
// argument checks shared by the three entry points (ORBX_OK or ORBX_E_INVALID with the message set); fills everything but the pointers
int orbx_rgbd_args(const char *fn, const orbx_rgbd_params *p, int w, int h, size_t depth_pitch, RgbdArgs *a);
// enqueue k_rgbd_depth for `batch` images on stream s (no host synchronisation)
int orbx_rgbd_launch(const RgbdArgs &a, int batch, hipStream_t s);

// ---- diagnostic builds (-DORBX_DIAG, tools/diag_*.py): phase stamps and wave life spans of the extraction kernels.  A kernel's file defines
// the arrays its kernel writes (g_<kernel>_stamp; g_span_<K> for SPAN_END(K)), its stamp macro on top of STAMP_TO and the orbx_diag_* reader;
// a normal build compiles all of it to nothing.
#ifdef ORBX_DIAG
#include <string.h>
#ifdef ORBX_DIAG_SPANS_ONLY     // the summed phase stamps perturb the waves they measure (an atomic per phase): this build keeps the spans only
                                // (and k_fast's per-wave phase log, orbx_fast.hip)
#define STAMP_TO(arr, k) do { (void)_t_prev; } while (0)
#else
#define STAMP_TO(arr, k) do { const unsigned long long _t = __builtin_amdgcn_s_memtime(); \
    if (threadIdx.x == 0) atomicAdd(&arr[((blockIdx.x * 131 + blockIdx.y) & 4095) * 8 + (k)], _t - _t_prev); _t_prev = _t; } while (0)
#endif
// wall-clock life of every wave of a launch (s_memrealtime, 100 MHz): (start, end) in the wave's own slot -- no atomics, nothing shared
#define SPAN_SLOTS 16384
#define SPAN_BEGIN() const unsigned _sp0 = (unsigned)__builtin_amdgcn_s_memrealtime()
#define SPAN_END(K) do { if ((threadIdx.x & 63) == 0) { const unsigned _id = blockIdx.x + gridDim.x * blockIdx.y; \
    if (_id < SPAN_SLOTS) g_span_##K[_id] = make_uint2(_sp0, (unsigned)__builtin_amdgcn_s_memrealtime()); } } while (0)
// host readers: the phase sums over a stamp array's 4096 slots -> out[8]; one span array -> out[SPAN_SLOTS][2]
static inline int orbx_diag_stamp_sums(const void *sym, unsigned long long *out, int reset)
{
    ORBX_HIP(hipDeviceSynchronize());
    static unsigned long long h[4096 * 8];
    ORBX_HIP(hipMemcpyFromSymbol(h, sym, sizeof h));
    for (int k = 0; k < 8; k++) { out[k] = 0; for (int i = 0; i < 4096; i++) out[k] += h[i * 8 + k]; }
    if (reset) { memset(h, 0, sizeof h); ORBX_HIP(hipMemcpyToSymbol(sym, h, sizeof h)); }
    return ORBX_OK;
}
static inline int orbx_diag_span_read(const void *sym, unsigned *out, int reset)
{
    ORBX_HIP(hipMemcpyFromSymbol(out, sym, sizeof(uint2) * SPAN_SLOTS));
    if (reset) {
        static uint2 z[SPAN_SLOTS];
        ORBX_HIP(hipMemcpyToSymbol(sym, z, sizeof z));
    }
    return ORBX_OK;
}
#else
#define SPAN_BEGIN() do { } while (0)
#define SPAN_END(K) do { } while (0)
#endif

// mfma_i8.hip -- what a v_mfma_i32_16x16x64_i8 costs a SIMD, for pricing k_desc's matrix-core row pass:
//   1. cycles per MFMA, back to back from one wave of the SIMD (four independent accumulators, and one dependent chain);
//   2. the rate of a fast-class VALU stream (v_xor_b32) issued by three OTHER waves of the same SIMD, with the MFMA wave idle and with
//      it issuing MFMAs back to back: the difference is the vector issue an MFMA takes from the rest of the SIMD.
// One workgroup of 16 waves per CU; waves 0..3 are the MFMA waves, waves 4..15 the VALU waves.  Every wave times itself with s_memtime
// (shader clock cycles) and reports the SIMD it ran on (HW_ID), by which the host groups the figures.
//   hipcc --offload-arch=gfx950 -O3 -o mfma_i8 mfma_i8.hip && ./mfma_i8
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
typedef int i32x4 __attribute__((ext_vector_type(4)));

#define MFMA_ITERS 8192     // x 8 MFMAs
#define VALU_ITERS 512      // x 32 v_xor_b32
#define BLOCKS 256

struct Rec { unsigned long long cycles; unsigned simd, role, sink, pad; };

// MODE bit 0: the MFMA waves run; bit 1: the VALU waves run; bit 2: the MFMAs form one dependent chain
template <int MODE>
__global__ __launch_bounds__(1024) void k_mix(Rec *out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    Rec r; r.simd = (hwid >> 4) & 3; r.role = wave < 4; r.sink = 0; r.pad = 0; r.cycles = 0;
    __syncthreads();
    if (wave < 4) {
        if (MODE & 1) {
            i32x4 a = { lane, lane * 3, lane ^ 5, 7 }, b = { 1, lane, 2, lane + 9 };
            i32x4 c0 = { 0, 0, 0, 0 }, c1 = c0, c2 = c0, c3 = c0;
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
            for (int it = 0; it < MFMA_ITERS; it++) {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (MODE & 4) {
                        c0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c0, 0, 0, 0);
                        c0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c0, 0, 0, 0);
                        c0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c0, 0, 0, 0);
                        c0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c0, 0, 0, 0);
                    } else {
                        c0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c1, 0, 0, 0);
                        c2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c2, 0, 0, 0);
                        c3 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c3, 0, 0, 0);
                    }
                }
            }
            const i32x4 s = c0 + c1 + c2 + c3;
            r.sink = (unsigned)(s.x + s.y + s.z + s.w);
            asm volatile("" :: "v"(r.sink));
            r.cycles = __builtin_amdgcn_s_memtime() - t0;
        }
    } else if (MODE & 2) {
        unsigned x[16];
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = threadIdx.x * 17 + i;
        const unsigned b = threadIdx.x ^ 5;
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        for (int it = 0; it < VALU_ITERS; it++) {
#pragma unroll
            for (int k = 0; k < 2; k++)
#pragma unroll
                for (int i = 0; i < 16; i++) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(x[i]) : "v"(b));
        }
        unsigned s = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) s += x[i];
        r.sink = s;
        asm volatile("" :: "v"(r.sink));
        r.cycles = __builtin_amdgcn_s_memtime() - t0;
    }
    if (lane == 0) out[blockIdx.x * 16 + wave] = r;
}

template <int MODE>
static void run(const char *name, Rec *d_out)
{
    std::vector<Rec> h(BLOCKS * 16);
    hipLaunchKernelGGL(k_mix<MODE>, dim3(BLOCKS), dim3(1024), 0, 0, d_out);   // warm-up
    CHECK(hipDeviceSynchronize());
    hipLaunchKernelGGL(k_mix<MODE>, dim3(BLOCKS), dim3(1024), 0, 0, d_out);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h.data(), d_out, h.size() * sizeof(Rec), hipMemcpyDeviceToHost));
    // The hardware does not place wave w on SIMD w % 4, so the waves are grouped by the SIMD they report: a group is the nm MFMA waves and
    // nv VALU waves of one workgroup on one SIMD; the VALU figure of a group is its slowest VALU wave's time over the group's nv x 32 x
    // VALU_ITERS instructions, the MFMA figure a wave's time over nm x 8 x MFMA_ITERS.  One line per (nm, nv) that occurs.
    printf("%s\n", name);
    for (int nm = 0; nm <= 4; nm++)
        for (int nv = 0; nv <= 12; nv++) {
            std::vector<double> m, v;
            for (int blk = 0; blk < BLOCKS; blk++)
                for (unsigned simd = 0; simd < 4; simd++) {
                    int cm = 0, cv = 0;
                    unsigned long long tm = 0, tv = 0;
                    for (int w = 0; w < 16; w++) {
                        const Rec &r = h[blk * 16 + w];
                        if (r.simd != simd) continue;
                        if (r.role) { cm++; tm = std::max(tm, r.cycles); } else { cv++; tv = std::max(tv, r.cycles); }
                    }
                    if (cm != nm || cv != nv) continue;
                    if ((MODE & 1) && cm) m.push_back((double)tm / (cm * 8.0 * MFMA_ITERS));
                    if ((MODE & 2) && cv) v.push_back((double)tv / (cv * 32.0 * VALU_ITERS));
                }
            if (m.empty() && v.empty()) continue;
            std::sort(m.begin(), m.end()); std::sort(v.begin(), v.end());
            printf("  SIMDs with %d MFMA + %2d VALU waves: %4zu", nm, nv, std::max(m.size(), v.size()));
            if (!m.empty()) printf("  cycles/MFMA min %.2f med %.2f max %.2f", m.front(), m[m.size() / 2], m.back());
            if (!v.empty()) printf("  cycles/v_xor min %.3f med %.3f max %.3f", v.front(), v[v.size() / 2], v.back());
            printf("\n");
        }
}

int main()
{
    Rec *d_out;
    CHECK(hipMalloc(&d_out, BLOCKS * 16 * sizeof(Rec)));
    run<1>("mfma x4 independent", d_out);
    run<5>("mfma dependent chain", d_out);
    run<2>("valu alone (3 waves)", d_out);
    run<3>("valu + mfma independent", d_out);
    run<7>("valu + mfma dependent", d_out);
    return 0;
}

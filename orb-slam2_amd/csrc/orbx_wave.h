// orbx_wave.h — the wave64 helpers that more than one kernel file uses: the wave-level barrier of the LDS-resident Jacobi routines (k_pnp,
// k_mono_hyp), the xor butterflies that close a sum or a maximum over the 64 lanes, and the double dot product of float triples that
// restates a cv::Mat product (k_sim3, k_triangulate, k_mono_*).  Device code only; every function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>

// what one lane wrote to LDS, every lane of the wave reads behind this
static __device__ __forceinline__ void wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the xor butterfly over strides 32 .. 1: both partners add the same two numbers (a + b == b + a), so every lane ends with the same bits
template <typename T>
static __device__ __forceinline__ T wave_sum(T v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

static __device__ __forceinline__ double wave_max(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

// (double) a . b, left to right
static __device__ __forceinline__ double dotd(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}

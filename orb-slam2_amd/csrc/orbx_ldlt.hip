// orbx_ldlt.hip — the contract's dense LDL^T (include/orbx.h: orbx_local_bundle_adjustment, "solve") in panels of LDLT_W columns, spread over
// many workgroups.  It computes what k_lba_solve (orbx_lba.hip) computes, bit for bit: every entry (i, k) of the lower triangle loses
// (l_ij * l_kj) * d_j in ascending j, every y_i loses l_ij * y_j in ascending j, every x_i loses l_ji * x_j in descending j, each operation
// rounded on its own (fp64 on the plain VALU: the f64 MFMA fuses).  A blocked right-looking factorisation keeps that order because a panel's
// columns reach the trailing matrix one after the other.  No atomics, no cooperative launch: the launch sequence is a function of n alone,
// and a launch after a failed pivot finds *ok == 0 and does nothing.
//
// Per panel [j0, j0 + w):   k_ldlt_diag   one workgroup factors the w x w diagonal block in LDS, its part of y carried along
//                           k_ldlt_rows   a thread per row below the block: the row's w entries of L, in registers, and its y
//                           k_ldlt_trail  a workgroup per 64 x 64 tile of the trailing lower triangle, the two L panels and d staged in LDS
// then                      k_ldlt_scale  y_i / d_i
// and per panel, last first: k_ldlt_back  every workgroup solves the panel's w unknowns in LDS (they are final once the later panels are
//                                         through) and takes them out of its 256 rows above the panel; workgroup 0 writes them to x
#include "orbx_ldlt.h"

namespace {

constexpr int W = LDLT_W, T = 64;   // panel width, trailing tile
// the thread layouts below are written for these two: an entry of the 32 x 32 block per thread of 1024 (tid >> 5, tid & 31), the block staged
// by a 64-thread workgroup, a 64 x 64 tile as 16 x 16 threads of 4 x 4 entries.  Another width needs them rewritten, not a new constant.
static_assert(W == 32 && T == 64, "orbx_ldlt.hip: the kernels' thread layouts hold for W = 32, T = 64 only");

__global__ __launch_bounds__(1024) void k_ldlt_diag(double *S, double *y, double *ok, int n, int j0)
{
    __shared__ double a[W][W + 1];
    __shared__ double ys[W];
    const int tid = threadIdx.x, i = tid >> 5, k = tid & 31, w = n - j0 < W ? n - j0 : W;
    if (j0 > 0 && *ok == 0.0) return;
    const bool in = i < w && k <= i;
    a[i][k] = in ? S[(size_t)(j0 + i) * n + j0 + k] : 0.0;
    if (tid < w) ys[tid] = y[j0 + tid];
    __syncthreads();
    for (int j = 0; j < w; j++) {
        const double d = a[j][j];
        if (!(d > 0.0)) {   // the same value for every thread: the whole workgroup leaves
            if (tid == 0) *ok = 0.0;
            return;
        }
        if (k == j && i > j && i < w) {
            const double li = a[i][j] / d;
            a[i][j] = li;
            ys[i] -= li * ys[j];
        }
        __syncthreads();
        if (in && k > j) a[i][k] -= (a[i][j] * a[k][j]) * d;
        __syncthreads();
    }
    if (in) S[(size_t)(j0 + i) * n + j0 + k] = a[i][k];
    if (tid < w) y[j0 + tid] = ys[tid];
    if (j0 == 0 && tid == 0) *ok = 1.0;
}

// only launched below a full panel (a panel narrower than W is the last one and has no row below it)
__global__ __launch_bounds__(64) void k_ldlt_rows(double *S, double *y, const double *ok, int n, int j0)
{
    __shared__ double Ld[W][W + 1];
    __shared__ double ds[W], ys[W];
    const int tid = threadIdx.x, i = j0 + W + blockIdx.x * 64 + tid;
    if (*ok == 0.0) return;
    for (int q = tid; q < W * W; q += 64) Ld[q >> 5][q & 31] = S[(size_t)(j0 + (q >> 5)) * n + j0 + (q & 31)];
    if (tid < W) { ds[tid] = S[(size_t)(j0 + tid) * n + j0 + tid]; ys[tid] = y[j0 + tid]; }
    __syncthreads();
    if (i >= n) return;
    double *row = S + (size_t)i * n + j0;
    double r[W], yi = y[i];
#pragma unroll
    for (int c = 0; c < W; c++) r[c] = row[c];
#pragma unroll
    for (int j = 0; j < W; j++) {
        const double d = ds[j], lj = r[j] / d;
        r[j] = lj;
        yi -= lj * ys[j];
#pragma unroll
        for (int k = j + 1; k < W; k++) r[k] -= (lj * Ld[k][j]) * d;
    }
#pragma unroll
    for (int c = 0; c < W; c++) row[c] = r[c];
    y[i] = yi;
}

// workgroup b is tile (ti, tk <= ti) of the trailing lower triangle, b = ti (ti + 1) / 2 + tk; a thread holds 4 x 4 entries, rows ty + 16 a,
// columns tx + 16 b
__global__ __launch_bounds__(256) void k_ldlt_trail(double *S, const double *ok, int n, int j0)
{
    __shared__ double Li[W][T + 1], Lk[W][T + 1];
    __shared__ double ds[W];
    if (*ok == 0.0) return;
    const int tid = threadIdx.x, b = blockIdx.x;
    int ti = (int)((sqrt(8.0 * b + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > b) ti--;
    while ((ti + 1) * (ti + 2) / 2 <= b) ti++;
    const int tk = b - ti * (ti + 1) / 2;
    const int i0 = j0 + W + T * ti, k0 = j0 + W + T * tk;
    for (int q = tid; q < T * W; q += 256) {
        const int r = q >> 5, j = q & 31;
        Li[j][r] = i0 + r < n ? S[(size_t)(i0 + r) * n + j0 + j] : 0.0;
        Lk[j][r] = k0 + r < n ? S[(size_t)(k0 + r) * n + j0 + j] : 0.0;
    }
    if (tid < W) ds[tid] = S[(size_t)(j0 + tid) * n + j0 + tid];
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int i = i0 + ty + 16 * a, k = k0 + tx + 16 * c;
            acc[a][c] = (i < n && k <= i) ? S[(size_t)i * n + k] : 0.0;
        }
#pragma unroll 4
    for (int j = 0; j < W; j++) {
        const double d = ds[j];
        double li[4], lk[4];
#pragma unroll
        for (int a = 0; a < 4; a++) { li[a] = Li[j][ty + 16 * a]; lk[a] = Lk[j][tx + 16 * a]; }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[a][c] -= (li[a] * lk[c]) * d;
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int i = i0 + ty + 16 * a, k = k0 + tx + 16 * c;
            if (i < n && k <= i) S[(size_t)i * n + k] = acc[a][c];
        }
}

__global__ __launch_bounds__(256) void k_ldlt_scale(const double *S, double *y, const double *ok, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (*ok == 0.0 || i >= n) return;
    y[i] = y[i] / S[(size_t)i * n + i];
}

__global__ __launch_bounds__(256) void k_ldlt_back(const double *S, double *y, double *x, const double *ok, int n, int j0)
{
    __shared__ double xs[W];
    const int tid = threadIdx.x, w = n - j0 < W ? n - j0 : W;
    if (*ok == 0.0) return;
    if (tid < w) xs[tid] = y[j0 + tid];
    __syncthreads();
    for (int j = w - 1; j >= 1; j--) {
        if (tid < j) xs[tid] -= S[(size_t)(j0 + j) * n + j0 + tid] * xs[j];
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid < w) x[j0 + tid] = xs[tid];
    const int i = blockIdx.x * 256 + tid;
    if (i >= j0) return;
    double yi = y[i];
    for (int j = w - 1; j >= 0; j--) yi -= S[(size_t)(j0 + j) * n + i] * xs[j];
    y[i] = yi;
}

}   // namespace

void orbx_ldlt_panel_launch(double *S, double *y, double *x, double *ok, int n, hipStream_t s)
{
    for (int j0 = 0; j0 < n; j0 += W) {
        hipLaunchKernelGGL(k_ldlt_diag, dim3(1), dim3(1024), 0, s, S, y, ok, n, j0);
        const int below = n - (j0 + W);
        if (below <= 0) break;
        const int nt = (below + T - 1) / T;
        hipLaunchKernelGGL(k_ldlt_rows, dim3((below + 63) / 64), dim3(64), 0, s, S, y, ok, n, j0);
        hipLaunchKernelGGL(k_ldlt_trail, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, S, ok, n, j0);
    }
    hipLaunchKernelGGL(k_ldlt_scale, dim3((n + 255) / 256), dim3(256), 0, s, S, y, ok, n);
    for (int j0 = (n - 1) / W * W; j0 >= 0; j0 -= W)
        hipLaunchKernelGGL(k_ldlt_back, dim3(j0 ? (j0 + 255) / 256 : 1), dim3(256), 0, s, S, y, x, ok, n, j0);
}

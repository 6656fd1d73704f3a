// orbx_ldlt_env.hip — the panel LDL^T of orbx_ldlt.hip on an ENVELOPE (skyline) matrix: row i stores its columns first[i] .. i only
// (orbx_ldlt_env.h), and the factorisation fills nothing to the left of a row's first stored column.  In the same row order as the dense
// solver it performs, per stored entry, exactly the dense solver's operations in the dense solver's order: (i, k) loses (l_ij * l_kj) * d_j
// in ascending j, y_i loses l_ij * y_j in ascending j, x_i loses l_ji * x_j in descending j, each operation rounded on its own (fp64 on the
// plain VALU).  What it leaves out are the terms whose l is an entry outside the envelope, which the dense solver holds as an exact zero:
// x - (l * 0) * d.  So the values are the dense solver's; only a -0 that the dense solver's x - (+-0) would turn into +0 can stay.  No
// atomics, no cooperative launch: the launch sequence is a function of the structure alone, and a launch after a failed pivot finds
// *ok == 0 and does nothing.
//
// The host's symbolic step (orbx_ldlt_env_plan) lists per panel [j0, j0 + W) its ACTIVE rows: i >= j0 + W with first[i] <= j0, ascending.
// first[] is a multiple of W, so an active row holds all W columns of the panel, and the W x W diagonal block is always stored.  If i > k
// are both active in a panel then first[i] <= j0 < k: the trailing entry (i, k) is always stored, and the trailing update never writes
// outside the envelope.
//
// Per panel:                 k_env_diag   one workgroup factors the diagonal block in LDS, its part of y carried along
//                            k_env_rows   a thread per active row: the row's W entries of L, in registers, and its y
//                            k_env_trail  a workgroup per 64 x 64 tile of (active rows) x (active rows), the two L panels and d in LDS
// then                       k_env_scale  y_i / d_i
// and per panel, last first: k_env_back   as k_ldlt_back; a row i above the panel loses S[j0 + j][i] * x[j] only where i >= first[j0 + j],
//                                         and only the rows from the panel's smallest first[] on are launched
// The LDS layouts are the dense kernels'; the tile kernel adds the tile's row bases and column numbers, since active rows are not
// contiguous in memory.
#include "orbx_ldlt_env.h"

namespace {

constexpr int W = LDLT_W, T = 64;
static_assert(W == 32 && T == 64, "orbx_ldlt_env.hip: the kernels' thread layouts hold for W = 32, T = 64 only");

// where column 0 of row i would lie: entry (i, j) is S[env_base(i) + j] for first[i] <= j <= i
__device__ __forceinline__ long long env_base(const int64_t *rowptr, const int32_t *first, int i) { return (long long)rowptr[i] - first[i]; }

__global__ __launch_bounds__(1024) void k_env_diag(double *S, const int64_t *rowptr, const int32_t *first, double *y, double *ok, int n, int j0)
{
    __shared__ double a[W][W + 1];
    __shared__ double ys[W];
    const int tid = threadIdx.x, i = tid >> 5, k = tid & 31, w = n - j0 < W ? n - j0 : W;
    if (j0 > 0 && *ok == 0.0) return;
    const bool in = i < w && k <= i;
    const long long at = in ? env_base(rowptr, first, j0 + i) + j0 + k : 0;   // first[j0 + i] <= j0: the block is stored
    a[i][k] = in ? S[at] : 0.0;
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
    if (in) S[at] = a[i][k];
    if (tid < w) y[j0 + tid] = ys[tid];
    if (j0 == 0 && tid == 0) *ok = 1.0;
}

// act: the panel's na active rows.  Only launched with na > 0, so the panel is a full one (there is a row at or below j0 + W).
__global__ __launch_bounds__(64) void k_env_rows(double *S, const int64_t *rowptr, const int32_t *first, const int32_t *act, int na, double *y,
                                                 const double *ok, int j0)
{
    __shared__ double Ld[W][W + 1];
    __shared__ double ds[W], ys[W];
    const int tid = threadIdx.x, q0 = blockIdx.x * 64 + tid;
    if (*ok == 0.0) return;
    for (int q = tid; q < W * W; q += 64) Ld[q >> 5][q & 31] = (q & 31) <= (q >> 5) ? S[env_base(rowptr, first, j0 + (q >> 5)) + j0 + (q & 31)] : 0.0;
    if (tid < W) { ds[tid] = S[env_base(rowptr, first, j0 + tid) + j0 + tid]; ys[tid] = y[j0 + tid]; }
    __syncthreads();
    if (q0 >= na) return;
    const int i = act[q0];
    double *row = S + (env_base(rowptr, first, i) + j0);
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

// workgroup b is tile (ti, tk <= ti) of the active list x the active list, b = ti (ti + 1) / 2 + tk; a thread holds 4 x 4 entries, list
// positions T ti + ty + 16 a by T tk + tx + 16 c.  The list ascends, so position order is row order: (i, k) is of the lower triangle where
// k's position is not above i's, and it is stored (the file's head).
__global__ __launch_bounds__(256) void k_env_trail(double *S, const int64_t *rowptr, const int32_t *first, const int32_t *act, int na, const double *ok,
                                                   int j0)
{
    __shared__ double Li[W][T + 1], Lk[W][T + 1];
    __shared__ double ds[W];
    __shared__ long long bi[T], bk[T];   // env_base of the tile's rows; -1 beyond the list
    __shared__ int ck[T];                // the row numbers of the tile's k side: the columns written
    if (*ok == 0.0) return;
    const int tid = threadIdx.x, b = blockIdx.x;
    int ti = (int)((sqrt(8.0 * b + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > b) ti--;
    while ((ti + 1) * (ti + 2) / 2 <= b) ti++;
    const int tk = b - ti * (ti + 1) / 2;
    const int pi0 = T * ti, pk0 = T * tk;
    if (tid < T) {
        const int pi = pi0 + tid, pk = pk0 + tid;
        bi[tid] = pi < na ? env_base(rowptr, first, act[pi]) : -1;
        const int k = pk < na ? act[pk] : -1;
        ck[tid] = k;
        bk[tid] = k >= 0 ? env_base(rowptr, first, k) : -1;
    }
    if (tid >= 64 && tid < 64 + W) ds[tid - 64] = S[env_base(rowptr, first, j0 + tid - 64) + j0 + tid - 64];
    __syncthreads();
    for (int q = tid; q < T * W; q += 256) {
        const int r = q >> 5, j = q & 31;
        Li[j][r] = bi[r] >= 0 ? S[bi[r] + j0 + j] : 0.0;
        Lk[j][r] = bk[r] >= 0 ? S[bk[r] + j0 + j] : 0.0;
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int ri = ty + 16 * a, rk = tx + 16 * c;
            acc[a][c] = (pi0 + ri < na && pk0 + rk <= pi0 + ri) ? S[bi[ri] + ck[rk]] : 0.0;
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
            const int ri = ty + 16 * a, rk = tx + 16 * c;
            if (pi0 + ri < na && pk0 + rk <= pi0 + ri) S[bi[ri] + ck[rk]] = acc[a][c];
        }
}

__global__ __launch_bounds__(256) void k_env_scale(const double *S, const int64_t *rowptr, const int32_t *first, double *y, const double *ok, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (*ok == 0.0 || i >= n) return;
    y[i] = y[i] / S[env_base(rowptr, first, i) + i];
}

// lo: the smallest first[] of the panel's rows (a multiple of W, <= j0); the grid covers the rows lo .. j0 - 1, one workgroup at the least
__global__ __launch_bounds__(256) void k_env_back(const double *S, const int64_t *rowptr, const int32_t *first, double *y, double *x, const double *ok,
                                                  int n, int j0, int lo)
{
    __shared__ double xs[W];
    __shared__ long long bs[W];
    __shared__ int fs[W];
    const int tid = threadIdx.x, w = n - j0 < W ? n - j0 : W;
    if (*ok == 0.0) return;
    if (tid < w) { xs[tid] = y[j0 + tid]; bs[tid] = env_base(rowptr, first, j0 + tid); fs[tid] = first[j0 + tid]; }
    __syncthreads();
    for (int j = w - 1; j >= 1; j--) {
        if (tid < j) xs[tid] -= S[bs[j] + j0 + tid] * xs[j];
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid < w) x[j0 + tid] = xs[tid];
    const int i = lo + blockIdx.x * 256 + tid;
    if (i >= j0) return;
    double yi = y[i];
    for (int j = w - 1; j >= 0; j--)
        if (i >= fs[j]) yi -= S[bs[j] + i] * xs[j];
    y[i] = yi;
}

}   // namespace

void orbx_ldlt_env_shape(int n, const int32_t *first, LdltEnvPlan *plan)
{
    LdltEnvPlan &P = *plan;
    P = LdltEnvPlan();
    P.n = n;
    P.first.resize(n);
    P.rowptr.resize((size_t)n + 1);
    P.rowptr[0] = 0;
    for (int i = 0; i < n; i++) {
        const int f = first[i] < 0 ? 0 : (first[i] > i ? i : first[i]);
        P.first[i] = f / W * W;
        P.rowptr[i + 1] = P.rowptr[i] + (i - P.first[i] + 1);
    }
    P.entries = P.rowptr[n];
}

void orbx_ldlt_env_plan(int n, const int32_t *first, LdltEnvPlan *plan)
{
    orbx_ldlt_env_shape(n, first, plan);
    LdltEnvPlan &P = *plan;
    const int panels = (n + W - 1) / W;
    // row i is active in the panels first[i] / W .. i / W - 1: those that lie wholly in front of its diagonal block's panel
    P.aoff.assign((size_t)panels + 1, 0);
    P.lo.resize(panels);
    for (int p = 0; p < panels; p++) P.lo[p] = p * W;
    for (int i = 0; i < n; i++) {
        for (int p = P.first[i] / W; p < i / W; p++) P.aoff[p + 1]++;
        if (P.first[i] < P.lo[i / W]) P.lo[i / W] = P.first[i];
    }
    for (int p = 0; p < panels; p++) P.aoff[p + 1] += P.aoff[p];
    P.act.resize(P.aoff[panels] ? P.aoff[panels] : 1);
    std::vector<int32_t> fill(P.aoff.begin(), P.aoff.end() - 1);
    for (int i = 0; i < n; i++)   // ascending i: every list ascends
        for (int p = P.first[i] / W; p < i / W; p++) P.act[fill[p]++] = i;
}

void orbx_ldlt_env_launch(double *S, double *y, double *x, double *ok, const LdltEnvPlan &P, hipStream_t s)
{
    const int n = P.n;
    const int64_t *rp = P.d_rowptr;
    const int32_t *fi = P.d_first;
    for (int j0 = 0, p = 0; j0 < n; j0 += W, p++) {
        hipLaunchKernelGGL(k_env_diag, dim3(1), dim3(1024), 0, s, S, rp, fi, y, ok, n, j0);
        const int na = P.aoff[p + 1] - P.aoff[p];
        if (na == 0) continue;
        const int32_t *act = P.d_act + P.aoff[p];
        const int nt = (na + T - 1) / T;
        hipLaunchKernelGGL(k_env_rows, dim3((na + 63) / 64), dim3(64), 0, s, S, rp, fi, act, na, y, ok, j0);
        hipLaunchKernelGGL(k_env_trail, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, S, rp, fi, act, na, ok, j0);
    }
    hipLaunchKernelGGL(k_env_scale, dim3((n + 255) / 256), dim3(256), 0, s, S, rp, fi, y, ok, n);
    for (int j0 = (n - 1) / W * W; j0 >= 0; j0 -= W) {
        const int lo = P.lo[j0 / W], above = j0 - lo;
        hipLaunchKernelGGL(k_env_back, dim3(above ? (above + 255) / 256 : 1), dim3(256), 0, s, S, rp, fi, y, x, ok, n, j0, lo);
    }
}

// ---------------------------------------------------------------- include/orbx.h: orbx_debug_ldlt_solve_envelope

extern "C" int orbx_debug_ldlt_solve_envelope(int device, int n, const int32_t *first, const double *S, const double *b, double *x, int *ok)
{
    const char *who = "orbx_debug_ldlt_solve_envelope";
    if (!first || !S || !b || !x || !ok) { orbx_set_error("%s: a NULL argument", who); return ORBX_E_INVALID; }
    if (n < 1) { orbx_set_error("%s: n = %d", who, n); return ORBX_E_INVALID; }
    if (n > 6 * 2048) { orbx_set_error("%s: n = %d beyond %d", who, n, 6 * 2048); return ORBX_E_CAPACITY; }
    for (int i = 0; i < n; i++)
        if (first[i] < 0 || first[i] > i) { orbx_set_error("%s: first[%d] = %d outside 0 .. %d", who, i, first[i], i); return ORBX_E_INVALID; }
    LdltEnvPlan P;
    orbx_ldlt_env_plan(n, first, &P);
    int rc;
    CallCtx *c;
    if ((rc = orbx_call_ctx(device, &c))) return rc;
    const size_t N = (size_t)n;
    BlobCursor bl = { nullptr, nullptr, 0 };
    const size_t o_S = bl.take(8 * (size_t)P.entries), o_b = bl.take(8 * N), o_x = bl.take(8 * N), o_rowptr = bl.take(8 * P.rowptr.size()),
                 o_first = bl.take(4 * P.first.size()), o_act = bl.take(4 * P.act.size());
    BlobCursor w = { nullptr, nullptr, 0 };
    const size_t w_status = w.take(64), w_x = w.take(8 * N);
    if ((rc = call_reserve(c, bl.o, w.o, w.o))) return rc;
    uint8_t *h = c->h_blob;
    double *hS = (double *)(h + o_S);
    for (size_t i = 0; i < N; i++) memcpy(hS + P.rowptr[i], S + i * N + P.first[i], 8 * (i - P.first[i] + 1));
    memcpy(h + o_b, b, 8 * N); memcpy(h + o_x, x, 8 * N);
    memcpy(h + o_rowptr, P.rowptr.data(), 8 * P.rowptr.size()); memcpy(h + o_first, P.first.data(), 4 * P.first.size());
    memcpy(h + o_act, P.act.data(), 4 * P.act.size());
    if ((rc = call_upload(c, bl.o))) return rc;
    P.d_rowptr = (const int64_t *)(c->d_blob + o_rowptr); P.d_first = (const int32_t *)(c->d_blob + o_first); P.d_act = (const int32_t *)(c->d_blob + o_act);
    double *status = (double *)(c->d_work + w_status), *dx = (double *)(c->d_work + w_x);
    ORBX_HIP(hipMemsetAsync(status, 0, 64, c->stream));
    ORBX_HIP(hipMemcpyAsync(dx, c->d_blob + o_x, 8 * N, hipMemcpyDeviceToDevice, c->stream));
    orbx_ldlt_env_launch((double *)(c->d_blob + o_S), (double *)(c->d_blob + o_b), dx, status + 3, P, c->stream);
    if ((rc = call_fetch(c, w.o))) return rc;
    *ok = ((const double *)c->h_out)[3] != 0.0;
    memcpy(x, (const uint8_t *)c->h_out + w_x, 8 * N);
    return ORBX_OK;
}

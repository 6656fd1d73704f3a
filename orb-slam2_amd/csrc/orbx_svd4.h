// orbx_svd4.h — the 4x4 null vector of the triangulation contract (include/orbx.h, orbx_triangulate_pairs, "SVD"): a one-sided Jacobi on
// the four columns of a float matrix, registers only.  Shared by k_triangulate (orbx_triangulate.hip) and the CheckRT of k_mono_reconstruct
// (orbx_initializer.hip); include it inside the file's anonymous namespace.
#pragma once

// One Jacobi rotation of columns i < j of A (rows i, j of At) and of the same rows of V; W holds the columns' squared norms.
__device__ __forceinline__ bool jacobi_pair(float (&Ai)[4], float (&Aj)[4], float (&Vi)[4], float (&Vj)[4], double &Wi, double &Wj)
{
    double a = Wi, b = Wj, p = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) p += (double)Ai[k] * (double)Aj[k];
    if (fabs(p) <= (double)(2.0f * 1.1920928955078125e-7f) * sqrt(a * b)) return false;
    p *= 2.0;
    const double beta = a - b, gamma = sqrt(p * p + beta * beta);
    float c, s;
    if (beta < 0.0) {
        const double delta = (gamma - beta) * 0.5;
        s = (float)sqrt(delta / gamma);
        c = (float)(p / ((gamma * (double)s) * 2.0));
    } else {
        c = (float)sqrt((gamma + beta) / (gamma * 2.0));
        s = (float)(p / ((gamma * (double)c) * 2.0));
    }
    a = 0.0; b = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float t0 = c * Ai[k] + s * Aj[k], t1 = (-s) * Ai[k] + c * Aj[k];
        Ai[k] = t0; Aj[k] = t1;
        a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
    }
    Wi = a; Wj = b;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float t0 = c * Vi[k] + s * Vj[k], t1 = (-s) * Vi[k] + c * Vj[k];
        Vi[k] = t0; Vj[k] = t1;
    }
    return true;
}

// the right singular vector of A's smallest singular value (At[i] = column i of A) -> v[4]
__device__ __forceinline__ void null_vector(float (&At)[4][4], float v[4])
{
    float V[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) { sd += (double)At[i][k] * (double)At[i][k]; V[i][k] = i == k ? 1.0f : 0.0f; }
        W[i] = sd;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
        changed |= jacobi_pair(At[0], At[1], V[0], V[1], W[0], W[1]);
        changed |= jacobi_pair(At[0], At[2], V[0], V[2], W[0], W[2]);
        changed |= jacobi_pair(At[0], At[3], V[0], V[3], W[0], W[3]);
        changed |= jacobi_pair(At[1], At[2], V[1], V[2], W[1], W[2]);
        changed |= jacobi_pair(At[1], At[3], V[1], V[3], W[1], W[3]);
        changed |= jacobi_pair(At[2], At[3], V[2], V[3], W[2], W[3]);
        if (!changed) break;
    }
    double best = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) sd += (double)At[i][k] * (double)At[i][k];
        if (i == 0 || sd <= best) {   // a tie takes the later column
            best = sd;
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = V[i][k];
        }
    }
}

// orbx_ldlt_env.h — the panel LDL^T of orbx_ldlt.hip restricted to an envelope (orbx_ldlt_env.hip): what orbx_essential.hip needs of it
#pragma once
#include "orbx_ldlt.h"
#include <vector>

// The envelope of an n x n lower triangle: row i holds its columns first[i] .. i contiguously, from S[rowptr[i]] on, so entry (i, j) is
// S[rowptr[i] + (j - first[i])].  first[i] is a multiple of LDLT_W with 0 <= first[i] <= i (the plan rounds down) and need not be monotone.
// A panel [j0, j0 + LDLT_W) is thus wholly inside a row or wholly outside it.
struct LdltEnvPlan {
    int n = 0;
    int64_t entries = 0;           // rowptr[n], the doubles of S
    std::vector<int32_t> first;    // [n], rounded
    std::vector<int64_t> rowptr;   // [n + 1]
    std::vector<int32_t> act;      // per panel the ascending list of its active rows (i >= j0 + LDLT_W with first[i] <= j0), concatenated
    std::vector<int32_t> aoff;     // [panels + 1] a panel's range of act; act.size() == entries / LDLT_W, up to the diagonal blocks
    std::vector<int32_t> lo;       // [panels] the smallest first[] among the panel's own rows: no row above it meets the panel's columns
    // the device's copies of rowptr, first and act: the caller uploads the three arrays and sets these before the first launch
    const int64_t *d_rowptr = nullptr;
    const int32_t *d_first = nullptr, *d_act = nullptr;
};

// the rounded first[], rowptr and entries alone: O(n), what a capacity check needs before anything is built
ORBX_LOCAL void orbx_ldlt_env_shape(int n, const int32_t *first, LdltEnvPlan *plan);
// the symbolic step, on the host, once per structure: orbx_ldlt_env_shape and the active lists
ORBX_LOCAL void orbx_ldlt_env_plan(int n, const int32_t *first, LdltEnvPlan *plan);

// S x = y on the stream, S packed as the plan says and factored in place, y overwritten, *ok = 1.0 and x = the solution, or *ok = 0.0 at a
// pivot that is not > 0, x left alone: orbx_ldlt_panel_launch's contract and, entry for entry of the envelope, its operations in its order
// (the operations left out are x - (l * 0) * d).  All device pointers; nothing is waited for.
ORBX_LOCAL void orbx_ldlt_env_launch(double *S, double *y, double *x, double *ok, const LdltEnvPlan &plan, hipStream_t s);

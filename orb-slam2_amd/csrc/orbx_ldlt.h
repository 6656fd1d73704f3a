// orbx_ldlt.h — the panel form of the contract's dense LDL^T (orbx_ldlt.hip), what orbx_lba.hip needs of it
#pragma once
#include "orbx_resident.h"

enum { LDLT_W = 32 };   // the panel width (orbx_debug_ldlt_panel_width)

// S x = y on the stream: S [n][n] row major, its lower triangle factored in place, y overwritten, *ok = 1.0 and x = the solution, or
// *ok = 0.0 at a pivot that is not > 0, x left alone.  All device pointers; n >= 1; nothing is waited for.
ORBX_LOCAL void orbx_ldlt_panel_launch(double *S, double *y, double *x, double *ok, int n, hipStream_t s);

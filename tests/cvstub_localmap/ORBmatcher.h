// overlay of tests/cvstub/ORBmatcher.h (placed in front of it on the include path): that header names "Frame.h" and "MapPoint.h" in quotes,
// which would find its own directory's stand-ins first; here this directory's overlays come first, then the header itself, unchanged
#include "MapPoint.h"
#include "Frame.h"
#include_next "ORBmatcher.h"

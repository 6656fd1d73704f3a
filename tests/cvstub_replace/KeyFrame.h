// overlay shim in front of tests/cvstub/KeyFrame.h: that header includes "MapPoint.h" by a quoted name, which finds the stub's own MapPoint.h
// beside it before any -I directory.  Including the overlay's MapPoint.h first settles the class (same include guard); the stub's header
// follows unchanged (the pattern of tests/cvstub_kfdb/ORBmatcher.h).
#include "MapPoint.h"
#include_next "KeyFrame.h"

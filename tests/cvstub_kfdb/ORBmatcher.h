// overlay shim in front of tests/cvstub/ORBmatcher.h: that header includes "KeyFrame.h" by a quoted name, which finds the stub's own
// KeyFrame.h beside it before any -I directory.  A translation unit that reached KeyFrame through ORBmatcher.h would then see the stub's class
// and one that named KeyFrame.h itself the overlay's: two layouts of ORB_SLAM2::KeyFrame in one program.  Including the overlay's KeyFrame.h
// first settles it (same include guard), then the stub's ORBmatcher.h follows unchanged.
#include "KeyFrame.h"
#include_next "ORBmatcher.h"

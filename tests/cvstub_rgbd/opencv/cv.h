// tests/cvstub_rgbd: put in FRONT of tests/cvstub on the include path of the RGB-D adaptor tests (tests/test_rgbd.py).  It forwards to the
// existing stub and adds the one constant the RGB-D adaptor (adapter/ORBextractor_rgbd.cc) needs: CV_16U, the element type of the TUM depth
// PNGs.  The stub Mat's elemSize() stays 1 for it, so the test driver builds its 16-bit Mats by hand (data / step / cols).
#ifndef CVSTUB_RGBD_CV_H
#define CVSTUB_RGBD_CV_H
#include "../../cvstub/opencv/cv.h"
#ifndef CV_16U
#define CV_16U 2
#endif
#endif

// stand-in for include/MapPoint.h: see RefreshStub.h
#include "RefreshStub.h"

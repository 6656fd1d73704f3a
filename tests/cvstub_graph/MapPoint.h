// stand-in for include/MapPoint.h: see GraphStub.h
#include "GraphStub.h"

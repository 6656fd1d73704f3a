// stand-in for include/KeyFrame.h: see GraphStub.h
#include "GraphStub.h"

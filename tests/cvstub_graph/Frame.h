// stand-in for include/Frame.h: see GraphStub.h
#include "GraphStub.h"

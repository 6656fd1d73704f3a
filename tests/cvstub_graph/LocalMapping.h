// stand-in for include/LocalMapping.h: see GraphStub.h
#include "GraphStub.h"

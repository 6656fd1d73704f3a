// stand-in for include/Map.h: see GraphStub.h
#include "GraphStub.h"

// stand-in for include/Map.h: see RefreshStub.h
#include "RefreshStub.h"

// stand-in for include/LocalMapping.h: see RefreshStub.h
#include "RefreshStub.h"

// stand-in for include/KeyFrame.h: see RefreshStub.h
#include "RefreshStub.h"

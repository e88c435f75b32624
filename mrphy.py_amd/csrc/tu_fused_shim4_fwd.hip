// tu_fused_shim4_fwd.hip -- K2sh at a capacity of 4 field channels: behind mrphy_blochsim_rfgr_shim_fwd
#define MRPHY_SHIM_MS 4
#include "tu_fused_shim_fwd.hpp"

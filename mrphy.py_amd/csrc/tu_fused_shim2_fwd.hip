// tu_fused_shim2_fwd.hip -- K2sh at a capacity of 2 field channels: behind mrphy_blochsim_rfgr_shim_fwd
#define MRPHY_SHIM_MS 2
#include "tu_fused_shim_fwd.hpp"

// tu_fused_shim8_fwd.hip -- K2sh at a capacity of 8 field channels: behind mrphy_blochsim_rfgr_shim_fwd
#define MRPHY_SHIM_MS 8
#include "tu_fused_shim_fwd.hpp"

// tu_fused_shim2_bwd.hip -- K2shb at a capacity of 2 field channels: behind mrphy_blochsim_rfgr_shim_bwd
#define MRPHY_SHIM_MS 2
#include "tu_fused_shim_bwd.hpp"

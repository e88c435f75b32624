// tu_fused_shim4_bwd.hip -- K2shb at a capacity of 4 field channels: behind mrphy_blochsim_rfgr_shim_bwd
#define MRPHY_SHIM_MS 4
#include "tu_fused_shim_bwd.hpp"

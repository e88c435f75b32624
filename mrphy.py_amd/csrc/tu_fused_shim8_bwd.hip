// tu_fused_shim8_bwd.hip -- K2shb at a capacity of 8 field channels: behind mrphy_blochsim_rfgr_shim_bwd
#define MRPHY_SHIM_MS 8
#include "tu_fused_shim_bwd.hpp"

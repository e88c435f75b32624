// tu_fused_jvp4_fwd.hip -- K2j at a capacity of 4 tangent directions: behind mrphy_blochsim_rfgr_jvp_fwd
#define MRPHY_JVP_MD 4
#include "tu_fused_jvp_fwd.hpp"

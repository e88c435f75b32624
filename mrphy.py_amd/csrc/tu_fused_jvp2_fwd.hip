// tu_fused_jvp2_fwd.hip -- K2j at a capacity of 2 tangent directions: behind mrphy_blochsim_rfgr_jvp_fwd
#define MRPHY_JVP_MD 2
#include "tu_fused_jvp_fwd.hpp"

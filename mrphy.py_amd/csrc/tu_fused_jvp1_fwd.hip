// tu_fused_jvp1_fwd.hip -- K2j at a capacity of 1 tangent direction: behind mrphy_blochsim_rfgr_jvp_fwd
#define MRPHY_JVP_MD 1
#include "tu_fused_jvp_fwd.hpp"

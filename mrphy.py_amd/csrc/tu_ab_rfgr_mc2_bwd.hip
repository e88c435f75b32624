// tu_ab_rfgr_mc2_bwd.hip -- K2abb-mc at a capacity of 2 transmit coils: behind mrphy_ab_rfgr_mc_bwd
#define MRPHY_AB_MC 2
#include "tu_ab_rfgr_mc_bwd.hpp"

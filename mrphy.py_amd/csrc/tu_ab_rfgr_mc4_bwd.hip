// tu_ab_rfgr_mc4_bwd.hip -- K2abb-mc at a capacity of 4 transmit coils: behind mrphy_ab_rfgr_mc_bwd
#define MRPHY_AB_MC 4
#include "tu_ab_rfgr_mc_bwd.hpp"

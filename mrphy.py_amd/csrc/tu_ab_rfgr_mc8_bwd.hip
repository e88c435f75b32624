// tu_ab_rfgr_mc8_bwd.hip -- K2abb-mc at a capacity of 8 transmit coils: behind mrphy_ab_rfgr_mc_bwd
#define MRPHY_AB_MC 8
#include "tu_ab_rfgr_mc_bwd.hpp"

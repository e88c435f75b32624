// tu_signal_consts4_bwd.hip -- the CONSTS build of K2bs at a capacity of 4 receive coils: behind mrphy_signal_rfgr_consts_bwd
#define MRPHY_RX_CAP 4
#include "tu_signal_consts_bwd.hpp"

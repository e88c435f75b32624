// tu_signal_consts1_bwd.hip -- the CONSTS build of K2bs at a capacity of 1 receive coil: behind mrphy_signal_rfgr_consts_bwd
#define MRPHY_RX_CAP 1
#include "tu_signal_consts_bwd.hpp"

// tu_signal_consts8_bwd.hip -- the CONSTS build of K2bs at a capacity of 8 receive coils: behind mrphy_signal_rfgr_consts_bwd
#define MRPHY_RX_CAP 8
#include "tu_signal_consts_bwd.hpp"

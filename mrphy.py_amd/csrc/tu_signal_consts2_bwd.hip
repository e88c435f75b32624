// tu_signal_consts2_bwd.hip -- the CONSTS build of K2bs at a capacity of 2 receive coils: behind mrphy_signal_rfgr_consts_bwd
#define MRPHY_RX_CAP 2
#include "tu_signal_consts_bwd.hpp"

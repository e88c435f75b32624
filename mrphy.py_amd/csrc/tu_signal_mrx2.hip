// tu_signal_mrx2.hip -- K2s at a capacity of 2 receive coils: launcher of mrphy_signal_rfgr_mrx_fwd
#define MRPHY_RX_CAP 2
#include "tu_signal.hpp"

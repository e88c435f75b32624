// tu_signal_mrx4.hip -- K2s at a capacity of 4 receive coils: launcher of mrphy_signal_rfgr_mrx_fwd
#define MRPHY_RX_CAP 4
#include "tu_signal.hpp"

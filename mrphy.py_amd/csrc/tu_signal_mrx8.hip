// tu_signal_mrx8.hip -- K2s at a capacity of 8 receive coils: launcher of mrphy_signal_rfgr_mrx_fwd
#define MRPHY_RX_CAP 8
#include "tu_signal.hpp"

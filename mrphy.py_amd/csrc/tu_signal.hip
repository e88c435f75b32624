// tu_signal.hip -- K2s at a capacity of 1 receive coil (or none): launcher of mrphy_signal_rfgr_fwd
#define MRPHY_RX_CAP 1
#include "tu_signal.hpp"

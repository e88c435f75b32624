// tu_ab_sequence_jvp1.hip -- Ksqj at a capacity of 1 tangent direction: behind mrphy_ab_sequence_jvp_fwd
#define MRPHY_SEQ_JVP_MD 1
#include "tu_ab_sequence_jvp.hpp"

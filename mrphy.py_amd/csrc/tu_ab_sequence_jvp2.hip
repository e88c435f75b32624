// tu_ab_sequence_jvp2.hip -- Ksqj at a capacity of 2 tangent directions: behind mrphy_ab_sequence_jvp_fwd
#define MRPHY_SEQ_JVP_MD 2
#include "tu_ab_sequence_jvp.hpp"

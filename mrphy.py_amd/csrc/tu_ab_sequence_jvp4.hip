// tu_ab_sequence_jvp4.hip -- Ksqj at a capacity of 4 tangent directions: behind mrphy_ab_sequence_jvp_fwd
#define MRPHY_SEQ_JVP_MD 4
#include "tu_ab_sequence_jvp.hpp"

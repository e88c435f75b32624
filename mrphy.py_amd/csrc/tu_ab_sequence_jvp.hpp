// tu_ab_sequence_jvp.hpp -- the body of the units tu_ab_sequence_jvp1 / 2 / 4.hip: Ksqj, Ksq with the forward-mode
// tangents of its records, at the direction capacity MRPHY_SEQ_JVP_MD (one unit per capacity, so that they compile side
// by side): behind mrphy_ab_sequence_jvp_fwd (tu_ab_sequence.hip).  Two data types, no constant type, as Ksq.
#include "host_common.hpp"

namespace {
#include "k_ab_train.hpp"
#include "k_train_signal.hpp"
#include "k_ab_sequence.hpp"
#include "k_ab_sequence_jvp.hpp"
}  // namespace

namespace mrphy_i {
template <int MD, typename T>
int run_ab_sequence_jvp(SeqJvpCall c, hipStream_t st)
{
    return launch_seq_jvp<MD, T>(c, st);
}
template int run_ab_sequence_jvp<MRPHY_SEQ_JVP_MD, float>(SeqJvpCall, hipStream_t);
template int run_ab_sequence_jvp<MRPHY_SEQ_JVP_MD, double>(SeqJvpCall, hipStream_t);
}  // namespace mrphy_i

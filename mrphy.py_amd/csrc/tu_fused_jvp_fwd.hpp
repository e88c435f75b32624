// tu_fused_jvp_fwd.hpp -- the body of the units tu_fused_jvp1 / 2 / 4_fwd.hip: K2j, K2 with the forward-mode tangents of Mo
// (one transmit coil), at the direction capacity MRPHY_JVP_MD (one unit per capacity, so that they compile side by
// side): behind mrphy_blochsim_rfgr_jvp_fwd.
#include "host_common.hpp"

namespace {
#include "k_fused_jvp.hpp"
}  // namespace

namespace mrphy_i {
template <int MD, typename T, typename CT>
int run_rfgr_jvp(const void* Mi, PulseOps in, JvpTangents tg, void* Mo, void* dMo, int64_t N, int64_t nM, int64_t nT,
                 hipStream_t st)
{
    return launch_jvp<MD, T, CT>(Mi, in, tg, Mo, dMo, N, nM, nT, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                                           \
    template int mrphy_i::run_rfgr_jvp<MRPHY_JVP_MD, T_, CT_>(const void*, PulseOps, JvpTangents, void*, void*, int64_t, \
                                                              int64_t, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

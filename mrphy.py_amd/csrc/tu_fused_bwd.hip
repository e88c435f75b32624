// tu_fused_bwd.hip -- K2b, its trajectory builds K2bt and its signal build K2bs at a capacity of 1 receive coil: the build
// PLAIN of the fused adjoint, behind mrphy_blochsim_rfgr_bwd, _traj_bwd and mrphy_signal_rfgr_bwd (one transmit coil)
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st) { return launch_k2b<B, T, CT>(r, in, st); }
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_fused_bwd<mrphy_i::AdjBuild::PLAIN, T_, CT_>(const AdjointReq&, PulseOps, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_fused_moving_bwd.hip -- K2vb: K2b (mode 0) for spins at constant velocity (one transmit coil): the build MOVING of
// the fused adjoint, behind mrphy_blochsim_rfgr_moving_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_moving.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st) { return launch_k2vb<T, CT>(r, in, st); }
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_fused_bwd<mrphy_i::AdjBuild::MOVING, T_, CT_>(const AdjointReq&, PulseOps, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_fused_consts_bwd.hip -- the CONSTS builds of K2b and K2bt (modes 0, 1, 2): the fused adjoint that also returns the
// gradients w.r.t. the step constants (gamma 2 pi dt, E1, E2, E1 - 1) per spin, and the map gradients of the MAPS
// builds with them; the build CONSTS, behind mrphy_blochsim_rfgr_consts_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st) { return launch_k2b<B, T, CT>(r, in, st); }
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_fused_bwd<mrphy_i::AdjBuild::CONSTS, T_, CT_>(const AdjointReq&, PulseOps, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_fused_maps_bwd.hip -- the MAPS builds of K2b and K2bt (modes 0, 1, 2): the fused adjoint that also returns the
// gradients w.r.t. loc, df / gamma and b1 of one transmit coil; the build MAPS, behind mrphy_blochsim_rfgr_maps_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st) { return launch_k2b<B, T, CT>(r, in, st); }
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_fused_bwd<mrphy_i::AdjBuild::MAPS, T_, CT_>(const AdjointReq&, PulseOps, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

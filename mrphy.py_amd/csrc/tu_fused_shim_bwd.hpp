// tu_fused_shim_bwd.hpp -- the body of the units tu_fused_shim2 / 4 / 8_bwd.hip: K2shb, the adjoint of K2sh w.r.t. Mi,
// rf, gr and the channels' waveforms, at the channel capacity MRPHY_SHIM_MS (one unit per capacity): the build
// SHIM<MRPHY_SHIM_MS> of the fused adjoint, behind mrphy_blochsim_rfgr_shim_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_shim.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st) { return launch_k2shb<MRPHY_SHIM_MS, T, CT>(r, in, st); }
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                                   \
    template int mrphy_i::run_fused_bwd<mrphy_i::shim_build(MRPHY_SHIM_MS), T_, CT_>(const AdjointReq&, PulseOps, \
                                                                                     hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

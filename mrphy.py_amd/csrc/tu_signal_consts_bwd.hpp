// tu_signal_consts_bwd.hpp -- the body of the units tu_signal_consts1 / 2 / 4 / 8_bwd.hip: the CONSTS build of K2bs (K2b's
// signal mode, which also returns the gradients w.r.t. the step constants per spin) at the coil capacity MRPHY_RX_CAP,
// the build SIG_CONSTS<MRPHY_RX_CAP> of the fused adjoint (one unit per capacity, so that they compile side by side);
// behind mrphy_signal_rfgr_consts_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st) { return launch_k2b<B, T, CT>(r, in, st); }
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                \
    template int mrphy_i::run_fused_bwd<mrphy_i::sig_consts_build(MRPHY_RX_CAP), T_, CT_>( \
        const AdjointReq&, PulseOps, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

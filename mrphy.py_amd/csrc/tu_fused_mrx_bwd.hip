// tu_fused_mrx_bwd.hip -- K2bs at the capacities of 2, 4 and 8 receive coils: K2b's signal build for a receive array in
// one launch; the build MRX of the fused adjoint, behind mrphy_signal_rfgr_mrx_bwd with 2 .. sig_max_rx coils
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st) { return launch_k2b<B, T, CT>(r, in, st); }
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_fused_bwd<mrphy_i::AdjBuild::MRX, T_, CT_>(const AdjointReq&, PulseOps, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

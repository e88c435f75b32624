// tu_fused_shim_bwd.hpp -- the body of the units tu_fused_shim2 / 4 / 8_bwd.hip: K2shb, the adjoint of K2sh w.r.t. Mi,
// rf, gr and the channels' waveforms, at the channel capacity MRPHY_SHIM_MS (one unit per capacity); behind
// mrphy_blochsim_rfgr_shim_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_shim.hpp"
}  // namespace

namespace mrphy_i {
template <int MS, typename T, typename CT>
int run_rfgr_shim_bwd(const AdjointReq& r, PulseOps in, const void* sh, int64_t sh_sn, const void* shMap, int64_t nS,
                      hipStream_t st)
{
    return launch_k2shb<MS, T, CT>(r, in, sh, sh_sn, shMap, nS, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                                          \
    template int mrphy_i::run_rfgr_shim_bwd<MRPHY_SHIM_MS, T_, CT_>(const AdjointReq&, PulseOps, const void*, int64_t, \
                                                                    const void*, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_fused_mc_bwd.hip -- K2b and K2bt, 2..8 transmit coils: the build MC of the fused adjoint, behind
// mrphy_blochsim_rfgr_mc_bwd and _mc_traj_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_mc_bwd.hpp"
}  // namespace

namespace mrphy_i {

// the frame and the common arguments are the one-coil launcher's (k_fused_bwd_common.hpp); the coil capacity and the
// choice of the mode are this kernel's own
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st)
{
    static_assert(B == AdjBuild::MC, "this unit compiles the multi-coil kernel");
    return fused_bwd_launch<T>(r, k2b_mc_waves(r.nM), st, [&](dim3 grid) {
        const FusedBwdTrajArgs<T> a = fused_bwd_args<T>(r, in, grid.x);
#define MRPHY_K2BMC(RX_, MC_, INJ_)                                                                 \
    hipLaunchKernelGGL((k_bloch_rfgr_bwd_mc<T, CT, RX_, MC_, INJ_>), grid, dim3(WAVE), 0, st, \
                       (static_cast<const FusedBwdArgsT<T, INJ_>&>(a)), (int)r.nC)
        // fp64 at 8 coils: the register build of INJ == 2 (three cotangents held across the recompute) spills -- that one
        // takes the LDS-staged injection, which is correct for any stride
#define MRPHY_K2BMCT(RX_, MC_)                                                                      \
    do {                                                                                            \
        constexpr bool lds_only = sizeof(T) == 8 && MC_ == 8;                                       \
        if (!r.gMt) MRPHY_K2BMC(RX_, MC_, 0);                                                       \
        else if (lds_only || r.every < SEG) MRPHY_K2BMC(RX_, MC_, 1);                               \
        else if constexpr (!lds_only) MRPHY_K2BMC(RX_, MC_, 2);                                     \
    } while (0)
        // the smallest coil capacity (2 / 4 / 8) that holds nC: the build's loops run over all of it, on zeros
#define MRPHY_K2BMCR(MC_) do { if (in.E1.p) MRPHY_K2BMCT(true, MC_); else MRPHY_K2BMCT(false, MC_); } while (0)
        if (r.nC <= 2) MRPHY_K2BMCR(2);
        else if (r.nC <= 4) MRPHY_K2BMCR(4);
        else MRPHY_K2BMCR(8);
#undef MRPHY_K2BMCR
#undef MRPHY_K2BMCT
#undef MRPHY_K2BMC
    });
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_fused_bwd<mrphy_i::AdjBuild::MC, T_, CT_>(const AdjointReq&, PulseOps, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

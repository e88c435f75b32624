// tu_fused_mc_bwd.hip -- K2b and K2bt, 2..8 transmit coils: launcher of mrphy_blochsim_rfgr_mc_bwd and _mc_traj_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_mc_bwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_mc_bwd(const void* Mck, PulseOps in, const void* gMo, const void* gMt, int64_t every, void* gMi, void* grf,
                    void* ggr, void* work, int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st)
{
    dim3 grid;
    int e;
    if (!fused_grid(N * nM * nT, k2b_mc_waves(nM), N, grid, e)) return e;
    const FusedBwdTrajArgs<T> a = fused_bwd_args<T>(Mck, in, gMo, gMt, every, gMi, work, N, nM, nT, grid.x);
#define MRPHY_K2BMC(RX_, MC_, INJ_)                                                                 \
    hipLaunchKernelGGL((k_bloch_rfgr_bwd_mc<T, CT, RX_, MC_, INJ_>), grid, dim3(WAVE), 0, st, \
                       (static_cast<const FusedBwdArgsT<T, INJ_>&>(a)), (int)nC)
    // fp64 at 8 coils: the register build of INJ == 2 (three cotangents held across the recompute) spills -- that one
    // takes the LDS-staged injection, which is correct for any stride
#define MRPHY_K2BMCT(RX_, MC_)                                                                      \
    do {                                                                                            \
        constexpr bool lds_only = sizeof(T) == 8 && MC_ == 8;                                       \
        if (!gMt) MRPHY_K2BMC(RX_, MC_, 0);                                                         \
        else if (lds_only || every < SEG) MRPHY_K2BMC(RX_, MC_, 1);                                 \
        else if constexpr (!lds_only) MRPHY_K2BMC(RX_, MC_, 2);                                     \
    } while (0)
    // the smallest coil capacity (2 / 4 / 8) that holds nC: the build's loops run over all of it, on zeros
#define MRPHY_K2BMCR(MC_) do { if (in.E1.p) MRPHY_K2BMCT(true, MC_); else MRPHY_K2BMCT(false, MC_); } while (0)
    if (nC <= 2) MRPHY_K2BMCR(2);
    else if (nC <= 4) MRPHY_K2BMCR(4);
    else MRPHY_K2BMCR(8);
#undef MRPHY_K2BMCR
#undef MRPHY_K2BMCT
#undef MRPHY_K2BMC
    e = launch_status();
    if (e || !(grf || ggr)) return e;
    return launch_p2<T>(work, ggr, 3, grf, nC, N, nT, a.P, st);
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_mc_bwd<T_, CT_>(const void* Mck, PulseOps in, const void* gMo, const void* gMt, int64_t every, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

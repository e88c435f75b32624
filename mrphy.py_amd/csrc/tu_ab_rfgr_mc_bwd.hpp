// tu_ab_rfgr_mc_bwd.hpp -- the body of the units tu_ab_rfgr_mc2 / 4 / 8_bwd.hip: K2abb-mc, the adjoint of K2ab under
// parallel transmit, at the coil capacity MRPHY_AB_MC (one unit per capacity, so that they compile side by side);
// behind mrphy_ab_rfgr_mc_bwd
#include "host_common.hpp"

namespace {
#include "k_ab_rfgr_mc.hpp"
}  // namespace

namespace mrphy_i {
template <int MC, typename T, typename CT>
int run_ab_rfgr_mc_bwd(const void* ABck, PulseOps in, const void* gA, const void* gB, void* grf, void* ggr, void* work,
                       int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st)
{
    return launch_k2abb_mc<T, CT, MC>(ABck, in, gA, gB, grf, ggr, work, N, nM, nT, nC, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                                       \
    template int mrphy_i::run_ab_rfgr_mc_bwd<MRPHY_AB_MC, T_, CT_>(const void*, PulseOps, const void*, const void*, \
                                                                   void*, void*, void*, int64_t, int64_t, int64_t, \
                                                                   int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

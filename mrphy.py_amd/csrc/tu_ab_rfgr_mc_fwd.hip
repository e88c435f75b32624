// tu_ab_rfgr_mc_fwd.hip -- K2ab-mc: fused rf, gr -> Hargreaves' A, B under parallel transmit (the coil capacities 2, 4, 8),
// behind mrphy_ab_rfgr_mc_fwd
#include "host_common.hpp"

namespace {
#include "k_ab_rfgr_mc.hpp"
}  // namespace

namespace mrphy_i {
template <typename T, typename CT>
int run_ab_rfgr_mc_fwd(PulseOps in, void* A, void* B, void* ABck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT,
                       int64_t nC, hipStream_t st)
{
    return launch_k2ab_mc<T, CT>(in, A, B, ABck, ck_every, N, nM, nT, nC, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                                         \
    template int mrphy_i::run_ab_rfgr_mc_fwd<T_, CT_>(PulseOps, void*, void*, void*, int64_t, int64_t, int64_t, int64_t, \
                                                      int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

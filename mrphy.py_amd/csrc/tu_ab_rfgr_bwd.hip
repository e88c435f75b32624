// tu_ab_rfgr_bwd.hip -- K2abb: the adjoint of K2ab, grad_A, grad_B -> grad_rf, grad_gr, behind mrphy_ab_rfgr_bwd
#include "host_common.hpp"

namespace {
#include "k_ab_rfgr.hpp"
}  // namespace

namespace mrphy_i {
template <typename T, typename CT>
int run_ab_rfgr_bwd(const void* ABck, PulseOps in, const void* gA, const void* gB, void* grf, void* ggr, void* work,
                    int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    return launch_k2abb<T, CT>(ABck, in, gA, gB, grf, ggr, work, N, nM, nT, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                                          \
    template int mrphy_i::run_ab_rfgr_bwd<T_, CT_>(const void*, PulseOps, const void*, const void*, void*, void*, void*, \
                                                   int64_t, int64_t, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

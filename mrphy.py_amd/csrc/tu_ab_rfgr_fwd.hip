// tu_ab_rfgr_fwd.hip -- K2ab: fused rf, gr -> Hargreaves' A, B (one transmit coil), behind mrphy_ab_rfgr_fwd
#include "host_common.hpp"

namespace {
#include "k_ab_rfgr.hpp"
}  // namespace

namespace mrphy_i {
template <typename T, typename CT>
int run_ab_rfgr_fwd(PulseOps in, void* A, void* B, void* ABck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT,
                    hipStream_t st)
{
    return launch_k2ab<T, CT>(in, A, B, ABck, ck_every, N, nM, nT, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_ab_rfgr_fwd<T_, CT_>(PulseOps, void*, void*, void*, int64_t, int64_t, int64_t, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_fused_moving_bwd.hip -- K2vb: K2b (mode 0) for spins at constant velocity (one transmit coil), behind
// mrphy_blochsim_rfgr_moving_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_moving.hpp"
}  // namespace

namespace mrphy_i {
template <typename T, typename CT>
int run_rfgr_moving_bwd(const AdjointReq& r, PulseOps in, const void* vdt, int64_t step0, hipStream_t st)
{
    return launch_k2vb<T, CT>(r, in, vdt, step0, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_rfgr_moving_bwd<T_, CT_>(const AdjointReq&, PulseOps, const void*, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

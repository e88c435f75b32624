// tu_fused_bwd.hip -- K2b, its trajectory builds K2bt and its signal build K2bs at a capacity of 1 receive coil: launcher
// of mrphy_blochsim_rfgr_bwd, _traj_bwd and mrphy_signal_rfgr_bwd (one transmit coil)
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_bwd(const void* Mck, PulseOps in, const void* gMo, const void* gMt, int64_t every, const void* rx,
                 const void* gsig, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT,
                 hipStream_t st)
{
    return launch_rfgr_bwd<T, CT, false>(Mck, in, gMo, gMt, every, rx, 1, gsig, gMi, grf, ggr, work, N, nM, nT, st);
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_bwd<T_, CT_>(const void* Mck, PulseOps in, const void* gMo, const void* gMt, int64_t every, const void* rx, const void* gsig, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

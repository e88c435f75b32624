// tu_signal_consts_bwd.hpp -- the body of the units tu_signal_consts1 / 2 / 4 / 8_bwd.hip: the CONSTS build of K2bs (K2b's
// signal mode, which also returns the gradients w.r.t. the step constants per spin) at the coil capacity MRPHY_RX_CAP
// and its launcher (one unit per capacity, so that they compile side by side); behind mrphy_signal_rfgr_consts_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT, int R>
int run_signal_consts_bwd(const void* Mck, PulseOps in, const void* gMo, int64_t every, const void* rx, int64_t nRx,
                          const void* gsig, void* gMi, void* grf, void* ggr, void* gC, void* work, int64_t N, int64_t nM,
                          int64_t nT, hipStream_t st)
{
    return launch_signal_consts_bwd<T, CT, R>(Mck, in, gMo, every, rx, nRx, gsig, gMi, grf, ggr, gC, work, N, nM, nT, st);
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_signal_consts_bwd<T_, CT_, MRPHY_RX_CAP>(const void* Mck, PulseOps in, const void* gMo, int64_t every, const void* rx, int64_t nRx, const void* gsig, void* gMi, void* grf, void* ggr, void* gC, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

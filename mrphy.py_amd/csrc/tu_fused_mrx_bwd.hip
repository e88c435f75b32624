// tu_fused_mrx_bwd.hip -- K2bs at the capacities of 2, 4 and 8 receive coils: K2b's signal build for a receive array in
// one launch; launcher of mrphy_signal_rfgr_mrx_bwd with 2 .. sig_max_rx coils
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_mrx_bwd(const void* Mck, PulseOps in, const void* gMo, int64_t every, const void* rx, int64_t nRx,
                     const void* gsig, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT,
                     hipStream_t st)
{
    return launch_rfgr_bwd<T, CT, true>(Mck, in, gMo, nullptr, every, rx, nRx, gsig, gMi, grf, ggr, work, N, nM, nT, st);
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_mrx_bwd<T_, CT_>(const void* Mck, PulseOps in, const void* gMo, int64_t every, const void* rx, int64_t nRx, const void* gsig, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

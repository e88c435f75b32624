// tu_fused_consts_bwd.hip -- the CONSTS builds of K2b and K2bt (modes 0, 1, 2): the fused adjoint that also returns the
// gradients w.r.t. the step constants (gamma 2 pi dt, E1, E2, E1 - 1) per spin, and the map gradients of the MAPS
// builds with them; launcher of mrphy_blochsim_rfgr_consts_bwd
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_consts_bwd(const void* Mck, PulseOps in, const void* gMo, const void* gMt, int64_t every, void* gMi,
                        void* grf, void* ggr, void* gloc, void* gBz, void* gb1, void* gC, void* work, int64_t N,
                        int64_t nM, int64_t nT, hipStream_t st)
{
    return launch_rfgr_consts_bwd<T, CT>(Mck, in, gMo, gMt, every, gMi, grf, ggr, gloc, gBz, gb1, gC, work, N, nM, nT, st);
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_consts_bwd<T_, CT_>(const void* Mck, PulseOps in, const void* gMo, const void* gMt, int64_t every, void* gMi, void* grf, void* ggr, void* gloc, void* gBz, void* gb1, void* gC, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_ab_rfgr_consts_bwd.hip -- the CONSTS build of K2abb: the adjoint of K2ab that also returns the gradients w.r.t. the
// step constants (gamma 2 pi dt, E1, E2, E1 - 1) per spin, and the map gradients of the MAPS build with them, behind
// mrphy_ab_rfgr_consts_bwd
#include "host_common.hpp"

namespace {
#include "k_ab_rfgr.hpp"
}  // namespace

namespace mrphy_i {
template <bool CONSTS, typename T, typename CT>
int run_ab_rfgr_spin_bwd(const void* ABck, PulseOps in, const void* gA, const void* gB, void* grf, void* ggr, void* gloc,
                         void* gBz, void* gb1, void* gC, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    static_assert(CONSTS, "this unit holds the CONSTS build");
    return launch_k2abb<T, CT, false, true>(ABck, in, gA, gB, grf, ggr, work, N, nM, nT, st, {gloc, gBz, gb1, gC});
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                                       \
    template int mrphy_i::run_ab_rfgr_spin_bwd<true, T_, CT_>(const void*, PulseOps, const void*, const void*, void*, \
                                                              void*, void*, void*, void*, void*, void*, int64_t,  \
                                                              int64_t, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

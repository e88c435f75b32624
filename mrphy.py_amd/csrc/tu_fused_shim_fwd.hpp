// tu_fused_shim_fwd.hpp -- the body of the units tu_fused_shim2 / 4 / 8_fwd.hip: K2sh, K2 with extra Bz field channels
// (one transmit coil), at the channel capacity MRPHY_SHIM_MS (one unit per capacity, so that they compile side by
// side): the forward of the build SHIM<MRPHY_SHIM_MS>, behind mrphy_blochsim_rfgr_shim_fwd.  The float builds are
// compiled with K2's ILP-first schedule (_lib.py: UNIT_FLAGS), as K2's one-coil float builds are, so that the two
// differ by the channels alone.
#include "host_common.hpp"

namespace {
#include "k_fused_shim.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_rfgr_ext_fwd(const void* Mi, PulseOps in, BzExt x, void* Mo, void* Mck, int64_t ck_every, int64_t N, int64_t nM,
                     int64_t nT, hipStream_t st)
{
    return launch_ext_fwd<ShimExt<T, MRPHY_SHIM_MS>, T, CT>(Mi, in, x, Mo, Mck, ck_every, N, nM, nT, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                              \
    template int mrphy_i::run_rfgr_ext_fwd<mrphy_i::shim_build(MRPHY_SHIM_MS), T_, CT_>( \
        const void*, PulseOps, BzExt, void*, void*, int64_t, int64_t, int64_t, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

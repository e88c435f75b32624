// tu_fused_moving_fwd.hip -- K2v: K2 for spins at constant velocity (one transmit coil): the forward of the build
// MOVING, behind mrphy_blochsim_rfgr_moving_fwd.  The float builds are compiled with K2's ILP-first schedule (_lib.py:
// UNIT_FLAGS), as the one-coil float builds of K2 are (tu_fused_fwd1.hip), so that the two differ by the motion alone.
#include "host_common.hpp"

namespace {
#include "k_fused_moving.hpp"
}  // namespace

namespace mrphy_i {
template <AdjBuild B, typename T, typename CT>
int run_rfgr_ext_fwd(const void* Mi, PulseOps in, BzExt x, void* Mo, void* Mck, int64_t ck_every, int64_t N, int64_t nM,
                     int64_t nT, hipStream_t st)
{
    return launch_ext_fwd<MovingExt<T>, T, CT>(Mi, in, x, Mo, Mck, ck_every, N, nM, nT, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                     \
    template int mrphy_i::run_rfgr_ext_fwd<mrphy_i::AdjBuild::MOVING, T_, CT_>( \
        const void*, PulseOps, BzExt, void*, void*, int64_t, int64_t, int64_t, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

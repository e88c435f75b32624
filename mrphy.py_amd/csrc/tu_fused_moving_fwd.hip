// tu_fused_moving_fwd.hip -- K2v: K2 for spins at constant velocity (one transmit coil), behind
// mrphy_blochsim_rfgr_moving_fwd.  The float builds are compiled with K2's ILP-first schedule (_lib.py: UNIT_FLAGS), as
// the one-coil float builds of K2 are (tu_fused_fwd1.hip), so that the two differ by the motion alone.
#include "host_common.hpp"

namespace {
#include "k_fused_moving.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_moving_fwd(const void* Mi, PulseOps in, const void* vdt, int64_t step0, void* Mo, void* Mck,
                        int64_t ck_every, int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    MovingFwdArgs<T> a;
    a.Mi = (const T*)Mi; a.in = typed<T>(in); a.vdt = (const T*)vdt; a.step0 = step0; a.Mo = (T*)Mo; a.Mck = (T*)Mck;
    a.ck_every = ck_every > 0 ? ck_every : 1;
    a.N = N; a.nM = nM; a.nT = nT;
    return launch_k2v<T, CT>(a, st);
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_moving_fwd<T_, CT_>(const void* Mi, PulseOps in, const void* vdt, int64_t step0, void* Mo, void* Mck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_fused_shim_fwd.hpp -- the body of the units tu_fused_shim2 / 4 / 8_fwd.hip: K2sh, K2 with extra Bz field channels
// (one transmit coil), at the channel capacity MRPHY_SHIM_MS (one unit per capacity, so that they compile side by
// side); behind mrphy_blochsim_rfgr_shim_fwd.  The float builds are compiled with K2's ILP-first schedule (_lib.py:
// UNIT_FLAGS), as K2's one-coil float builds are, so that the two differ by the channels alone.
#include "host_common.hpp"

namespace {
#include "k_fused_shim.hpp"
}  // namespace

namespace mrphy_i {
template <int MS, typename T, typename CT>
int run_rfgr_shim_fwd(const void* Mi, PulseOps in, const void* sh, int64_t sh_sn, const void* shMap, int64_t nS, void* Mo,
                      void* Mck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    ShimFwdArgs<T> a;
    a.Mi = (const T*)Mi; a.in = typed<T>(in); a.sh = (const T*)sh; a.sh_sn = sh_sn; a.shMap = (const T*)shMap; a.nS = nS;
    a.Mo = (T*)Mo; a.Mck = (T*)Mck;
    a.ck_every = ck_every > 0 ? ck_every : 1;
    a.N = N; a.nM = nM; a.nT = nT;
    return launch_k2sh<MS, T, CT>(a, st);
}
}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_)                                                                                          \
    template int mrphy_i::run_rfgr_shim_fwd<MRPHY_SHIM_MS, T_, CT_>(const void*, PulseOps, const void*, int64_t,      \
                                                                    const void*, int64_t, void*, void*, int64_t,     \
                                                                    int64_t, int64_t, int64_t, hipStream_t);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

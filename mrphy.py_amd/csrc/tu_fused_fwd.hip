// tu_fused_fwd.hip -- K2 and its trajectory builds K2t: launcher of mrphy_blochsim_rfgr_fwd and _traj_fwd
#include "host_common.hpp"

namespace {
#include "k_fused_fwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_fwd(const void* Mi, PulseOps in, void* Mo, void* Mck, int64_t ck_every, void* Mt, int64_t every,
                 int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st)
{
    // (the empty problem and the batch limit: launch_k2)
    if constexpr (sizeof(T) == 4) {
        if (nC == 1) return run_rfgr_fwd1<T, CT>(Mi, in, Mo, Mck, ck_every, Mt, every, N, nM, nT, nC, st);
    }
    const FusedTrajArgs<T> a = fused_args<T>(Mi, in, Mo, Mck, ck_every, Mt, every, N, nM, nT, nC);
    const void* b1 = in.b1;
    int e = 0;
#define MRPHY_K2C(NCM_) e = launch_k2<T, CT, NCM_, true>(a, st)
    // the smallest register/LDS coil capacity that holds nC (each build sizes its b1 registers and
    // its LDS rf buffer for exactly that capacity: never launch one with more coils than it holds)
    // (one coil in float: tu_fused_fwd1.hip, above)
    if (nC == 1 && b1) { if constexpr (sizeof(T) == 8) MRPHY_K2C(1); }
    else if (nC == 1) { if constexpr (sizeof(T) == 8) e = launch_k2<T, CT, 1, false>(a, st); }   // no b1 map: Bxy = rf, no complex product
    else if (nC <= 2 && b1) MRPHY_K2C(2);                // (round 3: 2 coils no longer pay for 8)
    else if (nC <= 4 && b1) MRPHY_K2C(4);
    else if (nC <= 8 && b1) MRPHY_K2C(8);
    else if (sizeof(T) == 4 && nC <= 16 && b1) { if constexpr (sizeof(T) == 4) MRPHY_K2C(16); }
    else if (sizeof(T) == 4 && nC <= 32 && b1) { if constexpr (sizeof(T) == 4) MRPHY_K2C(32); }
    else if (sizeof(T) == 4 && nC <= 40 && b1) { if constexpr (sizeof(T) == 4) MRPHY_K2C(40); }   // (round 4: no cliff at 33)
    else if (sizeof(T) == 4 && nC <= 48 && b1) { if constexpr (sizeof(T) == 4) MRPHY_K2C(48); }
    else if (sizeof(T) == 4 && nC <= K2_MAXC && b1) { if constexpr (sizeof(T) == 4) MRPHY_K2C(64); }
    // (fp64 with more than 8 coils: the 16- / 32-coil register builds would need 128-700 spilled VGPRs in
    // double precision; the host routes those to rfgr2beff + blochsim, and a direct caller gets the generic build)
    else MRPHY_K2C(0);
#undef MRPHY_K2C
    return e;
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_fwd<T_, CT_>(const void* Mi, PulseOps in, void* Mo, void* Mck, int64_t ck_every, void* Mt, int64_t every, int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

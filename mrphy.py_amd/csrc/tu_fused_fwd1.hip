// tu_fused_fwd1.hip -- K2 and K2t, one transmit coil, float: launcher called by run_rfgr_fwd (tu_fused_fwd.hip)
// A unit of its own because it is compiled with `-mllvm -amdgpu-sched-strategy=max-ilp` (_lib.py: UNIT_FLAGS):
// the ILP-first schedule of the step loop is 2-3 % faster for these builds (128^3 x 1024: 2.35 -> 2.28 ms, 128^3 x 4096:
// 9.5 -> 9.3 ms same box, profiles/r04_k2_ilp_ab.json) at 102-105 instead of 79-95 VGPRs, and costs the multi-coil
// builds (8 coils: 118 -> 199 VGPRs, +4 % time) and the fp64 ones what it gives these.
#include "host_common.hpp"

namespace {
#include "k_fused_fwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_fwd1(const void* Mi, PulseOps in, void* Mo, void* Mck, int64_t ck_every, void* Mt, int64_t every,
                  int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st)
{
    if constexpr (sizeof(T) != 4) {
        return MRPHY_EINVAL;                             // fp64 stays in tu_fused_fwd.hip
    } else {
        const FusedTrajArgs<T> a = fused_args<T>(Mi, in, Mo, Mck, ck_every, Mt, every, N, nM, nT, nC);
        if (in.b1) return launch_k2<T, CT, 1, true>(a, st);
        return launch_k2<T, CT, 1, false>(a, st);        // no b1 map: Bxy = rf, no complex product
    }
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_fwd1<T_, CT_>(const void* Mi, PulseOps in, void* Mo, void* Mck, int64_t ck_every, void* Mt, int64_t every, int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

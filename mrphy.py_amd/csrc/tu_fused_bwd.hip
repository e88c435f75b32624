// tu_fused_bwd.hip -- K2b, its trajectory builds K2bt and its signal build K2bs: launcher of mrphy_blochsim_rfgr_bwd,
// _traj_bwd and mrphy_signal_rfgr_bwd (one transmit coil)
#include "host_common.hpp"

namespace {
#include "k_fused_bwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_bwd(const void* Mck, PulseOps in, const void* gMo, const void* gMt, int64_t every, const void* rx,
                 const void* gsig, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT,
                 hipStream_t st)
{
    dim3 grid;
    int e;
    if (!fused_grid(N * nM * nT, k2b_waves(nM), N, grid, e)) return e;
    // gsig (the cotangent of the signal's samples, with the receive map rx) selects the signal build, which may have no
    // gMo; its records are counted as the trajectory's
    FusedBwdSigArgs<T> a;
    static_cast<FusedBwdTrajArgs<T>&>(a) = fused_bwd_args<T>(Mck, in, gMo, gMt, every, gMi, work, N, nM, nT,
                                                             grid.x);
    a.rx = (const T*)rx; a.gsig = (const T*)gsig;
    if (gsig) a.nRec = sig_records(nT, every);
#define MRPHY_K2B(RX_, HB_, INJ_)                                                               \
    hipLaunchKernelGGL((k_bloch_rfgr_bwd<T, CT, RX_, HB_, INJ_>), grid, dim3(WAVE), 0, st, \
                       (static_cast<const FusedBwdArgsT<T, INJ_>&>(a)))
#define MRPHY_K2BT(RX_, HB_)                                                                    \
    do {                                                                                        \
        if (gsig) MRPHY_K2B(RX_, HB_, 3);                                                       \
        else if (!gMt) MRPHY_K2B(RX_, HB_, 0);                                                  \
        else if (every < SEG) MRPHY_K2B(RX_, HB_, 1);                                           \
        else MRPHY_K2B(RX_, HB_, 2);                                                            \
    } while (0)
    if (in.b1) { if (in.E1.p) MRPHY_K2BT(true, true);  else MRPHY_K2BT(false, true); }
    else       { if (in.E1.p) MRPHY_K2BT(true, false); else MRPHY_K2BT(false, false); }   // no b1 map: Bxy = rf
#undef MRPHY_K2BT
#undef MRPHY_K2B
    e = launch_status();
    if (e || !(grf || ggr)) return e;
    return launch_p2<T>(work, ggr, 3, grf, 1, N, nT, a.P, st);
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_bwd<T_, CT_>(const void* Mck, PulseOps in, const void* gMo, const void* gMt, int64_t every, const void* rx, const void* gsig, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

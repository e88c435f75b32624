// tu_fused_mrx_bwd.hip -- K2bs-mrx: K2b's signal build for several receive coils in one launch; launcher of
// mrphy_signal_rfgr_mrx_bwd (one transmit coil, 2 .. sig_max_rx receive coils)
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
    dim3 grid;
    int e;
    if (!fused_grid(N * nM * nT, k2b_waves(nM), N, grid, e)) return e;
    FusedBwdMrxArgs<T> a;
    static_cast<FusedBwdTrajArgs<T>&>(a) = fused_bwd_args<T>(Mck, in, gMo, nullptr, every, gMi, work, N, nM, nT,
                                                             grid.x);
    a.rx = (const T*)rx; a.gsig = (const T*)gsig; a.nRx = nRx;
    a.nRec = sig_records(nT, every);
    // the smallest capacity that holds nRx coils: INJ = 4, 5, 6 for 2, 4, 8 (abi.hip has refused nRx > sig_max_rx = 8)
#define MRPHY_K2B(RX_, HB_, INJ_)                                                               \
    hipLaunchKernelGGL((k_bloch_rfgr_bwd<T, CT, RX_, HB_, INJ_>), grid, dim3(WAVE), 0, st, a)
#define MRPHY_K2BR(RX_, HB_)                                                                    \
    do {                                                                                        \
        if (nRx <= 2) MRPHY_K2B(RX_, HB_, 4);                                                   \
        else if (nRx <= 4) MRPHY_K2B(RX_, HB_, 5);                                              \
        else MRPHY_K2B(RX_, HB_, 6);                                                            \
    } while (0)
    if (in.b1) { if (in.E1.p) MRPHY_K2BR(true, true);  else MRPHY_K2BR(false, true); }
    else       { if (in.E1.p) MRPHY_K2BR(true, false); else MRPHY_K2BR(false, false); }
#undef MRPHY_K2BR
#undef MRPHY_K2B
    e = launch_status();
    if (e || !(grf || ggr)) return e;
    return launch_p2<T>(work, ggr, 3, grf, 1, N, nT, a.P, st);
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_rfgr_mrx_bwd<T_, CT_>(const void* Mck, PulseOps in, const void* gMo, int64_t every, const void* rx, int64_t nRx, const void* gsig, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_signal.hip -- K2s: launcher of mrphy_signal_rfgr_fwd (the received signal of the fused simulation, one transmit
// coil, no or one receive coil) and its second pass
#include "host_common.hpp"

namespace {
#include "k_signal_fwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_signal_fwd(const void* Mi, PulseOps in, const void* rx, void* Mo, void* Mck, int64_t ck_every, void* sig,
                   int64_t every, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    if (N * nM * nT == 0) return 0;
    if (N > 65535) return MRPHY_EINVAL;
    SignalArgs<T> a;
    a.Mi = (const T*)Mi; a.in = typed<T>(in); a.rx = (const T*)rx; a.Mo = (T*)Mo; a.Mck = (T*)Mck;
    a.ck_every = ck_every > 0 ? ck_every : 1;
    a.work = (T*)work; a.every = every; a.nRec = sig_records(nT, every);
    a.N = N; a.nM = nM; a.nT = nT; a.P = sig_waves(nM);
    const dim3 grid((unsigned)a.P, (unsigned)N);
#define MRPHY_K2S(CK_, RX_, HB_, EV_) \
    hipLaunchKernelGGL((k_signal_fwd<T, CT, CK_, RX_, HB_, EV_>), grid, dim3(WAVE), 0, st, a)
#define MRPHY_K2S_EV(CK_, RX_, HB_)                                                              \
    do {                                                                                         \
        if (every == 1) MRPHY_K2S(CK_, RX_, HB_, true); else MRPHY_K2S(CK_, RX_, HB_, false);    \
    } while (0)
#define MRPHY_K2S_HB(CK_, RX_)                                                                   \
    do {                                                                                         \
        if (in.b1) MRPHY_K2S_EV(CK_, RX_, true); else MRPHY_K2S_EV(CK_, RX_, false);             \
    } while (0)
    const bool ck = (Mck != nullptr), rlx = (in.E1.p != nullptr);
    if (ck) { if (rlx) MRPHY_K2S_HB(true, true); else MRPHY_K2S_HB(true, false); }
    else    { if (rlx) MRPHY_K2S_HB(false, true); else MRPHY_K2S_HB(false, false); }
#undef MRPHY_K2S_HB
#undef MRPHY_K2S_EV
#undef MRPHY_K2S
    int e = launch_status();
    if (e) return e;
    hipLaunchKernelGGL((k_signal_p2<T>), dim3((unsigned)((a.nRec + P2_T - 1) / P2_T), 2, (unsigned)N),
                       dim3(P2_T * P2_G), 0, st, (const T*)work, (T*)sig, N, a.nRec, a.P);
    return launch_status();
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_signal_fwd<T_, CT_>(const void* Mi, PulseOps in, const void* rx, void* Mo, void* Mck, int64_t ck_every, void* sig, int64_t every, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

// tu_signal.hpp -- the body of the units tu_signal.hip (capacity 1) and tu_signal_mrx2 / 4 / 8.hip: K2s at the coil
// capacity MRPHY_RX_CAP, its launcher and its second pass (one unit per capacity, so that they compile side by side)
#include "host_common.hpp"

namespace {
#include "k_signal_fwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT, int R>
int run_signal_fwd(const void* Mi, PulseOps in, const void* rx, int64_t nRx, void* Mo, void* Mck, int64_t ck_every,
                   void* sig, int64_t every, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    dim3 grid;
    int e;
    if (!fused_grid(N * nM * nT, sig_waves(nM), N, grid, e)) return e;
    SignalArgs<T> a;
    a.Mi = (const T*)Mi; a.in = typed<T>(in); a.rx = (const T*)rx; a.Mo = (T*)Mo; a.Mck = (T*)Mck;
    a.ck_every = ck_every > 0 ? ck_every : 1;
    a.work = (T*)work; a.every = every; a.nRec = sig_records(nT, every);
    a.N = N; a.nM = nM; a.nT = nT; a.P = grid.x; a.nRx = nRx;
#define MRPHY_K2S(CK_, RX_, HB_, EV_) \
    hipLaunchKernelGGL((k_signal_fwd<T, CT, CK_, RX_, HB_, EV_, R>), grid, dim3(WAVE), 0, st, a)
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
    e = launch_status();
    if (e) return e;
    return launch_p2<T>(work, nullptr, 0, sig, nRx, N, a.nRec, a.P, st);   // sig (N, 2, nRec, nRx)
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_signal_fwd<T_, CT_, MRPHY_RX_CAP>(const void* Mi, PulseOps in, const void* rx, int64_t nRx, void* Mo, void* Mck, int64_t ck_every, void* sig, int64_t every, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

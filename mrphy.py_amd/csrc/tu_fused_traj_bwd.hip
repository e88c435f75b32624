// tu_fused_traj_bwd.hip -- K2bt: launchers of mrphy_blochsim_rfgr_traj_bwd (one transmit coil) and
// mrphy_blochsim_rfgr_mc_traj_bwd (2..8 coils): K2b with a cotangent injected at every recorded step
// (k_fused_bwd.hpp / k_fused_mc_bwd.hpp compiled with MRPHY_K2B_TRAJ: kernels of their own, template parameter INJ).
// The workspace and its second pass are K2b's.
#include "host_common.hpp"

namespace {
#define MRPHY_K2B_TRAJ 1
#include "k_fused_bwd.hpp"
#include "k_fused_mc_bwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_rfgr_traj_bwd(const void* Mck, const void* rf, int64_t rf_sn, const void* gr, int64_t gr_sn,
                      const void* loc, Bc df, Bc gam, const void* b1, Bc g, Bc E1, Bc E2,
                      const void* E1m1, const void* gMt, int64_t every, void* gMi, void* grf, void* ggr,
                      void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    FusedBwdTrajArgs<T> a;
    a.Mck = (const T*)Mck; a.rf = (const T*)rf; a.rf_sn = rf_sn; a.gr = (const T*)gr;
    a.gr_sn = gr_sn; a.loc = (const T*)loc; a.df = df; a.gam = gam; a.b1 = (const T*)b1;
    a.g = g; a.E1 = E1; a.E2 = E2; a.E1m1 = E1m1; a.gMo = (const T*)gMt; a.gMi = (T*)gMi;
    a.work = (T*)work; a.N = N; a.nM = nM; a.nT = nT; a.P = k2b_waves(nM);
    a.every = every; a.nRec = (nT + every - 1) / every;
    if (N * nM * nT == 0) return 0;
    if (N > 65535) return MRPHY_EINVAL;
    const dim3 grid((unsigned)a.P, (unsigned)N);
#define MRPHY_K2BT(RX_, HB_)                                                                                   \
    do {                                                                                                       \
        if (every < SEG) hipLaunchKernelGGL((k_bloch_rfgr_traj_bwd<T, CT, RX_, HB_, 1>), grid, dim3(WAVE), 0, st, a); \
        else             hipLaunchKernelGGL((k_bloch_rfgr_traj_bwd<T, CT, RX_, HB_, 2>), grid, dim3(WAVE), 0, st, a); \
    } while (0)
    if (b1) { if (E1.p) MRPHY_K2BT(true, true);  else MRPHY_K2BT(false, true); }
    else    { if (E1.p) MRPHY_K2BT(true, false); else MRPHY_K2BT(false, false); }   // no b1 map: Bxy = rf
#undef MRPHY_K2BT
    int e = launch_status();
    if (e) return e;
    if (grf || ggr) {
        hipLaunchKernelGGL((k_bloch_rfgr_bwd_p2<T>),
                           dim3((unsigned)((nT + P2_T - 1) / P2_T), 5, (unsigned)N),
                           dim3(P2_T * P2_G), 0, st, (const T*)work, (T*)grf, (T*)ggr, N, nT, a.P);
        e = launch_status();
    }
    return e;
}

template <typename T, typename CT>
int run_rfgr_mc_traj_bwd(const void* Mck, const void* rf, int64_t rf_sn, const void* gr, int64_t gr_sn,
                         const void* loc, Bc df, Bc gam, const void* b1, Bc g, Bc E1, Bc E2,
                         const void* E1m1, const void* gMt, int64_t every, void* gMi, void* grf, void* ggr,
                         void* work, int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st)
{
    FusedBwdTrajArgs<T> a;
    a.Mck = (const T*)Mck; a.rf = (const T*)rf; a.rf_sn = rf_sn; a.gr = (const T*)gr;
    a.gr_sn = gr_sn; a.loc = (const T*)loc; a.df = df; a.gam = gam; a.b1 = (const T*)b1;
    a.g = g; a.E1 = E1; a.E2 = E2; a.E1m1 = E1m1; a.gMo = (const T*)gMt; a.gMi = (T*)gMi;
    a.work = (T*)work; a.N = N; a.nM = nM; a.nT = nT; a.P = k2b_mc_waves(nM);
    a.every = every; a.nRec = (nT + every - 1) / every;
    if (N * nM * nT == 0) return 0;
    if (N > 65535) return MRPHY_EINVAL;
    const dim3 grid((unsigned)a.P, (unsigned)N);
#define MRPHY_K2BMC(RX_, MC_, INJ_) \
    hipLaunchKernelGGL((k_bloch_rfgr_traj_bwd_mc<T, CT, RX_, MC_, INJ_>), grid, dim3(WAVE), 0, st, a, (int)nC)
    // fp64 at 8 coils: the register build of INJ == 2 (three cotangents held across the recompute) spills -- that one
    // takes the LDS-staged injection, which is correct for any stride
#define MRPHY_K2BMCT(MC_)                                                                                   \
    do {                                                                                                    \
        constexpr bool lds_only = sizeof(T) == 8 && MC_ == 8;                                               \
        if (lds_only || every < SEG) { if (E1.p) MRPHY_K2BMC(true, MC_, 1); else MRPHY_K2BMC(false, MC_, 1); } \
        else if constexpr (!lds_only) { if (E1.p) MRPHY_K2BMC(true, MC_, 2); else MRPHY_K2BMC(false, MC_, 2); } \
    } while (0)
    if (nC <= 2) MRPHY_K2BMCT(2);
    else if (nC <= 4) MRPHY_K2BMCT(4);
    else MRPHY_K2BMCT(8);
#undef MRPHY_K2BMCT
#undef MRPHY_K2BMC
    int e = launch_status();
    if (e) return e;
    if (grf || ggr) {
        hipLaunchKernelGGL((k_bloch_rfgr_bwd_mc_p2<T>),
                           dim3((unsigned)((nT + P2_T - 1) / P2_T), (unsigned)(3 + 2 * nC), (unsigned)N),
                           dim3(P2_T * P2_G), 0, st, (const T*)work, (T*)grf, (T*)ggr, N, nT, a.P,
                           (int)nC);
        e = launch_status();
    }
    return e;
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) \
    template int mrphy_i::run_rfgr_traj_bwd<T_, CT_>(const void* Mck, const void* rf, int64_t rf_sn, const void* gr, int64_t gr_sn, const void* loc, Bc df, Bc gam, const void* b1, Bc g, Bc E1, Bc E2, const void* E1m1, const void* gMt, int64_t every, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st); \
    template int mrphy_i::run_rfgr_mc_traj_bwd<T_, CT_>(const void* Mck, const void* rf, int64_t rf_sn, const void* gr, int64_t gr_sn, const void* loc, Bc df, Bc gam, const void* b1, Bc g, Bc E1, Bc E2, const void* E1m1, const void* gMt, int64_t every, void* gMi, void* grf, void* ggr, void* work, int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

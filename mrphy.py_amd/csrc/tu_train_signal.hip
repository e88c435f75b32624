// tu_train_signal.hip -- the signal of a pulse repeated K times (the transverse magnetisation of Ktr's records summed
// over the spins, for up to 8 receive coils per launch): the entry points of the C ABI together with their kernels
// (k_train_signal.hpp on k_ab_train.hpp).  Two data types, no constant type, as tu_ab_train.hip.
#include "host_common.hpp"

namespace {
#include "k_ab_train.hpp"
#include "k_train_signal.hpp"

template <typename T, bool BWD>
void launch_main(const TrainSigArgs& a, int cap, hipStream_t st)
{
    const dim3 grid((unsigned)a.P, (unsigned)a.N);
    trs_at_capacity(cap, [&](auto r) {
        constexpr int R = decltype(r)::value;
        if constexpr (BWD) hipLaunchKernelGGL((k_train_signal_bwd<T, R>), grid, dim3(WAVE), 0, st, a);
        else               hipLaunchKernelGGL((k_train_signal_fwd<T, R>), grid, dim3(WAVE), 0, st, a);
    });
}
}  // namespace

extern "C" {

int64_t mrphy_train_signal_ck_every(void) { return TRS_SEG; }

int mrphy_train_signal_max_rx(int dtype)
{
    return (dtype == MRPHY_F32 || dtype == MRPHY_F64) ? trs_max_rx(tsize(dtype)) : 0;
}

size_t mrphy_train_signal_workspace(int dtype, int64_t N, int64_t nM, int64_t K, int64_t rows)
{
    if ((dtype != MRPHY_F32 && dtype != MRPHY_F64) || N <= 0 || nM <= 0 || K <= 0 || rows <= 0) return 0;
    return trs_workspace(N, nM, K, rows);
}

int mrphy_train_signal_fwd(int dtype, const void* A, const void* B, const void* rest, int64_t rest_sn,
                           const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2, int64_t T2_sn, int64_t T2_sm,
                           const void* df, int64_t df_sn, int64_t df_sm, const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                           const void* cs, int64_t cs_sn, const void* rx, int64_t nRx, void* sig, void* Mlast,
                           void* ck, void* work, size_t work_bytes, int64_t N, int64_t nM, int64_t K, void* stream)
{
    bool empty;
    if (int e = train_check(dtype, A, B, rest, T1, T2, df, Mi, cs, N, nM, K, empty)) return e;
    if (empty) return 0;
    if (!sig) return MRPHY_EINVAL;
    if (int e = trs_signal_check(dtype, rx, nRx, work, work_bytes, trs_workspace(N, nM, K, 2 * (nRx > 0 ? nRx : 1))))
        return e;
    const size_t ts = tsize(dtype);
    if (!aligned_to(sig, ts) || !aligned_to(Mlast, ts) || !aligned_to(ck, sizeof(double))) return MRPHY_EALIGN;
    TrainSigArgs a{};
    train_fill(a.t, A, B, rest, rest_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, Mi, Mi_sn, Mi_sm,
               cs, cs_sn, N, nM, K);
    a.rx = rx; a.nRx = nRx; a.Mlast = Mlast; a.ck = reinterpret_cast<double*>(ck);
    a.work = reinterpret_cast<double*>(work); a.N = N; a.P = trs_waves(nM);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MRPHY_F32) launch_main<float, false>(a, trs_capacity(nRx), st);
    else                    launch_main<double, false>(a, trs_capacity(nRx), st);
    if (int e = launch_status()) return e;
    return dtype == MRPHY_F32 ? trs_launch_p2<float>(a.work, (float*)sig, N, 2 * nRx, 0, K, a.P, nRx, st)
                              : trs_launch_p2<double>(a.work, (double*)sig, N, 2 * nRx, 0, K, a.P, nRx, st);
}

int mrphy_train_signal_bwd(int dtype, const void* A, const void* B, const void* grad_sig, const void* grad_Mlast,
                           const void* rest, int64_t rest_sn, const void* T1, int64_t T1_sn, int64_t T1_sm,
                           const void* T2, int64_t T2_sn, int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm,
                           const void* Mi, int64_t Mi_sn, int64_t Mi_sm, const void* cs, int64_t cs_sn, const void* rx,
                           int64_t nRx, const void* ck, void* grad_A, void* grad_B, void* grad_consts, void* grad_Mi,
                           void* grad_phase, void* grad_rx, void* work, size_t work_bytes, int64_t N, int64_t nM,
                           int64_t K, void* stream)
{
    bool empty;
    if (int e = train_check(dtype, A, B, rest, T1, T2, df, Mi, cs, N, nM, K, empty)) return e;
    if (empty) return 0;
    if ((!grad_sig && !grad_Mlast) || !ck ||
        (!grad_A && !grad_B && !grad_consts && !grad_Mi && !grad_phase && !grad_rx))
        return MRPHY_EINVAL;
    if (int e = trs_signal_check(dtype, rx, nRx, work, work_bytes, grad_phase ? trs_workspace(N, nM, K, 1) : 0))
        return e;
    const size_t ts = tsize(dtype);
    if (!aligned_to(grad_sig, sizeof(double)) || !aligned_to(grad_Mlast, ts) || !aligned_to(ck, sizeof(double)) ||
        !aligned_to(grad_A, ts) || !aligned_to(grad_B, ts) || !aligned_to(grad_consts, sizeof(double)) ||
        !aligned_to(grad_Mi, ts) || !aligned_to(grad_phase, ts) || !aligned_to(grad_rx, ts))
        return MRPHY_EALIGN;
    TrainSigArgs a{};
    train_fill(a.t, A, B, rest, rest_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, Mi, Mi_sn, Mi_sm,
               cs, cs_sn, N, nM, K);
    a.t.gA = grad_A; a.t.gB = grad_B; a.t.gC = grad_consts; a.t.gMi = grad_Mi;
    a.rx = rx; a.nRx = nRx; a.ck = const_cast<double*>(reinterpret_cast<const double*>(ck));
    a.work = grad_phase ? reinterpret_cast<double*>(work) : nullptr;
    a.gs = reinterpret_cast<const double*>(grad_sig); a.gMl = grad_Mlast; a.grx = grad_rx;
    a.N = N; a.P = trs_waves(nM);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MRPHY_F32) launch_main<float, true>(a, trs_capacity(nRx), st);
    else                    launch_main<double, true>(a, trs_capacity(nRx), st);
    if (int e = launch_status()) return e;
    if (!grad_phase) return 0;
    return dtype == MRPHY_F32 ? trs_launch_p2<float>(a.work, (float*)grad_phase, N, 1, 0, K, a.P, 0, st)
                              : trs_launch_p2<double>(a.work, (double*)grad_phase, N, 1, 0, K, a.P, 0, st);
}

}  // extern "C"

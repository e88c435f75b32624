// tu_sequence_signal.hip -- the signal of a scheduled sequence (the transverse magnetisation of Ksq's records summed
// over the spins, for up to 8 receive coils per launch): the entry points of the C ABI together with their kernels
// (k_sequence_signal.hpp on k_ab_train.hpp, k_train_signal.hpp and k_ab_sequence.hpp, whose second passes it launches).
// Two data types, no constant type, as tu_train_signal.hip.  The segment length and the coil capacity are
// mrphy_train_signal_ck_every / mrphy_train_signal_max_rx: one geometry for both signal families.
#include "host_common.hpp"

namespace {
#include "k_ab_train.hpp"
#include "k_train_signal.hpp"
#include "k_ab_sequence.hpp"
#include "k_sequence_signal.hpp"

template <typename T, bool BWD>
void launch_main(const SeqSigArgs& a, int cap, hipStream_t st)
{
    const dim3 grid((unsigned)a.Pw, (unsigned)a.N);
    trs_at_capacity(cap, [&](auto r) {
        constexpr int R = decltype(r)::value;
        if constexpr (BWD) hipLaunchKernelGGL((k_sequence_signal_bwd<T, R>), grid, dim3(WAVE), 0, st, a);
        else               hipLaunchKernelGGL((k_sequence_signal_fwd<T, R>), grid, dim3(WAVE), 0, st, a);
    });
}
}  // namespace

extern "C" {

size_t mrphy_sequence_signal_workspace(int dtype, int64_t N, int64_t nM, int64_t K, int64_t rows)
{
    return mrphy_train_signal_workspace(dtype, N, nM, K, rows);
}

size_t mrphy_sequence_signal_bank_workspace(int dtype, int64_t P, int64_t N, int64_t nM)
{
    if ((dtype != MRPHY_F32 && dtype != MRPHY_F64) || P <= 0 || N <= 0 || nM <= 0) return 0;
    return seq_bank_bytes(P, N, nM);
}

int mrphy_sequence_signal_fwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse, const void* rs,
                              int64_t rs_sn, const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2,
                              int64_t T2_sn, int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm,
                              const void* Mi, int64_t Mi_sn, int64_t Mi_sm, const void* cs, int64_t cs_sn,
                              const void* rx, int64_t nRx, void* sig, void* Mlast, void* ck, void* work,
                              size_t work_bytes, int64_t N, int64_t nM, int64_t K, void* stream)
{
    bool empty; int align;
    if (int e = seq_check(dtype, A, B, P, pulse, rs, T1, T2, df, Mi, cs, N, nM, K, false, empty, align)) return e;
    if (empty) return 0;
    if (!sig) return MRPHY_EINVAL;
    if (int e = trs_signal_check(dtype, rx, nRx, work, work_bytes, trs_workspace(N, nM, K, 2 * (nRx > 0 ? nRx : 1))))
        return e;
    const size_t ts = tsize(dtype);
    if (align || !aligned_to(sig, ts) || !aligned_to(Mlast, ts) || !aligned_to(ck, sizeof(double))) return MRPHY_EALIGN;
    SeqSigArgs a{};
    seq_fill(a.s, A, B, P, pulse, rs, rs_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, Mi, Mi_sn,
             Mi_sm, cs, cs_sn, N, nM, K);
    a.rx = rx; a.nRx = nRx; a.Mlast = Mlast; a.ck = reinterpret_cast<double*>(ck);
    a.sums = reinterpret_cast<double*>(work); a.qphi = a.qrest = -1; a.N = N; a.Pw = trs_waves(nM);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MRPHY_F32) launch_main<float, false>(a, trs_capacity(nRx), st);
    else                    launch_main<double, false>(a, trs_capacity(nRx), st);
    if (int e = launch_status()) return e;
    return dtype == MRPHY_F32 ? trs_launch_p2<float>(a.sums, (float*)sig, N, 2 * nRx, 0, K, a.Pw, nRx, st)
                              : trs_launch_p2<double>(a.sums, (double*)sig, N, 2 * nRx, 0, K, a.Pw, nRx, st);
}

int mrphy_sequence_signal_bwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                              const void* grad_sig, const void* grad_Mlast, const void* rs, int64_t rs_sn,
                              const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2, int64_t T2_sn,
                              int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm, const void* Mi,
                              int64_t Mi_sn, int64_t Mi_sm, const void* cs, int64_t cs_sn, const void* rx, int64_t nRx,
                              const void* ck, void* grad_A, void* grad_B, void* grad_consts, void* grad_rest,
                              void* grad_Mi, void* grad_phase, void* grad_rx, void* work, size_t work_bytes,
                              void* bank, size_t bank_bytes, int64_t N, int64_t nM, int64_t K, void* stream)
{
    bool empty; int align;
    if (int e = seq_check(dtype, A, B, P, pulse, rs, T1, T2, df, Mi, cs, N, nM, K, false, empty, align)) return e;
    if (empty) return 0;
    if ((!grad_sig && !grad_Mlast) || !ck ||
        (!grad_A && !grad_B && !grad_consts && !grad_rest && !grad_Mi && !grad_phase && !grad_rx))
        return MRPHY_EINVAL;
    const int nQ = (grad_phase ? 1 : 0) + (grad_rest ? 1 : 0);
    if (int e = trs_signal_check(dtype, rx, nRx, work, work_bytes, nQ ? trs_workspace(N, nM, K, nQ) : 0)) return e;
    const bool wantbank = grad_A || grad_B;
    const size_t need = wantbank ? seq_bank_bytes(P, N, nM) : 0;
    if (need && !bank) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype);
    if (align || !aligned_to(grad_sig, sizeof(double)) || !aligned_to(grad_Mlast, ts) || !aligned_to(ck, sizeof(double)) ||
        !aligned_to(grad_A, ts) || !aligned_to(grad_B, ts) || !aligned_to(grad_consts, sizeof(double)) ||
        !aligned_to(grad_rest, sizeof(double)) || !aligned_to(grad_Mi, ts) || !aligned_to(grad_phase, sizeof(double)) ||
        !aligned_to(grad_rx, ts) || !aligned_to(bank, sizeof(double)))
        return MRPHY_EALIGN;
    if (bank_bytes < need) return MRPHY_ENOSPC;
    SeqSigArgs a{};
    seq_fill(a.s, A, B, P, pulse, rs, rs_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, Mi, Mi_sn,
             Mi_sm, cs, cs_sn, N, nM, K);
    a.s.gC = grad_consts; a.s.gMi = grad_Mi;
    a.s.work = wantbank ? reinterpret_cast<double*>(bank) : nullptr;
    a.rx = rx; a.nRx = nRx; a.ck = const_cast<double*>(reinterpret_cast<const double*>(ck));
    a.sums = nQ ? reinterpret_cast<double*>(work) : nullptr;
    a.nQ = nQ; a.qphi = grad_phase ? 0 : -1; a.qrest = grad_rest ? nQ - 1 : -1;
    a.gs = reinterpret_cast<const double*>(grad_sig); a.gMl = grad_Mlast; a.grx = grad_rx;
    a.N = N; a.Pw = trs_waves(nM);
    hipStream_t st = (hipStream_t)stream;
    if (wantbank)
        if (hipError_t e = hipMemsetAsync(bank, 0, need, st)) return (int)e;
    if (dtype == MRPHY_F32) launch_main<float, true>(a, trs_capacity(nRx), st);
    else                    launch_main<double, true>(a, trs_capacity(nRx), st);
    if (int e = launch_status()) return e;
    // the sums over the spins stay fp64 whatever the data type: the caller folds them further before rounding
    if (grad_phase)
        if (int e = trs_launch_p2<double>(a.sums, (double*)grad_phase, N, nQ, a.qphi, K, a.Pw, 0, st)) return e;
    if (grad_rest)
        if (int e = trs_launch_p2<double>(a.sums, (double*)grad_rest, N, nQ, a.qrest, K, a.Pw, 0, st)) return e;
    if (!wantbank) return 0;
    return seq_launch_bank_p2(dtype, a.s.work, grad_A, grad_B, a.s.rows, P, st);
}

}  // extern "C"

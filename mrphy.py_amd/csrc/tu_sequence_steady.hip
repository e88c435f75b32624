// tu_sequence_steady.hip -- the steady state of a scheduled period (Ksq's K repetitions composed and solved for their
// fixed point): the entry points of the C ABI together with their kernels (k_sequence_steady.hpp on k_ab_train.hpp,
// k_train_signal.hpp and k_ab_sequence.hpp).  The adjoint forms lambda here and hands the sweep to
// mrphy_sequence_signal_bwd (tu_sequence_signal.hip): Ksqsb from the checkpoints, no signal cotangent, lambda as the
// cotangent of the last state -- there is no second copy of the sweep.  Two data types, no constant type.
#include "host_common.hpp"

namespace {
#include "k_ab_train.hpp"
#include "k_train_signal.hpp"
#include "k_ab_sequence.hpp"
#include "k_sequence_steady.hpp"
}  // namespace

extern "C" {

int mrphy_sequence_steadystate_fwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                                   const void* rs, int64_t rs_sn, const void* T1, int64_t T1_sn, int64_t T1_sm,
                                   const void* T2, int64_t T2_sn, int64_t T2_sm, const void* df, int64_t df_sn,
                                   int64_t df_sm, const void* cs, int64_t cs_sn, void* Mss, void* per, void* ck,
                                   int64_t N, int64_t nM, int64_t K, void* stream)
{
    bool empty; int align;
    if (int e = seq_check(dtype, A, B, P, pulse, rs, T1, T2, df, nullptr, cs, N, nM, K, true, empty, align)) return e;
    if (empty) return 0;
    if (!Mss) return MRPHY_EINVAL;
    if (align || !aligned_to(Mss, tsize(dtype)) || !aligned_to(per, sizeof(double)) || !aligned_to(ck, sizeof(double)))
        return MRPHY_EALIGN;
    SeqSteadyArgs a{};
    seq_fill(a.s, A, B, P, pulse, rs, rs_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, nullptr, 0,
             0, cs, cs_sn, N, nM, K);
    a.Mss = Mss; a.per = reinterpret_cast<double*>(per); a.ck = reinterpret_cast<double*>(ck);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((nM + 255) / 256), (unsigned)N);
    if (dtype == MRPHY_F32) hipLaunchKernelGGL((k_sequence_steady_fwd<float>), grid, dim3(256), 0, st, a);
    else                    hipLaunchKernelGGL((k_sequence_steady_fwd<double>), grid, dim3(256), 0, st, a);
    return launch_status();
}

int mrphy_sequence_steadystate_bwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                                   const void* grad_Mss, const void* rs, int64_t rs_sn, const void* T1, int64_t T1_sn,
                                   int64_t T1_sm, const void* T2, int64_t T2_sn, int64_t T2_sm, const void* df,
                                   int64_t df_sn, int64_t df_sm, const void* cs, int64_t cs_sn, const void* per,
                                   const void* ck, void* lam, void* grad_A, void* grad_B, void* grad_consts,
                                   void* grad_rest, void* grad_phase, void* work, size_t work_bytes, void* bank,
                                   size_t bank_bytes, int64_t N, int64_t nM, int64_t K, void* stream)
{
    bool empty; int align;
    if (int e = seq_check(dtype, A, B, P, pulse, rs, T1, T2, df, nullptr, cs, N, nM, K, true, empty, align)) return e;
    if (empty) return 0;
    if (!grad_Mss || !per || !ck || !lam || (!grad_A && !grad_B && !grad_consts && !grad_rest && !grad_phase))
        return MRPHY_EINVAL;
    // the workspaces in mrphy_sequence_signal_bwd's order, so that the sweep below has nothing left to refuse once
    // lambda has been launched
    const int nQ = (grad_phase ? 1 : 0) + (grad_rest ? 1 : 0);
    const size_t need_w = nQ ? mrphy_sequence_signal_workspace(dtype, N, nM, K, nQ) : 0;
    if (!aligned_to(work, sizeof(double))) return MRPHY_EALIGN;
    if (need_w && (!work || work_bytes < need_w)) return work ? MRPHY_ENOSPC : MRPHY_EINVAL;
    const size_t need_b = (grad_A || grad_B) ? mrphy_sequence_signal_bank_workspace(dtype, P, N, nM) : 0;
    if (need_b && !bank) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype);
    if (align || !aligned_to(grad_Mss, ts) || !aligned_to(per, sizeof(double)) || !aligned_to(ck, sizeof(double)) ||
        !aligned_to(lam, ts) || !aligned_to(grad_A, ts) || !aligned_to(grad_B, ts) ||
        !aligned_to(grad_consts, sizeof(double)) || !aligned_to(grad_rest, sizeof(double)) ||
        !aligned_to(grad_phase, sizeof(double)) || !aligned_to(bank, sizeof(double)))
        return MRPHY_EALIGN;
    if (bank_bytes < need_b) return MRPHY_ENOSPC;
    SeqSteadyArgs a{};
    a.s.rows = N * nM; a.s.nM = nM; a.s.K = K;
    a.per = const_cast<double*>(reinterpret_cast<const double*>(per)); a.g = grad_Mss; a.lam = lam;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((a.s.rows + 255) / 256));
    if (dtype == MRPHY_F32) hipLaunchKernelGGL((k_sequence_steady_lambda<float>), grid, dim3(256), 0, st, a);
    else                    hipLaunchKernelGGL((k_sequence_steady_lambda<double>), grid, dim3(256), 0, st, a);
    if (int e = launch_status()) return e;
    // Ksqsb on the period started at Mss: the states come from ck, so Mi is not read; one coil without a map and no
    // signal cotangent: grad_Mlast = lambda alone drives the sweep
    return mrphy_sequence_signal_bwd(dtype, A, B, P, pulse, nullptr, lam, rs, rs_sn, T1, T1_sn, T1_sm, T2, T2_sn, T2_sm,
                                     df, df_sn, df_sm, nullptr, 0, 0, cs, cs_sn, nullptr, 1, ck, grad_A, grad_B,
                                     grad_consts, grad_rest, nullptr, grad_phase, nullptr, work, work_bytes, bank,
                                     bank_bytes, N, nM, K, stream);
}

}  // extern "C"

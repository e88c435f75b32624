// tu_ab_sequence.hip -- a train with a pulse of a bank and a rest per repetition, from Hargreaves' A, B: the entry
// points of the C ABI together with their kernels (k_ab_sequence.hpp on k_ab_train.hpp, train_rep of
// k_train_signal.hpp).  Two data types, no constant type, as tu_ab_train.hip.
#include "host_common.hpp"

namespace {
#include "k_ab_train.hpp"
#include "k_train_signal.hpp"
#include "k_ab_sequence.hpp"
}  // namespace

extern "C" {

size_t mrphy_ab_sequence_bwd_workspace(int dtype, int64_t P, int64_t N, int64_t nM)
{
    if ((dtype != MRPHY_F32 && dtype != MRPHY_F64) || P <= 0 || N <= 0 || nM <= 0) return 0;
    return seq_bank_bytes(P, N, nM);
}

int mrphy_ab_sequence_fwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse, const void* rs,
                          int64_t rs_sn, const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2, int64_t T2_sn,
                          int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm, const void* Mi, int64_t Mi_sn,
                          int64_t Mi_sm, const void* cs, int64_t cs_sn, void* Mt, int64_t N, int64_t nM, int64_t K,
                          void* stream)
{
    bool empty; int align;
    if (int e = seq_check(dtype, A, B, P, pulse, rs, T1, T2, df, Mi, cs, N, nM, K, false, empty, align)) return e;
    if (empty) return 0;
    if (!Mt) return MRPHY_EINVAL;
    if (align || !aligned_to(Mt, tsize(dtype))) return MRPHY_EALIGN;
    SeqArgs q{};
    seq_fill(q, A, B, P, pulse, rs, rs_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, Mi, Mi_sn,
             Mi_sm, cs, cs_sn, N, nM, K);
    q.Mt = Mt;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((nM + 255) / 256), (unsigned)N);
    if (dtype == MRPHY_F32) hipLaunchKernelGGL((k_ab_sequence_fwd<float>), grid, dim3(256), 0, st, q);
    else                    hipLaunchKernelGGL((k_ab_sequence_fwd<double>), grid, dim3(256), 0, st, q);
    return launch_status();
}

int mrphy_ab_sequence_jvp_max_dirs(int dtype)
{
    if (dtype != MRPHY_F32 && dtype != MRPHY_F64) return MRPHY_EINVAL;
    return seq_jvp_max_dirs(tsize(dtype));
}

// Ksqj: the forward's checks in its order; then the direction count against the capacity, the tangents whose operand the
// call does not have (dT1 / dT2 without T1, ddf / drest / dT* without a rest table), the required dMt (Mt is not), the
// alignment of what it adds.  The build is the smallest capacity 1, 2, 4 that holds D (tu_ab_sequence_jvp1 / 2 / 4.hip)
int mrphy_ab_sequence_jvp_fwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse, const void* rs,
                              int64_t rs_sn, const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2, int64_t T2_sn,
                              int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm, const void* Mi, int64_t Mi_sn,
                              int64_t Mi_sm, const void* cs, int64_t cs_sn, int64_t D, const void* dA, const void* dB,
                              const void* dMi, const void* dT1, const void* dT2, const void* ddf, const void* dphase,
                              int64_t dphase_sn, const void* drest, int64_t drest_sn, void* Mt, void* dMt, int64_t N,
                              int64_t nM, int64_t K, void* stream)
{
    bool empty; int align;
    if (int e = seq_check(dtype, A, B, P, pulse, rs, T1, T2, df, Mi, cs, N, nM, K, false, empty, align)) return e;
    if (empty) return 0;
    if (D < 1 || D > seq_jvp_max_dirs(tsize(dtype))) return MRPHY_EINVAL;
    if (((dT1 || dT2) && !T1) || ((ddf || drest || dT1 || dT2) && !rs)) return MRPHY_EINVAL;
    if (!dMt) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype);
    if (align || !aligned_to(Mt, ts) || !aligned_to(dMt, ts) || !aligned_to(dA, ts) || !aligned_to(dB, ts) ||
        !aligned_to(dMi, ts) || !aligned_to(dT1, ts) || !aligned_to(dT2, ts) || !aligned_to(ddf, ts) ||
        !aligned_to(dphase, sizeof(double)) || !aligned_to(drest, sizeof(double)))
        return MRPHY_EALIGN;
    const SeqJvpCall c{A, B, P, pulse, rs, rs_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm},
                       Mi, Mi_sn, Mi_sm, cs, cs_sn, D, dA, dB, dMi, dT1, dT2, ddf, dphase, dphase_sn, drest, drest_sn,
                       Mt, dMt, N, nM, K};
    hipStream_t st = (hipStream_t)stream;
    using namespace mrphy_i;
#define MRPHY_SQJ(MD_) \
    return dtype == MRPHY_F32 ? run_ab_sequence_jvp<MD_, float>(c, st) : run_ab_sequence_jvp<MD_, double>(c, st)
    if (D == 1) { MRPHY_SQJ(1); }
    if (D == 2) { MRPHY_SQJ(2); }
    MRPHY_SQJ(4);
#undef MRPHY_SQJ
}
static_assert(SEQ_JVP_MAXD_F32 == 4 && SEQ_JVP_MAXD_F64 == 4, "mrphy_ab_sequence_jvp_fwd: every capacity in every data type");

int mrphy_ab_sequence_bwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse, const void* grad_Mt,
                          const void* rs, int64_t rs_sn, const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2,
                          int64_t T2_sn, int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm, const void* Mi,
                          int64_t Mi_sn, int64_t Mi_sm, const void* cs, int64_t cs_sn, const void* Mt, void* grad_A,
                          void* grad_B, void* grad_consts, void* grad_rest, void* grad_Mi, void* grad_phase, void* work,
                          size_t work_bytes, int64_t N, int64_t nM, int64_t K, void* stream)
{
    bool empty; int align;
    if (int e = seq_check(dtype, A, B, P, pulse, rs, T1, T2, df, Mi, cs, N, nM, K, false, empty, align)) return e;
    if (empty) return 0;
    if (!grad_Mt || !Mt || (!grad_A && !grad_B && !grad_consts && !grad_rest && !grad_Mi && !grad_phase))
        return MRPHY_EINVAL;
    const bool bank = grad_A || grad_B;
    const size_t need = bank ? seq_bank_bytes(P, N, nM) : 0;
    if (need && !work) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype);
    if (align || !aligned_to(grad_Mt, ts) || !aligned_to(Mt, ts) || !aligned_to(grad_A, ts) || !aligned_to(grad_B, ts) ||
        !aligned_to(grad_consts, ts) || !aligned_to(grad_rest, ts) || !aligned_to(grad_Mi, ts) ||
        !aligned_to(grad_phase, ts) || !aligned_to(work, sizeof(double)))
        return MRPHY_EALIGN;
    if (work_bytes < need) return MRPHY_ENOSPC;
    SeqArgs q{};
    seq_fill(q, A, B, P, pulse, rs, rs_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, Mi, Mi_sn,
             Mi_sm, cs, cs_sn, N, nM, K);
    q.g = grad_Mt; q.Mt = const_cast<void*>(Mt);
    q.gC = grad_consts; q.grest = grad_rest; q.gMi = grad_Mi; q.gphi = grad_phase;
    q.work = bank ? reinterpret_cast<double*>(work) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (bank)
        if (hipError_t e = hipMemsetAsync(work, 0, need, st)) return (int)e;
    const dim3 grid((unsigned)((nM + 255) / 256), (unsigned)N);
    if (dtype == MRPHY_F32) hipLaunchKernelGGL((k_ab_sequence_bwd<float>), grid, dim3(256), 0, st, q);
    else                    hipLaunchKernelGGL((k_ab_sequence_bwd<double>), grid, dim3(256), 0, st, q);
    if (int e = launch_status()) return e;
    if (!bank) return 0;
    return seq_launch_bank_p2(dtype, q.work, grad_A, grad_B, q.rows, P, st);
}

}  // extern "C"

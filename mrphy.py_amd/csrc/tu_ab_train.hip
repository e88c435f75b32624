// tu_ab_train.hip -- the transient of a pulse repeated K times from Hargreaves' A, B: the two entry points of the C ABI
// together with their kernels (k_ab_train.hpp).  Two data types, no constant type, as tu_ab_steady.hip.
#include "host_common.hpp"

namespace {
#include "k_ab_train.hpp"
}  // namespace

extern "C" {

int mrphy_ab_train_fwd(int dtype, const void* A, const void* B, const void* rest, int64_t rest_sn,
                       const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2, int64_t T2_sn, int64_t T2_sm,
                       const void* df, int64_t df_sn, int64_t df_sm, const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                       const void* cs, int64_t cs_sn, void* Mt, int64_t N, int64_t nM, int64_t K, void* stream)
{
    bool empty;
    if (int e = train_check(dtype, A, B, rest, T1, T2, df, Mi, cs, N, nM, K, empty)) return e;
    if (empty) return 0;
    if (!Mt) return MRPHY_EINVAL;
    if (!aligned_to(Mt, tsize(dtype))) return MRPHY_EALIGN;
    TrainArgs q{};
    train_fill(q, A, B, rest, rest_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, Mi, Mi_sn, Mi_sm,
               cs, cs_sn, N, nM, K);
    q.Mt = Mt;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((nM + 255) / 256), (unsigned)N);
    if (dtype == MRPHY_F32) hipLaunchKernelGGL((k_ab_train_fwd<float>), grid, dim3(256), 0, st, q);
    else                    hipLaunchKernelGGL((k_ab_train_fwd<double>), grid, dim3(256), 0, st, q);
    return launch_status();
}

int mrphy_ab_train_bwd(int dtype, const void* A, const void* B, const void* grad_Mt, const void* rest,
                       int64_t rest_sn, const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2, int64_t T2_sn,
                       int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm, const void* Mi, int64_t Mi_sn,
                       int64_t Mi_sm, const void* cs, int64_t cs_sn, const void* Mt, void* grad_A, void* grad_B,
                       void* grad_consts, void* grad_Mi, void* grad_phase, int64_t N, int64_t nM, int64_t K,
                       void* stream)
{
    bool empty;
    if (int e = train_check(dtype, A, B, rest, T1, T2, df, Mi, cs, N, nM, K, empty)) return e;
    if (empty) return 0;
    if (!grad_Mt || !Mt || (!grad_A && !grad_B && !grad_consts && !grad_Mi && !grad_phase)) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype);
    if (!aligned_to(grad_Mt, ts) || !aligned_to(Mt, ts) || !aligned_to(grad_A, ts) || !aligned_to(grad_B, ts) ||
        !aligned_to(grad_consts, ts) || !aligned_to(grad_Mi, ts) || !aligned_to(grad_phase, ts))
        return MRPHY_EALIGN;
    TrainArgs q{};
    train_fill(q, A, B, rest, rest_sn, Bc{T1, T1_sn, T1_sm}, Bc{T2, T2_sn, T2_sm}, Bc{df, df_sn, df_sm}, Mi, Mi_sn, Mi_sm,
               cs, cs_sn, N, nM, K);
    q.g = grad_Mt; q.Mt = const_cast<void*>(Mt);
    q.gA = grad_A; q.gB = grad_B; q.gC = grad_consts; q.gMi = grad_Mi; q.gphi = grad_phase;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((nM + 255) / 256), (unsigned)N);
    if (dtype == MRPHY_F32) hipLaunchKernelGGL((k_ab_train_bwd<float>), grid, dim3(256), 0, st, q);
    else                    hipLaunchKernelGGL((k_ab_train_bwd<double>), grid, dim3(256), 0, st, q);
    return launch_status();
}

}  // extern "C"

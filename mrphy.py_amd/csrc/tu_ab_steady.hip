// tu_ab_steady.hip -- the steady state of a periodic pulse from Hargreaves' A, B: the two entry points of the C ABI
// together with their kernels (k_ab_steady.hpp).  Two data types, no constant type, as tu_aux.hip.
#include "host_common.hpp"

namespace {
#include "k_ab_steady.hpp"

// What both entry points check alike, in the order of the other entry points: dtype and sizes, the empty problem (0),
// null pointers and the operand rules, alignment.  `empty` is set for a problem without spins.
int steady_check(int dtype, const void* A, const void* B, const void* rest, const void* T1, const void* T2,
                 const void* df, int64_t N, int64_t nM, bool& empty)
{
    empty = false;
    if ((dtype != MRPHY_F32 && dtype != MRPHY_F64) || N < 0 || nM < 0) return MRPHY_EINVAL;
    if (N * nM == 0) { empty = true; return 0; }
    if ((N * nM + 255) / 256 > (int64_t)0x7fffffff) return MRPHY_EINVAL;
    if (!A || !B) return MRPHY_EINVAL;
    if (!rest && (T1 || T2 || df)) return MRPHY_EINVAL;               // no rest period: nothing to relax or precess in
    if ((T1 == nullptr) != (T2 == nullptr)) return MRPHY_EINVAL;      // both or neither
    const size_t ts = tsize(dtype);
    if (!aligned_to(A, ts) || !aligned_to(B, ts) || !aligned_to(rest, ts) || !aligned_to(T1, ts) ||
        !aligned_to(T2, ts) || !aligned_to(df, ts))
        return MRPHY_EALIGN;
    return 0;
}
}  // namespace

extern "C" {

int mrphy_ab_steadystate_fwd(int dtype, const void* A, const void* B, const void* rest, int64_t rest_sn,
                             const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2, int64_t T2_sn,
                             int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm, void* Mss, int64_t N,
                             int64_t nM, void* stream)
{
    bool empty;
    if (int e = steady_check(dtype, A, B, rest, T1, T2, df, N, nM, empty)) return e;
    if (empty) return 0;
    if (!Mss) return MRPHY_EINVAL;
    if (!aligned_to(Mss, tsize(dtype))) return MRPHY_EALIGN;
    SteadyArgs q{};
    q.A = A; q.B = B; q.rest = rest; q.rest_sn = rest_sn;
    q.T1 = Bc{T1, T1_sn, T1_sm}; q.T2 = Bc{T2, T2_sn, T2_sm}; q.df = Bc{df, df_sn, df_sm};
    q.Mss = Mss; q.rows = N * nM; q.nM = nM;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((q.rows + 255) / 256));
    if (dtype == MRPHY_F32) hipLaunchKernelGGL((k_ab_steadystate_fwd<float>), grid, dim3(256), 0, st, q);
    else                    hipLaunchKernelGGL((k_ab_steadystate_fwd<double>), grid, dim3(256), 0, st, q);
    return launch_status();
}

int mrphy_ab_steadystate_bwd(int dtype, const void* A, const void* B, const void* grad_Mss, const void* rest,
                             int64_t rest_sn, const void* T1, int64_t T1_sn, int64_t T1_sm, const void* T2,
                             int64_t T2_sn, int64_t T2_sm, const void* df, int64_t df_sn, int64_t df_sm,
                             void* grad_A, void* grad_B, void* grad_consts, int64_t N, int64_t nM, void* stream)
{
    bool empty;
    if (int e = steady_check(dtype, A, B, rest, T1, T2, df, N, nM, empty)) return e;
    if (empty) return 0;
    if (!grad_Mss || (!grad_A && !grad_B && !grad_consts)) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype);
    if (!aligned_to(grad_Mss, ts) || !aligned_to(grad_A, ts) || !aligned_to(grad_B, ts) || !aligned_to(grad_consts, ts))
        return MRPHY_EALIGN;
    SteadyArgs q{};
    q.A = A; q.B = B; q.g = grad_Mss; q.rest = rest; q.rest_sn = rest_sn;
    q.T1 = Bc{T1, T1_sn, T1_sm}; q.T2 = Bc{T2, T2_sn, T2_sm}; q.df = Bc{df, df_sn, df_sm};
    q.gA = grad_A; q.gB = grad_B; q.gC = grad_consts; q.rows = N * nM; q.nM = nM;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((q.rows + 255) / 256));
    if (dtype == MRPHY_F32) hipLaunchKernelGGL((k_ab_steadystate_bwd<float>), grid, dim3(256), 0, st, q);
    else                    hipLaunchKernelGGL((k_ab_steadystate_bwd<double>), grid, dim3(256), 0, st, q);
    return launch_status();
}

}  // extern "C"

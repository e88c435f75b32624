// tu_blochsim_bwd.hip -- K3: launcher of mrphy_blochsim_bwd / _bwd_consts (line-granular and chunked adjoint kernels)
#include "host_common.hpp"

namespace {
#include "k_blochsim_bwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_bwd(HistParts hist, const void* Beff, Bc g, Bc E1, Bc E2, const void* gMo, void* gMi,
            void* gBeff, void* gC, int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    BwdArgs<T> a;
    a.hist = hist; a.Beff = (const T*)Beff; a.gMo = (const T*)gMo;
    a.gMi = (T*)gMi; a.gBeff = (T*)gBeff; a.gC = (T*)gC;
    a.g = g; a.E1 = E1; a.E2 = E2;
    a.rows = N * nM; a.nM = nM; a.nT = nT;
    a.vec_ok = aligned_to(Beff, sizeof(T)) && (!gBeff || aligned_to(gBeff, sizeof(T)));
    a.per_xcd = 0;
    if (a.rows == 0) return 0;
    dim3 grid((unsigned)((a.rows + WAVE - 1) / WAVE));
    if (gC) {      // gradients w.r.t. the constants as well: the chunked kernel's GC build (any shape)
        hipLaunchKernelGGL((k_bloch_bwd<T, CT, TC_BWD<T>, true>), grid, dim3(WAVE), 0, st, a);
        return launch_status();
    }
    if (lines_shape_ok<T>(Beff, nT) && (!gBeff || aligned_to(gBeff, LINE_BYTES))) {
        // The line-granular adjoints, XCD-contiguous tile order: fp32 at 3 waves/SIMD, fp64 at 2 (the chunked fp64
        // adjoint needs 430-456 VGPRs = one).  The A/Bs: docs/LABNOTES.md, "K1 / K3 launchers: how the builds were chosen".
        a.per_xcd = xcd_pad(grid);
        if constexpr (sizeof(T) == 8) {
            if (E1.p) hipLaunchKernelGGL((k_bloch_bwd_lines_f64<CT, true>), grid, dim3(WAVE), 0, st, a);
            else      hipLaunchKernelGGL((k_bloch_bwd_lines_f64<CT, false>), grid, dim3(WAVE), 0, st, a);
        } else {
            if (E1.p) hipLaunchKernelGGL((k_bloch_bwd_lines<CT, true>), grid, dim3(WAVE), 0, st, a);
            else      hipLaunchKernelGGL((k_bloch_bwd_lines<CT, false>), grid, dim3(WAVE), 0, st, a);
        }
        return launch_status();
    }
    hipLaunchKernelGGL((k_bloch_bwd<T, CT, TC_BWD<T>, false>), grid, dim3(WAVE), 0, st, a);
    return launch_status();
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_bwd<T_, CT_>(HistParts hist, const void* Beff, Bc g, Bc E1, Bc E2, const void* gMo, void* gMi, void* gBeff, void* gC, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

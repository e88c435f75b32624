// tu_blochsim_fwd.hip -- K1: launcher of mrphy_blochsim_fwd / _1step (line-granular and chunked forward kernels)
#include "host_common.hpp"

namespace {
#include "k_blochsim_fwd.hpp"
}  // namespace

namespace mrphy_i {

template <typename T, typename CT>
int run_fwd(const void* Mi, const void* Beff, Bc g, Bc E1, Bc E2, const void* E1m1, void* Mo,
            HistParts hist, int64_t N, int64_t nM, int64_t nT, hipStream_t st)
{
    FwdArgs<T> a;
    a.Mi = (const T*)Mi; a.Beff = (const T*)Beff; a.Mo = (T*)Mo; a.hist = hist;
    const bool Mpre = hist.n_parts > 0;            // the history-saving builds (K1h)
    a.g = g; a.E1 = E1; a.E2 = E2; a.E1m1 = E1m1;
    a.rows = N * nM; a.nM = nM; a.nT = nT;
    // vector path of the chunked kernel (16-B global accesses need element alignment only)
    a.vec_ok = aligned_to(Beff, sizeof(T));      // element alignment is enough (V16::utype)
    a.per_xcd = 0;
    if (a.rows == 0) return 0;
    dim3 grid((unsigned)((a.rows + WAVE - 1) / WAVE));
    if (lines_shape_ok<T>(Beff, nT)) {
        // The line-granular kernels.  XCD-contiguous tile order where the kernel writes (the history); the read-only
        // forward runs in plain order behind a K0 that writes Beff with `sc1 nt` stores.  Which build runs which mode:
        // docs/LABNOTES.md, "K1 / K3 launchers: how the builds were chosen".
        if (Mpre) a.per_xcd = xcd_pad(grid);
#define MRPHY_L(K_, ...)                                                                         \
    do {                                                                                         \
        if (E1.p) hipLaunchKernelGGL((K_<CT, true, __VA_ARGS__>), grid, dim3(WAVE), 0, st, a);   \
        else      hipLaunchKernelGGL((K_<CT, false, __VA_ARGS__>), grid, dim3(WAVE), 0, st, a);  \
    } while (0)
        if constexpr (sizeof(T) == 8) {         // fp64: one schedule (batches of 2/2/1), with or without history
            if (Mpre) MRPHY_L(k_bloch_fwd_lines_f64, true);
            else      MRPHY_L(k_bloch_fwd_lines_f64, false);
        } else if (Mpre) {                      // with history: 3-/4-step batches, 3 waves/SIMD
            MRPHY_L(k_bloch_fwd_lines, 3, true, false);
        } else if (CTr<CT>::precise) {          // precise step: pinned 5-/6-step batches
            MRPHY_L(k_bloch_fwd_lines, 2, false, true);
        } else {                                // fast step: unpinned 3-/4-step batches
            MRPHY_L(k_bloch_fwd_lines, 3, false, false);
        }
#undef MRPHY_L
        return launch_status();
    }
    if (Mpre)
        hipLaunchKernelGGL((k_bloch_fwd<T, CT, TC_FWD<T>, true>), grid, dim3(WAVE), 0, st, a);
    else
        hipLaunchKernelGGL((k_bloch_fwd<T, CT, TC_FWD<T>, false>), grid, dim3(WAVE), 0, st, a);
    return launch_status();
}

}  // namespace mrphy_i

#define MRPHY_INST(T_, CT_) template int mrphy_i::run_fwd<T_, CT_>(const void* Mi, const void* Beff, Bc g, Bc E1, Bc E2, const void* E1m1, void* Mo, HistParts hist, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
MRPHY_FOR_DTYPES(MRPHY_INST)
#undef MRPHY_INST

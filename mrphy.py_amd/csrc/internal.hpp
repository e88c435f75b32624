// internal.hpp -- the launchers behind the C ABI.  abi.hip validates arguments and dispatches on the dtype
// code; the launchers (and the kernels they start) live in the tu_*.hip units, one explicit instantiation
// per dtype code, so that the library compiles as independent units in parallel (mrphy_amd._lib.build).
// Hidden visibility: none of this is part of the exported interface (include/mrphy_hip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "geom.hpp"

#pragma GCC visibility push(hidden)
namespace mrphy_i {
using mrphy::Bc;
using mrphy::PulseOps;
using mrphy::AdjointReq;
using mrphy::BzExt;
using mrphy::JvpTangents;
using mrphy::SeqJvpCall;
using mrphy::HistParts;

template <typename T, typename CT>
int run_fwd(const void* Mi, const void* Beff, Bc g, Bc E1, Bc E2, const void* E1m1, void* Mo,
            HistParts hist, int64_t N, int64_t nM, int64_t nT, hipStream_t st);

template <typename T, typename CT>
int run_bwd(HistParts hist, const void* Beff, Bc g, Bc E1, Bc E2, const void* gMo, void* gMi,
            void* gBeff, void* gC, int64_t N, int64_t nM, int64_t nT, hipStream_t st);

template <typename T>
int run_rfgr2beff(const void* rf, int64_t rf_sn, const void* gr, int64_t gr_sn, const void* loc,
                  Bc df, Bc gam, const void* b1, void* beff, int64_t N, int64_t nM, int64_t nT,
                  int64_t nC, int store, hipStream_t st);

template <typename T>
int run_rfgr2beff_bwd(const void* gB, const void* loc, const void* b1, void* grf, void* ggr,
                      void* work, int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st);

// The fused family.  Its operands -- the pulse on the spins and the step constants -- travel as ONE struct, PulseOps
// (geom.hpp): abi.hip packs and checks it, every launcher below takes it by value and hands it on to its kernel's
// argument struct in one assignment.  What differs between the members follows it.
// K2 / K2b and their trajectory builds K2t / K2bt (the same kernels, trailing mode parameter): a null Mt / gMt runs
// the plain kernel, which writes Mo / reads gMo; otherwise Mt / gMt hold the records taken every `every` steps
template <typename T, typename CT>
int run_rfgr_fwd(const void* Mi, PulseOps in, void* Mo, void* Mck, int64_t ck_every, void* Mt, int64_t every,
                 int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st);

// the one-coil float builds of K2 live in a unit of their own (tu_fused_fwd1.hip: compiled with the max-ILP
// scheduling strategy, which the multi-coil and fp64 builds pay for in registers); called by run_rfgr_fwd
template <typename T, typename CT>
int run_rfgr_fwd1(const void* Mi, PulseOps in, void* Mo, void* Mck, int64_t ck_every, void* Mt, int64_t every,
                  int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st);

// K2s / K2bs: the received signal of the fused simulation (one transmit coil) for nRx <= sig_max_rx receive coils in one
// launch, rx (N, nM, 2, nRx), sig / gsig (N, 2, nRec, nRx).  The forward has one unit per coil capacity R >= nRx
// (tu_signal.hip: 1, where rx may be null = (1, 0); tu_signal_mrx2 / 4 / 8.hip).  Its adjoint takes a non-null
// gsig (the cotangent of the samples) and the receive map rx, and gMo may then be null: the builds PLAIN for one coil
// and MRX for more of run_fused_bwd below
template <typename T, typename CT, int R>
int run_signal_fwd(const void* Mi, PulseOps in, const void* rx, int64_t nRx, void* Mo, void* Mck, int64_t ck_every,
                   void* sig, int64_t every, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);

// The adjoints of the fused family: ONE launcher declaration.  A build is the set of kernels one translation unit
// compiles; each tu_*_bwd unit defines run_fused_bwd for its own build and instantiates it for its dtype codes.  The call
// travels as the request (geom.hpp: AdjointReq) next to the operands; abi.hip has validated both and chosen the build.
enum class AdjBuild {
    PLAIN,      // tu_fused_bwd.hip: K2b, K2bt (a non-null gMt), and K2bs at a capacity of 1 receive coil (a non-null gsig)
    MRX,        // tu_fused_mrx_bwd.hip: K2bs at the smallest capacity 2, 4, 8 that holds nRx; gsig is not null
    MAPS,       // tu_fused_maps_bwd.hip: K2b / K2bt that also return gloc, gBz, gb1, each of which may be null
    CONSTS,     // tu_fused_consts_bwd.hip: the MAPS builds that also return gC = [dL/dg, dL/dE1, dL/dE2, dL/dE1m1] per spin
    SIG_CONSTS1, SIG_CONSTS2, SIG_CONSTS4, SIG_CONSTS8,     // tu_signal_consts1 / 2 / 4 / 8_bwd.hip, one unit per capacity
                // R >= nRx: K2bs that also returns gC; gsig is not null, rx may be null at R = 1 only
    MC,         // tu_fused_mc_bwd.hip: K2b / K2bt for nC <= K2B_MAXC transmit coils with their b1 map
    MOVING,     // tu_fused_moving_bwd.hip: K2vb, K2b's mode 0 for spins at constant velocity (r.ext: vdt, step0)
    SHIM2, SHIM4, SHIM8,    // tu_fused_shim2 / 4 / 8_bwd.hip, one unit per capacity MS >= nS: K2shb, K2b's mode 0 with nS extra
                // Bz field channels (r.ext: sh, sh_sn, shMap, nS); ggr is the lead buffer (N, 3 + nS, nT), the workspace
                // that of mrphy_blochsim_rfgr_shim_bwd_workspace
};
constexpr AdjBuild sig_consts_build(int R)
{
    return R == 1 ? AdjBuild::SIG_CONSTS1 : R == 2 ? AdjBuild::SIG_CONSTS2 : R == 4 ? AdjBuild::SIG_CONSTS4
                                                                                      : AdjBuild::SIG_CONSTS8;
}
// K2sh / K2shb: the build of the smallest channel capacity 2, 4, 8 that holds nS (every data type has them all)
constexpr AdjBuild shim_build(int64_t nS)
{
    return nS <= 2 ? AdjBuild::SHIM2 : nS <= 4 ? AdjBuild::SHIM4 : AdjBuild::SHIM8;
}
static_assert(mrphy::SHIM_MAXS_F32 == 8 && mrphy::SHIM_MAXS_F64 == 8, "shim_build: every capacity in every data type");
template <AdjBuild B, typename T, typename CT>
int run_fused_bwd(const AdjointReq& r, PulseOps in, hipStream_t st);

// K2v and K2sh, the forwards of the builds MOVING and SHIM2 / 4 / 8 (tu_fused_moving_fwd.hip, tu_fused_shim2 / 4 / 8_fwd.hip):
// K2 for spins at constant velocity, resp. with nS <= MS extra Bz field channels; one transmit coil, the extension by value
template <AdjBuild B, typename T, typename CT>
int run_rfgr_ext_fwd(const void* Mi, PulseOps in, BzExt x, void* Mo, void* Mck, int64_t ck_every, int64_t N, int64_t nM,
                     int64_t nT, hipStream_t st);

// K2j (tu_fused_jvp1 / 2 / 4_fwd.hip, one unit per direction capacity MD >= tg.D): K2 with the forward-mode tangents of
// Mo along tg.D directions; one transmit coil, Mo may be null
template <int MD, typename T, typename CT>
int run_rfgr_jvp(const void* Mi, PulseOps in, JvpTangents tg, void* Mo, void* dMo, int64_t N, int64_t nM, int64_t nT,
                 hipStream_t st);

// Ksqj (tu_ab_sequence_jvp1 / 2 / 4.hip, one unit per direction capacity MD >= c.D): Ksq with the forward-mode tangents
// of its records along c.D directions; checked by mrphy_ab_sequence_jvp_fwd (tu_ab_sequence.hip)
template <int MD, typename T>
int run_ab_sequence_jvp(SeqJvpCall c, hipStream_t st);

// K2ab / K2abb (tu_ab_rfgr_fwd.hip, tu_ab_rfgr_bwd.hip): Hargreaves' A, B of the fused family's operands, one transmit
// coil, and the adjoint w.r.t. the pulse.  ABck (nCk, 4, N*nM, 3): the four columns' checkpoints, null for none
template <typename T, typename CT>
int run_ab_rfgr_fwd(PulseOps in, void* A, void* B, void* ABck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT,
                    hipStream_t st);

template <typename T, typename CT>
int run_ab_rfgr_bwd(const void* ABck, PulseOps in, const void* gA, const void* gB, void* grf, void* ggr, void* work,
                    int64_t N, int64_t nM, int64_t nT, hipStream_t st);

// the MAPS (CONSTS == false: tu_ab_rfgr_maps_bwd.hip) and CONSTS (tu_ab_rfgr_consts_bwd.hip) builds of K2abb: the same
// adjoint, which also returns gloc, gBz, gb1 -- and gC = [dL/dg, dL/dE1, dL/dE2, dL/dE1m1] -- per spin, each may be null
template <bool CONSTS, typename T, typename CT>
int run_ab_rfgr_spin_bwd(const void* ABck, PulseOps in, const void* gA, const void* gB, void* grf, void* ggr, void* gloc,
                         void* gBz, void* gb1, void* gC, void* work, int64_t N, int64_t nM, int64_t nT, hipStream_t st);

// K2ab-mc / K2abb-mc (tu_ab_rfgr_mc_fwd.hip; tu_ab_rfgr_mc2 / 4 / 8_bwd.hip, one unit per coil capacity MC >= nC): the same
// under parallel transmit, rf (N|1, 2, nT, nC), b1 (N, nM, 2, nC) not null, 1 <= nC <= ab_mc_max_coils (geom.hpp)
template <typename T, typename CT>
int run_ab_rfgr_mc_fwd(PulseOps in, void* A, void* B, void* ABck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT,
                       int64_t nC, hipStream_t st);

template <int MC, typename T, typename CT>
int run_ab_rfgr_mc_bwd(const void* ABck, PulseOps in, const void* gA, const void* gB, void* grf, void* ggr, void* work,
                       int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st);

template <typename T, typename CT>
int run_beff2ab(const void* Beff, Bc g, Bc E1, Bc E2, const void* E1m1, void* A, void* B, void* hist,
                int64_t N, int64_t nM, int64_t nT, hipStream_t st);

template <typename T, typename CT>
int run_beff2ab_bwd(const void* hist, const void* Beff, Bc g, Bc E1, Bc E2, const void* gA,
                    const void* gB, void* gBeff, void* gC, int64_t N, int64_t nM, int64_t nT, hipStream_t st);
}  // namespace mrphy_i
#pragma GCC visibility pop

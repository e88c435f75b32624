// abi.hip -- the C ABI of libmrphy_hip.so (include/mrphy_hip.h): argument validation and dispatch on the
// dtype code to the launchers of the tu_*.hip units (internal.hpp).  No kernel is defined here.  The operands of the
// fused family are packed into one struct at the entry point (MRPHY_PULSE_OPS below) and travel as that struct; so does
// everything else an adjoint call of that family carries (MRPHY_ADJOINT_REQ).
#include "host_common.hpp"

using namespace mrphy_i;

namespace {
#define MRPHY_DISPATCH(dtype, CALL)                          \
    switch (dtype) {                                         \
    case MRPHY_F32:     { using T = float;  using CT = float;  return CALL; } \
    case MRPHY_F64:     { using T = double; using CT = double; return CALL; } \
    case MRPHY_F32_C64: { using T = float;  using CT = double; return CALL; } \
    case MRPHY_F32P:     { using T = float;  using CT = prec_f32; return CALL; } \
    case MRPHY_F32P_C64: { using T = float;  using CT = prec_f64; return CALL; } \
    default: return MRPHY_EINVAL;                            \
    }

// the host's table of part pointers -> the by-value descriptor of the kernels (geom.hpp); MRPHY_E* or 0
int make_hist_parts(int dtype, void* const* parts, int64_t n_parts, int layout, int64_t N, int64_t nM, HistParts& h)
{
    h = HistParts{};
    if (n_parts < 0 || n_parts > HIST_MAX_PARTS) return MRPHY_EINVAL;
    if (layout != MRPHY_HIST_BLOCKED && layout != MRPHY_HIST_INTERLEAVED) return MRPHY_EINVAL;
    if (n_parts == 0 || !parts) return 0;
    for (int64_t i = 0; i < n_parts; ++i) {
        if (!parts[i]) return MRPHY_EINVAL;
        if (!aligned_to(parts[i], tsize(dtype))) return MRPHY_EALIGN;
        h.p[i] = parts[i];
    }
    h.n_parts = (int32_t)n_parts;
    h.interleaved = layout == MRPHY_HIST_INTERLEAVED;
    h.tiles_per_part = (uint32_t)hist_tiles_per_part(N, nM, n_parts);
    return 0;
}

// The fused family (K2, K2b, K2s, their trajectory and multi-coil builds).  Every entry point takes the same 24 scalars
// -- the pulse on the spins plus the step constants, rf .. E1m1 of include/mrphy_hip.h -- under the same names:
// MRPHY_PULSE_OPS packs them, once per entry point, into the PulseOps (geom.hpp) that the checks, the launchers and
// the kernel arguments take from there on.
#define MRPHY_PULSE_OPS_PARAMS                                                                                     \
    const void* rf, int64_t rf_sn, const void* gr, int64_t gr_sn, const void* loc, const void* df, int64_t df_sn,  \
    int64_t df_sm, const void* gamma, int64_t gamma_sn, int64_t gamma_sm, const void* b1, const void* g,           \
    int64_t g_sn, int64_t g_sm, const void* E1, int64_t E1_sn, int64_t E1_sm, const void* E2, int64_t E2_sn,       \
    int64_t E2_sm, const void* E1m1
#define MRPHY_PULSE_OPS                                                                                            \
    PulseOps{rf, rf_sn, gr, gr_sn, loc, {df, df_sn, df_sm}, {gamma, gamma_sn, gamma_sm}, b1, {g, g_sn, g_sm},      \
             {E1, E1_sn, E1_sm}, {E2, E2_sn, E2_sm}, E1m1}

// The null checks of the operands, shared by all eight: loc and g always; df only with gamma; E1, E2 and E1m1 all or
// none.  What differs is a parameter: the plain forward runs without a pulse at nT == 0 (need_pulse), the multi-coil
// adjoint cannot do without a b1 map (need_b1).  No alignment checks: the fused entry points have none.
int check_ops(const PulseOps& in, bool need_pulse, bool need_b1)
{
    if (!in.loc || !in.g.p || (need_pulse && (!in.rf || !in.gr)) || (need_b1 && !in.b1) || (in.df.p && !in.gam.p))
        return MRPHY_EINVAL;
    if ((in.E1.p == nullptr) != (in.E2.p == nullptr) || (in.E1.p == nullptr) != (in.E1m1 == nullptr))
        return MRPHY_EINVAL;
    return 0;
}

// K2v / K2vb form step0 + t + 1/2 in the data type: exact below 2^23 steps in the float types (k_fused_moving.hpp: step_mid)
inline bool moving_steps_ok(size_t ts, int64_t step0, int64_t nT)
{
    return ts == 8 || (step0 < ((int64_t)1 << 23) && nT < ((int64_t)1 << 23) - step0);
}

// K2sh / K2shb: 1 .. capacity channels, whose waveforms (nS, nT) the kernels index with an int (k_fused_shim.hpp: ShimCP)
inline bool shim_channels_ok(size_t ts, int64_t nS, int64_t nT)
{
    return nS >= 1 && nS <= shim_max_channels(ts) && nS * nT <= INT32_MAX;
}

// The Bz-extended builds (internal.hpp: MOVING, SHIM2 / 4 / 8), forward and adjoint: what the extension adds to a
// validator's mode arguments (refused on an empty problem too) and to its required pointers.  Both hold for any other build.
inline bool is_shim(AdjBuild b) { return b == AdjBuild::SHIM2 || b == AdjBuild::SHIM4 || b == AdjBuild::SHIM8; }
inline bool ext_mode_ok(AdjBuild b, size_t ts, const BzExt& x, int64_t nT)
{
    if (b == AdjBuild::MOVING) return x.step0 >= 0 && moving_steps_ok(ts, x.step0, nT);
    return !is_shim(b) || shim_channels_ok(ts, x.nS, nT);
}
inline bool ext_given(AdjBuild b, const BzExt& x, bool steps)       // (without a step no waveform is read)
{
    if (b == AdjBuild::MOVING) return x.vdt != nullptr;
    return !is_shim(b) || (x.shMap && (x.sh || !steps));
}

// Each plain entry point and its `_traj_` twin share one validation and dispatch.  `traj` tells them apart; what
// differs is written out where it differs.  The launchers take a null Mt / grad_Mt for the plain kernels.  Order of
// the checks, everywhere: dtype and sizes, the mode arguments, the empty problem (0), null pointers, the workspace.
int rfgr_fwd(bool traj, int dtype, const void* Mi, const PulseOps& in, void* Mo, void* Mck, int64_t ck_every, void* Mt,
             int64_t every, int64_t N, int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    // (a forward of several coils needs their b1 map: a mode argument, rejected on an empty problem too)
    if ((traj && every < 1) || nC < 1 || (!in.b1 && nC != 1) || (Mck && (ck_every < 8 || ck_every % 8 != 0)))
        return MRPHY_EINVAL;
    if (N * nM * (traj ? nT : 1) == 0) return 0;          // the plain forward runs at nT == 0: Mo = Mi
    // the trajectory's Mo is optional (it equals the last record)
    if (!Mi || !(traj ? Mt : Mo)) return MRPHY_EINVAL;
    if (int e = check_ops(in, nT > 0, false)) return e;
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_rfgr_fwd<T, CT>(Mi, in, Mo, Mck, ck_every, Mt, every, N, nM, nT, nC, st)));
}

// K2v and K2sh: the checks of the plain forward in their order, for one transmit coil; the extension's mode arguments
// (step0 and the range in which step0 + t + 1/2 is exact; the channel count against the data type's capacity) and its
// required pointers (vdt; shMap, and sh if there is a step) join theirs
int rfgr_ext_fwd(AdjBuild b, int dtype, const void* Mi, const PulseOps& in, const BzExt& x, void* Mo, void* Mck,
                 int64_t ck_every, int64_t N, int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (!ext_mode_ok(b, tsize(dtype), x, nT) || nC != 1 || (Mck && (ck_every < 8 || ck_every % 8 != 0)))
        return MRPHY_EINVAL;
    if (N * nM == 0) return 0;                            // runs at nT == 0: Mo = Mi
    if (!Mi || !Mo || !ext_given(b, x, nT > 0)) return MRPHY_EINVAL;
    if (int e = check_ops(in, nT > 0, false)) return e;
    hipStream_t st = (hipStream_t)stream;
#define MRPHY_EXT_FWD(B_) \
    case AdjBuild::B_:    \
        MRPHY_DISPATCH(dtype, (run_rfgr_ext_fwd<AdjBuild::B_, T, CT>(Mi, in, x, Mo, Mck, ck_every, N, nM, nT, st)))
    switch (b) {
        MRPHY_EXT_FWD(MOVING);
        MRPHY_EXT_FWD(SHIM2);
        MRPHY_EXT_FWD(SHIM4);
        MRPHY_EXT_FWD(SHIM8);
    default: return MRPHY_EINVAL;
    }
#undef MRPHY_EXT_FWD
}

// K2j: the checks of the plain forward in their order, for one transmit coil; the direction count against the data type's
// capacity and the tangents that need an operand the call does not have (db1 a b1 map, ddf gamma, dE* relaxation) are
// mode arguments; dMo is required, Mo is not.  The build is the smallest capacity 1, 2, 4 that holds D
int rfgr_jvp(int dtype, const void* Mi, const PulseOps& in, const JvpTangents& tg, void* Mo, void* dMo, int64_t N,
             int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (tg.D < 1 || tg.D > jvp_max_dirs(tsize(dtype)) || nC != 1 || (tg.db1 && !in.b1) || (tg.ddf && !in.gam.p) ||
        ((tg.dE1 || tg.dE2 || tg.dE1m1) && !in.E1.p))
        return MRPHY_EINVAL;
    if (N * nM == 0) return 0;                            // runs at nT == 0: Mo = Mi, dMo = dMi or zeros
    if (!Mi || !dMo) return MRPHY_EINVAL;
    if (int e = check_ops(in, nT > 0, false)) return e;
    hipStream_t st = (hipStream_t)stream;
#define MRPHY_JVP(MD_) MRPHY_DISPATCH(dtype, (run_rfgr_jvp<MD_, T, CT>(Mi, in, tg, Mo, dMo, N, nM, nT, st)))
    if (tg.D == 1) { MRPHY_JVP(1); }
    if (tg.D == 2) { MRPHY_JVP(2); }
    MRPHY_JVP(4);
#undef MRPHY_JVP
}
static_assert(JVP_MAXD_F32 == 4 && JVP_MAXD_F64 == 4, "rfgr_jvp: every capacity in every data type");

// What an adjoint entry point packs besides MRPHY_PULSE_OPS: the request (geom.hpp: AdjointReq), once -- the part every
// one of them has, under the same names; the cotangents and per-spin outputs it has itself it sets by name.
#define MRPHY_ADJOINT_REQ(nC_) \
    AdjointReq r{};            \
    r.Mck = Mck; r.gMi = grad_Mi; r.grf = grad_rf; r.ggr = grad_gr; r.work = work; r.N = N; r.nM = nM; r.nT = nT; r.nC = nC_

// The one dispatch of a validated request to its build's launcher (internal.hpp: AdjBuild), one row per build
int dispatch_adjoint(AdjBuild b, int dtype, const AdjointReq& r, const PulseOps& in, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
#define MRPHY_ADJ(B_) \
    case AdjBuild::B_: MRPHY_DISPATCH(dtype, (run_fused_bwd<AdjBuild::B_, T, CT>(r, in, st)))
    switch (b) {
        MRPHY_ADJ(PLAIN);
        MRPHY_ADJ(MRX);
        MRPHY_ADJ(MAPS);
        MRPHY_ADJ(CONSTS);
        MRPHY_ADJ(SIG_CONSTS1);
        MRPHY_ADJ(SIG_CONSTS2);
        MRPHY_ADJ(SIG_CONSTS4);
        MRPHY_ADJ(SIG_CONSTS8);
        MRPHY_ADJ(MC);
        MRPHY_ADJ(MOVING);
        MRPHY_ADJ(SHIM2);
        MRPHY_ADJ(SHIM4);
        MRPHY_ADJ(SHIM8);
    }
#undef MRPHY_ADJ
    return MRPHY_EINVAL;
}

// The adjoints of K2b / K2bt, builds PLAIN, MAPS, CONSTS and MC: grad_Mo (mode 0) or grad_Mt (modes 1, 2), exactly one of
// them; a grad_b1 needs a b1 map to differentiate.  The plain call is the MAPS call without per-spin outputs.  `traj`:
// a `_traj_` entry point, whose `every` counts whether or not grad_Mt is given.  The multi-coil build adds its coil
// count, cannot do without a b1 map and has a workspace of its own.  The builds MOVING and SHIM2 / 4 / 8 (K2vb, K2shb:
// grad_Mo only) add their extension's mode arguments and required pointers, the shim builds their workspace.
int rfgr_bwd(AdjBuild b, bool traj, int dtype, const AdjointReq& r, const PulseOps& in, size_t work_bytes, void* stream)
{
    const bool mc = b == AdjBuild::MC;
    if (int e = check_common(dtype, r.N, r.nM, r.nT)) return e;
    if (r.nT % SEG != 0 || ((traj || r.gMt) && r.every < 1) || (r.gMo && r.gMt) || (r.gb1 && !in.b1) ||
        (mc && (r.nC < 1 || r.nC > K2B_MAXC)) || !ext_mode_ok(b, tsize(dtype), r.ext, r.nT))
        return MRPHY_EINVAL;                                         // whole checkpoint segments only
    if (r.N * r.nM * r.nT == 0) return 0;
    if (!r.Mck || !(r.gMo || r.gMt) || !r.work || !ext_given(b, r.ext, true)) return MRPHY_EINVAL;
    if (int e = check_ops(in, true, mc)) return e;
    if (work_bytes < (mc          ? mrphy_blochsim_rfgr_mc_bwd_workspace(dtype, r.N, r.nM, r.nT, r.nC)
                      : is_shim(b) ? mrphy_blochsim_rfgr_shim_bwd_workspace(dtype, r.N, r.nM, r.nT, r.ext.nS)
                                   : mrphy_blochsim_rfgr_bwd_workspace(dtype, r.N, r.nM, r.nT)))
        return MRPHY_ENOSPC;
    return dispatch_adjoint(b, dtype, r, in, stream);
}

// The signal entry points and their `_mrx_` twins (a receive array: rx with a coil axis of nRx, never null) likewise; the
// one-coil ones pass nRx = 1.  The forward runs the smallest coil capacity that holds nRx.
int signal_fwd(bool mrx, int dtype, const void* Mi, const PulseOps& in, const void* rx, int64_t nRx, void* Mo, void* Mck,
               int64_t ck_every, void* sig, int64_t every, void* work, size_t work_bytes, int64_t N, int64_t nM,
               int64_t nT, int64_t nC, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (every < 1 || nC != 1 || N > 65535 || (Mck && (ck_every < 8 || ck_every % 8 != 0))) return MRPHY_EINVAL;
    if (nRx < 1 || nRx > sig_max_rx(tsize(dtype))) return MRPHY_EINVAL;
    if (N * nM * nT == 0) return 0;
    if (!Mi || (mrx && !rx) || !sig || !work) return MRPHY_EINVAL;
    if (int e = check_ops(in, true, false)) return e;
    if (work_bytes < mrphy_signal_rfgr_mrx_fwd_workspace(dtype, N, nM, nT, every, nRx)) return MRPHY_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
#define MRPHY_SIGNAL_FWD(R_) \
    MRPHY_DISPATCH(dtype, (run_signal_fwd<T, CT, R_>(Mi, in, rx, nRx, Mo, Mck, ck_every, sig, every, work, N, nM, nT, st)))
    if (nRx == 1) MRPHY_SIGNAL_FWD(1);
    if (nRx <= 2) MRPHY_SIGNAL_FWD(2);
    if (nRx <= 4) MRPHY_SIGNAL_FWD(4);
    MRPHY_SIGNAL_FWD(8);
#undef MRPHY_SIGNAL_FWD
}

// `consts`: the CONSTS builds, which return grad_consts (optional) besides; rx may then be null for nRx == 1, the one-coil
// entry point's (1, 0), and the smallest capacity 1, 2, 4, 8 that holds nRx runs
int signal_bwd(bool mrx, bool consts, int dtype, const AdjointReq& r, const PulseOps& in, size_t work_bytes, void* stream)
{
    if (int e = check_common(dtype, r.N, r.nM, r.nT)) return e;
    // whole checkpoint segments only; at least one of the two cotangents
    if (r.nT % SEG != 0 || r.every < 1 || r.N > 65535 || (!r.gMo && !r.gsig)) return MRPHY_EINVAL;
    if (r.nRx < 1 || r.nRx > sig_max_rx(tsize(dtype))) return MRPHY_EINVAL;
    if (r.N * r.nM * r.nT == 0) return 0;
    if (!r.Mck || (mrx && !r.rx && !(consts && r.nRx == 1)) || !r.work) return MRPHY_EINVAL;
    if (int e = check_ops(in, true, false)) return e;
    if (work_bytes < mrphy_blochsim_rfgr_bwd_workspace(dtype, r.N, r.nM, r.nT)) return MRPHY_ENOSPC;
    // without grad_sig there is nothing of the signal to inject: K2b on grad_Mo, its CONSTS build for grad_consts.  A
    // receive array: the capacities 2 .. 8 are a unit of their own, which picks the smallest that holds nRx
    const AdjBuild b = !r.gsig ? (consts ? AdjBuild::CONSTS : AdjBuild::PLAIN)
                       : consts ? sig_consts_build(r.nRx == 1 ? 1 : r.nRx <= 2 ? 2 : r.nRx <= 4 ? 4 : 8)
                                : (r.nRx > 1 ? AdjBuild::MRX : AdjBuild::PLAIN);
    return dispatch_adjoint(b, dtype, r, in, stream);
}

// K2abb-mc: the unit of the smallest coil capacity 2, 4, 8 that holds nC (the caller has checked nC against the data
// type's largest)
template <typename T, typename CT>
int ab_rfgr_mc_bwd(const void* ABck, const PulseOps& in, const void* gA, const void* gB, void* grf, void* ggr, void* work,
                   int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st)
{
    if (nC <= 2) return run_ab_rfgr_mc_bwd<2, T, CT>(ABck, in, gA, gB, grf, ggr, work, N, nM, nT, nC, st);
    if (nC <= 4) return run_ab_rfgr_mc_bwd<4, T, CT>(ABck, in, gA, gB, grf, ggr, work, N, nM, nT, nC, st);
    if constexpr (ab_mc_max_coils(sizeof(T)) >= 8)
        return run_ab_rfgr_mc_bwd<8, T, CT>(ABck, in, gA, gB, grf, ggr, work, N, nM, nT, nC, st);
    return MRPHY_EINVAL;
}
}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int mrphy_abi_version(void) { return MRPHY_ABI_VERSION; }

const char* mrphy_arch(void) { return "gfx950"; }

const char* mrphy_error_string(int code)
{
    switch (code) {
    case 0: return "success";
    case MRPHY_EINVAL: return "mrphy: invalid argument";
    case MRPHY_EALIGN: return "mrphy: pointer not aligned to its element size";
    case MRPHY_ENOSPC: return "mrphy: workspace too small";
    default: return hipGetErrorString((hipError_t)code);
    }
}

int mrphy_rfgr2beff(int dtype, const void* rf, int64_t rf_sn, const void* gr, int64_t gr_sn,
                    const void* loc, const void* df, int64_t df_sn, int64_t df_sm,
                    const void* gamma, int64_t gamma_sn, int64_t gamma_sm, const void* b1,
                    void* beff, int64_t N, int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    return mrphy_rfgr2beff_st(dtype, rf, rf_sn, gr, gr_sn, loc, df, df_sn, df_sm, gamma, gamma_sn, gamma_sm, b1, beff,
                              N, nM, nT, nC, MRPHY_STORE_AUTO, stream);
}

int mrphy_rfgr2beff_st(int dtype, const void* rf, int64_t rf_sn, const void* gr, int64_t gr_sn,
                       const void* loc, const void* df, int64_t df_sn, int64_t df_sm,
                       const void* gamma, int64_t gamma_sn, int64_t gamma_sm, const void* b1,
                       void* beff, int64_t N, int64_t nM, int64_t nT, int64_t nC, int store_policy, void* stream)
{
    if (store_policy < MRPHY_STORE_AUTO || store_policy > MRPHY_STORE_SC1NT) return MRPHY_EINVAL;
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (dtype != MRPHY_F32 && dtype != MRPHY_F64) return MRPHY_EINVAL;   // K0 has no constant type
    if (nC < 1 || (!b1 && nC != 1)) return MRPHY_EINVAL;
    if (N * nM * nT == 0) return 0;
    if (!rf || !gr || !loc || !beff || (df && !gamma)) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype);
    if (!aligned_to(rf, ts) || !aligned_to(gr, ts) || !aligned_to(loc, ts) ||
        !aligned_to(beff, ts) || (b1 && !aligned_to(b1, ts)))
        return MRPHY_EALIGN;
    const Bc bdf = {df, df_sn, df_sm}, bgam = {gamma, gamma_sn, gamma_sm};
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MRPHY_F32)
        return run_rfgr2beff<float>(rf, rf_sn, gr, gr_sn, loc, bdf, bgam, b1, beff, N, nM, nT, nC, store_policy, st);
    return run_rfgr2beff<double>(rf, rf_sn, gr, gr_sn, loc, bdf, bgam, b1, beff, N, nM, nT, nC, store_policy, st);
}

size_t mrphy_rfgr2beff_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t nC)
{
    if (N <= 0 || nM <= 0 || nT <= 0 || nC < 1) return 0;
    // single coil: 3 sums x 3 nT per spin group (k_..._p1v).  2..32 coils: (3 + 2 nC) x nT per spin group
    // -- grad_gr's three rows and a re and an im row per coil -- followed by the packed coefficient rows of
    // the SGPR pass, (2 MC + 4) per spin for the padded coil count MC the launcher picks (the query cannot see
    // whether a b1 map will be passed; mrphy_rfgr2beff_bwd rejects nC >= 2 without one).  More coils: the
    // generic passes, (3 + 2 nC) x nT.
    if (bwd_capacity(nC, true))
        return bwd_pack_offset(tsize(dtype), N, nM, nT, nC) +
               (size_t)(N * nM * (2 * bwd_padded_coils(nC, true) + 4)) * tsize(dtype);
    const int64_t rows = (nC == 1) ? 9 : (3 + 2 * nC);
    return (size_t)(bwd_spin_groups(nM) * N * rows * nT) * tsize(dtype);
}

int mrphy_rfgr2beff_bwd(int dtype, const void* grad_beff, const void* loc, const void* b1,
                        void* grad_rf, void* grad_gr, void* work, size_t work_bytes, int64_t N,
                        int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if ((dtype != MRPHY_F32 && dtype != MRPHY_F64) || nC < 1) return MRPHY_EINVAL;
    // as mrphy_rfgr2beff: without a b1 map the field is Bxy = rf of ONE coil (the host sums a
    // multi-coil rf first), so there is no multi-coil gradient to form.  The workspace query
    // relies on this: nC >= 2 implies a map, i.e. the one-pass layout it sizes for.
    if (!b1 && nC != 1) return MRPHY_EINVAL;
    if (N * nT == 0) return 0;
    if (!grad_beff || !loc || !work) return MRPHY_EINVAL;
    if (work_bytes < mrphy_rfgr2beff_bwd_workspace(dtype, N, nM, nT, nC)) return MRPHY_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MRPHY_F32)
        return run_rfgr2beff_bwd<float>(grad_beff, loc, b1, grad_rf, grad_gr, work, N, nM, nT, nC, st);
    return run_rfgr2beff_bwd<double>(grad_beff, loc, b1, grad_rf, grad_gr, work, N, nM, nT, nC, st);
}

size_t mrphy_blochsim_hist_bytes(int dtype, int64_t N, int64_t nM, int64_t nT)
{
    if (N <= 0 || nM <= 0 || nT <= 0) return 0;
    return (size_t)hist_elems(N, nM, nT) * tsize(dtype);
}

size_t mrphy_blochsim_hist_part_bytes(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t n_parts)
{
    if (N <= 0 || nM <= 0 || nT <= 0 || n_parts < 1 || n_parts > HIST_MAX_PARTS) return 0;
    return (size_t)(hist_tiles_per_part(N, nM, n_parts) * nT * HIST_STEP) * tsize(dtype);
}

int mrphy_blochsim_fwd_parts(int dtype, const void* Mi, const void* Beff, const void* g, int64_t g_sn,
                             int64_t g_sm, const void* E1, int64_t E1_sn, int64_t E1_sm, const void* E2,
                             int64_t E2_sn, int64_t E2_sm, const void* E1m1, void* Mo,
                             void* const* hist_parts, int64_t n_parts, int layout,
                             int64_t N, int64_t nM, int64_t nT, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    HistParts hist;
    if (int e = make_hist_parts(dtype, hist_parts, n_parts, layout, N, nM, hist)) return e;
    if (N * nM == 0) return 0;
    if (!Mi || !Mo || !g || (nT > 0 && !Beff)) return MRPHY_EINVAL;
    if ((E1 == nullptr) != (E2 == nullptr) || (E1 == nullptr) != (E1m1 == nullptr))
        return MRPHY_EINVAL;                              // both or neither (sims.py:68)
    const size_t ts = tsize(dtype), cs = csize(dtype);
    if (!aligned_to(Mi, ts) || !aligned_to(Mo, ts) || !aligned_to(Beff, ts) ||
        !aligned_to(g, cs) || (E1 && (!aligned_to(E1, cs) || !aligned_to(E2, cs))))
        return MRPHY_EALIGN;
    const Bc bg = {g, g_sn, g_sm}, b1 = {E1, E1_sn, E1_sm}, b2 = {E2, E2_sn, E2_sm};
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_fwd<T, CT>(Mi, Beff, bg, b1, b2, E1m1, Mo, hist, N, nM, nT, st)));
}
int mrphy_blochsim_fwd(int dtype, const void* Mi, const void* Beff, const void* g, int64_t g_sn,
                       int64_t g_sm, const void* E1, int64_t E1_sn, int64_t E1_sm, const void* E2,
                       int64_t E2_sn, int64_t E2_sm, const void* E1m1, void* Mo, void* Mpre,
                       int64_t N, int64_t nM, int64_t nT, void* stream)
{
    void* parts[1] = {Mpre};
    return mrphy_blochsim_fwd_parts(dtype, Mi, Beff, g, g_sn, g_sm, E1, E1_sn, E1_sm, E2, E2_sn, E2_sm, E1m1, Mo,
                                    Mpre ? parts : nullptr, Mpre ? 1 : 0, MRPHY_HIST_BLOCKED, N, nM, nT, stream);
}

int mrphy_blochsim_bwd_parts(int dtype, const void* const* hist_parts, int64_t n_parts, int layout,
                             const void* Beff, const void* g, int64_t g_sn, int64_t g_sm,
                             const void* E1, int64_t E1_sn, int64_t E1_sm, const void* E2, int64_t E2_sn,
                             int64_t E2_sm, const void* grad_Mo, void* grad_Mi, void* grad_Beff,
                             void* grad_consts, int64_t N, int64_t nM, int64_t nT, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    HistParts hist;
    if (int e = make_hist_parts(dtype, const_cast<void* const*>(reinterpret_cast<const void* const*>(hist_parts)),
                                n_parts, layout, N, nM, hist)) return e;
    if (N * nM == 0) return 0;
    if (!g || !grad_Mo || (nT > 0 && (!Beff || hist.n_parts == 0))) return MRPHY_EINVAL;
    if ((E1 == nullptr) != (E2 == nullptr)) return MRPHY_EINVAL;
    const Bc bg = {g, g_sn, g_sm}, b1 = {E1, E1_sn, E1_sm}, b2 = {E2, E2_sn, E2_sm};
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_bwd<T, CT>(hist, Beff, bg, b1, b2, grad_Mo, grad_Mi, grad_Beff, grad_consts,
                                          N, nM, nT, st)));
}

int mrphy_blochsim_bwd(int dtype, const void* Mpre, const void* Beff, const void* g, int64_t g_sn,
                       int64_t g_sm, const void* E1, int64_t E1_sn, int64_t E1_sm, const void* E2,
                       int64_t E2_sn, int64_t E2_sm, const void* grad_Mo, void* grad_Mi,
                       void* grad_Beff, int64_t N, int64_t nM, int64_t nT, void* stream)
{
    const void* parts[1] = {Mpre};
    return mrphy_blochsim_bwd_parts(dtype, parts, Mpre ? 1 : 0, MRPHY_HIST_BLOCKED, Beff, g, g_sn, g_sm, E1, E1_sn,
                                    E1_sm, E2, E2_sn, E2_sm, grad_Mo, grad_Mi, grad_Beff, nullptr, N, nM, nT, stream);
}

int mrphy_blochsim_bwd_consts(int dtype, const void* Mpre, const void* Beff, const void* g,
                              int64_t g_sn, int64_t g_sm, const void* E1, int64_t E1_sn,
                              int64_t E1_sm, const void* E2, int64_t E2_sn, int64_t E2_sm,
                              const void* grad_Mo, void* grad_Mi, void* grad_Beff, void* grad_consts,
                              int64_t N, int64_t nM, int64_t nT, void* stream)
{
    if (!grad_consts) return MRPHY_EINVAL;
    const void* parts[1] = {Mpre};
    return mrphy_blochsim_bwd_parts(dtype, parts, Mpre ? 1 : 0, MRPHY_HIST_BLOCKED, Beff, g, g_sn, g_sm, E1, E1_sn,
                                    E1_sm, E2, E2_sn, E2_sm, grad_Mo, grad_Mi, grad_Beff, grad_consts, N, nM, nT,
                                    stream);
}

int mrphy_blochsim_1step(int dtype, const void* M, const void* b, const void* g, int64_t g_sn,
                         int64_t g_sm, const void* E1, int64_t E1_sn, int64_t E1_sm,
                         const void* E2, int64_t E2_sn, int64_t E2_sm, const void* E1m1,
                         void* Mout, int64_t N, int64_t nM, void* stream)
{
    // one step of the same integrator: Beff (N, nM, 1, 3) == b (N, nM, 3)
    return mrphy_blochsim_fwd(dtype, M, b, g, g_sn, g_sm, E1, E1_sn, E1_sm, E2, E2_sn, E2_sm,
                              E1m1, Mout, nullptr, N, nM, 1, stream);
}

int mrphy_blochsim_rfgr_fwd(int dtype, const void* Mi, MRPHY_PULSE_OPS_PARAMS, void* Mo, void* Mck, int64_t ck_every,
                            int64_t N, int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    return rfgr_fwd(false, dtype, Mi, MRPHY_PULSE_OPS, Mo, Mck, ck_every, nullptr, 0, N, nM, nT, nC, stream);
}

int64_t mrphy_blochsim_rfgr_ck_every(void) { return SEG; }

size_t mrphy_blochsim_rfgr_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT)
{
    if (N <= 0 || nM <= 0 || nT <= 0) return 0;
    return (size_t)(k2b_waves(nM) * N * 5 * nT) * tsize(dtype);
}

int mrphy_blochsim_rfgr_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* grad_Mo, void* grad_Mi,
                            void* grad_rf, void* grad_gr, void* work, size_t work_bytes, int64_t N, int64_t nM,
                            int64_t nT, void* stream)
{
    MRPHY_ADJOINT_REQ(1);
    r.gMo = grad_Mo;
    return rfgr_bwd(AdjBuild::PLAIN, false, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

// K2v / K2vb and K2sh / K2shb: the plain entry points' checks in their order (rfgr_ext_fwd, rfgr_bwd) with the extension's
// own among them
int mrphy_blochsim_rfgr_moving_fwd(int dtype, const void* Mi, MRPHY_PULSE_OPS_PARAMS, const void* vdt, int64_t step0,
                                   void* Mo, void* Mck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT, int64_t nC,
                                   void* stream)
{
    const BzExt x{vdt, step0, nullptr, 0, nullptr, 0};
    return rfgr_ext_fwd(AdjBuild::MOVING, dtype, Mi, MRPHY_PULSE_OPS, x, Mo, Mck, ck_every, N, nM, nT, nC, stream);
}

int mrphy_blochsim_rfgr_moving_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* vdt, int64_t step0,
                                   const void* grad_Mo, void* grad_Mi, void* grad_rf, void* grad_gr, void* work,
                                   size_t work_bytes, int64_t N, int64_t nM, int64_t nT, void* stream)
{
    MRPHY_ADJOINT_REQ(1);
    r.gMo = grad_Mo; r.ext = BzExt{vdt, step0, nullptr, 0, nullptr, 0};
    return rfgr_bwd(AdjBuild::MOVING, false, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

int mrphy_blochsim_rfgr_shim_max_channels(int dtype)
{
    if (check_common(dtype, 0, 0, 0)) return 0;
    return shim_max_channels(tsize(dtype));
}

size_t mrphy_blochsim_rfgr_shim_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t nS)
{
    if (check_common(dtype, N, nM, nT) || N == 0 || nM == 0 || nT == 0 || nS < 0) return 0;   // an unknown dtype code among them
    return (size_t)(k2b_waves(nM) * N * (5 + nS) * nT) * tsize(dtype);
}

int mrphy_blochsim_rfgr_shim_fwd(int dtype, const void* Mi, MRPHY_PULSE_OPS_PARAMS, const void* sh, int64_t sh_sn,
                                 const void* shMap, int64_t nS, void* Mo, void* Mck, int64_t ck_every, int64_t N,
                                 int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    const BzExt x{nullptr, 0, sh, sh_sn, shMap, nS};
    return rfgr_ext_fwd(shim_build(nS), dtype, Mi, MRPHY_PULSE_OPS, x, Mo, Mck, ck_every, N, nM, nT, nC, stream);
}

int mrphy_blochsim_rfgr_shim_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* sh, int64_t sh_sn,
                                 const void* shMap, int64_t nS, const void* grad_Mo, void* grad_Mi, void* grad_rf,
                                 void* grad_lead, void* work, size_t work_bytes, int64_t N, int64_t nM, int64_t nT,
                                 void* stream)
{
    void* const grad_gr = grad_lead;                                 // the request's lead buffer: (N, 3 + nS, nT)
    MRPHY_ADJOINT_REQ(1);
    r.gMo = grad_Mo; r.ext = BzExt{nullptr, 0, sh, sh_sn, shMap, nS};
    return rfgr_bwd(shim_build(nS), false, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

int mrphy_blochsim_rfgr_jvp_max_dirs(int dtype)
{
    if (check_common(dtype, 0, 0, 0)) return MRPHY_EINVAL;
    return jvp_max_dirs(tsize(dtype));
}

int mrphy_blochsim_rfgr_jvp_fwd(int dtype, const void* Mi, MRPHY_PULSE_OPS_PARAMS, int64_t D, const void* dMi,
                                const void* drf, const void* dgr, const void* dloc, const void* ddf, const void* db1,
                                const void* dE1, const void* dE2, const void* dE1m1, void* Mo, void* dMo, int64_t N,
                                int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    const JvpTangents tg{D, dMi, drf, dgr, dloc, ddf, db1, dE1, dE2, dE1m1};
    return rfgr_jvp(dtype, Mi, MRPHY_PULSE_OPS, tg, Mo, dMo, N, nM, nT, nC, stream);
}

int64_t mrphy_blochsim_rfgr_mc_max_coils(void) { return K2B_MAXC; }

size_t mrphy_blochsim_rfgr_mc_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t nC)
{
    if (N <= 0 || nM <= 0 || nT <= 0 || nC <= 0) return 0;
    return (size_t)(k2b_mc_waves(nM) * N * (3 + 2 * nC) * nT) * tsize(dtype);
}

int mrphy_blochsim_rfgr_mc_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* grad_Mo, void* grad_Mi,
                               void* grad_rf, void* grad_gr, void* work, size_t work_bytes, int64_t N, int64_t nM,
                               int64_t nT, int64_t nC, void* stream)
{
    MRPHY_ADJOINT_REQ(nC);
    r.gMo = grad_Mo;
    return rfgr_bwd(AdjBuild::MC, false, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

int mrphy_blochsim_rfgr_traj_fwd(int dtype, const void* Mi, MRPHY_PULSE_OPS_PARAMS, void* Mo, void* Mck,
                                 int64_t ck_every, void* Mt, int64_t every, int64_t N, int64_t nM, int64_t nT,
                                 int64_t nC, void* stream)
{
    return rfgr_fwd(true, dtype, Mi, MRPHY_PULSE_OPS, Mo, Mck, ck_every, Mt, every, N, nM, nT, nC, stream);
}

int mrphy_blochsim_rfgr_traj_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* grad_Mt, int64_t every,
                                 void* grad_Mi, void* grad_rf, void* grad_gr, void* work, size_t work_bytes, int64_t N,
                                 int64_t nM, int64_t nT, void* stream)
{
    MRPHY_ADJOINT_REQ(1);
    r.gMt = grad_Mt; r.every = every;
    return rfgr_bwd(AdjBuild::PLAIN, true, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

int mrphy_blochsim_rfgr_maps_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* grad_Mo,
                                 const void* grad_Mt, int64_t every, void* grad_Mi, void* grad_rf, void* grad_gr,
                                 void* grad_loc, void* grad_Bz, void* grad_b1, void* work, size_t work_bytes, int64_t N,
                                 int64_t nM, int64_t nT, void* stream)
{
    MRPHY_ADJOINT_REQ(1);
    r.gMo = grad_Mo; r.gMt = grad_Mt; r.every = every; r.gloc = grad_loc; r.gBz = grad_Bz; r.gb1 = grad_b1;
    return rfgr_bwd(AdjBuild::MAPS, false, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

int mrphy_blochsim_rfgr_consts_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* grad_Mo,
                                   const void* grad_Mt, int64_t every, void* grad_Mi, void* grad_rf, void* grad_gr,
                                   void* grad_loc, void* grad_Bz, void* grad_b1, void* grad_consts, void* work,
                                   size_t work_bytes, int64_t N, int64_t nM, int64_t nT, void* stream)
{
    MRPHY_ADJOINT_REQ(1);
    r.gMo = grad_Mo; r.gMt = grad_Mt; r.every = every; r.gloc = grad_loc; r.gBz = grad_Bz; r.gb1 = grad_b1;
    r.gC = grad_consts;
    return rfgr_bwd(AdjBuild::CONSTS, false, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

int mrphy_blochsim_rfgr_mc_traj_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* grad_Mt,
                                    int64_t every, void* grad_Mi, void* grad_rf, void* grad_gr, void* work,
                                    size_t work_bytes, int64_t N, int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    MRPHY_ADJOINT_REQ(nC);
    r.gMt = grad_Mt; r.every = every;
    return rfgr_bwd(AdjBuild::MC, true, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

size_t mrphy_signal_rfgr_fwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t every)
{
    if (N <= 0 || nM <= 0 || nT <= 0 || every < 1) return 0;
    return (size_t)(sig_waves(nM) * N * 2 * sig_records(nT, every)) * tsize(dtype);
}

int mrphy_signal_rfgr_fwd(int dtype, const void* Mi, MRPHY_PULSE_OPS_PARAMS, const void* rx, void* Mo, void* Mck,
                          int64_t ck_every, void* sig, int64_t every, void* work, size_t work_bytes, int64_t N,
                          int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    return signal_fwd(false, dtype, Mi, MRPHY_PULSE_OPS, rx, 1, Mo, Mck, ck_every, sig, every, work, work_bytes, N, nM,
                      nT, nC, stream);
}

int mrphy_signal_rfgr_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* rx, const void* grad_Mo,
                          const void* grad_sig, int64_t every, void* grad_Mi, void* grad_rf, void* grad_gr, void* work,
                          size_t work_bytes, int64_t N, int64_t nM, int64_t nT, void* stream)
{
    MRPHY_ADJOINT_REQ(1);
    r.gMo = grad_Mo; r.gsig = grad_sig; r.every = every; r.rx = rx; r.nRx = 1;
    return signal_bwd(false, false, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

int mrphy_signal_rfgr_max_rx(int dtype)
{
    if (check_common(dtype, 0, 0, 0)) return 0;
    return sig_max_rx(tsize(dtype));
}

size_t mrphy_signal_rfgr_mrx_fwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t every, int64_t nRx)
{
    if (nRx < 1) return 0;
    return mrphy_signal_rfgr_fwd_workspace(dtype, N, nM, nT, every) * (size_t)nRx;
}

int mrphy_signal_rfgr_mrx_fwd(int dtype, const void* Mi, MRPHY_PULSE_OPS_PARAMS, const void* rx, int64_t nRx, void* Mo,
                              void* Mck, int64_t ck_every, void* sig, int64_t every, void* work, size_t work_bytes,
                              int64_t N, int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    return signal_fwd(true, dtype, Mi, MRPHY_PULSE_OPS, rx, nRx, Mo, Mck, ck_every, sig, every, work, work_bytes, N, nM,
                      nT, nC, stream);
}

int mrphy_signal_rfgr_mrx_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* rx, int64_t nRx,
                              const void* grad_Mo, const void* grad_sig, int64_t every, void* grad_Mi, void* grad_rf,
                              void* grad_gr, void* work, size_t work_bytes, int64_t N, int64_t nM, int64_t nT,
                              void* stream)
{
    MRPHY_ADJOINT_REQ(1);
    r.gMo = grad_Mo; r.gsig = grad_sig; r.every = every; r.rx = rx; r.nRx = nRx;
    return signal_bwd(true, false, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

int mrphy_signal_rfgr_consts_bwd(int dtype, const void* Mck, MRPHY_PULSE_OPS_PARAMS, const void* rx, int64_t nRx,
                                 const void* grad_Mo, const void* grad_sig, int64_t every, void* grad_Mi, void* grad_rf,
                                 void* grad_gr, void* grad_consts, void* work, size_t work_bytes, int64_t N, int64_t nM,
                                 int64_t nT, void* stream)
{
    MRPHY_ADJOINT_REQ(1);
    r.gMo = grad_Mo; r.gsig = grad_sig; r.every = every; r.rx = rx; r.nRx = nRx; r.gC = grad_consts;
    return signal_bwd(true, true, dtype, r, MRPHY_PULSE_OPS, work_bytes, stream);
}

// K2ab / K2abb.  Order of the checks as in the rest of the fused family: dtype and sizes, the mode arguments, the empty
// problem, null pointers, the workspace.  The forward runs at nT == 0 (A = I, B = 0), without a pulse then.
int mrphy_ab_rfgr_fwd(int dtype, MRPHY_PULSE_OPS_PARAMS, void* A, void* B, void* ABck, int64_t ck_every, int64_t N,
                      int64_t nM, int64_t nT, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (N > 65535 || (ABck && (ck_every < 8 || ck_every % 8 != 0))) return MRPHY_EINVAL;
    if (N * nM == 0) return 0;
    if (!A || !B) return MRPHY_EINVAL;
    const PulseOps in = MRPHY_PULSE_OPS;
    if (int e = check_ops(in, nT > 0, false)) return e;
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_ab_rfgr_fwd<T, CT>(in, A, B, ABck, ck_every, N, nM, nT, st)));
}

int mrphy_ab_rfgr_bwd(int dtype, const void* ABck, MRPHY_PULSE_OPS_PARAMS, const void* grad_A, const void* grad_B,
                      void* grad_rf, void* grad_gr, void* work, size_t work_bytes, int64_t N, int64_t nM, int64_t nT,
                      void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (N > 65535 || nT % SEG != 0) return MRPHY_EINVAL;               // whole checkpoint segments only
    if (N * nM * nT == 0) return 0;
    if (!ABck || !work) return MRPHY_EINVAL;
    const PulseOps in = MRPHY_PULSE_OPS;
    if (int e = check_ops(in, true, false)) return e;
    if (work_bytes < mrphy_blochsim_rfgr_bwd_workspace(dtype, N, nM, nT)) return MRPHY_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_ab_rfgr_bwd<T, CT>(ABck, in, grad_A, grad_B, grad_rf, grad_gr, work, N, nM, nT, st)));
}

// The MAPS and CONSTS builds of K2abb: mrphy_ab_rfgr_bwd's checks in its order, and a grad_b1 needs a b1 map to
// differentiate (a mode argument, as in mrphy_blochsim_rfgr_maps_bwd: refused on an empty problem too)
#define MRPHY_AB_SPIN_BWD(CONSTS_, GC_)                                                                              \
    if (int e = check_common(dtype, N, nM, nT)) return e;                                                            \
    if (N > 65535 || nT % SEG != 0 || (grad_b1 && !b1)) return MRPHY_EINVAL;                                         \
    if (N * nM * nT == 0) return 0;                                                                                  \
    if (!ABck || !work) return MRPHY_EINVAL;                                                                         \
    const PulseOps in = MRPHY_PULSE_OPS;                                                                             \
    if (int e = check_ops(in, true, false)) return e;                                                                \
    if (work_bytes < mrphy_blochsim_rfgr_bwd_workspace(dtype, N, nM, nT)) return MRPHY_EINVAL;                       \
    hipStream_t st = (hipStream_t)stream;                                                                            \
    MRPHY_DISPATCH(dtype, (run_ab_rfgr_spin_bwd<CONSTS_, T, CT>(ABck, in, grad_A, grad_B, grad_rf, grad_gr, grad_loc, \
                                                                grad_Bz, grad_b1, GC_, work, N, nM, nT, st)))

int mrphy_ab_rfgr_maps_bwd(int dtype, const void* ABck, MRPHY_PULSE_OPS_PARAMS, const void* grad_A, const void* grad_B,
                           void* grad_rf, void* grad_gr, void* grad_loc, void* grad_Bz, void* grad_b1, void* work,
                           size_t work_bytes, int64_t N, int64_t nM, int64_t nT, void* stream)
{
    MRPHY_AB_SPIN_BWD(false, nullptr);
}

int mrphy_ab_rfgr_consts_bwd(int dtype, const void* ABck, MRPHY_PULSE_OPS_PARAMS, const void* grad_A,
                             const void* grad_B, void* grad_rf, void* grad_gr, void* grad_loc, void* grad_Bz,
                             void* grad_b1, void* grad_consts, void* work, size_t work_bytes, int64_t N, int64_t nM,
                             int64_t nT, void* stream)
{
    MRPHY_AB_SPIN_BWD(true, grad_consts);
}
#undef MRPHY_AB_SPIN_BWD

// K2ab-mc / K2abb-mc: the one-coil entry points' checks in their order; the coil count is a mode argument (refused on
// an empty problem too), the b1 map a required pointer, and a short workspace is MRPHY_ENOSPC
int mrphy_ab_rfgr_mc_max_coils(int dtype)
{
    if (check_common(dtype, 0, 0, 0)) return 0;
    return ab_mc_max_coils(tsize(dtype));
}

size_t mrphy_ab_rfgr_mc_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t nC)
{
    return mrphy_blochsim_rfgr_mc_bwd_workspace(dtype, N, nM, nT, nC);
}

int mrphy_ab_rfgr_mc_fwd(int dtype, MRPHY_PULSE_OPS_PARAMS, void* A, void* B, void* ABck, int64_t ck_every, int64_t N,
                         int64_t nM, int64_t nT, int64_t nC, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (N > 65535 || (ABck && (ck_every < 8 || ck_every % 8 != 0)) || nC < 1 || nC > mrphy_ab_rfgr_mc_max_coils(dtype))
        return MRPHY_EINVAL;
    if (N * nM == 0) return 0;
    if (!A || !B) return MRPHY_EINVAL;
    const PulseOps in = MRPHY_PULSE_OPS;
    if (int e = check_ops(in, nT > 0, true)) return e;
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_ab_rfgr_mc_fwd<T, CT>(in, A, B, ABck, ck_every, N, nM, nT, nC, st)));
}

int mrphy_ab_rfgr_mc_bwd(int dtype, const void* ABck, MRPHY_PULSE_OPS_PARAMS, const void* grad_A, const void* grad_B,
                         void* grad_rf, void* grad_gr, void* work, size_t work_bytes, int64_t N, int64_t nM, int64_t nT,
                         int64_t nC, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (N > 65535 || nT % SEG != 0 || nC < 1 || nC > mrphy_ab_rfgr_mc_max_coils(dtype))
        return MRPHY_EINVAL;                                            // whole checkpoint segments only
    if (N * nM * nT == 0) return 0;
    if (!ABck || !work || (!grad_A && !grad_B)) return MRPHY_EINVAL;
    const PulseOps in = MRPHY_PULSE_OPS;
    if (int e = check_ops(in, true, true)) return e;
    if (work_bytes < mrphy_ab_rfgr_mc_bwd_workspace(dtype, N, nM, nT, nC)) return MRPHY_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (ab_rfgr_mc_bwd<T, CT>(ABck, in, grad_A, grad_B, grad_rf, grad_gr, work, N, nM, nT, nC, st)));
}

int mrphy_beff2ab(int dtype, const void* Beff,
                  const void* g, int64_t g_sn, int64_t g_sm,
                  const void* E1, int64_t E1_sn, int64_t E1_sm,
                  const void* E2, int64_t E2_sn, int64_t E2_sm,
                  const void* E1m1, void* A, void* B,
                  int64_t N, int64_t nM, int64_t nT, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (N * nM == 0) return 0;
    if (!A || !B || !g || !E1 || !E2 || !E1m1 || (nT > 0 && !Beff)) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype), cs = csize(dtype);
    if (!aligned_to(A, ts) || !aligned_to(B, ts) || !aligned_to(Beff, ts) || !aligned_to(g, cs) ||
        !aligned_to(E1, cs) || !aligned_to(E2, cs) || !aligned_to(E1m1, cs))
        return MRPHY_EALIGN;
    const Bc bg = {g, g_sn, g_sm}, b1 = {E1, E1_sn, E1_sm}, b2 = {E2, E2_sn, E2_sm};
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_beff2ab<T, CT>(Beff, bg, b1, b2, E1m1, A, B, nullptr, N, nM, nT, st)));
}

size_t mrphy_beff2ab_hist_bytes(int dtype, int64_t N, int64_t nM, int64_t nT)
{
    if (N <= 0 || nM <= 0 || nT <= 0) return 0;
    return (size_t)(((N * nM + WAVE - 1) / WAVE) * nT * AB_HIST_STEP) * tsize(dtype);
}

int mrphy_beff2ab_save(int dtype, const void* Beff,
                       const void* g, int64_t g_sn, int64_t g_sm,
                       const void* E1, int64_t E1_sn, int64_t E1_sm,
                       const void* E2, int64_t E2_sn, int64_t E2_sm,
                       const void* E1m1, void* A, void* B, void* hist,
                       int64_t N, int64_t nM, int64_t nT, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (N * nM == 0) return 0;
    if (!A || !B || !g || !E1 || !E2 || !E1m1 || (nT > 0 && (!Beff || !hist))) return MRPHY_EINVAL;
    const size_t ts = tsize(dtype), cs = csize(dtype);
    if (!aligned_to(A, ts) || !aligned_to(B, ts) || !aligned_to(Beff, ts) || !aligned_to(hist, ts) ||
        !aligned_to(g, cs) || !aligned_to(E1, cs) || !aligned_to(E2, cs) || !aligned_to(E1m1, cs))
        return MRPHY_EALIGN;
    const Bc bg = {g, g_sn, g_sm}, b1 = {E1, E1_sn, E1_sm}, b2 = {E2, E2_sn, E2_sm};
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_beff2ab<T, CT>(Beff, bg, b1, b2, E1m1, A, B, hist, N, nM, nT, st)));
}

int mrphy_beff2ab_bwd(int dtype, const void* hist, const void* Beff,
                      const void* g, int64_t g_sn, int64_t g_sm,
                      const void* E1, int64_t E1_sn, int64_t E1_sm,
                      const void* E2, int64_t E2_sn, int64_t E2_sm,
                      const void* grad_A, const void* grad_B, void* grad_Beff,
                      int64_t N, int64_t nM, int64_t nT, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (N * nM * nT == 0) return 0;
    if (!hist || !Beff || !g || !E1 || !E2 || !grad_Beff) return MRPHY_EINVAL;
    const Bc bg = {g, g_sn, g_sm}, b1 = {E1, E1_sn, E1_sm}, b2 = {E2, E2_sn, E2_sm};
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_beff2ab_bwd<T, CT>(hist, Beff, bg, b1, b2, grad_A, grad_B, grad_Beff,
                                                  nullptr, N, nM, nT, st)));
}

int mrphy_beff2ab_bwd_consts(int dtype, const void* hist, const void* Beff,
                      const void* g, int64_t g_sn, int64_t g_sm,
                      const void* E1, int64_t E1_sn, int64_t E1_sm,
                      const void* E2, int64_t E2_sn, int64_t E2_sm,
                      const void* grad_A, const void* grad_B, void* grad_Beff, void* grad_consts,
                      int64_t N, int64_t nM, int64_t nT, void* stream)
{
    if (int e = check_common(dtype, N, nM, nT)) return e;
    if (N * nM == 0) return 0;
    if (nT == 0) {
        // an empty pulse: A = I, B = 0 whatever the constants are, so their gradients are exact zeros (the reference's
        // autograd gives them, beffective.py:73-100) -- written here, not left to the caller's allocation
        if (!grad_consts) return MRPHY_EINVAL;
        return (int)hipMemsetAsync(grad_consts, 0, (size_t)(N * nM) * 4 * tsize(dtype), (hipStream_t)stream);
    }
    if (!hist || !Beff || !g || !E1 || !E2 || !grad_Beff || !grad_consts) return MRPHY_EINVAL;
    const Bc bg = {g, g_sn, g_sm}, b1 = {E1, E1_sn, E1_sm}, b2 = {E2, E2_sn, E2_sm};
    hipStream_t st = (hipStream_t)stream;
    MRPHY_DISPATCH(dtype, (run_beff2ab_bwd<T, CT>(hist, Beff, bg, b1, b2, grad_A, grad_B, grad_Beff,
                                                  grad_consts, N, nM, nT, st)));
}

}  // extern "C"

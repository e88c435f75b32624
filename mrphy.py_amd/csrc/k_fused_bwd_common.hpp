// k_fused_bwd_common.hpp -- what the one-coil and the multi-coil fused adjoints share
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_common.hpp"

// =============================================================================================
// K2b: adjoint of the fused kernel -- grad_Mo -> grad_Mi, grad_rf, grad_gr without Beff, history
// or grad_Beff in HBM (single-coil rf).  K2 leaves a checkpoint of M every SEG = 16 steps.  A wave
// walks the segments of its 64 spins backwards; per segment it
//   1. recomputes the 16 pre-step states from the checkpoint into registers (the very states the
//      forward pass went through, so no inversion error),
//   2. sweeps the adjoint over the 16 steps, re-assembling the field on the fly,
//   3. reduces the five per-step contributions
//        gr_x,y,z += loc_{x,y,z} * gBz     rf_re += b1r*gBx + b1i*gBy     rf_im += b1r*gBy - b1i*gBx
//      over its 64 spins with an LDS transpose-sum (80 rows x 64 lanes, slot-swizzled: conflict-free
//      ds_read_b128), and adds the 80 sums into ITS OWN row of the workspace.
// Waves are persistent (grid.x = min(tiles, 2048)) and take tiles w, w+P, ... in order, so every
// workspace row is accumulated in a fixed order; a second pass sums the rows in fixed order:
// deterministic, no float atomics.
// =============================================================================================
// (SEG = 16 steps per checkpoint segment: geom.hpp)
// (the reduction tile's index red_idx, RED_PITCH, and the second pass over the workspace rows: k_fused_common.hpp)
// (K2B_MAX_WAVES = 256 * 8 resident waves, 8 per CU: geom.hpp)
// The single-coil kernel needs 5 * SEG <= 2 * WAVE rows (two passes of row sums) and batches of 4 steps; the
// multi-coil kernel needs SEG == 16 outright (k_fused_mc_bwd.hpp).
static_assert(SEG % 4 == 0 && 5 * SEG <= 2 * WAVE, "K2b: 4-step batches, 5 * SEG reduction rows in two passes");
static_assert(SEG == 16, "K2b's reduction tile (red_idx: row & 15, 20480 B = 1/8 of a CU's LDS) is laid out for SEG = 16");

template <typename T>
struct FusedBwdArgs {
    const T* Mck;                    // (nT/SEG, N*nM, 3)
    PulseOpsT<T> in;                 // b1: (N, nM, 2) or null; the multi-coil kernel's (N, nM, 2, nC)
    const T* gMo;
    T* gMi;                          // may be null
    T* work;                         // (P, N, 5, nT)
    int64_t N, nM, nT, P;
};

// The trajectory adjoints (K2bt: mrphy_blochsim_rfgr_traj_bwd / _mc_traj_bwd) are the same kernels with INJ > 0 and
// FusedBwdTrajArgs; INJ == 0 is the plain K2b, whose sweep holds none of the additions (`if constexpr`) and whose
// kernarg layout stays FusedBwdArgs.
// The cotangent of a record taken after step e enters the carried state just before the sweep passes step e
// backwards.  In the plain modes the state is h = dL/dM and the cotangent adds as it is; in the precise fp32 t-state
// mode (bloch_math.hpp: AdjMode) the state is t = E h, so it enters as t += (E2, E2, E1) . g, rounded as adj_begin
// rounds the first cotangent (a raw add there would be off by a factor E per record).
// INJ: 1 = every < SEG (up to SEG records per segment, staged in the reduction tile: see k_fused_bwd.hpp; correct for
// any stride, and what the fp64 8-coil pTx build takes for every stride);
// 2 = every >= SEG (at most one record per segment besides the last, in registers).  The last record's cotangent
// starts the sweep, as grad_Mo does in K2b.
template <typename T>
struct FusedBwdTrajArgs : FusedBwdArgs<T> {
    int64_t every, nRec;             // gMo is grad_Mt (nRec, N*nM, 3)
};
// INJ >= 3 (one transmit coil only: k_fused_bwd.hpp) is the adjoint of the signal kernel K2s (k_signal_fwd.hpp,
// mrphy_signal_rfgr_bwd / _mrx_bwd) at the coil capacity R = inj_rx_cap(INJ) = 1, 2, 4, 8 for INJ = 3, 4, 5, 6 (nRx <= R
// receive coils).  The cotangent of record j is the same for every spin -- gsig[n, :, j, :], 2 nRx wave-uniform numbers
// read with scalar loads as the pulse is -- scaled by the lane's own receive weights and summed over the coils,
//     g = (sum_c rx_re,c g0,c + rx_im,c g1,c,  sum_c rx_re,c g1,c - rx_im,c g0,c,  0),
// formed in ascending c (R = 1: the one term) and injected once, like a trajectory record's.  No per-spin cotangent
// loads and no staging; the last record is injected like any other (the sweep starts from grad_Mo, or from zero when
// that is null).
template <typename T>
struct FusedBwdSigArgs : FusedBwdTrajArgs<T> {
    const T* rx;                     // (N, nM, 2, nRx); R = 1 only: or null = (1, 0)
    const T* gsig;                   // (N, 2, nRec, nRx)
    int64_t nRx;
};
constexpr int inj_rx_cap(int INJ) { return INJ < 3 ? 1 : 1 << (INJ - 3); }
template <typename T, int INJ>
using FusedBwdArgsT = std::conditional_t<INJ == 0, FusedBwdArgs<T>,
                      std::conditional_t<(INJ >= 3), FusedBwdSigArgs<T>, FusedBwdTrajArgs<T>>>;
// MAPS builds of the one-coil kernel in modes 0 .. 2 (k_fused_bwd.hpp; mrphy_blochsim_rfgr_maps_bwd): the gradients
// w.r.t. the spin-side operands, one value set per spin, each pointer may be null (not wanted).  Mode 0 takes this
// struct as well (every, nRec unused): one argument type per build family.
template <typename T>
struct FusedBwdMapsArgs : FusedBwdTrajArgs<T> {
    T* gloc;                         // (N, nM, 3): dL/dloc
    T* gBz;                          // (N, nM): dL/d(df / gamma) = sum over time of dL/dBz
    T* gb1;                          // (N, nM, 2): dL/db1; builds with a b1 map only
};
// CONSTS builds (k_fused_bwd.hpp; mrphy_blochsim_rfgr_consts_bwd, mrphy_signal_rfgr_consts_bwd): the gradients w.r.t. the
// lane's step constants besides, one more optional pointer after the arguments of the build they extend -- the MAPS
// struct in modes 0 .. 2 (whose map sums the CONSTS build forms too), the signal struct in modes 3 .. 6.
template <typename T>
struct FusedBwdConstsArgs : FusedBwdMapsArgs<T> {
    T* gC;                           // (N, nM, 4): [dL/dg, dL/dE1, dL/dE2, dL/dE1m1], g = gamma 2 pi dt
};
template <typename T>
struct FusedBwdSigConstsArgs : FusedBwdSigArgs<T> {
    T* gC;                           // as above
};
template <typename T, int INJ, bool MAPS, bool CONSTS = false>
using FusedBwdKArgsT =
    std::conditional_t<CONSTS, std::conditional_t<(INJ >= 3), FusedBwdSigConstsArgs<T>, FusedBwdConstsArgs<T>>,
                       std::conditional_t<MAPS, FusedBwdMapsArgs<T>, FusedBwdArgsT<T, INJ>>>;
// the kernarg layout is part of the kernels' machine code: `in` sits where its twelve fields were written out
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
template <typename T>
constexpr bool fused_bwd_args_layout =
    offsetof(FusedBwdArgs<T>, in) == 8 && offsetof(FusedBwdArgs<T>, gMo) == 184 && offsetof(FusedBwdArgs<T>, P) == 232 &&
    sizeof(FusedBwdArgs<T>) == 240 && offsetof(FusedBwdTrajArgs<T>, every) == 240 &&
    offsetof(FusedBwdTrajArgs<T>, nRec) == 248 && sizeof(FusedBwdTrajArgs<T>) == 256 &&
    offsetof(FusedBwdSigArgs<T>, rx) == 256 && offsetof(FusedBwdSigArgs<T>, gsig) == 264 &&
    offsetof(FusedBwdSigArgs<T>, nRx) == 272 && sizeof(FusedBwdSigArgs<T>) == 280;
template <typename T>
constexpr bool fused_bwd_maps_args_layout =
    offsetof(FusedBwdMapsArgs<T>, every) == 240 && offsetof(FusedBwdMapsArgs<T>, nRec) == 248 &&
    offsetof(FusedBwdMapsArgs<T>, gloc) == 256 && offsetof(FusedBwdMapsArgs<T>, gBz) == 264 &&
    offsetof(FusedBwdMapsArgs<T>, gb1) == 272 && sizeof(FusedBwdMapsArgs<T>) == 280;
template <typename T>
constexpr bool fused_bwd_consts_args_layout =
    offsetof(FusedBwdConstsArgs<T>, gloc) == 256 && offsetof(FusedBwdConstsArgs<T>, gb1) == 272 &&
    offsetof(FusedBwdConstsArgs<T>, gC) == 280 && sizeof(FusedBwdConstsArgs<T>) == 288 &&
    offsetof(FusedBwdSigConstsArgs<T>, rx) == 256 && offsetof(FusedBwdSigConstsArgs<T>, nRx) == 272 &&
    offsetof(FusedBwdSigConstsArgs<T>, gC) == 280 && sizeof(FusedBwdSigConstsArgs<T>) == 288;
#pragma clang diagnostic pop
static_assert(fused_bwd_args_layout<float> && fused_bwd_args_layout<double>, "K2b's kernel arguments moved");
static_assert(fused_bwd_maps_args_layout<float> && fused_bwd_maps_args_layout<double>,
              "the MAPS builds' kernel arguments moved");
static_assert(fused_bwd_consts_args_layout<float> && fused_bwd_consts_args_layout<double>,
              "the CONSTS builds' kernel arguments moved");

// Host: the arguments every fused adjoint takes, from the request: a null gMt selects the plain kernel (INJ == 0), which
// takes the FusedBwdArgs part; otherwise gMt is the cotangent the kernel reads.  P: the grid's persistent waves
template <typename T>
FusedBwdTrajArgs<T> fused_bwd_args(const AdjointReq& r, const PulseOps& in, int64_t P)
{
    FusedBwdTrajArgs<T> a;
    a.Mck = (const T*)r.Mck; a.in = typed<T>(in); a.gMo = (const T*)(r.gMt ? r.gMt : r.gMo); a.gMi = (T*)r.gMi;
    a.work = (T*)r.work; a.N = r.N; a.nM = r.nM; a.nT = r.nT; a.P = P;
    a.every = r.every; a.nRec = r.gMt ? (r.nT + r.every - 1) / r.every : 0;
    return a;
}

// Host: the frame of every fused adjoint launch.  `waves` persistent one-wave blocks per batch entry; `kernel(grid)`
// starts the caller's choice among its builds on that grid; then, if a pulse gradient is wanted, the second pass
// sums the workspace rows of the grid's waves into the `lead` rows of ggr (grad_gr's three; K2shb: and grad_sh's) and
// the nC coils of grf.
template <typename T, typename K>
int fused_bwd_launch(const AdjointReq& r, int64_t waves, hipStream_t st, K&& kernel, int lead = 3)
{
    dim3 grid;
    int e;
    if (!fused_grid(r.N * r.nM * r.nT, waves, r.N, grid, e)) return e;
    kernel(grid);
    e = launch_status();
    if (e || !(r.grf || r.ggr)) return e;
    return launch_p2<T>(r.work, r.ggr, lead, r.grf, r.nC, r.N, r.nT, grid.x, st);
}

template <bool RELAX, typename T, typename CT>
__device__ __forceinline__ void adj_inject(const SpinConst<T, CT>& k, T& hx, T& hy, T& hz, T gx, T gy, T gz)
{
#pragma clang fp contract(off)
    adj_begin<RELAX, T, CT>(k, gx, gy, gz);
    hx += gx; hy += gy; hz += gz;
}

// One adjoint step of the CONSTS builds: rot_apply_adj's expressions -- the core, then dL/dB = g dL/db, so (gx, gy, gz)
// and the carried state keep rot_apply_adj's bits -- and the step's terms of the constants' gradients added to acc
// (adj_const_accumulate, as K3's GC builds call it).  (Bx, By, Bz): the unscaled field of the step; (hx, hy, hz) comes
// in as the carried state AFTER the step's record injection, which is the `s` the accumulation wants (t = E h in the
// precise fp32 mode: adj_const_finish divides the E out of the finished sums).  `offset`: the step has the relaxation
// offset, whose gradient is then summed -- false for K2abb's A columns (k_ab_rfgr.hpp), which run without it.
template <bool RELAX, typename T, typename CT>
__device__ __forceinline__ void rot_apply_adj_consts(const SpinConst<T, CT>& k, const RotAdj<T>& r, T Bx, T By, T Bz,
                                                     T mx, T my, T mz, T& hx, T& hy, T& hz, T& gx, T& gy, T& gz,
                                                     T (&acc)[4], bool offset = true)
{
#pragma clang fp contract(off)
    using R = typename CTr<CT>::reg;
    const T sx = hx, sy = hy, sz = hz;
    T dbx, dby, dbz;
    rot_apply_adj_core<RELAX, T, CT>(k, r, mx, my, mz, hx, hy, hz, dbx, dby, dbz);
    gx = T(R(dbx) * k.g);
    gy = T(R(dby) * k.g);
    gz = T(R(dbz) * k.g);
    adj_const_accumulate<RELAX, T, CT>(r, Bx, By, Bz, mx, my, mz, sx, sy, sz, dbx, dby, dbz, acc, offset);
    // The sums are read at the end of the segment only, and the compiler sinks each step's terms below the guards of
    // the following steps' cold large-angle paths, down to there -- with the step's m, b, S, C, s and B alive all the
    // way: a private segment in fp64.  Pinned as bloch_math.hpp's pin_state pins the forward state: the step's terms are
    // complete here.  No instruction is emitted.
    asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
}

// Two global round trips per segment used to sit on the critical path: the checkpoint (used
// at once by the recompute) and the read-modify-write of the workspace rows.  Both are now
// issued a segment's worth of work ahead: the next checkpoint at the top of the current
// segment, the old workspace values before the sweep that produces what is added to them.
// The lane's checkpoint that segment `seg` - 1 starts from:
template <typename T>
__device__ __forceinline__ const T* ck_before(const T* Mck, int64_t seg, int64_t rows, int64_t row)
{
    return Mck + ((seg - 1) * rows + row) * 3;
}

// The SEG states before each step of the segment at t0, recomputed from its checkpoint (mx, my, mz; the very states the forward
// pass went through), with the S, C of each rotation
template <typename T> struct SegStates { T M0[SEG], M1[SEG], M2[SEG], Sv[SEG], Cv[SEG]; };

template <bool RELAX, typename T, typename CT, typename F>
__device__ __forceinline__ void seg_recompute(const SpinConst<T, CT>& k, int64_t t0, T& mx, T& my, T& mz, F&& field,
                                              SegStates<T>& h)
{
#pragma unroll
    for (int sb = 0; sb < SEG / 4; ++sb) {
        T Bx[4], By[4], Bz[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) field(t0 + sb * 4 + j, Bx[j], By[j], Bz[j]);
        Rot<T> r[4];
        rot_prepare<T, CT, 4>(k, Bx, By, Bz, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int st = sb * 4 + j;
            h.M0[st] = mx; h.M1[st] = my; h.M2[st] = mz;
            h.Sv[st] = r[j].S; h.Cv[st] = r[j].C;     // reused by the sweep
            rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
        }
    }
}

// k_fused_fwd.hpp -- K2 (fused rf,gr -> Mo)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_common.hpp"

// =============================================================================================
// K2: fused rf,gr -> Mo.  No Beff in HBM: the pulse sample of step t is wave-uniform (one block
// = one wave = 64 spins of ONE batch entry, so rf/gr addresses are scalar loads) and the lane's
// own loc / df/gamma / b1 sit in registers.  The field is assembled exactly as K0 rounds it
// (B first, then g*B) so that K2 == K1(K0(.)) bit for bit.  VALU-bound, not HBM-bound.
// =============================================================================================
template <typename T>
struct FusedArgs {
    const T* Mi;
    PulseOpsT<T> in;
    T* Mo;
    T* Mck;  int64_t ck_every;
    int64_t N, nM, nT, nC;
};

// The trajectory builds (K2t, mrphy_blochsim_rfgr_traj_fwd) are the same kernel with TR > 0 and FusedTrajArgs;
// TR == 0 is the plain K2, whose step loop holds none of the additions (`if constexpr`) and whose kernarg layout
// stays FusedArgs.
// TR: 1 = M after EVERY step into Mt, stored inside the unrolled step batch; 2 = M after steps every-1, 2 every-1, ...
// (a running destination and the next step, as the checkpoints: no 64-bit division in the loop) and after step nT-1.
// Record j is M after step min((j+1) every, nT) - 1, time-major: Mt[j] is (N*nM, 3), 768 B per wave and record.
template <typename T>
struct FusedTrajArgs : FusedArgs<T> {
    T* Mt;   int64_t every;                              // (nRec, N*nM, 3), nRec = ceil(nT / every)
};
template <typename T, int TR>
using FusedArgsT = std::conditional_t<TR == 0, FusedArgs<T>, FusedTrajArgs<T>>;
// the kernarg layout is part of the kernels' machine code: `in` sits where its twelve fields were written out
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
template <typename T>
constexpr bool fused_args_layout =
    offsetof(FusedArgs<T>, in) == 8 && offsetof(FusedArgs<T>, Mo) == 184 && offsetof(FusedArgs<T>, nC) == 232 &&
    sizeof(FusedArgs<T>) == 240 && offsetof(FusedTrajArgs<T>, Mt) == 240 && offsetof(FusedTrajArgs<T>, every) == 248 &&
    sizeof(FusedTrajArgs<T>) == 256;
#pragma clang diagnostic pop
static_assert(fused_args_layout<float> && fused_args_layout<double>, "K2's kernel arguments moved");

// CK: write checkpoints (every ck_every steps, a multiple of the 8-step chunk).  Kept out of the
// plain instantiation so that its step loop contains no store: the pulse loads are then provably
// unclobbered and become (batched) scalar loads.
// NCM: 1 = one coil (pulse samples are scalar loads); 2 / 4 / 8 / 16 / 32 = up to that many coils (the
// lane's b1 in 2 NCM registers, the chunk's rf samples staged in LDS and read as broadcasts; the
// coil sum is ONE ascending FMA chain whatever NCM is, so every capacity -- and K0 -- rounds alike);
// 0 = any number of coils (b1 and rf from memory inside the coil loop: slow, correctness path).
// Measured at 64^3 x 1024 before the 16 / 32 capacities existed: 8 coils 0.75 ms, 9 coils 5.85 ms,
// 16 coils 20.8 ms on the memory path (tools/ptx_timing.py).
constexpr int K2_MAXC = 64;                              // largest register/LDS coil capacity (48 / 64: float only)
// HB1 (one-coil builds): the coil has a b1 map (load_b1, k_fused_common.hpp).
// K2t: M after step t into the running record destination mtp if a record is taken there (TR == 1: after every step;
// TR == 2: after the step `next`, which then moves on by `every`)
template <int TR, typename T>
__device__ __forceinline__ void traj_record(int64_t t, bool valid, T mx, T my, T mz, T*& mtp, int64_t pitch,
                                            int64_t& next, int64_t every)
{
    if constexpr (TR == 1) {
        if (valid) { mtp[0] = mx; mtp[1] = my; mtp[2] = mz; }
        mtp += pitch;
    } else {
        ck_store(t, valid, mx, my, mz, mtp, pitch, next, every);
    }
}

template <typename T, typename CT, int NCM, bool CK, bool RELAX, bool HB1, int TR>
__global__ __launch_bounds__(WAVE) void k_bloch_rfgr_fwd(FusedArgsT<T, TR> a)
{
    // trajectory state (TR > 0, set before the loop): running destination, and (TR == 2) the step after which the next
    // record is taken.  Declared first and left uninitialised: dead locals further down reorder LLVM's promotion of the
    // others in the plain build, and with it the register assignment of nearly every TR == 0 kernel
    T* mtp;
    int64_t tr_every, tr_next;
    constexpr int NS = (sizeof(T) == 8 && NCM == 1) ? 4 : 8;   // fp64, one coil: 8 steps' pulse samples (80 SGPRs) spill to VGPR lanes
    constexpr bool NC1 = (NCM == 1);
    constexpr bool NCR = (NCM >= 2);                     // coils in registers / LDS
    constexpr int MC = NCR ? NCM : 1;                    // coil capacity of this instantiation
    static_assert(NCM == 0 || NCM == 1 || NCM == 2 || NCM == 4 || NCM == 8 || NCM == 16 || NCM == 32 || NCM == 40 ||
                  NCM == 48 || NCM == 64, "coil capacities: 2/4/8/16/32/40/48/64");
    static_assert(MC <= K2_MAXC, "capacity above K2_MAXC: the launcher would never select it");
    __shared__ __attribute__((aligned(16))) T srf[NCR ? 2 * NS * MC : 4];  // [re|im][j][c]
    const int lane = threadIdx.x;
    const int64_t n = blockIdx.y;
    bool valid;
    const int64_t s = lane_spin(blockIdx.x, lane, a.nM, valid);
    const int64_t row = n * a.nM + s;
    const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
    T mx = a.Mi[row * 3], my = a.Mi[row * 3 + 1], mz = a.Mi[row * 3 + 2];
    // (load_spin's loads, written out: through the helper every build of K2 gains or loses an s_waitcnt, LABNOTES)
    Spin<T> sp;
    sp.lx = a.in.loc[row * 3]; sp.ly = a.in.loc[row * 3 + 1]; sp.lz = a.in.loc[row * 3 + 2];
    sp.delta = T(0);
    if (a.in.df.p) sp.delta = bc_load<T>(a.in.df, n, s) / bc_load<T>(a.in.gam, n, s);
    T br, bi;
    load_b1<NC1 && HB1>(a.in.b1, row, br, bi);

    const int64_t nT = a.nT, nC = a.nC;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, nC);
    const T* b1 = a.in.b1 ? a.in.b1 + row * 2 * nC : nullptr;
    const int64_t rows = a.N * a.nM;
    T b1r[MC], b1i[MC];
    if (NCR) {
#pragma unroll
        for (int c = 0; c < MC; ++c) {
            b1r[c] = (c < nC) ? b1[c] : T(0);
            b1i[c] = (c < nC) ? b1[nC + c] : T(0);
        }
    }
    // NCR: rf samples of steps [tb, tb + cnt) -> LDS as [step][MC], ZERO beyond nC: the coil loop
    // of field_staged then needs no `c < nC` test (b1r/b1i are zero there too; adding exact zeros changes
    // nothing), stays one basic block, and its broadcast reads are batched.  With the test it compiled
    // to a branch and an exposed LDS round trip per coil, as in K0 (8 coils: 0.81 ms at 64^3 x 1024).
    auto stage_rf = [&](int64_t tb, int cnt) {
        __syncthreads();
        for (int i = lane; i < cnt * MC; i += WAVE) {
            const int j = i / MC, c = i - j * MC;
            const bool on = c < (int)nC;
            srf[i] = on ? pc.rfr[(tb + j) * nC + c] : T(0);
            srf[NS * MC + i] = on ? pc.rfi[(tb + j) * nC + c] : T(0);
        }
        __syncthreads();
    };
    int64_t tstage = 0;                                       // first step held in srf

    auto field = [&](int64_t t, T& Bx, T& By, T& Bz) {
        if (NC1) field_1coil<HB1>(br, bi, pc, t, sp, Bx, By, Bz);
        else if (NCR) field_staged<MC>(b1r, b1i, srf + (t - tstage) * MC, NS * MC, pc, t, sp, Bx, By, Bz);
        else {                                                // any number of coils, from memory
            Bx = T(0); By = T(0);
            for (int64_t c = 0; c < nC; ++c)
                field_xy_fma<T>(b1[c], b1[nC + c], pc.rfr[t * nC + c], pc.rfi[t * nC + c], Bx, By);
            Bz = field_z<T>(pc.gx[t], pc.gy[t], pc.gz[t], sp.lx, sp.ly, sp.lz, sp.delta);
        }
    };

    // The checkpoint build: all of the prologue's vector loads are awaited HERE, before the loop.  Otherwise the
    // wait for them lands in the loop header (the join of the prologue and the back edge) as s_waitcnt
    // vmcnt(0), where it also waits, every 8 steps, for the checkpoint store of the iteration before.
    if constexpr (TR != 0) { mtp = a.Mt + row * 3; tr_every = a.every; tr_next = tr_every - 1; }
    if (CK) __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
    int64_t ck_next = 0;
    T* ckp = CK ? a.Mck + row * 3 : nullptr;
    const int64_t ck_pitch = rows * 3;
    int64_t t0 = 0;
    for (; t0 + NS <= nT; t0 += NS) {
        if (NCR) { tstage = t0; stage_rf(t0, NS); }
        if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
        T Bx[NS], By[NS], Bz[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) field(t0 + j, Bx[j], By[j], Bz[j]);
        Rot<T> r[NS];
        rot_prepare<T, CT, NS>(k, Bx, By, Bz, r);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
            if constexpr (TR != 0) traj_record<TR>(t0 + j, valid, mx, my, mz, mtp, ck_pitch, tr_next, tr_every);
        }
    }
    if (NCR && t0 < nT) { tstage = t0; stage_rf(t0, (int)(nT - t0)); }
    for (; t0 < nT; ++t0) {                                   // nT % 8 tail
        if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
        T Bx[1], By[1], Bz[1];
        field(t0, Bx[0], By[0], Bz[0]);
        Rot<T> r[1];
        rot_prepare<T, CT, 1>(k, Bx, By, Bz, r);
        rot_apply<RELAX, T, CT>(k, r[0], mx, my, mz);
        if constexpr (TR != 0) traj_record<TR>(t0, valid, mx, my, mz, mtp, ck_pitch, tr_next, tr_every);
    }
    // the last record is M after step nT - 1 whatever `every` is: TR == 2 took it in the loop iff every | nT.  Mo is
    // optional in the trajectory builds (it equals that record)
    if constexpr (TR == 2) {
        if (tr_next - tr_every != nT - 1 && valid) { mtp[0] = mx; mtp[1] = my; mtp[2] = mz; }
    }
    if (valid && (TR == 0 || a.Mo)) { a.Mo[row * 3] = mx; a.Mo[row * 3 + 1] = my; a.Mo[row * 3 + 2] = mz; }
}

// ---------------------------------------------------------------------------------------------
// Host side of K2, shared by the launchers of tu_fused_fwd.hip and tu_fused_fwd1.hip.  A null Mt selects the plain
// kernel (TR == 0), which takes the FusedArgs part of the arguments; otherwise `every` picks TR.
// ---------------------------------------------------------------------------------------------
template <typename T>
FusedTrajArgs<T> fused_args(const void* Mi, const PulseOps& in, void* Mo, void* Mck, int64_t ck_every, void* Mt,
                            int64_t every, int64_t N, int64_t nM, int64_t nT, int64_t nC)
{
    FusedTrajArgs<T> a;
    a.Mi = (const T*)Mi; a.in = typed<T>(in); a.Mo = (T*)Mo; a.Mck = (T*)Mck;
    a.ck_every = ck_every > 0 ? ck_every : 1;
    a.N = N; a.nM = nM; a.nT = nT; a.nC = nC;
    a.Mt = (T*)Mt; a.every = every;
    return a;
}

// the build of coil capacity NCM for the checkpoint, relaxation and trajectory modes of `a`
template <typename T, typename CT, int NCM, bool HB1>
int launch_k2(const FusedTrajArgs<T>& a, hipStream_t st)
{
    // the plain kernel runs at nT == 0 too (it writes Mo = Mi); a trajectory then has no record
    dim3 grid;
    int rc;
    if (!fused_grid(a.N * a.nM * (a.Mt ? a.nT : 1), (a.nM + WAVE - 1) / WAVE, a.N, grid, rc)) return rc;
#define MRPHY_K2(CK_, RX_, TR_)                                                                         \
    hipLaunchKernelGGL((k_bloch_rfgr_fwd<T, CT, NCM, CK_, RX_, HB1, TR_>), grid, dim3(WAVE), 0, st, \
                       (static_cast<const FusedArgsT<T, TR_>&>(a)))
#define MRPHY_K2T(CK_, RX_)                                                                                 \
    do {                                                                                                    \
        if (!a.Mt) MRPHY_K2(CK_, RX_, 0);                                                                   \
        else if (a.every == 1) MRPHY_K2(CK_, RX_, 1);                                                       \
        else MRPHY_K2(CK_, RX_, 2);                                                                         \
    } while (0)
    const bool ck = (a.Mck != nullptr), rx = (a.in.E1.p != nullptr);
    if (ck) { if (rx) MRPHY_K2T(true, true); else MRPHY_K2T(true, false); }
    else    { if (rx) MRPHY_K2T(false, true); else MRPHY_K2T(false, false); }
#undef MRPHY_K2T
#undef MRPHY_K2
    return launch_status();
}

// k_fused_ext_fwd.hpp -- the forward frame of the Bz-extended kernels K2v (k_fused_moving.hpp) and K2sh (k_fused_shim.hpp)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_bwd_common.hpp"

// =============================================================================================
// K2's frame (one block = one wave = 64 spins of one batch entry), operands, build axes CK x RELAX x HB1 and step batches,
// then a per-step tail -- with the step's field from an extension policy X:
//     X::Args   X::args(BzExt)             the kernarg tail, where the entry points have it: between the operands and Mo
//     X::BATCH                             steps per batch
//     X::Lane   X::lane(args, row)         what the lane keeps in registers (the displacement per step; the channels' maps)
//     X::Wave   X::wave(args, n, nT)       what the wave keeps in scalar registers (step0; the waveforms' rows)
//     X::Tau    X::batch(wave, t)          a wave-uniform value of the batch -- or of the tail's step -- that starts at t,
//               X::step(tb, j)             and what step j of the batch makes of it (nothing where the field needs none)
//     X::field<HB1>(br, bi, pc, wave, lane, t, tau, sp, Bx, By, Bz)      the field of step t
// =============================================================================================
template <typename T, typename X>
struct ExtFwdArgs {
    const T* Mi;
    PulseOpsT<T> in;
    typename X::Args x;
    T* Mo;
    T* Mck;  int64_t ck_every;
    int64_t N, nM, nT;
};

template <typename T, typename CT, bool CK, bool RELAX, bool HB1, typename X>
__global__ __launch_bounds__(WAVE) void k_bloch_rfgr_ext_fwd(ExtFwdArgs<T, X> a)
{
    constexpr int NS = X::BATCH;
    const int lane = threadIdx.x;
    const int64_t n = blockIdx.y;
    bool valid;
    const int64_t s = lane_spin(blockIdx.x, lane, a.nM, valid);
    const int64_t row = n * a.nM + s;
    const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
    T mx = a.Mi[row * 3], my = a.Mi[row * 3 + 1], mz = a.Mi[row * 3 + 2];
    const Spin<T> sp = load_spin<T>(a.in, n, s, row);
    const typename X::Lane xl = X::lane(a.x, row);
    T br, bi;
    load_b1<HB1>(a.in.b1, row, br, bi);

    const int64_t nT = a.nT;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    const typename X::Wave xw = X::wave(a.x, n, nT);
    const int64_t rows = a.N * a.nM;
    // (the checkpoint build awaits the prologue's vector loads here, not in the loop header: k_fused_fwd.hpp)
    if (CK) __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
    int64_t ck_next = 0;
    T* ckp = CK ? a.Mck + row * 3 : nullptr;
    const int64_t ck_pitch = rows * 3;
    int64_t t0 = 0;
    for (; t0 + NS <= nT; t0 += NS) {
        if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
        const typename X::Tau tb = X::batch(xw, t0);
        T Bx[NS], By[NS], Bz[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j)
            X::template field<HB1>(br, bi, pc, xw, xl, t0 + j, X::step(tb, j), sp, Bx[j], By[j], Bz[j]);
        Rot<T> r[NS];
        rot_prepare<T, CT, NS>(k, Bx, By, Bz, r);
#pragma unroll
        for (int j = 0; j < NS; ++j) rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
    }
    for (; t0 < nT; ++t0) {                                   // nT % NS tail
        if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
        T Bx[1], By[1], Bz[1];
        X::template field<HB1>(br, bi, pc, xw, xl, t0, X::batch(xw, t0), sp, Bx[0], By[0], Bz[0]);
        Rot<T> r[1];
        rot_prepare<T, CT, 1>(k, Bx, By, Bz, r);
        rot_apply<RELAX, T, CT>(k, r[0], mx, my, mz);
    }
    if (valid) { a.Mo[row * 3] = mx; a.Mo[row * 3 + 1] = my; a.Mo[row * 3 + 2] = mz; }
}

// Host: the arguments from what the launcher of a forward build gets (internal.hpp: run_rfgr_ext_fwd), and the launch of
// the build CK x RELAX x HB1 they ask for.  Runs at nT == 0 too (Mo = Mi), as K2
template <typename X, typename T, typename CT>
int launch_ext_fwd(const void* Mi, const PulseOps& in, const BzExt& x, void* Mo, void* Mck, int64_t ck_every, int64_t N,
                   int64_t nM, int64_t nT, hipStream_t st)
{
    ExtFwdArgs<T, X> a;
    a.Mi = (const T*)Mi; a.in = typed<T>(in); a.x = X::args(x); a.Mo = (T*)Mo; a.Mck = (T*)Mck;
    a.ck_every = ck_every > 0 ? ck_every : 1;
    a.N = N; a.nM = nM; a.nT = nT;
    dim3 grid;
    int rc;
    if (!fused_grid(N * nM, (nM + WAVE - 1) / WAVE, N, grid, rc)) return rc;
#define MRPHY_K2X(CK_, RX_, HB_) \
    hipLaunchKernelGGL((k_bloch_rfgr_ext_fwd<T, CT, CK_, RX_, HB_, X>), grid, dim3(WAVE), 0, st, a)
#define MRPHY_K2X_HB(CK_, RX_) \
    do { if (a.in.b1) MRPHY_K2X(CK_, RX_, true); else MRPHY_K2X(CK_, RX_, false); } while (0)
    const bool ck = (a.Mck != nullptr), rx = (a.in.E1.p != nullptr);
    if (ck) { if (rx) MRPHY_K2X_HB(true, true); else MRPHY_K2X_HB(true, false); }
    else    { if (rx) MRPHY_K2X_HB(false, true); else MRPHY_K2X_HB(false, false); }
#undef MRPHY_K2X_HB
#undef MRPHY_K2X
    return launch_status();
}

// k_signal_fwd.hpp -- K2s (fused rf,gr -> received signal: the transverse magnetisation summed over the spins)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_common.hpp"

// =============================================================================================
// K2s: K2's step loop (one block = one wave = 64 spins of ONE batch entry, the pulse through scalar loads, the same
// field / rot_prepare / rot_apply and therefore the same bits of M), but instead of M the wave keeps what a receive
// coil sees: at each record step (the trajectory's convention: after steps min((j+1) every, nT) - 1) the lane forms
//     s0 = rx_re Mx - rx_im My,   s1 = rx_re My + rx_im Mx                    (the product of b1Map . rf, no conjugate)
// and puts the two numbers into an LDS tile of 2 SEG rows x 64 lanes (K2b's swizzle).  When the tile holds SEG records
// (or the pulse ends) the 2 SEG rows are summed over the lanes in K2b's fixed four-chain order and added into the
// wave's OWN workspace row; waves are persistent over the tiles w, w + P, ... as in K2b, so every row is accumulated in
// a fixed order, and a second pass sums the P rows in fixed order: deterministic, no float atomics, and no per-spin
// record ever reaches HBM.  A stride of SEG or more fills the tile over several segments and reduces once per SEG
// records, so it costs next to nothing over K2.
// =============================================================================================
template <typename T>
struct SignalArgs {
    const T* Mi;
    PulseOpsT<T> in;                 // b1: (N, nM, 2) or null
    const T* rx;                     // (N, nM, 2) or null = (1, 0)
    T* Mo;                           // may be null
    T* Mck;  int64_t ck_every;       // may be null
    T* work;                         // (P, N, 2, nRec)
    int64_t every, nRec;
    int64_t N, nM, nT, P;
};
// the kernarg layout is part of the kernel's machine code: `in` sits where its twelve fields were written out
static_assert(offsetof(SignalArgs<float>, in) == 8 && offsetof(SignalArgs<float>, rx) == 184 &&
              offsetof(SignalArgs<float>, P) == 264 && sizeof(SignalArgs<float>) == 272 &&
              offsetof(SignalArgs<double>, rx) == 184 && offsetof(SignalArgs<double>, P) == 264 &&
              sizeof(SignalArgs<double>) == 272, "K2s's kernel arguments moved");

// What a coil with weight (rxr, rxi) sees of the lane's (mx, my): s0 = rxr mx - rxi my, s1 = rxr my + rxi mx, with the
// roundings spelled out -- one product rounded, the other fused into the sum.  K2s and the multi-coil kernel
// (k_signal_mrx_fwd.hpp) both form their records here, so a coil's terms are the same bits in both whatever a compiler
// would have made of the plain expressions (these are the forms K2s was compiled to when the choice was the compiler's).
template <typename T>
__device__ __forceinline__ void rx_products(T rxr, T rxi, T mx, T my, T& s0, T& s1)
{
#pragma clang fp contract(off)
    s0 = fma_(rxr, mx, -(rxi * my));
    s1 = fma_(rxi, mx, rxr * my);
}

// CK, RELAX, HB1: as K2.  EV1: every == 1 -- a record after every step, its slot known at compile time inside the
// unrolled step batch; otherwise the step of the next record is carried (wave-uniform) and compared, as in K2t.
template <typename T, typename CT, bool CK, bool RELAX, bool HB1, bool EV1>
__global__ __launch_bounds__(WAVE) void k_signal_fwd(SignalArgs<T> a)
{
    constexpr int NS = sizeof(T) == 8 ? 4 : 8;               // steps per batch, as K2's one-coil builds
    static_assert(SEG % NS == 0, "a batch of records must fit the tile");
    __shared__ __attribute__((aligned(16))) T red[2 * SEG * RED_PITCH];
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y;
    const int64_t nT = a.nT, rows = a.N * a.nM, nRec = a.nRec, every = a.every;
    const int64_t ntiles = (a.nM + WAVE - 1) / WAVE;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    // row sums: lane (r, h) forms chains 2h and 2h + 1 of row r = q SEG + slot; the two halves meet as
    // (p0 + p1) + (p2 + p3), K2b's order
    const int rr = lane >> 1, rh = lane & 1;
    T* wdst = a.work + ((w * a.N + n) * 2 + rr / SEG) * nRec + (rr % SEG);
    // the most records a batch of NS steps can take: those of the stride, and the one after the last step
    const int maxrec = EV1 ? NS : (int)((NS - 1) / every + 2 < NS ? (NS - 1) / every + 2 : NS);
    const int64_t ck_pitch = rows * 3;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.P) {
        bool valid;
        const int64_t s = lane_spin(tile, lane, a.nM, valid);
        const int64_t row = n * a.nM + s;
        const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
        T mx = a.Mi[row * 3], my = a.Mi[row * 3 + 1], mz = a.Mi[row * 3 + 2];
        // (load_spin's loads, written out as in K2: through the helper the checkpoint builds gain an s_waitcnt, LABNOTES)
        Spin<T> sp;
        sp.lx = a.in.loc[row * 3]; sp.ly = a.in.loc[row * 3 + 1]; sp.lz = a.in.loc[row * 3 + 2];
        sp.delta = T(0);
        if (a.in.df.p) sp.delta = bc_load<T>(a.in.df, n, s) / bc_load<T>(a.in.gam, n, s);
        T br, bi;
        load_b1<HB1>(a.in.b1, row, br, bi);
        // lanes past nM (they hold a copy of the last valid spin) receive with weight zero: their two products are
        // exact zeros -- masked here, once per tile
        T rxr = valid ? T(1) : T(0), rxi = T(0);
        if (a.rx && valid) { rxr = a.rx[row * 2]; rxi = a.rx[row * 2 + 1]; }

        auto field = [&](int64_t t, T& Bx, T& By, T& Bz) { field_1coil<HB1>(br, bi, pc, t, sp, Bx, By, Bz); };
        int cnt = 0;                                             // records in the tile (wave-uniform)
        int64_t jbase = 0;                                       // records of this spin tile already reduced
        int64_t next = every - 1 < nT - 1 ? every - 1 : nT - 1;  // the step after which the next record is taken
        auto rec = [&](int slot) {
            T s0, s1;
            rx_products(rxr, rxi, mx, my, s0, s1);
            red[red_idx(slot, lane)] = s0;
            red[red_idx(SEG + slot, lane)] = s1;
        };
        auto take = [&](int64_t t) {                             // the record after step t, if one is due
            if (t == next) {
                rec(cnt); ++cnt;
                next = every < nT - 1 - next ? next + every : nT - 1;   // the last one: after step nT - 1
            }
        };
        // reduce the cnt records of the tile into the workspace rows of records jbase .. jbase + cnt - 1 (rows past
        // cnt hold stale numbers: summed, never stored).  The old workspace value is requested before the row sums.
        auto flush = [&]() {
            const bool mine = rh == 0 && (rr % SEG) < cnt;
            T old = T(0);
            if (!first && mine) old = wdst[jbase];
            __syncthreads();
            T p0 = T(0), p1 = T(0);
#pragma unroll
            for (int i = 0; i < WAVE; i += 4) {
                const T* q = red + red_idx(rr, i) + 2 * rh;
                p0 += q[0]; p1 += q[1];
            }
            T p = p0 + p1;
            p += __shfl_xor(p, 1);
            if (mine) wdst[jbase] = old + p;
            __syncthreads();
            jbase += cnt; cnt = 0;
        };

        // (checkpoints as in K2: a running destination; the prologue's vector loads are awaited before the loop)
        if (CK) __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
        int64_t ck_next = 0;
        T* ckp = CK ? a.Mck + row * 3 : nullptr;
        int64_t t0 = 0;
        for (; t0 + NS <= nT; t0 += NS) {
            if (cnt + maxrec > SEG) flush();
            if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
            T Bx[NS], By[NS], Bz[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) field(t0 + j, Bx[j], By[j], Bz[j]);
            Rot<T> r[NS];
            rot_prepare<T, CT, NS>(k, Bx, By, Bz, r);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
                if constexpr (EV1) rec(cnt + j);
                else take(t0 + j);
            }
            if constexpr (EV1) cnt += NS;
        }
        for (; t0 < nT; ++t0) {                                   // nT % NS tail
            if (cnt == SEG) flush();
            if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
            T Bx[1], By[1], Bz[1];
            field(t0, Bx[0], By[0], Bz[0]);
            Rot<T> r[1];
            rot_prepare<T, CT, 1>(k, Bx, By, Bz, r);
            rot_apply<RELAX, T, CT>(k, r[0], mx, my, mz);
            if constexpr (EV1) { rec(cnt); ++cnt; }
            else take(t0);
        }
        if (cnt > 0) flush();
        if (valid && a.Mo) { a.Mo[row * 3] = mx; a.Mo[row * 3 + 1] = my; a.Mo[row * 3 + 2] = mz; }
        first = false;
    }
}

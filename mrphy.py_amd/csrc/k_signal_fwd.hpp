// k_signal_fwd.hpp -- K2s (fused rf,gr -> received signal: the transverse magnetisation summed over the spins, for one
// receive coil or an array of them)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_common.hpp"

// =============================================================================================
// K2s: K2's step loop (one block = one wave = 64 spins of ONE batch entry, the pulse through scalar loads, the same
// field / rot_prepare / rot_apply and therefore the same bits of M), but instead of M the wave keeps what the receive
// coils see.  R is the coil capacity of the build (1, 2, 4, 8; nRx <= R coils are used, the pad coils have weight zero
// and their rows are never stored).  At each record step (the trajectory's convention: after steps
// min((j+1) every, nT) - 1) the lane forms, per coil c,
//     s0 = rx_re Mx - rx_im My,   s1 = rx_re My + rx_im Mx                    (the product of b1Map . rf, no conjugate)
// and puts the 2 R numbers into an LDS tile of 2 SEG rows x 64 lanes (K2b's swizzle), which therefore holds SEG / R
// records.  When the tile is full (or the pulse ends) the 2 SEG rows are summed over the lanes in K2b's fixed four-chain
// order and added into the wave's OWN workspace row (P, N, 2 nRx, nRec); waves are persistent over the tiles w, w + P,
// ... as in K2b, so every row is accumulated in a fixed order, and a second pass sums the P rows in fixed order:
// deterministic, no float atomics, and no per-spin record ever reaches HBM.  A stride of SEG or more fills the tile over
// several segments and reduces once per tile, so it costs next to nothing over K2.
// The sum of a row depends on nothing but that row and a workspace element is accumulated in tile order, so coil c
// comes out with the same bits at every capacity, in whatever row of the tile its record sits and wherever the tile is
// flushed: the one-coil kernel is this kernel at R = 1.
// =============================================================================================
template <typename T>
struct SignalArgs {
    const T* Mi;
    PulseOpsT<T> in;                 // b1: (N, nM, 2) or null
    const T* rx;                     // (N, nM, 2, nRx); R = 1 only: or null = (1, 0)
    T* Mo;                           // may be null
    T* Mck;  int64_t ck_every;       // may be null
    T* work;                         // (P, N, 2 nRx, nRec)
    int64_t every, nRec;
    int64_t N, nM, nT, P;
    int64_t nRx;
};
// the kernarg layout is part of the kernel's machine code: `in` sits where its twelve fields were written out
static_assert(offsetof(SignalArgs<float>, in) == 8 && offsetof(SignalArgs<float>, rx) == 184 &&
              offsetof(SignalArgs<float>, P) == 264 && offsetof(SignalArgs<float>, nRx) == 272 &&
              sizeof(SignalArgs<float>) == 280 && offsetof(SignalArgs<double>, rx) == 184 &&
              offsetof(SignalArgs<double>, P) == 264 && offsetof(SignalArgs<double>, nRx) == 272 &&
              sizeof(SignalArgs<double>) == 280, "K2s's kernel arguments moved");

// What a coil with weight (rxr, rxi) sees of the lane's (mx, my): s0 = rxr mx - rxi my, s1 = rxr my + rxi mx, with the
// roundings spelled out -- one product rounded, the other fused into the sum -- so that a coil's terms are the same bits
// at every capacity whatever a compiler would have made of the plain expressions (these are the forms the one-coil
// kernel was compiled to when the choice was the compiler's).
template <typename T>
__device__ __forceinline__ void rx_products(T rxr, T rxi, T mx, T my, T& s0, T& s1)
{
#pragma clang fp contract(off)
    s0 = fma_(rxr, mx, -(rxi * my));
    s1 = fma_(rxi, mx, rxr * my);
}

// The tile row of quantity q = 2 c + ri of the record in slot `slot`, and its inverse.  One coil keeps the quantities
// apart (q SEG + slot), an array keeps a record's rows together (slot 2R + q): the orders each capacity was written and
// timed with.  Nothing but the address arithmetic depends on it.
template <int R> constexpr int sig_row(int slot, int q) { return R == 1 ? q * SEG + slot : slot * (2 * R) + q; }
template <int R> constexpr int sig_row_slot(int row) { return R == 1 ? row % SEG : row / (2 * R); }
template <int R> constexpr int sig_row_q(int row) { return R == 1 ? row / SEG : row % (2 * R); }

// CK, RELAX, HB1: as K2.  EV1: every == 1 -- a record after every step, its slot known at compile time inside the
// unrolled step batch; otherwise the step of the next record is carried (wave-uniform) and compared, as in K2t.
// Where the tile is flushed is one rule: a tile that holds at least a batch's NS records (PRE) is tested once before
// the batch, for the most records the batch can take; a smaller one is tested at each record -- in the EV1 builds at
// the points of the unrolled batch that are known at compile time.
template <typename T, typename CT, bool CK, bool RELAX, bool HB1, bool EV1, int R>
__global__ __launch_bounds__(WAVE) void k_signal_fwd(SignalArgs<T> a)
{
    constexpr int NS = sizeof(T) == 8 ? 4 : 8;               // steps per batch, as K2's one-coil builds
    constexpr int RC = SEG / R;                              // records per tile
    constexpr bool PRE = RC >= NS;
    static_assert(SEG % R == 0 && (RC % NS == 0 || NS % RC == 0), "a record's rows and a batch's records tile the tile");
    __shared__ __attribute__((aligned(16))) T red[2 * SEG * RED_PITCH];
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y;
    const int64_t nT = a.nT, rows = a.N * a.nM, nRec = a.nRec, every = a.every;
    const int64_t ntiles = (a.nM + WAVE - 1) / WAVE;
    const int64_t nRx = R == 1 ? 1 : a.nRx;                  // 1 <= nRx <= R
    const int nrx = (int)nRx;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    // row sums: lane (r, h) forms chains 2h and 2h + 1 of row r; the two halves meet as (p0 + p1) + (p2 + p3), K2b's
    // order.  The rows of the pad coils (q >= 2 nRx) are summed and never stored
    const int rr = lane >> 1, rh = lane & 1;
    const int rslot = sig_row_slot<R>(rr), rq = sig_row_q<R>(rr);
    const bool stored = rh == 0 && rq < 2 * nrx;
    T* wdst = a.work + ((w * a.N + n) * 2 * nrx + (stored ? rq : 0)) * nRec + rslot;
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
        // lanes past nM (they hold a copy of the last valid spin) and the pad coils receive with weight zero: their
        // products are exact zeros -- masked here, once per tile.  No map (R = 1 only): weight (1, 0)
        T rxr[R], rxi[R];
        {
            const T* q = a.rx + row * 2 * nRx;               // (from a null rx at R = 1: formed, never dereferenced)
#pragma unroll
            for (int c = 0; c < R; ++c) {
                rxr[c] = R == 1 && valid ? T(1) : T(0); rxi[c] = T(0);
                if ((R > 1 || a.rx) && c < nrx && valid) { rxr[c] = q[c]; rxi[c] = q[nRx + c]; }
            }
        }

        auto field = [&](int64_t t, T& Bx, T& By, T& Bz) { field_1coil<HB1>(br, bi, pc, t, sp, Bx, By, Bz); };
        int cnt = 0;                                             // records in the tile (wave-uniform)
        int64_t jbase = 0;                                       // records of this spin tile already reduced
        int64_t next = every - 1 < nT - 1 ? every - 1 : nT - 1;  // the step after which the next record is taken
        auto rec = [&](int slot) {
#pragma unroll
            for (int c = 0; c < R; ++c) {
                T s0, s1;
                rx_products(rxr[c], rxi[c], mx, my, s0, s1);
                red[red_idx(sig_row<R>(slot, 2 * c), lane)] = s0;
                red[red_idx(sig_row<R>(slot, 2 * c + 1), lane)] = s1;
            }
        };
        // reduce the cnt records of the tile into the workspace rows of records jbase .. jbase + cnt - 1 (rows past
        // cnt hold stale numbers: summed, never stored).  The old workspace value is requested before the row sums.
        auto flush = [&]() {
            const bool mine = stored && rslot < cnt;
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
        auto room = [&](int n_) {                                // PRE: before steps that can take n_ records
            if constexpr (PRE) { if (cnt + n_ > RC) flush(); }
        };
        auto put = [&]() {                                       // one record into the next slot
            if constexpr (!PRE) { if (cnt == RC) flush(); }
            rec(cnt); ++cnt;
        };
        auto take = [&](int64_t t) {                             // the record after step t, if one is due
            if constexpr (EV1) put();
            else if (t == next) {
                put();
                next = every < nT - 1 - next ? next + every : nT - 1;   // the last one: after step nT - 1
            }
        };

        // (checkpoints as in K2: a running destination; the prologue's vector loads are awaited before the loop)
        if (CK) __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
        int64_t ck_next = 0;
        T* ckp = CK ? a.Mck + row * 3 : nullptr;
        int64_t t0 = 0;
        for (; t0 + NS <= nT; t0 += NS) {
            room(maxrec);
            if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
            T Bx[NS], By[NS], Bz[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) field(t0 + j, Bx[j], By[j], Bz[j]);
            Rot<T> r[NS];
            rot_prepare<T, CT, NS>(k, Bx, By, Bz, r);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
                if constexpr (EV1 && PRE) rec(cnt + j);
                else if constexpr (EV1) {                         // a batch fills the tile NS / RC times
                    rec(j % RC);
                    if (j % RC == RC - 1) { cnt = RC; flush(); }
                } else take(t0 + j);
            }
            if constexpr (EV1 && PRE) cnt += NS;
        }
        for (; t0 < nT; ++t0) {                                   // nT % NS tail
            room(1);
            if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
            T Bx[1], By[1], Bz[1];
            field(t0, Bx[0], By[0], Bz[0]);
            Rot<T> r[1];
            rot_prepare<T, CT, 1>(k, Bx, By, Bz, r);
            rot_apply<RELAX, T, CT>(k, r[0], mx, my, mz);
            take(t0);
        }
        if (cnt > 0) flush();
        if (valid && a.Mo) { a.Mo[row * 3] = mx; a.Mo[row * 3 + 1] = my; a.Mo[row * 3 + 2] = mz; }
        first = false;
    }
}

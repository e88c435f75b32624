// k_signal_mrx_fwd.hpp -- K2s-mrx (K2s for several receive coils: one simulation, every coil's signal)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_signal_fwd.hpp"

// =============================================================================================
// K2s-mrx: K2s's step loop, tile and row sums, with 2 R receive weights per lane instead of two (R: the coil capacity of
// the build, nRx <= R coils are used; the pad coils have weight zero and their rows are never stored).  A record takes
// 2 R rows of the 2 SEG-row tile -- row (slot, q) = slot 2R + q, quantity q = 2 c + ri -- so the tile holds SEG / R
// records.  Every row is summed over the lanes as K2s sums it (lane (r, h) chains 2h, 2h + 1, met as (p0 + p1) +
// (p2 + p3)) and added into the wave's own workspace row (P, N, 2 nRx, nRec) in tile order; the second pass is K2s's.
// The sum of a row depends on nothing but that row, so coil c comes out bit for bit as K2s gives it for that coil
// alone, wherever the tile is flushed: when it is full -- in the every == 1 builds at points known at compile time
// (before a batch that would not fit, or after every SEG / R steps of a batch longer than that), otherwise at the
// record that finds it full.
// =============================================================================================
template <typename T>
struct SignalMrxArgs : SignalArgs<T> {   // rx: (N, nM, 2, nRx), never null; work: (P, N, 2 nRx, nRec)
    int64_t nRx;
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(offsetof(SignalMrxArgs<float>, rx) == 184 && offsetof(SignalMrxArgs<float>, P) == 264 &&
              offsetof(SignalMrxArgs<float>, nRx) == 272 && sizeof(SignalMrxArgs<float>) == 280 &&
              offsetof(SignalMrxArgs<double>, nRx) == 272 && sizeof(SignalMrxArgs<double>) == 280,
              "K2s-mrx's kernel arguments moved");
#pragma clang diagnostic pop

template <typename T, typename CT, bool CK, bool RELAX, bool HB1, bool EV1, int R>
__global__ __launch_bounds__(WAVE) void k_signal_mrx_fwd(SignalMrxArgs<T> a)
{
    constexpr int NS = sizeof(T) == 8 ? 4 : 8;               // steps per batch, as K2s
    constexpr int Q = 2 * R;                                 // rows per record
    constexpr int RC = SEG / R;                              // records per tile
    static_assert(R >= 2 && SEG % R == 0 && (RC % NS == 0 || NS % RC == 0), "a record's rows and a batch's records tile the tile");
    __shared__ __attribute__((aligned(16))) T red[2 * SEG * RED_PITCH];
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y;
    const int64_t nT = a.nT, rows = a.N * a.nM, nRec = a.nRec, every = a.every;
    const int64_t ntiles = (a.nM + WAVE - 1) / WAVE;
    const int nrx = (int)a.nRx;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    // row sums: lane (r, h) forms chains 2h and 2h + 1 of row r = slot Q + q, K2s's order; the rows of the pad coils
    // (q >= 2 nRx) are summed and never stored
    const int rr = lane >> 1, rh = lane & 1;
    const int rslot = rr / Q, rq = rr % Q;
    const bool stored = rh == 0 && rq < 2 * nrx;
    T* wdst = a.work + ((w * a.N + n) * 2 * nrx + (stored ? rq : 0)) * nRec + rslot;
    const int64_t ck_pitch = rows * 3;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.P) {
        bool valid;
        const int64_t s = lane_spin(tile, lane, a.nM, valid);
        const int64_t row = n * a.nM + s;
        const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
        T mx = a.Mi[row * 3], my = a.Mi[row * 3 + 1], mz = a.Mi[row * 3 + 2];
        Spin<T> sp;
        sp.lx = a.in.loc[row * 3]; sp.ly = a.in.loc[row * 3 + 1]; sp.lz = a.in.loc[row * 3 + 2];
        sp.delta = T(0);
        if (a.in.df.p) sp.delta = bc_load<T>(a.in.df, n, s) / bc_load<T>(a.in.gam, n, s);
        T br, bi;
        load_b1<HB1>(a.in.b1, row, br, bi);
        // lanes past nM (they hold a copy of the last valid spin) and the pad coils receive with weight zero
        T rxr[R], rxi[R];
        {
            const T* q = a.rx + row * 2 * a.nRx;
#pragma unroll
            for (int c = 0; c < R; ++c) {
                rxr[c] = rxi[c] = T(0);
                if (c < nrx && valid) { rxr[c] = q[c]; rxi[c] = q[a.nRx + c]; }
            }
        }

        auto field = [&](int64_t t, T& Bx, T& By, T& Bz) { field_1coil<HB1>(br, bi, pc, t, sp, Bx, By, Bz); };
        int cnt = 0;                                             // records in the tile (wave-uniform)
        int64_t jbase = 0;                                       // records of this spin tile already reduced
        int64_t next = every - 1 < nT - 1 ? every - 1 : nT - 1;  // the step after which the next record is taken
        auto rec = [&](int slot) {                               // K2s's two products (rx_products), per coil
#pragma unroll
            for (int c = 0; c < R; ++c) {
                T s0, s1;
                rx_products(rxr[c], rxi[c], mx, my, s0, s1);
                red[red_idx(slot * Q + 2 * c, lane)] = s0;
                red[red_idx(slot * Q + 2 * c + 1, lane)] = s1;
            }
        };
        // reduce the cnt records of the tile into the workspace rows of records jbase .. jbase + cnt - 1 (K2s's flush)
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
        auto take = [&](int64_t t) {                             // the record after step t, if one is due
            if (t == next) {
                if (cnt == RC) flush();
                rec(cnt); ++cnt;
                next = every < nT - 1 - next ? next + every : nT - 1;   // the last one: after step nT - 1
            }
        };

        if (CK) __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0), as K2s
        int64_t ck_next = 0;
        T* ckp = CK ? a.Mck + row * 3 : nullptr;
        int64_t t0 = 0;
        for (; t0 + NS <= nT; t0 += NS) {
            if constexpr (EV1 && RC >= NS) { if (cnt + NS > RC) flush(); }
            if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
            T Bx[NS], By[NS], Bz[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) field(t0 + j, Bx[j], By[j], Bz[j]);
            Rot<T> r[NS];
            rot_prepare<T, CT, NS>(k, Bx, By, Bz, r);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
                if constexpr (EV1 && RC >= NS) rec(cnt + j);
                else if constexpr (EV1) {                         // a batch fills the tile NS / RC times
                    rec(j % RC);
                    if (j % RC == RC - 1) { cnt = RC; flush(); }
                } else take(t0 + j);
            }
            if constexpr (EV1 && RC >= NS) cnt += NS;
        }
        for (; t0 < nT; ++t0) {                                   // nT % NS tail
            if (CK) ck_store(t0, valid, mx, my, mz, ckp, ck_pitch, ck_next, a.ck_every);
            T Bx[1], By[1], Bz[1];
            field(t0, Bx[0], By[0], Bz[0]);
            Rot<T> r[1];
            rot_prepare<T, CT, 1>(k, Bx, By, Bz, r);
            rot_apply<RELAX, T, CT>(k, r[0], mx, my, mz);
            if constexpr (EV1) { if (cnt == RC) flush(); rec(cnt); ++cnt; }
            else take(t0);
        }
        if (cnt > 0) flush();
        if (valid && a.Mo) { a.Mo[row * 3] = mx; a.Mo[row * 3 + 1] = my; a.Mo[row * 3 + 2] = mz; }
        first = false;
    }
}

// k_train_signal.hpp -- the signal of a pulse repeated K times: Ktr's recursion with the transverse magnetisation
// summed over the spins per repetition, for one receive coil or an array of them, and its adjoint (Ktrs / Ktrsb)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp and k_ab_train.hpp
// (TrainArgs, TrainSpin, train_spin, train_rep, TrainCP).  Not a standalone header.
#pragma once

// =============================================================================================
// Ktrs: Ktr's recursion (train_rep: the same fp64 arithmetic, the same bits of M), one thread per spin, one block =
// one wave = 64 spins of ONE batch entry (blockIdx.y = n), the phase table through scalar loads.  Instead of the
// records the wave keeps what the receive coils see of them.  R is the coil capacity of the build (1, 2, 4, 8; nRx <= R
// coils are used, the pad coils have weight zero and their rows are never stored).  After each repetition k the lane
// forms, per coil c, in fp64
//     s0 = rx_re Mx - rx_im My,   s1 = rx_re My + rx_im Mx                 (K2s's product, no conjugate)
// at M_{k+1} and puts the 2 R numbers into an LDS tile of TRS_ROWS rows x 64 lanes, which holds TRS_ROWS / 2R records.
// A full tile (or the end of the train) is summed over the lanes, each row in one fixed order, and added into the
// wave's OWN workspace row (P, N, 2 nRx, K) fp64 -- stored by the wave's first spin tile, read-modify-written from its
// second on: waves are persistent over the tiles w, w + P, ...  A second pass (k_train_signal_p2) sums the P rows in
// fixed order and rounds ONCE into the data type: sig (N, 2, K, nRx).  No float atomics; the same inputs give the
// same bits; the sum of a row depends on that row alone and a workspace element receives one term per spin tile in
// tile order, so coil c has the same bits at every capacity.  Nothing of size K x spins reaches memory: with a
// checkpoint pointer the fp64 state BEFORE repetitions 0, S, 2S, ... (S = TRS_SEG) is written time-major,
// ck (ceil(K/S), rows, 3); without one nothing is written per spin but Mlast.
//
// Ktrsb: Ktrb's sweep, per segment of S repetitions from the last to the first.  The segment's states M_k .. M_{k+S}
// are recomputed from its checkpoint into registers (fully unrolled, compile-time indices; the tail segment by
// wave-uniform guards), then walked downwards exactly as Ktrb walks, with the cotangent of record k formed from the
// wave-uniform table gs (N, K, nRx, 2) fp64 (scalar loads) and the lane's receive weights,
//     G_k = (sum_c rx_re g0 + rx_im g1,  sum_c rx_re g1 - rx_im g0,  0)       in ascending c,
// from h = the cotangent of Mlast (or 0).  grad_rx is a lane-private sum over k at M_{k+1}:
//     d/d rx_re = g0 Mx + g1 My,   d/d rx_im = g1 Mx - g0 My.
// dL/dphi_k is summed over the spins here: one tile row per repetition of the segment, reduced and accumulated as the
// forward's rows, workspace (P, N, K) and the same second pass -> grad_phase (N, K).  grad_A, grad_B and grad_Mi per
// spin as Ktrb writes them; grad_consts per spin with Ktrb's formulas, but in fp64 whatever the data type.
// =============================================================================================
struct TrainSigArgs {
    TrainArgs t;                    // A .. cs, gA, gB, gMi, rows, nM, K as Ktr / Ktrb take them; gC (rows, 4) is fp64
                                    // here; g, Mt, gphi unused
    const void* rx; int64_t nRx;    // (rows, 2, nRx); R = 1 only: or null = (1, 0)
    void* Mlast;                    // (rows, 3): the last record (forward; may be null)
    double* ck;                     // (ceil(K/S), rows, 3) fp64: written by the forward (null: not wanted), read by the adjoint
    double* work;                   // forward: (P, N, 2 nRx, K); adjoint: (P, N, K), null = no phase gradient
    const double* gs;               // adjoint: (N, K, nRx, 2) fp64, the cotangent of sig; null: none
    const void* gMl;                // adjoint: (rows, 3), the cotangent of Mlast; null: none
    void* grx;                      // adjoint: (rows, 2, nRx); may be null
    int64_t N, P;
};

// One repetition, M := Rz(phi) [ A Rz(-phi) (F M + f) + B ] with (cp, sp) = (cos phi, sin phi): Ktr's expressions
// (k_ab_train.hpp) with every rounding spelled out -- which product is rounded and which is fused into the sum is
// written as Ktr's loop is compiled, so that the state has Ktr's bits whatever a compiler would make of the plain
// expressions in another kernel (sharing them as one inline function changed the contractions of Ktr itself).
__device__ __forceinline__ void train_rep(const TrainSpin& v, double a0, double a1, double a2, double a3, double a4,
                                          double a5, double a6, double a7, double a8, double b0, double b1, double b2,
                                          double cp, double sp, double& mx, double& my, double& mz)
{
#pragma clang fp contract(off)
    const double rx = fma(v.c, mx, -(v.s * my)), ry = fma(v.c, my, v.s * mx);
    const double px = rx * v.e2, py = ry * v.e2, pz = fma(mz, v.e1, v.f3);       // M- = F M + f
    const double qx = fma(sp, py, cp * px), qy = fma(cp, py, -(sp * px));        // Rz(-phi) M-
    const double tx = fma(a2, pz, fma(a0, qx, a1 * qy)) + b0;
    const double ty = fma(a5, pz, fma(a3, qx, a4 * qy)) + b1;
    mz = fma(a8, pz, fma(a6, qx, a7 * qy)) + b2;
    mx = fma(cp, tx, -(sp * ty)); my = fma(sp, tx, cp * ty);                     // Rz(phi) (A . + B)
}

// pitch of the reduction tile in doubles: 132 dwords = 4 mod 64 banks, so that the 32 lanes (row, half) of one pass of
// an 8-byte read hit 32 different bank pairs; a record's stores (lane-contiguous) are conflict-free at any pitch
constexpr int TRS_PITCH = WAVE + 2;

// The sum of tile row rr over the 64 lanes, on both lanes (rr, 0) and (rr, 1): lane (rr, rh) adds the elements
// rh, rh + 2, ... in two chains; the halves meet as (p0 + p1) + (p0' + p1').  One fixed order whatever the build.
__device__ __forceinline__ double trs_row_sum(const double* red, int rr, int rh)
{
    const double* q = red + rr * TRS_PITCH + rh;
    double p0 = 0.0, p1 = 0.0;
#pragma unroll
    for (int i = 0; i < WAVE; i += 4) { p0 += q[i]; p1 += q[i + 2]; }
    double p = p0 + p1;
    p += __shfl_xor(p, 1);
    return p;
}

// What a coil with weight (rxr, rxi) sees of (mx, my), with the roundings spelled out as K2s's rx_products has them:
// a coil's terms are the same bits at every capacity.
__device__ __forceinline__ void trs_products(double rxr, double rxi, double mx, double my, double& s0, double& s1)
{
#pragma clang fp contract(off)
    s0 = fma(rxr, mx, -(rxi * my));
    s1 = fma(rxi, mx, rxr * my);
}

template <typename T, int R>
__global__ __launch_bounds__(WAVE) void k_train_signal_fwd(TrainSigArgs a)
{
    constexpr int RC = TRS_ROWS / (2 * R);                    // records per tile
    static_assert(TRS_ROWS == WAVE / 2 && TRS_ROWS % (2 * R) == 0, "two lanes per tile row, whole records per tile");
    __shared__ double red[TRS_ROWS * TRS_PITCH];
    const TrainArgs& q = a.t;
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y, K = q.K;
    const int64_t ntiles = (q.nM + WAVE - 1) / WAVE;
    const int nrx = R == 1 ? 1 : (int)a.nRx;                 // 1 <= nRx <= R
    const int rr = lane >> 1, rh = lane & 1;
    const int rslot = rr / (2 * R), rq = rr % (2 * R);       // tile row rr = record slot rslot, quantity rq = 2 c + ri
    const bool stored = rh == 0 && rq < 2 * nrx;
    double* wdst = a.work + ((w * a.N + n) * 2 * nrx + (stored ? rq : 0)) * K + rslot;
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    const int64_t ck_pitch = q.rows * 3;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.P) {
        // lanes past nM work on a copy of the last spin and receive with weight zero: their products are exact zeros
        const int64_t s_ = tile * WAVE + lane;
        const bool valid = s_ < q.nM;
        const int64_t sidx = valid ? s_ : q.nM - 1, r = n * q.nM + sidx;
        const TrainSpin v = train_spin<T>(q, n, sidx);
        const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
        const T* pb = reinterpret_cast<const T*>(q.B) + r * 3;
        const double a0 = double(pa[0]), a1 = double(pa[1]), a2 = double(pa[2]), a3 = double(pa[3]), a4 = double(pa[4]),
                     a5 = double(pa[5]), a6 = double(pa[6]), a7 = double(pa[7]), a8 = double(pa[8]);
        const double b0 = double(pb[0]), b1 = double(pb[1]), b2 = double(pb[2]);
        double rxr[R], rxi[R];
        {
            const T* pr = reinterpret_cast<const T*>(a.rx) + r * 2 * nrx;   // (from a null rx: formed, never dereferenced)
#pragma unroll
            for (int c = 0; c < R; ++c) {
                rxr[c] = R == 1 && valid ? 1.0 : 0.0; rxi[c] = 0.0;
                if (a.rx && c < nrx && valid) { rxr[c] = double(pr[c]); rxi[c] = double(pr[nrx + c]); }
            }
        }
        double* ckp = a.ck ? a.ck + r * 3 : nullptr;
        int64_t ck_next = 0, jbase = 0;                      // jbase: records of this spin tile already reduced
        int cnt = 0;                                         // records in the tile (wave-uniform)
        // reduce the cnt records of the tile into the workspace elements of records jbase .. jbase + cnt - 1 (rows past
        // cnt hold stale numbers: summed, never stored).  The old workspace value is requested before the row sums.
        auto flush = [&]() {
            const bool mine = stored && rslot < cnt;
            double old = 0.0;
            if (!first && mine) old = wdst[jbase];
            __syncthreads();
            const double p = trs_row_sum(red, rr, rh);
            if (mine) wdst[jbase] = old + p;
            __syncthreads();
            jbase += cnt; cnt = 0;
        };
        double mx = v.m0, my = v.m1, mz = v.m2;
        for (int64_t k = 0; k < K; ++k) {
            if (ckp && k == ck_next) {                       // wave-uniform
                if (valid) { ckp[0] = mx; ckp[1] = my; ckp[2] = mz; }
                ckp += ck_pitch; ck_next += TRS_SEG;
            }
            double cp = 1.0, sp = 0.0;
            if (cs) { cp = cs[2 * k]; sp = cs[2 * k + 1]; }
            train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, b0, b1, b2, cp, sp, mx, my, mz);
#pragma unroll
            for (int c = 0; c < R; ++c) {
                double s0, s1;
                trs_products(rxr[c], rxi[c], mx, my, s0, s1);
                red[(cnt * 2 * R + 2 * c) * TRS_PITCH + lane] = s0;
                red[(cnt * 2 * R + 2 * c + 1) * TRS_PITCH + lane] = s1;
            }
            if (++cnt == RC) flush();
        }
        if (cnt > 0) flush();
        if (valid && a.Mlast) {
            T* o = reinterpret_cast<T*>(a.Mlast) + r * 3;
            o[0] = T(mx); o[1] = T(my); o[2] = T(mz);
        }
        first = false;
    }
}

template <typename T, int R>
__global__ __launch_bounds__(WAVE) void k_train_signal_bwd(TrainSigArgs a)
{
    constexpr int S = TRS_SEG;
    static_assert(S <= WAVE / 2, "two lanes per tile row");
    __shared__ double red[S * TRS_PITCH];
    const TrainArgs& q = a.t;
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y, K = q.K;
    const int64_t ntiles = (q.nM + WAVE - 1) / WAVE;
    const int nrx = R == 1 ? 1 : (int)a.nRx;
    const int rr = lane >> 1, rh = lane & 1;                 // tile row rr = repetition k0 + rr of the segment
    const bool stored = rh == 0 && rr < S;
    const bool wantphi = a.work != nullptr;
    double* wdst = a.work + (w * a.N + n) * K + rr;
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    const TrainCP gs = (TrainCP)(a.gs ? a.gs + n * K * 2 * nrx : nullptr);
    const int64_t ck_pitch = q.rows * 3;
    const bool relax = q.rest && q.T1.p, prec = q.rest && q.df.p;
    const int64_t nseg = (K + S - 1) / S;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.P) {
        const int64_t s_ = tile * WAVE + lane;
        const bool valid = s_ < q.nM;
        const int64_t sidx = valid ? s_ : q.nM - 1, r = n * q.nM + sidx;
        const TrainSpin v = train_spin<T>(q, n, sidx);
        const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
        const T* pb = reinterpret_cast<const T*>(q.B) + r * 3;
        const double a0 = double(pa[0]), a1 = double(pa[1]), a2 = double(pa[2]), a3 = double(pa[3]), a4 = double(pa[4]),
                     a5 = double(pa[5]), a6 = double(pa[6]), a7 = double(pa[7]), a8 = double(pa[8]);
        const double b0 = double(pb[0]), b1 = double(pb[1]), b2 = double(pb[2]);
        T rxr[R], rxi[R];                                    // kept in the data type: converted where they are used
        {
            const T* pr = reinterpret_cast<const T*>(a.rx) + r * 2 * nrx;
#pragma unroll
            for (int c = 0; c < R; ++c) {
                rxr[c] = R == 1 ? T(1) : T(0); rxi[c] = T(0);
                if (a.rx && c < nrx) { rxr[c] = pr[c]; rxi[c] = pr[nrx + c]; }
            }
        }
        double grr[R], gri[R];
#pragma unroll
        for (int c = 0; c < R; ++c) { grr[c] = 0.0; gri[c] = 0.0; }
        double gA0 = 0, gA1 = 0, gA2 = 0, gA3 = 0, gA4 = 0, gA5 = 0, gA6 = 0, gA7 = 0, gA8 = 0;
        double gB0 = 0, gB1 = 0, gB2 = 0;
        double sphi = 0, sa1 = 0, sa2 = 0;         // sums of dL/dphi_rest, dL/da1, dL/da2 (a_i = -rest / T_i)
        double hx = 0, hy = 0, hz = 0;
        if (a.gMl) {
            const T* pg = reinterpret_cast<const T*>(a.gMl) + r * 3;
            hx = double(pg[0]); hy = double(pg[1]); hz = double(pg[2]);
        }

        for (int64_t j = nseg - 1; j >= 0; --j) {
            const int64_t k0 = j * S;
            // the segment's states: st[i] = M_{k0 + i}, recomputed from the checkpoint M_{k0}
            double sx[S + 1], sy[S + 1], sz[S + 1];
            {
                const double* pc = a.ck + j * ck_pitch + r * 3;
                sx[0] = pc[0]; sy[0] = pc[1]; sz[0] = pc[2];
            }
#pragma unroll
            for (int i = 0; i < S; ++i) {
                double x = sx[i], y = sy[i], z = sz[i];
                if (k0 + i < K) {                            // wave-uniform: the tail segment
                    double cp = 1.0, sp = 0.0;
                    if (cs) { cp = cs[2 * (k0 + i)]; sp = cs[2 * (k0 + i) + 1]; }
                    train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, b0, b1, b2, cp, sp, x, y, z);
                }
                sx[i + 1] = x; sy[i + 1] = y; sz[i + 1] = z;
            }
#pragma unroll
            for (int i = S - 1; i >= 0; --i) {
                if (k0 + i < K) {
                    const int64_t k = k0 + i;
                    const double cx = sx[i + 1], cy = sy[i + 1];                             // M_{k+1}
                    const double px_ = sx[i], py_ = sy[i], pz_ = sz[i];                      // M_k
                    double gx = 0.0, gy = 0.0;
                    if (gs) {
#pragma unroll
                        for (int c = 0; c < R; ++c) {
                            if (c < nrx) {
                                const double g0 = gs[(k * nrx + c) * 2], g1 = gs[(k * nrx + c) * 2 + 1];
                                const double wr = double(rxr[c]), wi = double(rxi[c]);
                                gx += wr * g0 + wi * g1; gy += wr * g1 - wi * g0;
                                grr[c] += g0 * cx + g1 * cy; gri[c] += g1 * cx - g0 * cy;
                            }
                        }
                    }
                    double cp = 1.0, sp = 0.0;
                    if (cs) { cp = cs[2 * k]; sp = cs[2 * k + 1]; }
                    const double lx = hx + gx, ly = hy + gy, lz = hz;                            // lambda
                    const double ux = cp * lx + sp * ly, uy = cp * ly - sp * lx, uz = lz;        // u = Rz(-phi) lambda
                    const double rx = v.c * px_ - v.s * py_, ry = v.s * px_ + v.c * py_;         // M_k rotated, before relaxation
                    const double mmx = rx * v.e2, mmy = ry * v.e2, mmz = pz_ * v.e1 + v.f3;      // M- = F M_k + f
                    const double qx = cp * mmx + sp * mmy, qy = cp * mmy - sp * mmx, qz = mmz;   // p = Rz(-phi) M-
                    gB0 += ux; gB1 += uy; gB2 += uz;
                    gA0 += ux * qx; gA1 += ux * qy; gA2 += ux * qz;
                    gA3 += uy * qx; gA4 += uy * qy; gA5 += uy * qz;
                    gA6 += uz * qx; gA7 += uz * qy; gA8 += uz * qz;
                    const double wx = a0 * ux + a3 * uy + a6 * uz;                               // A^T u
                    const double wy = a1 * ux + a4 * uy + a7 * uz;
                    const double wz = a2 * ux + a5 * uy + a8 * uz;
                    const double mx = cp * wx - sp * wy, my = sp * wx + cp * wy, mz = wz;        // gM- = Rz(phi) A^T u
                    if (wantphi) red[i * TRS_PITCH + lane] = valid ? (ly * cx - lx * cy) - (my * mmx - mx * mmy) : 0.0;
                    // k_freeprec_gc's formulas with (x, y, z) = M_k and the cotangent gM-
                    sphi += prec ? v.e2 * (my * rx - mx * ry) : 0.0;
                    sa2 += relax ? (mx * rx + my * ry) * v.e2 : 0.0;
                    sa1 += relax ? mz * (pz_ - 1.0) * v.e1 : 0.0;
                    // h = F^T gM-
                    hx = v.e2 * (v.c * mx + v.s * my); hy = v.e2 * (v.c * my - v.s * mx); hz = v.e1 * mz;
                }
            }
            if (wantphi) {                                   // rows of repetitions past K hold stale numbers: never stored
                const bool mine = stored && k0 + rr < K;
                double old = 0.0;
                if (!first && mine) old = wdst[k0];
                __syncthreads();
                const double p = rr < S ? trs_row_sum(red, rr, rh) : 0.0;
                if (mine) wdst[k0] = old + p;
                __syncthreads();
            }
        }
        if (valid) {
            if (q.gB) {
                T* o = reinterpret_cast<T*>(q.gB) + r * 3;
                o[0] = T(gB0); o[1] = T(gB1); o[2] = T(gB2);
            }
            if (q.gA) {
                T* o = reinterpret_cast<T*>(q.gA) + r * 9;
                o[0] = T(gA0); o[1] = T(gA1); o[2] = T(gA2); o[3] = T(gA3); o[4] = T(gA4); o[5] = T(gA5);
                o[6] = T(gA6); o[7] = T(gA7); o[8] = T(gA8);
            }
            if (q.gC) {
                const double twopi = 6.283185307179586476925;
                // fp64 whatever the data type: an operand shared by the spins (rest; a broadcast T1, T2, df) gets the sum
                // of these over the spins, which the caller forms in fp64 and rounds once
                double* o = reinterpret_cast<double*>(q.gC) + r * 4;
                o[0] = -twopi * v.df * sphi - sa1 / v.t1 - sa2 / v.t2;
                o[1] = sa1 * v.rest / (v.t1 * v.t1);
                o[2] = sa2 * v.rest / (v.t2 * v.t2);
                o[3] = -twopi * v.rest * sphi;
            }
            if (q.gMi) {
                T* o = reinterpret_cast<T*>(q.gMi) + r * 3;
                o[0] = T(hx); o[1] = T(hy); o[2] = T(hz);
            }
            if (a.grx) {
                T* o = reinterpret_cast<T*>(a.grx) + r * 2 * nrx;
#pragma unroll
                for (int c = 0; c < R; ++c)
                    if (c < nrx) { o[c] = T(grr[c]); o[nrx + c] = T(gri[c]); }
            }
        }
        first = false;
    }
}

// Pass 2: sum the P workspace rows (P, N, nQ, K) per (n, quantity, k) in a fixed order and round once into the data
// type.  Block = 16 repetitions x 16 row groups (group g takes rows g, g + 16, ...: 128-B coalesced reads per row),
// the sixteen partial sums combined through LDS in group order.  nRx > 0: quantity q = 2 c + ri goes to
// sig (N, 2, K, nRx); nRx == 0 (nQ == 1): to out (N, K).
constexpr int TP2_K = 16, TP2_G = 16;
template <typename T>
__global__ __launch_bounds__(TP2_K * TP2_G) void k_train_signal_p2(const double* work, T* out, int64_t N, int64_t nQ,
                                                                   int64_t K, int64_t P, int64_t nRx)
{
    __shared__ double part[TP2_G][TP2_K];
    const int kl = threadIdx.x % TP2_K, g = threadIdx.x / TP2_K;
    const int64_t k = (int64_t)blockIdx.x * TP2_K + kl;
    const int64_t qn = blockIdx.y, n = blockIdx.z;
    double acc = 0.0;
    if (k < K)
        for (int64_t w = g; w < P; w += TP2_G) acc += work[((w * N + n) * nQ + qn) * K + k];
    part[g][kl] = acc;
    __syncthreads();
    if (g != 0 || k >= K) return;
    double sum = part[0][kl];
#pragma unroll
    for (int i = 1; i < TP2_G; ++i) sum += part[i][kl];
    if (nRx > 0) out[((n * 2 + (qn & 1)) * K + k) * nRx + (qn >> 1)] = T(sum);
    else         out[n * K + k] = T(sum);
}

// Host: what the entry points of Ktrs / Ktrsb and of Ksqs / Ksqsb (tu_sequence_signal.hip) share.
// the coil capacity a launch with nRx coils runs at
inline int trs_capacity(int64_t nRx) { return nRx <= 1 ? 1 : (nRx <= 2 ? 2 : (nRx <= 4 ? 4 : 8)); }

// f(std::integral_constant<int, R>) for the capacity R = cap of a launch: the kernels take it as a template argument
template <typename F>
void trs_at_capacity(int cap, F f)
{
    switch (cap) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

// what they check after train_check / seq_check: the coil count, the receive map and the workspace of the sums
inline int trs_signal_check(int dtype, const void* rx, int64_t nRx, const void* work, size_t work_bytes, size_t need)
{
    if (nRx < 1 || nRx > trs_max_rx(tsize(dtype)) || (!rx && nRx != 1)) return MRPHY_EINVAL;
    if (!aligned_to(rx, tsize(dtype)) || !aligned_to(work, sizeof(double))) return MRPHY_EALIGN;
    if (need && (!work || work_bytes < need)) return work ? MRPHY_ENOSPC : MRPHY_EINVAL;
    return 0;
}

// the sums of quantity qn of the workspace (Pw, N, nQ, K) into out: sig (N, 2, K, nRx) for nRx > 0 (all nQ = 2 nRx
// quantities in one launch), else one quantity into out (N, K)
template <typename T>
int trs_launch_p2(const double* work, T* out, int64_t N, int64_t nQ, int64_t qn, int64_t K, int64_t Pw, int64_t nRx,
                  hipStream_t st)
{
    const unsigned gy = nRx > 0 ? (unsigned)nQ : 1u;
    hipLaunchKernelGGL((k_train_signal_p2<T>), dim3((unsigned)((K + TP2_K - 1) / TP2_K), gy, (unsigned)N),
                       dim3(TP2_K * TP2_G), 0, st, work + qn * K, out, N, nQ, K, Pw, nRx);
    return launch_status();
}

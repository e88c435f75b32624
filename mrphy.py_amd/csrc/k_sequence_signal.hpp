// k_sequence_signal.hpp -- the signal of a scheduled sequence: Ksq's repetition (a pulse of a bank and a rest per
// repetition) inside Ktrs's frame (the transverse magnetisation summed over the spins per repetition, for one receive
// coil or an array of them), and its adjoint (Ksqs / Ksqsb)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp, k_ab_train.hpp (TrainSpin,
// TrainCP), k_train_signal.hpp (train_rep, trs_products, trs_row_sum, TRS_PITCH, k_train_signal_p2) and
// k_ab_sequence.hpp (SeqArgs, SeqIP, seq_spin, seq_rest, seq_load_a, k_ab_sequence_p2).  Not a standalone header.
#pragma once

// =============================================================================================
// Ksqs: Ktrs's frame -- one block = one wave = 64 spins of ONE batch entry (blockIdx.y = n), persistent over the spin
// tiles w, w + Pw, ..., coil capacity R = 1, 2, 4, 8, the products of a repetition through an LDS tile of TRS_ROWS x
// TRS_PITCH doubles, the tile's rows summed in one fixed order into the wave's OWN workspace row (Pw, N, 2 nRx, K) fp64,
// k_train_signal_p2 rounding once into sig (N, 2, K, nRx) -- around Ksq's repetition: the int32 pulse (K,), the fp64
// cs (N|1, K, 2) and rs (N|1, K) through scalar loads, A_p, B_p reloaded when pulse_k changes, the rest's constants
// re-formed (seq_rest) when the BITS of rs_k change, both block-uniform, then train_rep and trs_products.  The state has
// Ksq's bits (and so Ktr's without a schedule), a coil's terms Ktrs's.  With a checkpoint pointer the fp64 state BEFORE
// repetitions 0, S, 2S, ... (S = TRS_SEG) is written time-major, ck (ceil(K/S), rows, 3); Mlast is the last record.
// Lanes past nM work on a copy of the last spin and receive with weight zero.
//
// Ksqsb: Ktrsb's sweep per segment of S repetitions from the last to the first, with Ksqb's two refreshes, its flush of
// the 12 accumulators into the bank workspace and a grad_rest per repetition.  Where Ktrsb keeps the segment's states
// M_k0 .. M_k0+S in register arrays and unrolls both loops (which would inline seq_rest's sincos / exp / expm1 sixteen
// times), the states live in LDS here, (S + 1) x 3 x 64 doubles, element (i, c) of the 64 lanes contiguous -- each lane
// reads what it wrote, no barrier, no bank conflict -- and both loops stay rolled: seq_rest appears twice.
//   - The recompute of a segment starts from its checkpoint with A_p, B_p of its first repetition loaded
//     unconditionally (B is dead during the walk), and reloads on a change; the walk reloads A alone.  `pload` is the
//     entry whose A is in registers, `pacc` the entry the 12 accumulators belong to: they are added into the lane's own
//     slots of the fp64 workspace bank (P, 12, rows) only when a WALKED repetition plays another entry, and once at the
//     end.  The entry point clears the workspace; k_ab_sequence_p2 rounds it once and writes the zeros of entries never
//     played.
//   - Lanes past nM sit on a copy of the last spin: they put zeros into the tile and touch neither the bank workspace
//     nor grad_consts, grad_Mi, grad_rx -- a flush from them would be several lanes read-modify-writing one slot.
//   - dL/dphi_k and dL/drest_k are summed over the spins here: tile row i (phase) and row S + i (rest) per repetition of
//     the segment, 2 S = 16 rows <= 32, reduced by trs_row_sum and accumulated into the wave's workspace row
//     sums (Pw, N, nQ, K), nQ = the number of the two that are wanted; k_train_signal_p2 gives (N, K) each in fp64.
//   - grad_consts (rows, 3) = Ksqb's [ sum_k da1_k rest_k / T1^2, sum_k da2_k rest_k / T2^2, -2 pi sum_k rest_k dphi_k ],
//     in fp64 whatever the data type, as Ktrsb hands its constants over.
//   - grad_rx lane-private, grad_Mi, the cotangent of Mlast as the initial h and the table gs (N, K, nRx, 2) fp64
//     through scalar loads: as Ktrsb.
// No float atomics; every sum runs in a fixed order; the same inputs give the same bits.
// =============================================================================================
struct SeqSigArgs {
    SeqArgs s;                      // A .. cs, gMi, rows, nM, K as Ksq / Ksqb take them; gC (rows, 3) is fp64 here;
                                    // work = the bank's (P, 12, rows), null: neither grad_A nor grad_B;
                                    // g, Mt, grest, gphi unused
    const void* rx; int64_t nRx;    // (rows, 2, nRx); R = 1 only: or null = (1, 0)
    void* Mlast;                    // (rows, 3): the last record (forward; may be null)
    double* ck;                     // (ceil(K/S), rows, 3) fp64: written by the forward (null: not wanted), read by the adjoint
    double* sums;                   // forward: (Pw, N, 2 nRx, K); adjoint: (Pw, N, nQ, K), null = neither phase nor rest
    int32_t qphi, qrest, nQ;        // adjoint: the quantity index of the phase / rest row in sums, -1 = not wanted
    const double* gs;               // adjoint: (N, K, nRx, 2) fp64, the cotangent of sig; null: none
    const void* gMl;                // adjoint: (rows, 3), the cotangent of Mlast; null: none
    void* grx;                      // adjoint: (rows, 2, nRx); may be null
    int64_t N, Pw;
};

template <typename T, int R>
__global__ __launch_bounds__(WAVE) void k_sequence_signal_fwd(SeqSigArgs a)
{
    constexpr int RC = TRS_ROWS / (2 * R);                    // records per tile
    static_assert(TRS_ROWS == WAVE / 2 && TRS_ROWS % (2 * R) == 0, "two lanes per tile row, whole records per tile");
    __shared__ double red[TRS_ROWS * TRS_PITCH];
    const SeqArgs& q = a.s;
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y, K = q.K;
    const int64_t ntiles = (q.nM + WAVE - 1) / WAVE;
    const int nrx = R == 1 ? 1 : (int)a.nRx;                 // 1 <= nRx <= R
    const int rr = lane >> 1, rh = lane & 1;
    const int rslot = rr / (2 * R), rq = rr % (2 * R);       // tile row rr = record slot rslot, quantity rq = 2 c + ri
    const bool stored = rh == 0 && rq < 2 * nrx;
    double* wdst = a.sums + ((w * a.N + n) * 2 * nrx + (stored ? rq : 0)) * K + rslot;
    const bool prec = q.rs && q.df.p, relax = q.rs && q.T1.p;
    const SeqIP pl = (SeqIP)q.pulse;
    const TrainCP rs = (TrainCP)(q.rs ? q.rs + n * q.rs_sn : nullptr);
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    const int64_t ck_pitch = q.rows * 3;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.Pw) {
        // lanes past nM work on a copy of the last spin and receive with weight zero: their products are exact zeros
        const int64_t s_ = tile * WAVE + lane;
        const bool valid = s_ < q.nM;
        const int64_t sidx = valid ? s_ : q.nM - 1, r = n * q.nM + sidx;
        TrainSpin v = seq_spin<T>(q, n, sidx);
        const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
        const T* pb = reinterpret_cast<const T*>(q.B) + r * 3;
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
        // Ktrs's flush: the cnt records of the tile into the workspace elements of records jbase .. jbase + cnt - 1
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
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0, b0 = 0, b1 = 0, b2 = 0;
        int32_t pcur = -1;
        long long rbits = 0;
        double mx = v.m0, my = v.m1, mz = v.m2;
        for (int64_t k = 0; k < K; ++k) {
            if (ckp && k == ck_next) {                       // wave-uniform
                if (valid) { ckp[0] = mx; ckp[1] = my; ckp[2] = mz; }
                ckp += ck_pitch; ck_next += TRS_SEG;
            }
            const int32_t p = pl ? pl[k] : 0;
            if (p != pcur) {                                 // block-uniform
                seq_load_a(pa + (int64_t)p * q.rows * 9, a0, a1, a2, a3, a4, a5, a6, a7, a8);
                const T* b = pb + (int64_t)p * q.rows * 3;
                b0 = double(b[0]); b1 = double(b[1]); b2 = double(b[2]);
                pcur = p;
            }
            if (rs) {
                const double rk = rs[k];
                const long long bits = __double_as_longlong(rk);
                if (k == 0 || bits != rbits) { seq_rest(v, rk, prec, relax); rbits = bits; }   // block-uniform
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
__global__ __launch_bounds__(WAVE) void k_sequence_signal_bwd(SeqSigArgs a)
{
    constexpr int S = TRS_SEG;
    static_assert(2 * S <= WAVE / 2, "two lanes per tile row, a phase and a rest row per repetition");
    __shared__ double red[2 * S * TRS_PITCH];
    __shared__ double st[(S + 1) * 3 * WAVE];                 // st[(i * 3 + c) * WAVE + lane] = component c of M_{k0 + i}
    const SeqArgs& q = a.s;
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y, K = q.K;
    const int64_t ntiles = (q.nM + WAVE - 1) / WAVE;
    const int nrx = R == 1 ? 1 : (int)a.nRx;
    const int rr = lane >> 1, rh = lane & 1;                 // tile row rr: quantity rr / S of repetition k0 + rr % S
    const int ri = rr % S;
    const bool wantphi = a.qphi >= 0, wantrest = a.qrest >= 0;
    const int qrow = rr < S ? a.qphi : (rr < 2 * S ? a.qrest : -1);
    const bool stored = rh == 0 && qrow >= 0;
    double* wdst = a.sums + ((w * a.N + n) * a.nQ + (stored ? qrow : 0)) * K + ri;
    const bool prec = q.rs && q.df.p, relax = q.rs && q.T1.p;
    const SeqIP pl = (SeqIP)q.pulse;
    const TrainCP rs = (TrainCP)(q.rs ? q.rs + n * q.rs_sn : nullptr);
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    const TrainCP gs = (TrainCP)(a.gs ? a.gs + n * K * 2 * nrx : nullptr);
    const int64_t ck_pitch = q.rows * 3;
    const int64_t nseg = (K + S - 1) / S;
    const double twopi = 6.283185307179586476925;
    double* sl = st + lane;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.Pw) {
        const int64_t s_ = tile * WAVE + lane;
        const bool valid = s_ < q.nM;
        const int64_t sidx = valid ? s_ : q.nM - 1, r = n * q.nM + sidx;
        TrainSpin v = seq_spin<T>(q, n, sidx);
        const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
        const T* pb = reinterpret_cast<const T*>(q.B) + r * 3;
        double* wk = (q.work && valid) ? q.work + r : nullptr;   // lanes past nM never touch the bank workspace
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
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0;
        double gA0 = 0, gA1 = 0, gA2 = 0, gA3 = 0, gA4 = 0, gA5 = 0, gA6 = 0, gA7 = 0, gA8 = 0;
        double gB0 = 0, gB1 = 0, gB2 = 0;
        double sphi = 0, sa1 = 0, sa2 = 0;         // sums of rest_k dphi_k, rest_k da1_k, rest_k da2_k
        double hx = 0, hy = 0, hz = 0;
        if (a.gMl) {
            const T* pg = reinterpret_cast<const T*>(a.gMl) + r * 3;
            hx = double(pg[0]); hy = double(pg[1]); hz = double(pg[2]);
        }
        int32_t pload = -1, pacc = -1;             // the entry whose A is in registers; the entry the accumulators belong to
        long long rbits = 0;
        bool rok = false;                          // v holds the constants of the rest with the bits rbits

        // add the accumulators into the lane's slots of bank entry pacc and clear them
        auto flush = [&]() {
            if (wk) {
                double* o = wk + (int64_t)pacc * 12 * q.rows;
                const int64_t Rw = q.rows;
                o[0] += gA0; o[Rw] += gA1; o[2 * Rw] += gA2; o[3 * Rw] += gA3; o[4 * Rw] += gA4; o[5 * Rw] += gA5;
                o[6 * Rw] += gA6; o[7 * Rw] += gA7; o[8 * Rw] += gA8; o[9 * Rw] += gB0; o[10 * Rw] += gB1; o[11 * Rw] += gB2;
            }
            gA0 = gA1 = gA2 = gA3 = gA4 = gA5 = gA6 = gA7 = gA8 = 0.0;
            gB0 = gB1 = gB2 = 0.0;
        };

        for (int64_t j = nseg - 1; j >= 0; --j) {
            const int64_t k0 = j * S;
            const int cnt = (int)(K - k0 < S ? K - k0 : S);  // repetitions of this segment (wave-uniform)
            // the segment's states into LDS: st[i] = M_{k0 + i}, recomputed from the checkpoint M_{k0}
            {
                const double* pc = a.ck + j * ck_pitch + r * 3;
                double x = pc[0], y = pc[1], z = pc[2];
                sl[0] = x; sl[WAVE] = y; sl[2 * WAVE] = z;
                double b0, b1, b2;
                {
                    const int32_t p = pl ? pl[k0] : 0;
                    seq_load_a(pa + (int64_t)p * q.rows * 9, a0, a1, a2, a3, a4, a5, a6, a7, a8);
                    const T* b = pb + (int64_t)p * q.rows * 3;
                    b0 = double(b[0]); b1 = double(b[1]); b2 = double(b[2]);
                    pload = p;
                }
                for (int i = 0; i < cnt; ++i) {
                    const int64_t k = k0 + i;
                    const int32_t p = pl ? pl[k] : 0;
                    if (p != pload) {                        // block-uniform
                        seq_load_a(pa + (int64_t)p * q.rows * 9, a0, a1, a2, a3, a4, a5, a6, a7, a8);
                        const T* b = pb + (int64_t)p * q.rows * 3;
                        b0 = double(b[0]); b1 = double(b[1]); b2 = double(b[2]);
                        pload = p;
                    }
                    if (rs) {
                        const double rk = rs[k];
                        const long long bits = __double_as_longlong(rk);
                        if (!rok || bits != rbits) { seq_rest(v, rk, prec, relax); rbits = bits; rok = true; }
                    }
                    double cp = 1.0, sp = 0.0;
                    if (cs) { cp = cs[2 * k]; sp = cs[2 * k + 1]; }
                    train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, b0, b1, b2, cp, sp, x, y, z);
                    double* o = sl + (i + 1) * 3 * WAVE;
                    o[0] = x; o[WAVE] = y; o[2 * WAVE] = z;
                }
            }
            for (int i = cnt - 1; i >= 0; --i) {
                const int64_t k = k0 + i;
                const int32_t p = pl ? pl[k] : 0;
                if (p != pload) {                            // block-uniform; the walk needs A alone
                    seq_load_a(pa + (int64_t)p * q.rows * 9, a0, a1, a2, a3, a4, a5, a6, a7, a8);
                    pload = p;
                }
                if (p != pacc) {                             // block-uniform
                    if (pacc >= 0) flush();
                    pacc = p;
                }
                if (rs) {
                    const double rk = rs[k];
                    const long long bits = __double_as_longlong(rk);
                    if (!rok || bits != rbits) { seq_rest(v, rk, prec, relax); rbits = bits; rok = true; }
                }
                const double* m1 = sl + (i + 1) * 3 * WAVE;
                const double* m0 = sl + i * 3 * WAVE;
                const double cx = m1[0], cy = m1[WAVE];                                      // M_{k+1}
                const double px_ = m0[0], py_ = m0[WAVE], pz_ = m0[2 * WAVE];                // M_k
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
                // k_freeprec_gc's formulas with (x, y, z) = M_k and the cotangent gM-, per repetition
                const double dphi = prec ? v.e2 * (my * rx - mx * ry) : 0.0;
                const double da2 = relax ? (mx * rx + my * ry) * v.e2 : 0.0;
                const double da1 = relax ? mz * (pz_ - 1.0) * v.e1 : 0.0;
                if (wantrest)
                    red[(S + i) * TRS_PITCH + lane] = valid ? -twopi * v.df * dphi - da1 / v.t1 - da2 / v.t2 : 0.0;
                sphi += v.rest * dphi; sa1 += v.rest * da1; sa2 += v.rest * da2;
                // h = F^T gM-
                hx = v.e2 * (v.c * mx + v.s * my); hy = v.e2 * (v.c * my - v.s * mx); hz = v.e1 * mz;
            }
            if (a.sums) {                                    // rows of repetitions past K hold stale numbers: never stored
                const bool mine = stored && ri < cnt;
                double old = 0.0;
                if (!first && mine) old = wdst[k0];
                __syncthreads();
                const double p = rr < 2 * S ? trs_row_sum(red, rr, rh) : 0.0;
                if (mine) wdst[k0] = old + p;
                __syncthreads();
            }
        }
        if (pacc >= 0) flush();
        if (valid) {
            if (q.gC) {
                double* o = reinterpret_cast<double*>(q.gC) + r * 3;
                o[0] = sa1 / (v.t1 * v.t1);
                o[1] = sa2 / (v.t2 * v.t2);
                o[2] = -twopi * sphi;
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

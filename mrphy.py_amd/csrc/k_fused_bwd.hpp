// k_fused_bwd.hpp -- K2b (adjoint of the fused kernel), one transmit coil
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_bwd_common.hpp"

// MAPS (modes 0 .. 2 only; tu_fused_maps_bwd.hip): the same sweep also gives the gradients w.r.t. the lane's own
// loc, df / gamma and b1.  They are the (g0, g1, g2) = dL/dB that every step forms for grad_gr / grad_rf, summed over
// TIME instead of over the wave's spins: lane-private running sums, no LDS, no workspace, no second pass, and a fixed
// order of summation.  Two levels: the 16 steps of a segment go into partials that start at zero (steps descending),
// the partials into the running sums once per segment (segments descending) -- the sequential sum's rounding error then
// grows with 16 + nT / 16 terms, not nT.  Lanes past nM carry a zero cotangent, so their sums are exact zeros; their
// stores are guarded by `valid`.  Everything the MAPS = false build computes is computed by the same expressions.
//
// CONSTS (tu_fused_consts_bwd.hip: modes 0 .. 2; tu_signal_consts*_bwd.hip: the signal modes 3 .. 6, i.e. the capacities
// 1, 2, 4 and 8 -- every capacity K2bs has): the same sweep also gives the gradients w.r.t. the lane's own step
// constants, gC = [dL/dg, dL/dE1, dL/dE2, dL/dE1m1] (g = gamma 2 pi dt), by the arithmetic of K3's GC builds
// (bloch_math.hpp: adj_const_accumulate, adj_const_finish): lane-private sums over time in the two levels of the map
// sums, no LDS, no workspace, no second pass.  In modes 0 .. 2 the CONSTS build forms the MAPS sums as well, each of
// gloc, gBz, gb1, gC optional: one launch serves any mix of per-spin gradients, and the map outputs are the MAPS
// build's bits.  The signal modes have CONSTS without MAPS.
template <typename T, typename CT, bool RELAX, bool HB1, int INJ, bool MAPS = false, bool CONSTS = false>
__global__ __launch_bounds__(WAVE) void k_bloch_rfgr_bwd(FusedBwdKArgsT<T, INJ, MAPS, CONSTS> a)
{
    static_assert(!MAPS || INJ < 3, "the map gradients are built for the plain and the trajectory modes");
    static_assert(!(MAPS && CONSTS), "the CONSTS build of modes 0 .. 2 forms the map sums itself");
    constexpr bool MSUM = MAPS || (CONSTS && INJ < 3);      // the sums over time of dL/dB
    __shared__ __attribute__((aligned(16))) T red[5 * SEG * RED_PITCH];
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y;
    const int64_t nT = a.nT, rows = a.N * a.nM;
    const int64_t ntiles = (a.nM + WAVE - 1) / WAVE;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    using CP = typename PulseCP<T>::CP;
    T* wsrow = a.work + ((w * a.N + n) * 5) * nT;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.P) {
        bool valid;
        const int64_t s = lane_spin(tile, lane, a.nM, valid);
        const int64_t row = n * a.nM + s;
        const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
        const Spin<T> sp = load_spin<T>(a.in, n, s, row);
        T br, bi;
        load_b1<HB1>(a.in.b1, row, br, bi);
        const T vmask = valid ? T(1) : T(0);
        // lanes past nM (they hold a copy of the last valid spin) start from a zero cotangent: the adjoint state and every
        // dL/dB they form stay exact zeros (all of it is linear in the state), so they add nothing to the row sums --
        // round 6: masked here, once per tile, instead of three multiplications per step
        // grad_Mo; in the trajectory builds grad_Mt, whose last record is Mo
        const T* gM = a.gMo;
        if constexpr (INJ == 1 || INJ == 2) gM += (a.nRec - 1) * rows * 3;
        T hx = T(0), hy = T(0), hz = T(0);
        if (INJ < 3 || gM) { hx = gM[row * 3] * vmask; hy = gM[row * 3 + 1] * vmask; hz = gM[row * 3 + 2] * vmask; }
        // trajectory: the latest record not yet injected, index jr, taken after step er (both wave-uniform)
        int64_t every = 0, jr = 0, er = 0;
        if constexpr (INJ == 1 || INJ == 2) { every = a.every; jr = a.nRec - 2; er = (a.nRec - 1) * every - 1; }
        // signal (INJ >= 3, capacity R = inj_rx_cap(INJ)): every record is injected, the last one (after step nT - 1)
        // included; the lane's R receive weights in registers (zero past nM and for the pad coils c >= nRx; no map, R = 1
        // only: (1, 0)); the cotangents gsig (N, 2, nRec, nRx), a record's nRx values contiguous, through the constant
        // address space, as the pulse
        // (declared in every mode because the sweep below reads them: one unused element each in modes 0-2, which
        // compile to the instructions they had without them)
        constexpr int R = inj_rx_cap(INJ);
        T wr[R], wi[R];
        int nrx = 1;
        CP gs0 = nullptr, gs1 = nullptr;
        if constexpr (INJ >= 3) {
            every = a.every; jr = a.nRec - 1; er = nT - 1;
            int64_t nRx = 1;                                    // 1 <= nRx <= R
            if constexpr (R > 1) nRx = a.nRx;
            nrx = (int)nRx;
            const T* q = a.rx + row * 2 * nRx;                  // (from a null rx at R = 1: formed, never dereferenced)
#pragma unroll
            for (int c = 0; c < R; ++c) {
                wr[c] = R == 1 ? vmask : T(0); wi[c] = T(0);
                if ((R > 1 || a.rx) && c < nrx) { wr[c] = q[c] * vmask; wi[c] = q[nRx + c] * vmask; }
            }
            gs0 = (CP)(a.gsig + n * 2 * a.nRec * nRx);
            gs1 = gs0 + a.nRec * nRx;
        }
        adj_begin<RELAX, T, CT>(k, hx, hy, hz);
        // MAPS: the running sums over time, reset per tile -- aZ = sum g2, aL = sum g2 gr_i, and with a b1 map
        // (aBr, aBi) = sum (g0 rf_re + g1 rf_im, g1 rf_re - g0 rf_im), the transpose of field_xy_acc's product
        // (one unused element each without MAPS, as wr / wi above)
        T aZ = T(0), aL[3] = {T(0), T(0), T(0)}, aBr = T(0), aBi = T(0);
        // CONSTS: the running sums of the constants' gradients, reset per tile likewise
        T aC[4] = {T(0), T(0), T(0), T(0)};

        auto field = [&](int64_t t, T& Bx, T& By, T& Bz) { field_1coil<HB1>(br, bi, pc, t, sp, Bx, By, Bz); };

        // (the checkpoint and the old workspace values are fetched a segment ahead: ck_before, k_fused_bwd_common.hpp)
        const int64_t nseg = nT / SEG;
        T cx = T(0), cy = T(0), cz = T(0);
        if (nseg > 0) { const T* ck = ck_before(a.Mck, nseg, rows, row); cx = ck[0]; cy = ck[1]; cz = ck[2]; }
        // rows 64..79 (the second pass of the row sums): four lanes per row, one of the four chains each
        const int r1 = WAVE + (lane >> 2);
        for (int64_t seg = nseg - 1; seg >= 0; --seg) {
            const int64_t t0 = seg * SEG;
            T mx = cx, my = cy, mz = cz;
            if (seg > 0) { const T* ck = ck_before(a.Mck, seg, rows, row); cx = ck[0]; cy = ck[1]; cz = ck[2]; }
            // the trajectory cotangents of this segment.  INJ == 2: at most one, at step ist of the segment (-1: none),
            // in registers, requested here and used in the sweep after the recompute.  INJ == 1: the lane's cotangent of
            // step st goes to the slots red[(0|1|2) SEG + st][lane] that the sweep overwrites at that very step with
            // its own contributions -- the same lane reads it just before (lane-private: no barrier; the previous
            // segment's reduction released the tile at the barrier that ended it); zero where no record is taken.
            // No LDS beyond K2b's, no registers beyond the staging loads.
            // (the staging and its injection are written out in both adjoints: shared helpers cost registers, LABNOTES)
            int ist = -1;
            T ijx = T(0), ijy = T(0), ijz = T(0);
            if constexpr (INJ == 2) {
                if (er >= t0) {
                    const T* q = a.gMo + (jr * rows + row) * 3;
                    ijx = q[0] * vmask; ijy = q[1] * vmask; ijz = q[2] * vmask;
                    ist = (int)(er - t0); --jr; er -= every;
                }
            } else if constexpr (INJ == 1) {
                T gv[SEG][3];
#pragma unroll
                for (int st = SEG - 1; st >= 0; --st) {
                    gv[st][0] = gv[st][1] = gv[st][2] = T(0);
                    if (t0 + st == er) {                            // wave-uniform
                        const T* q = a.gMo + (jr * rows + row) * 3;
                        gv[st][0] = q[0] * vmask; gv[st][1] = q[1] * vmask; gv[st][2] = q[2] * vmask;
                        --jr; er -= every;
                    }
                }
#pragma unroll
                for (int st = 0; st < SEG; ++st) {
                    red[red_idx(0 * SEG + st, lane)] = gv[st][0];
                    red[red_idx(1 * SEG + st, lane)] = gv[st][1];
                    red[red_idx(2 * SEG + st, lane)] = gv[st][2];
                }
            }
            T* dst0 = wsrow + (lane / SEG) * nT + t0 + (lane % SEG);
            T* dst1 = wsrow + (r1 / SEG) * nT + t0 + (r1 % SEG);
            T old0 = T(0), old1 = T(0);
            if (!first) { old0 = *dst0; old1 = *dst1; }
            // 1. forward recompute, keeping the state before each step
            SegStates<T> h;
            seg_recompute<RELAX>(k, t0, mx, my, mz, field, h);
            T pZ = T(0), pL[3] = {T(0), T(0), T(0)}, pBr = T(0), pBi = T(0);      // MAPS: this segment's partial sums
            T pC[4] = {T(0), T(0), T(0), T(0)};                                   // CONSTS: likewise
            // 2. adjoint sweep, contributions to LDS
#pragma unroll
            for (int sb = SEG / 4 - 1; sb >= 0; --sb) {
                T Bx[4], By[4], Bz[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) field(t0 + sb * 4 + j, Bx[j], By[j], Bz[j]);
                RotAdj<T> ra[4];
                const T S4[4] = {h.Sv[sb * 4], h.Sv[sb * 4 + 1], h.Sv[sb * 4 + 2], h.Sv[sb * 4 + 3]};
                const T C4[4] = {h.Cv[sb * 4], h.Cv[sb * 4 + 1], h.Cv[sb * 4 + 2], h.Cv[sb * 4 + 3]};
                rot_prepare_adj_given<T, CT, 4>(k, Bx, By, Bz, S4, C4, ra);
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    const int st = sb * 4 + j;
                    if constexpr (INJ == 1)
                        adj_inject<RELAX, T, CT>(k, hx, hy, hz, red[red_idx(0 * SEG + st, lane)],
                                                 red[red_idx(1 * SEG + st, lane)], red[red_idx(2 * SEG + st, lane)]);
                    else if constexpr (INJ == 2) {
                        if (st == ist) adj_inject<RELAX, T, CT>(k, hx, hy, hz, ijx, ijy, ijz);
                    } else if constexpr (INJ >= 3) {
                        if (t0 + st == er) {                            // wave-uniform
                            // the coils' cotangents summed in ascending c, then ONE injection: in the t = E h state of
                            // the precise modes the sum is scaled and rounded once
                            const CP q0 = gs0 + jr * nrx, q1 = gs1 + jr * nrx;
                            T ix = wr[0] * q0[0] + wi[0] * q1[0], iy = wr[0] * q1[0] - wi[0] * q0[0];
#pragma unroll
                            for (int c = 1; c < R; ++c)
                                if (c < nrx) {                          // wave-uniform: no load past the record's nRx
                                    const T g0 = q0[c], g1 = q1[c];
                                    ix += wr[c] * g0 + wi[c] * g1;
                                    iy += wr[c] * g1 - wi[c] * g0;
                                }
                            adj_inject<RELAX, T, CT>(k, hx, hy, hz, ix, iy, T(0));
                            er = (jr == a.nRec - 1) ? jr * every - 1 : er - every;
                            --jr;
                        }
                    }
                    T g0, g1, g2;
                    if constexpr (CONSTS)     // (the carried state as it stands after the injection above goes in)
                        rot_apply_adj_consts<RELAX, T, CT>(k, ra[j], Bx[j], By[j], Bz[j], h.M0[st], h.M1[st], h.M2[st],
                                                           hx, hy, hz, g0, g1, g2, pC);
                    else
                        rot_apply_adj<RELAX, T, CT>(k, ra[j], h.M0[st], h.M1[st], h.M2[st], hx, hy, hz, g0, g1, g2);
                    red[red_idx(0 * SEG + st, lane)] = sp.lx * g2;
                    red[red_idx(1 * SEG + st, lane)] = sp.ly * g2;
                    red[red_idx(2 * SEG + st, lane)] = sp.lz * g2;
                    red[red_idx(3 * SEG + st, lane)] = HB1 ? br * g0 + bi * g1 : g0;
                    red[red_idx(4 * SEG + st, lane)] = HB1 ? br * g1 - bi * g0 : g1;
                    if constexpr (MSUM) {
                        // the step's pulse sample: the wave-uniform scalars `field` read above
                        const int64_t t = t0 + st;
                        pZ += g2;
                        pL[0] += g2 * pc.gx[t]; pL[1] += g2 * pc.gy[t]; pL[2] += g2 * pc.gz[t];
                        if constexpr (HB1) {
                            const T rr = pc.rfr[t], ri = pc.rfi[t];
                            pBr += g0 * rr + g1 * ri;
                            pBi += g1 * rr - g0 * ri;
                        }
                    }
                }
            }
            if constexpr (CONSTS) {
#pragma unroll
                for (int i = 0; i < 4; ++i) aC[i] += pC[i];
            }
            if constexpr (MSUM) {
                aZ += pZ; aL[0] += pL[0]; aL[1] += pL[1]; aL[2] += pL[2];
                if constexpr (HB1) { aBr += pBr; aBi += pBi; }
            }
            __syncthreads();
            // 3. 80 row sums: lanes 0..63 take rows 0..63, then lane (r, j) chain j of row 64 + r
            // (the old workspace values and the checkpoint were requested a segment ago: ONE explicit wait for
            // all vector loads here, or the compiler -- which loses count of them across the loops in between --
            // puts s_waitcnt vmcnt(0) in front of EACH store below, and every store then waits for the one before)
            __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0) (gfx9 encoding; expcnt / lgkmcnt untouched)
            {                                                      // pass 0: rows 0..63, one per lane
                T p0 = T(0), p1 = T(0), p2 = T(0), p3 = T(0);      // 4 chains for ILP; fixed order
#pragma unroll
                for (int i = 0; i < WAVE; i += 4) {                // logical lanes i..i+3: one slot
                    const T* q = red + red_idx(lane, i);
                    p0 += q[0]; p1 += q[1]; p2 += q[2]; p3 += q[3];
                }
                *dst0 = old0 + ((p0 + p1) + (p2 + p3));            // old = 0 on the wave's first tile
            }
            static_assert(5 * SEG - WAVE == WAVE / 4, "second pass: 16 rows x 4 chains = one wave");
            {   // pass 1: rows 64..79.  Round 5 ran the loop above once more with 16 of the 64 lanes active (64 adds and 16
                // 16-byte reads issued for a quarter of a wave); now lane (row, j) forms chain p_j of its row -- the same
                // sixteen additions in the same order -- and the four chains meet through DPP as (p0 + p1) + (p2 + p3):
                // the same bits (x + y == y + x), a quarter of the instructions
                const int j = lane & 3;
                T p = T(0);
#pragma unroll
                for (int i = 0; i < WAVE; i += 4) p += red[red_idx(r1, i) + j];
                p += __shfl_xor(p, 1);                             // lanes 0, 1: p0 + p1;  lanes 2, 3: p2 + p3
                p += __shfl_xor(p, 2);                             // (p0 + p1) + (p2 + p3)
                if (j == 0) *dst1 = old1 + p;
            }
            __syncthreads();
        }
        adj_end<RELAX, T, CT>(k, hx, hy, hz);
        if (valid && a.gMi) { a.gMi[row * 3] = hx; a.gMi[row * 3 + 1] = hy; a.gMi[row * 3 + 2] = hz; }
        if constexpr (CONSTS) {
            adj_const_finish<T, CT>(k, aC);                 // the precise fp32 mode carried t = E h: E divided out once
            if (valid && a.gC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) a.gC[row * 4 + i] = aC[i];
            }
        }
        if constexpr (MSUM) {
            // once per spin; each output optional.  gBz is dL/d(df / gamma): the division by gamma and the folds to
            // the operands' own shapes are the host's
            if (valid && a.gloc) { a.gloc[row * 3] = aL[0]; a.gloc[row * 3 + 1] = aL[1]; a.gloc[row * 3 + 2] = aL[2]; }
            if (valid && a.gBz) a.gBz[row] = aZ;
            if constexpr (HB1)
                if (valid && a.gb1) { a.gb1[row * 2] = aBr; a.gb1[row * 2 + 1] = aBi; }
        }
        first = false;
    }
}

// Host: what a build's kernels take after the common arguments (fused_bwd_args), from the request.  The signal's records
// are counted as the trajectory's; a request without gsig leaves nRec to the plain and trajectory modes.
template <typename T>
void k2b_extra_args(FusedBwdSigArgs<T>& a, const AdjointReq& r)
{
    a.rx = (const T*)r.rx; a.gsig = (const T*)r.gsig; a.nRx = r.nRx;
    if (r.gsig) a.nRec = sig_records(r.nT, r.every);
}
template <typename T>
void k2b_extra_args(FusedBwdMapsArgs<T>& a, const AdjointReq& r)
{
    a.gloc = (T*)r.gloc; a.gBz = (T*)r.gBz; a.gb1 = (T*)r.gb1;
}
template <typename T>
void k2b_extra_args(FusedBwdConstsArgs<T>& a, const AdjointReq& r)
{
    k2b_extra_args(static_cast<FusedBwdMapsArgs<T>&>(a), r); a.gC = (T*)r.gC;
}
template <typename T>
void k2b_extra_args(FusedBwdSigConstsArgs<T>& a, const AdjointReq& r)
{
    k2b_extra_args(static_cast<FusedBwdSigArgs<T>&>(a), r); a.gC = (T*)r.gC;
}

// Host: the launcher of every unit that compiles this kernel.  The build B (internal.hpp: AdjBuild) says which kernels the
// unit instantiates: which of MAPS / CONSTS, and which modes INJ the request chooses among --
//   PLAIN         0 .. 2 as below, and 3 (the signal at a capacity of 1 receive coil) for a non-null gsig;
//   MRX           4, 5, 6: the smallest capacity 2, 4, 8 that holds nRx (abi.hip has refused nRx > sig_max_rx = 8);
//   MAPS, CONSTS  0 without gMt, else 1 for every < SEG and 2 otherwise (abi.hip has refused a gb1 without a b1 map);
//   SIG_CONSTS<R> the one mode of capacity R; 1 <= nRx <= R, a null rx at R = 1 only.
// Everything else is the same for all of them: the grid, the workspace and the second pass (fused_bwd_launch), the
// common arguments, RELAX x HB1 from the operands.
template <mrphy_i::AdjBuild B, typename T, typename CT>
int launch_k2b(const AdjointReq& r, const PulseOps& in, hipStream_t st)
{
    using mrphy_i::AdjBuild;
    constexpr int RC = B == AdjBuild::SIG_CONSTS1 ? 1 : B == AdjBuild::SIG_CONSTS2 ? 2 : B == AdjBuild::SIG_CONSTS4 ? 4 :
                       B == AdjBuild::SIG_CONSTS8 ? 8 : 0;
    constexpr bool MAPS = B == AdjBuild::MAPS, CONSTS = B == AdjBuild::CONSTS || RC > 0;
    constexpr bool SIGNAL = B == AdjBuild::PLAIN || B == AdjBuild::MRX || RC > 0;
    static_assert(SIGNAL || MAPS || CONSTS, "a build of the one-coil kernel");
    return fused_bwd_launch<T>(r, k2b_waves(r.nM), st, [&](dim3 grid) {
        // the widest argument struct of the build's kernels; each takes the part it was compiled for
        FusedBwdKArgsT<T, SIGNAL ? 3 : 0, MAPS, CONSTS> a;
        static_cast<FusedBwdTrajArgs<T>&>(a) = fused_bwd_args<T>(r, in, grid.x);
        k2b_extra_args(a, r);
        auto start = [&](auto inj) {
            constexpr int INJ = decltype(inj)::value;
            const FusedBwdKArgsT<T, INJ, MAPS, CONSTS>& ka = a;
#define MRPHY_K2B(RX_, HB_) \
    hipLaunchKernelGGL((k_bloch_rfgr_bwd<T, CT, RX_, HB_, INJ, MAPS, CONSTS>), grid, dim3(WAVE), 0, st, ka)
            if (in.b1) { if (in.E1.p) MRPHY_K2B(true, true);  else MRPHY_K2B(false, true); }
            else       { if (in.E1.p) MRPHY_K2B(true, false); else MRPHY_K2B(false, false); }   // no b1 map: Bxy = rf
#undef MRPHY_K2B
        };
        using std::integral_constant;
        if constexpr (RC > 0) {
            constexpr int INJ = RC == 1 ? 3 : RC == 2 ? 4 : RC == 4 ? 5 : 6;
            static_assert(inj_rx_cap(INJ) == RC, "capacities 1, 2, 4, 8");
            start(integral_constant<int, INJ>{});
        } else if constexpr (B == AdjBuild::MRX) {
            if (r.nRx <= 2) start(integral_constant<int, 4>{});
            else if (r.nRx <= 4) start(integral_constant<int, 5>{});
            else start(integral_constant<int, 6>{});
        } else {
            if constexpr (B == AdjBuild::PLAIN)
                if (r.gsig) return start(integral_constant<int, 3>{});
            if (!r.gMt) start(integral_constant<int, 0>{});
            else if (r.every < SEG) start(integral_constant<int, 1>{});
            else start(integral_constant<int, 2>{});
        }
    });
}

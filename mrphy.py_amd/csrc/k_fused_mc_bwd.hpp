// k_fused_mc_bwd.hpp -- K2b for parallel transmit (2..8 coils)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_bwd_common.hpp"

// =============================================================================================
// K2b for parallel transmit: nC <= K2B_MAXC coils, rf (N|1, 2, nT, nC), b1 (N, nM, 2, nC).
// Same sweep as the single-coil kernel.  The per-coil sums over the 64 spins of a tile
//     grad_rf_re[c][t] = sum_l b1r[c][l] gBx[t][l] + b1i[c][l] gBy[t][l]
//     grad_rf_im[c][t] = sum_l b1r[c][l] gBy[t][l] - b1i[c][l] gBx[t][l]
// are small dot products: the raw gBx, gBy rows of the segment (2 x 16 rows) sit in the reduction
// tile next to the three loc*gBz rows, the tile's b1 in a second LDS array (2 nC rows x 64), and
// lane (step, re|im, half of the spins) forms its dot product per coil in spin order; the two
// halves are added in fixed order.  Workspace rows per wave: [gr_x, gr_y, gr_z, (re, im) x nC].
// =============================================================================================
// (K2B_MAXC = 8; K2B_MC_MAX_WAVES = 256 * 8 -- 18 KB of LDS per wave -> 8 per CU = 2 per SIMD: geom.hpp)

// MC: coil capacity of the build (2 / 4 / 8, the smallest that holds nC).  b1 registers, the staged rf
// samples and the coefficient rows are ZERO beyond nC, so that neither the field's coil loop nor the
// reduction's has a `c < nC` test in it (round 3: with the test every coil was its own basic block -- a
// wave-uniform branch and an exposed LDS round trip per coil, twice per step in the field alone; K0 and
// K2 had been rid of that in round 2).  Adding exact zeros changes nothing (at most the sign of a zero
// sum): the recomputed states stay those of K2's forward.
template <typename T, typename CT, bool RELAX, int MC, int INJ>
__global__ __launch_bounds__(WAVE) void k_bloch_rfgr_bwd_mc(FusedBwdArgsT<T, INJ> a, int nC)
{
    constexpr int K2B_NCF = 2 * MC + 3;             // coefficient rows: b1r[c], b1i[c], loc x y z
    // NOT generic in SEG: the workspace update and the dot products below take their step from the lane as
    // `lane >> 2` (64 lanes = 16 steps x (re|im) x (half of the spins)), while raw[], srf[] and the workspace
    // rows are sized from SEG.  With any other SEG lanes 32..63 would index steps past the segment (LDS reads
    // past raw[], global stores past t0 + SEG: the round-5 SEG = 8 dev build faulted exactly there).
    static_assert(SEG * 4 == WAVE && SEG == 16,
                  "k_bloch_rfgr_bwd_mc derives the step from the lane as lane >> 2: SEG must be 16 (geom.hpp)");
    // raw dL/dB rows of one segment: [gBx | gBy | gBz][step][lane], slot-swizzled like `red`
    __shared__ __attribute__((aligned(16))) T raw[3 * SEG * RED_PITCH];
    // the tile's coefficients [b1r c0..7 | b1i c0..7 | loc x y z][lane], zero for lanes past nM
    __shared__ __attribute__((aligned(16))) T cfs[K2B_NCF * WAVE];
    __shared__ __attribute__((aligned(16))) T srf[2 * SEG * MC];             // [re|im][step][c], zero beyond nC
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y;
    const int64_t nT = a.nT, rows = a.N * a.nM;
    const int64_t ntiles = (a.nM + WAVE - 1) / WAVE;
    const int nQ = 3 + 2 * nC;
    const T* __restrict__ rfr = a.in.rf + n * a.in.rf_sn;      // [nT][nC]
    const T* __restrict__ rfi = rfr + nT * nC;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, nC);        // wave-uniform gradient samples: scalar loads
    T* wsrow = a.work + ((w * a.N + n) * nQ) * nT;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.P) {
        bool valid;
        const int64_t s = lane_spin(tile, lane, a.nM, valid);
        const int64_t row = n * a.nM + s;
        const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
        const Spin<T> sp = load_spin<T>(a.in, n, s, row);
        T br[MC], bi[MC];
#pragma unroll
        for (int c = 0; c < MC; ++c) {
            br[c] = (c < nC) ? a.in.b1[row * 2 * nC + c] : T(0);
            bi[c] = (c < nC) ? a.in.b1[row * 2 * nC + nC + c] : T(0);
        }
        const T vmask = valid ? T(1) : T(0);
        __syncthreads();                                   // previous tile's coefficients released
#pragma unroll
        for (int c = 0; c < MC; ++c) {
            cfs[c * WAVE + lane] = br[c] * vmask;
            cfs[(MC + c) * WAVE + lane] = bi[c] * vmask;
        }
        cfs[(2 * MC + 0) * WAVE + lane] = sp.lx * vmask;
        cfs[(2 * MC + 1) * WAVE + lane] = sp.ly * vmask;
        cfs[(2 * MC + 2) * WAVE + lane] = sp.lz * vmask;
        // grad_Mo; in the trajectory builds grad_Mt, whose last record is Mo
        const T* gM = a.gMo;
        if constexpr (INJ != 0) gM += (a.nRec - 1) * rows * 3;
        T hx = gM[row * 3], hy = gM[row * 3 + 1], hz = gM[row * 3 + 2];
        // trajectory: the latest record not yet injected, index jr, taken after step er (both wave-uniform)
        int64_t every = 0, jr = 0, er = 0;
        if constexpr (INJ != 0) { every = a.every; jr = a.nRec - 2; er = (a.nRec - 1) * every - 1; }
        adj_begin<RELAX, T, CT>(k, hx, hy, hz);

        int64_t tstage = 0;
        auto field = [&](int64_t t, T& Bx, T& By, T& Bz) {
            field_staged<MC>(br, bi, srf + (t - tstage) * MC, SEG * MC, pc, t, sp, Bx, By, Bz);
        };

        const int64_t nseg = nT / SEG;                      // checkpoint and workspace values are
        T cx = T(0), cy = T(0), cz = T(0);                  // fetched a segment ahead (ck_before)
        if (nseg > 0) { const T* ck = ck_before(a.Mck, nseg, rows, row); cx = ck[0]; cy = ck[1]; cz = ck[2]; }
        for (int64_t seg = nseg - 1; seg >= 0; --seg) {
            const int64_t t0 = seg * SEG;
            // the segment's rf samples (SEG * MC <= 128 floats per part) -> LDS; the barrier at the
            // end of the previous segment has released srf
            tstage = t0;
            for (int i = lane; i < SEG * MC; i += WAVE) {
                const int st_ = i / MC, c_ = i - st_ * MC;
                const bool on = c_ < nC;
                srf[i] = on ? rfr[(t0 + st_) * nC + c_] : T(0);
                srf[SEG * MC + i] = on ? rfi[(t0 + st_) * nC + c_] : T(0);
            }
            __syncthreads();
            T mx = cx, my = cy, mz = cz;
            if (seg > 0) { const T* ck = ck_before(a.Mck, seg, rows, row); cx = ck[0]; cy = ck[1]; cz = ck[2]; }
            // the trajectory cotangents of this segment.  INJ == 2: at most one, at step ist of the segment (-1: none),
            // in registers, requested here and used in the sweep after the recompute.  INJ == 1: the lane's cotangent of
            // step st goes to the slots raw[(0|1|2) SEG + st][lane] that the sweep overwrites at that very step with
            // its own contributions -- the same lane reads it just before (lane-private: no barrier; the previous
            // segment's reduction released the tile at the barrier that ended it); zero where no record is taken.
            // No LDS beyond K2b's, no registers beyond the staging loads.
            // (the staging and its injection are written out in both adjoints: shared helpers cost registers, LABNOTES)
            int ist = -1;
            T ijx = T(0), ijy = T(0), ijz = T(0);
            if constexpr (INJ == 2) {
                if (er >= t0) {
                    const T* q = a.gMo + (jr * rows + row) * 3;
                    ijx = q[0]; ijy = q[1]; ijz = q[2];
                    ist = (int)(er - t0); --jr; er -= every;
                }
            } else if constexpr (INJ == 1) {
                T gv[SEG][3];
#pragma unroll
                for (int st = SEG - 1; st >= 0; --st) {
                    gv[st][0] = gv[st][1] = gv[st][2] = T(0);
                    if (t0 + st == er) {                            // wave-uniform
                        const T* q = a.gMo + (jr * rows + row) * 3;
                        gv[st][0] = q[0]; gv[st][1] = q[1]; gv[st][2] = q[2];
                        --jr; er -= every;
                    }
                }
#pragma unroll
                for (int st = 0; st < SEG; ++st) {
                    raw[red_idx(0 * SEG + st, lane)] = gv[st][0];
                    raw[red_idx(1 * SEG + st, lane)] = gv[st][1];
                    raw[red_idx(2 * SEG + st, lane)] = gv[st][2];
                }
            }
            // old workspace values of the rows this lane updates at the end of the segment
            const int st_w = lane >> 2, ri_w = (lane >> 1) & 1;
            const bool wr_w = (lane & 1) == 0;
            T* dst0 = wsrow + (3 + ri_w) * nT + t0 + st_w;        // + 2 c nT per coil
            T* dg0 = wsrow + ri_w * nT + t0 + st_w;               // grad_gr axis ri
            T* dg2 = wsrow + 2 * nT + t0 + st_w;                  // grad_gr axis z (ri == 0 lanes)
            T old[MC], oldg0 = T(0), oldg2 = T(0);
#pragma unroll
            for (int c = 0; c < MC; ++c)
                old[c] = (!first && wr_w && c < nC) ? dst0[2 * c * nT] : T(0);
            if (!first && wr_w) { oldg0 = *dg0; if (ri_w == 0) oldg2 = *dg2; }
            SegStates<T> h;
            seg_recompute<RELAX>(k, t0, mx, my, mz, field, h);
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
                        adj_inject<RELAX, T, CT>(k, hx, hy, hz, raw[red_idx(0 * SEG + st, lane)],
                                                 raw[red_idx(1 * SEG + st, lane)], raw[red_idx(2 * SEG + st, lane)]);
                    else if constexpr (INJ == 2) {
                        if (st == ist) adj_inject<RELAX, T, CT>(k, hx, hy, hz, ijx, ijy, ijz);
                    }
                    T g0, g1, g2;
                    rot_apply_adj<RELAX, T, CT>(k, ra[j], h.M0[st], h.M1[st], h.M2[st], hx, hy, hz, g0, g1, g2);
                    raw[red_idx(0 * SEG + st, lane)] = g0;   // lanes past nM: zero coefficients
                    raw[red_idx(1 * SEG + st, lane)] = g1;
                    raw[red_idx(2 * SEG + st, lane)] = g2;
                }
            }
            __syncthreads();
            // All sums over the tile's spins are dot products of a raw row with coefficient rows:
            //   lane = (step, kind, half of the spins), kind 0: re, 1: im  -> per coil c
            //     re: b1r[c].gBx + b1i[c].gBy        im: b1r[c].gBy - b1i[c].gBx
            //   and for grad_gr lane = (step, axis i < 3, -, half), kind 2:  loc_i . gBz
            // spins outer, accumulators inner; halves added in fixed order; one load round trip
            // for the workspace update.
            {
                const int st = lane >> 2, ri = (lane >> 1) & 1, half = lane & 1;
                T acc[MC], accg[2];                 // accg: this lane's 1-2 grad_gr axes
#pragma unroll
                for (int c = 0; c < MC; ++c) acc[c] = T(0);
                accg[0] = accg[1] = T(0);
                // grad_gr: (st, ri, half) lanes take axis ri (0: x, 1: y); axis z rides on ri == 0
                const T* l0 = cfs + (2 * MC + ri) * WAVE;
                const T* l2 = cfs + (2 * MC + 2) * WAVE;
#pragma unroll 2
                for (int i = half * 32; i < half * 32 + 32; i += 4) {
                    const T* qx = raw + red_idx(0 * SEG + st, i);
                    const T* qy = raw + red_idx(1 * SEG + st, i);
                    const T* qz = raw + red_idx(2 * SEG + st, i);
                    T pp[4], qq[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        pp[u] = ri == 0 ? qx[u] : qy[u];
                        qq[u] = ri == 0 ? qy[u] : -qx[u];
                        accg[0] += l0[i + u] * qz[u];
                        accg[1] += l2[i + u] * qz[u];
                    }
#pragma unroll
                    for (int c = 0; c < MC; ++c) {
                        const T* b_r = cfs + c * WAVE + i;
                        const T* b_i = cfs + (MC + c) * WAVE + i;
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[c] += b_r[u] * pp[u] + b_i[u] * qq[u];
                    }
                }
                const bool wr = half == 0;
                // one wait for the old workspace values (requested at the start of the segment) instead of a
                // compiler-inserted s_waitcnt vmcnt(0) in front of EVERY store below -- which made each of the
                // 2 nC + 3 stores wait for the one before it: 19 store round trips per segment at 8 coils
                __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0) (gfx9 encoding; expcnt / lgkmcnt untouched)
#pragma unroll
                for (int c = 0; c < MC; ++c) {
                    const T other = __shfl_xor(acc[c], 1);
                    const T sum = half == 0 ? acc[c] + other : other + acc[c];
                    if (wr && c < nC) dst0[2 * c * nT] = old[c] + sum;   // old = 0 on the first tile
                }
                {
                    const T o0 = __shfl_xor(accg[0], 1), o2 = __shfl_xor(accg[1], 1);
                    const T s0 = half == 0 ? accg[0] + o0 : o0 + accg[0];
                    const T s2 = half == 0 ? accg[1] + o2 : o2 + accg[1];
                    if (wr) {
                        *dg0 = oldg0 + s0;
                        if (ri == 0) *dg2 = oldg2 + s2;
                    }
                }
            }
            __syncthreads();
        }
        adj_end<RELAX, T, CT>(k, hx, hy, hz);
        if (valid && a.gMi) { a.gMi[row * 3] = hx; a.gMi[row * 3 + 1] = hy; a.gMi[row * 3 + 2] = hz; }
        first = false;
    }
}

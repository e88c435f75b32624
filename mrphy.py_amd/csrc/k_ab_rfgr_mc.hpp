// k_ab_rfgr_mc.hpp -- K2ab-mc / K2abb-mc: K2ab and its adjoint K2abb under parallel transmit (2..8 coils with their b1 map)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_ab_rfgr.hpp"

// =============================================================================================
// K2ab-mc: K2ab (k_ab_rfgr.hpp) with the field of K2's coil-capacity builds (k_fused_fwd.hpp, NCM = 2 / 4 / 8): rf
// (N|1, 2, nT, nC), b1 (N, nM, 2, nC), nC <= MC.  The lane's b1 sits in 2 MC registers, the step batch's rf samples are
// staged in LDS as [re|im][step][MC], ZERO beyond nC (so the coil loop has no `c < nC` test in it), and the coil sum is
// field_staged's one ascending FMA chain -- what K0 and K2 form, so A, B are k_beff2ab(K0(.)) bit for bit and B is
// K2(Mi = 0)'s bits.  Everything else is K2ab's: one field and one rot_prepare per step for the four columns of [I | 0],
// the A columns with a zero offset, the B column with the real one and not stepped without relaxation, the checkpoints
// ABck (nCk, 4, N*nM, 3).
// =============================================================================================
template <typename T, typename CT, int MC, bool CK, bool RELAX>
__global__ __launch_bounds__(WAVE) void k_ab_rfgr_mc_fwd(AbFusedArgs<T> a, int nC)
{
    static_assert(MC == 2 || MC == 4 || MC == 8, "coil capacities: 2 / 4 / 8");
    constexpr int NS = sizeof(T) == 8 ? 4 : 8;              // steps per batch, as K2ab's
    __shared__ __attribute__((aligned(16))) T srf[2 * NS * MC];             // [re|im][j][c]
    const int lane = threadIdx.x;
    const int64_t n = blockIdx.y;
    bool valid;
    const int64_t s = lane_spin(blockIdx.x, lane, a.nM, valid);
    const int64_t row = n * a.nM + s;
    const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
    SpinConst<T, CT> kl = k;
    kl.e1m1 = typename CTr<CT>::reg(0);                     // the A columns: linear part only
    const Spin<T> sp = load_spin<T>(a.in, n, s, row);
    const T* b1 = a.in.b1 + row * 2 * nC;
    T b1r[MC], b1i[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        b1r[c] = (c < nC) ? b1[c] : T(0);
        b1i[c] = (c < nC) ? b1[nC + c] : T(0);
    }

    const int64_t nT = a.nT;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, nC);
    const int64_t rows = a.N * a.nM;
    T cx[4] = {T(1), T(0), T(0), T(0)}, cy[4] = {T(0), T(1), T(0), T(0)}, cz[4] = {T(0), T(0), T(1), T(0)};

    // rf samples of steps [tb, tb + cnt) -> LDS, as K2 stages them
    auto stage_rf = [&](int64_t tb, int cnt) {
        __syncthreads();
        for (int i = lane; i < cnt * MC; i += WAVE) {
            const int j = i / MC, c = i - j * MC;
            const bool on = c < nC;
            srf[i] = on ? pc.rfr[(tb + j) * nC + c] : T(0);
            srf[NS * MC + i] = on ? pc.rfi[(tb + j) * nC + c] : T(0);
        }
        __syncthreads();
    };
    int64_t tstage = 0;                                     // first step held in srf
    auto field = [&](int64_t t, T& Bx, T& By, T& Bz) {
        field_staged<MC>(b1r, b1i, srf + (t - tstage) * MC, NS * MC, pc, t, sp, Bx, By, Bz);
    };
    auto apply = [&](const Rot<T>& r) {
#pragma unroll
        for (int j = 0; j < 3; ++j) rot_apply<RELAX, T, CT>(kl, r, cx[j], cy[j], cz[j]);
        if constexpr (RELAX) rot_apply<RELAX, T, CT>(k, r, cx[3], cy[3], cz[3]);
    };
    int64_t ck_next = 0;
    T* ckp = CK ? a.ABck + row * 3 : nullptr;
    const int64_t ck_pitch = rows * 3;
    auto checkpoint = [&](int64_t t) {
        if (t == ck_next) {                                 // wave-uniform
            if (valid) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    T* q = ckp + j * ck_pitch;
                    q[0] = cx[j]; q[1] = cy[j]; q[2] = cz[j];
                }
            }
            ckp += 4 * ck_pitch; ck_next += a.ck_every;
        }
    };

    if (CK) __builtin_amdgcn_s_waitcnt(0x0F70);             // vmcnt(0), as K2ab (k_ab_rfgr.hpp)
    int64_t t0 = 0;
    for (; t0 + NS <= nT; t0 += NS) {
        tstage = t0; stage_rf(t0, NS);
        if (CK) checkpoint(t0);
        T Bx[NS], By[NS], Bz[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) field(t0 + j, Bx[j], By[j], Bz[j]);
        Rot<T> r[NS];
        rot_prepare<T, CT, NS>(k, Bx, By, Bz, r);
#pragma unroll
        for (int j = 0; j < NS; ++j) apply(r[j]);
    }
    if (t0 < nT) { tstage = t0; stage_rf(t0, (int)(nT - t0)); }
    for (; t0 < nT; ++t0) {                                 // nT % NS tail
        if (CK) checkpoint(t0);
        T Bx[1], By[1], Bz[1];
        field(t0, Bx[0], By[0], Bz[0]);
        Rot<T> r[1];
        rot_prepare<T, CT, 1>(k, Bx, By, Bz, r);
        apply(r[0]);
    }
    if (valid) {
        T* A = a.A + row * 9;
#pragma unroll
        for (int j = 0; j < 3; ++j) { A[j] = cx[j]; A[3 + j] = cy[j]; A[6 + j] = cz[j]; }
        a.B[row * 3] = cx[3]; a.B[row * 3 + 1] = cy[3]; a.B[row * 3 + 2] = cz[3];
    }
}

// Host: the smallest capacity 2 / 4 / 8 that holds nC, for the checkpoint and relaxation modes of the arguments.  Runs
// at nT == 0 too (A = I, B = 0).  The caller has checked 1 <= nC <= ab_mc_max_coils and a non-null b1.
template <typename T, typename CT>
int launch_k2ab_mc(const PulseOps& in, void* A, void* B, void* ABck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT,
                   int64_t nC, hipStream_t st)
{
    AbFusedArgs<T> a;
    a.in = typed<T>(in); a.A = (T*)A; a.B = (T*)B; a.ABck = (T*)ABck; a.ck_every = ck_every > 0 ? ck_every : 1;
    a.N = N; a.nM = nM; a.nT = nT;
    dim3 grid;
    int rc;
    if (!fused_grid(N * nM, (nM + WAVE - 1) / WAVE, N, grid, rc)) return rc;
#define MRPHY_K2ABMC(MC_, CK_, RX_) \
    hipLaunchKernelGGL((k_ab_rfgr_mc_fwd<T, CT, MC_, CK_, RX_>), grid, dim3(WAVE), 0, st, a, (int)nC)
#define MRPHY_K2ABMC_M(MC_)                                                                    \
    do {                                                                                       \
        if (ck) { if (rx) MRPHY_K2ABMC(MC_, true, true); else MRPHY_K2ABMC(MC_, true, false); } \
        else    { if (rx) MRPHY_K2ABMC(MC_, false, true); else MRPHY_K2ABMC(MC_, false, false); } \
    } while (0)
    const bool ck = (ABck != nullptr), rx = (in.E1.p != nullptr);
    if (nC <= 2) MRPHY_K2ABMC_M(2);
    else if (nC <= 4) MRPHY_K2ABMC_M(4);
    else if constexpr (ab_mc_max_coils(sizeof(T)) >= 8) MRPHY_K2ABMC_M(8);
    else return MRPHY_EINVAL;
#undef MRPHY_K2ABMC_M
#undef MRPHY_K2ABMC
    return launch_status();
}

// =============================================================================================
// K2abb-mc: the adjoint of K2ab-mc -- grad_A, grad_B -> grad_rf (N, 2, nT, nC), grad_gr.  K2abb's frame (k_ab_rfgr.hpp):
// persistent waves, the column loop NOT unrolled, S and C formed in column 0 and reused, the carried state rotated
// through slot 0, and the columns' dL/dB summed as ((c0 + c1) + c2) + c3 in the lane's own slots of rows 0..2 of the
// reduction tile.  That is the layout the parallel-transmit reduction of k_bloch_rfgr_bwd_mc (k_fused_mc_bwd.hpp)
// consumes, which replaces K2abb's step 4 and row sums: the tile's coefficients [b1r | b1i | loc] in LDS (zero for lanes
// past nM and coils past nC), lane (step, re|im, half of the spins) forms its dot product per coil in spin order, the
// two halves are added in a fixed order.  Workspace rows per wave: [gr_x, gr_y, gr_z, (re, im) x nC]; then the second
// pass.  No atomics: the same inputs give the same bits.
// The field is field_staged on the segment's rf samples in LDS, with the lane's b1 in 2 MC registers (capacity 8: in the
// coefficient rows, see B1LDS below), as in the forward and in k_bloch_rfgr_bwd_mc: the recomputed states are the forward's.
// The fp32 builds are bound to two waves per SIMD (K2b-mc's occupancy by LDS): a build that outgrows 256 VGPRs then
// spills, which tools/kregs.py --scratch and the suite's scratch test name, instead of halving the occupancy unseen.
// =============================================================================================
template <typename T, typename CT, bool RELAX, int MC>
__global__ __launch_bounds__(WAVE, (sizeof(T) == 4 ? 2 : 1))
void k_ab_rfgr_mc_bwd(AbFusedBwdArgs<T> a, int nC)
{
    static_assert(MC == 2 || MC == 4 || MC == 8, "coil capacities: 2 / 4 / 8");
    constexpr int NCF = 2 * MC + 3;                         // coefficient rows: b1r[c], b1i[c], loc x y z
    constexpr int NCOL = AB_COLS<RELAX>;
    // Capacity 8: K2abb's sweep is at 209-226 VGPRs in fp32, and 16 more for the lane's b1 plus the 10 old workspace values
    // held across the column loop do not fit the 256 of two waves per SIMD.  That build reads its b1 pairs from its own
    // column of the coefficient rows instead (valid lanes: b1 * 1, the same bits; lanes past nM: zeros, with a zero
    // cotangent), and requests the old workspace values after the column loop.
    constexpr bool B1LDS = MC == 8;
    using R = typename CTr<CT>::reg;
    // NOT generic in SEG, as k_bloch_rfgr_bwd_mc: the workspace update and the dot products take their step from the
    // lane as `lane >> 2` (64 lanes = 16 steps x (re|im) x (half of the spins))
    static_assert(SEG * 4 == WAVE && SEG == 16,
                  "k_ab_rfgr_mc_bwd derives the step from the lane as lane >> 2: SEG must be 16 (geom.hpp)");
    // the column-summed raw dL/dB rows of one segment: [gBx | gBy | gBz][step][lane], slot-swizzled like `red`
    __shared__ __attribute__((aligned(16))) T raw[3 * SEG * RED_PITCH];
    // the tile's coefficients [b1r c0.. | b1i c0.. | loc x y z][lane], zero for lanes past nM
    __shared__ __attribute__((aligned(16))) T cfs[NCF * WAVE];
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
        // lanes past nM start from a zero cotangent and have zero coefficients: everything they add is an exact zero
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
        T hx[4], hy[4], hz[4];                              // the carried adjoint state of column j: dL/d(column j)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            hx[j] = a.gA ? a.gA[row * 9 + j] * vmask : T(0);
            hy[j] = a.gA ? a.gA[row * 9 + 3 + j] * vmask : T(0);
            hz[j] = a.gA ? a.gA[row * 9 + 6 + j] * vmask : T(0);
        }
        hx[3] = a.gB ? a.gB[row * 3] * vmask : T(0);
        hy[3] = a.gB ? a.gB[row * 3 + 1] * vmask : T(0);
        hz[3] = a.gB ? a.gB[row * 3 + 2] * vmask : T(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) adj_begin<RELAX, T, CT>(k, hx[j], hy[j], hz[j]);

        // the checkpoints: segments descending, columns ascending, each requested one column ahead of its use (K2abb)
        const int64_t nseg = nT / SEG;
        const int64_t plane = rows * 3;
        const T* ckq = a.ABck + ((nseg - 1) * 4 * rows + row) * 3;       // (formed, not dereferenced, at nseg == 0)
        T cx = T(0), cy = T(0), cz = T(0);
        if (nseg > 0) { cx = ckq[0]; cy = ckq[1]; cz = ckq[2]; }
        for (int64_t seg = nseg - 1; seg >= 0; --seg) {
            const int64_t t0 = seg * SEG;
            // the segment's rf samples -> LDS; the barrier that ended the previous segment (or the one above) released srf
            for (int i = lane; i < SEG * MC; i += WAVE) {
                const int st_ = i / MC, c_ = i - st_ * MC;
                const bool on = c_ < nC;
                srf[i] = on ? rfr[(t0 + st_) * nC + c_] : T(0);
                srf[SEG * MC + i] = on ? rfi[(t0 + st_) * nC + c_] : T(0);
            }
            __syncthreads();
            // old workspace values of the rows this lane updates at the end of the segment
            const int st_w = lane >> 2, ri_w = (lane >> 1) & 1;
            const bool wr_w = (lane & 1) == 0;
            T* dst0 = wsrow + (3 + ri_w) * nT + t0 + st_w;        // + 2 c nT per coil
            T* dg0 = wsrow + ri_w * nT + t0 + st_w;               // grad_gr axis ri
            T* dg2 = wsrow + 2 * nT + t0 + st_w;                  // grad_gr axis z (ri == 0 lanes)
            T old[MC], oldg0 = T(0), oldg2 = T(0);
            auto load_old = [&]() {
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    old[c] = (!first && wr_w && c < nC) ? dst0[2 * c * nT] : T(0);
                if (!first && wr_w) { oldg0 = *dg0; if (ri_w == 0) oldg2 = *dg2; }
            };
            if constexpr (!B1LDS) load_old();               // a segment's worth of work ahead of their use
            SegStates<T> h;
#pragma unroll 1
            for (int j = 0; j < NCOL; ++j) {
                T mx = cx, my = cy, mz = cz;
                const bool last = j == NCOL - 1;
                ckq += last ? -(4 + NCOL - 1) * plane : plane;      // the next column; after the last: (seg - 1, 0)
                if (!last || seg > 0) { cx = ckq[0]; cy = ckq[1]; cz = ckq[2]; }
                // 1. forward recompute, keeping the state before each step; the offset acts on the B column only
                SpinConst<T, CT> kc = k;
                kc.e1m1 = j == 3 ? k.e1m1 : R(0);
                // the lane's operands of the field and of b = g B pinned per column, as in K2abb: nothing but S and C is
                // carried from one column to the next (no instruction is emitted)
                Spin<T> spc = sp;
                T brc[MC], bic[MC];
                if constexpr (!B1LDS) {
#pragma unroll
                    for (int c = 0; c < MC; ++c) {
                        brc[c] = br[c]; bic[c] = bi[c];
                        asm volatile("" : "+v"(brc[c]), "+v"(bic[c]));
                    }
                }
                asm volatile("" : "+v"(spc.lx), "+v"(spc.ly), "+v"(spc.lz), "+v"(spc.delta), "+v"(kc.g));
                auto field = [&](int64_t t, T& Bx, T& By, T& Bz) {
                    if constexpr (B1LDS) {
                        // field_staged's coil sum with the lane's b1 pairs from its own column of the coefficient rows
                        Bx = T(0); By = T(0);
                        const T* qr = srf + (t - t0) * MC;
                        const T* qi = qr + SEG * MC;
                        const T* cb = cfs + lane;
#pragma unroll
                        for (int c = 0; c < MC; ++c)
                            field_xy_fma<T>(cb[c * WAVE], cb[(MC + c) * WAVE], qr[c], qi[c], Bx, By);
                        Bz = field_z<T>(pc.gx[t], pc.gy[t], pc.gz[t], spc.lx, spc.ly, spc.lz, spc.delta);
                    } else {
                        field_staged<MC>(brc, bic, srf + (t - t0) * MC, SEG * MC, pc, t, spc, Bx, By, Bz);
                    }
                };
                if (j == 0) ab_seg_recompute<RELAX, false>(kc, t0, mx, my, mz, field, h);
                else        ab_seg_recompute<RELAX, true>(kc, t0, mx, my, mz, field, h);
                // 2. adjoint sweep of this column, 3. its dL/dB added to the columns before it
#pragma unroll
                for (int sb = SEG / 4 - 1; sb >= 0; --sb) {
                    T Bx[4], By[4], Bz[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) field(t0 + sb * 4 + q, Bx[q], By[q], Bz[q]);
                    RotAdj<T> ra[4];
                    const T S4[4] = {h.Sv[sb * 4], h.Sv[sb * 4 + 1], h.Sv[sb * 4 + 2], h.Sv[sb * 4 + 3]};
                    const T C4[4] = {h.Cv[sb * 4], h.Cv[sb * 4 + 1], h.Cv[sb * 4 + 2], h.Cv[sb * 4 + 3]};
                    rot_prepare_adj_given<T, CT, 4>(kc, Bx, By, Bz, S4, C4, ra);
#pragma unroll
                    for (int q = 3; q >= 0; --q) {
                        const int st = sb * 4 + q;
                        T g0, g1, g2;
                        rot_apply_adj<RELAX, T, CT>(kc, ra[q], h.M0[st], h.M1[st], h.M2[st], hx[0], hy[0], hz[0],
                                                    g0, g1, g2);
                        T* q0 = raw + red_idx(0 * SEG + st, lane);
                        T* q1 = raw + red_idx(1 * SEG + st, lane);
                        T* q2 = raw + red_idx(2 * SEG + st, lane);
                        if (j != 0) { g0 = *q0 + g0; g1 = *q1 + g1; g2 = *q2 + g2; }      // wave-uniform
                        *q0 = g0; *q1 = g1; *q2 = g2;
                    }
                }
                // the next column's carried state into slot 0, this one's to the back
                const T tx = hx[0], ty = hy[0], tz = hz[0];
#pragma unroll
                for (int i = 0; i + 1 < NCOL; ++i) { hx[i] = hx[i + 1]; hy[i] = hy[i + 1]; hz[i] = hz[i + 1]; }
                hx[NCOL - 1] = tx; hy[NCOL - 1] = ty; hz[NCOL - 1] = tz;
            }
            if constexpr (B1LDS) load_old();                // (the dot products below cover their latency)
            __syncthreads();
            // 4. the sums over the tile's spins: dot products of a raw row with coefficient rows, as k_bloch_rfgr_bwd_mc
            //   lane = (step, kind, half of the spins), kind 0: re, 1: im  -> per coil c
            //     re: b1r[c].gBx + b1i[c].gBy        im: b1r[c].gBy - b1i[c].gBx
            //   and for grad_gr lane = (step, axis i < 3, -, half):  loc_i . gBz
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
                // ONE wait for the old workspace values requested at the start of the segment (k_fused_mc_bwd.hpp says why)
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
        first = false;
    }
}

// Host: K2abb-mc at the capacity MC on k2b_mc_waves persistent waves per batch entry, then the second pass into
// grad_gr / grad_rf (N, 2, nT, nC).  The caller has checked nC <= MC and a non-null b1.
template <typename T, typename CT, int MC>
int launch_k2abb_mc(const void* ABck, const PulseOps& in, const void* gA, const void* gB, void* grf, void* ggr,
                    void* work, int64_t N, int64_t nM, int64_t nT, int64_t nC, hipStream_t st)
{
    dim3 grid;
    int e;
    if (!fused_grid(N * nM * nT, k2b_mc_waves(nM), N, grid, e)) return e;
    AbFusedBwdArgs<T> a;
    a.ABck = (const T*)ABck; a.in = typed<T>(in); a.gA = (const T*)gA; a.gB = (const T*)gB; a.work = (T*)work;
    a.N = N; a.nM = nM; a.nT = nT; a.P = grid.x;
    if (in.E1.p) hipLaunchKernelGGL((k_ab_rfgr_mc_bwd<T, CT, true, MC>), grid, dim3(WAVE), 0, st, a, (int)nC);
    else         hipLaunchKernelGGL((k_ab_rfgr_mc_bwd<T, CT, false, MC>), grid, dim3(WAVE), 0, st, a, (int)nC);
    e = launch_status();
    if (e || !(grf || ggr)) return e;
    return launch_p2<T>(work, ggr, 3, grf, nC, N, nT, grid.x, st);
}

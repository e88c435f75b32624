// k_fused_shim.hpp -- K2sh / K2shb: K2 and K2b (mode 0) with extra Bz field channels, one transmit coil
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_ext_fwd.hpp"

// =============================================================================================
// nS channels, each a waveform sh[k, t] (wave-uniform, read with scalar loads as the pulse is) times a map shMap[k]
// at the spin (in the lane's registers), add to the longitudinal field of a step:
//     Bz_t = gr_t . loc + df / gamma + sum_k sh[k, t] shMap[k].
// THE FIELD, DEFINED ONCE (field_shim): K2's Bz first, then one FMA per channel in ascending k.  The forward, the
// adjoint's recompute and its sweep all call field_shim, so they see the same bits; a channel whose waveform or map
// is zero adds an exact zero (Bz keeps K2's bits), and so does a channel past nS in a build of a larger capacity.
// MS: the channel capacity of the build (2 / 4 / 8, the smallest that holds nS).  The lane's maps are ZERO beyond nS,
// and the rows read for those channels are the last real channel's (finite, wave-uniform offsets formed once), so the
// channel loop has no `k < nS` test in it (k_fused_mc_bwd.hpp: with the test every channel is a basic block).
// The guarantees are those of adding exact zeros, no more: they hold for FINITE waveforms and maps (0 * inf is NaN -- and a
// channel past nS multiplies the last real channel's samples by its zero map), and up to the sign of a zero Bz
// (fma(s, 0, -0.0) is +0.0).
// Everything else in the step is K2's / K2b's, whose helpers these kernels are built on.
// =============================================================================================
template <typename T, int MS>
struct ShimCP {
    typename PulseCP<T>::CP p;                                // sh of batch entry n: [nS][nT]
    unsigned ro[MS];                                          // row offset of channel k: min(k, nS - 1) nT, which fits an
                                                              // int (abi.hip refuses anything else): half the scalar
                                                              // registers of 64-bit offsets, which the fp64 capacity-8
                                                              // adjoint does not have to spare
};

template <typename T, int MS>
__device__ __forceinline__ ShimCP<T, MS> shim_cp(const T* sh, int64_t sh_sn, int64_t n, int64_t nT, int nS)
{
    ShimCP<T, MS> c;
    c.p = (typename PulseCP<T>::CP)(sh + n * sh_sn);
#pragma unroll
    for (int k = 0; k < MS; ++k) c.ro[k] = (unsigned)(k < nS ? k : nS - 1) * (unsigned)nT;
    return c;
}

// the lane's maps: shMap (N nM, nS) contiguous; zero beyond nS
template <typename T, int MS>
__device__ __forceinline__ void load_shim_map(const T* shMap, int64_t row, int nS, T (&sm)[MS])
{
#pragma unroll
    for (int k = 0; k < MS; ++k) sm[k] = (k < nS) ? shMap[row * nS + k] : T(0);
}

// field_1coil (k_fused_common.hpp), then the channels: ONE ascending FMA chain on K2's Bz, whatever MS is
template <bool HB1, int MS, typename T>
__device__ __forceinline__ void field_shim(T br, T bi, const PulseCP<T>& p, const ShimCP<T, MS>& c, int64_t t,
                                           const Spin<T>& sp, const T (&sm)[MS], T& Bx, T& By, T& Bz)
{
    field_1coil<HB1>(br, bi, p, t, sp, Bx, By, Bz);
#pragma unroll
    for (int k = 0; k < MS; ++k) Bz = fma_(T(c.p[c.ro[k] + t]), sm[k], Bz);
}

// Steps per batch of the forward.  A batch holds (5 + MS) samples per step in scalar registers: K2's 8 steps (4 in
// fp64) up to capacity 4; at capacity 8 half of that, or the 104 sample registers of a batch alone would pass the
// scalar file (the result's bits do not depend on the batch: rot_prepare is per step)
template <typename T, int MS>
constexpr int shim_batch() { return (sizeof(T) == 8 ? 4 : 8) / (MS > 4 ? 2 : 1); }

// ---------------------------------------------------------------------------------------------
// K2sh: the forward -- the frame of k_fused_ext_fwd.hpp at the capacities MS, shim_batch steps per batch.
// ---------------------------------------------------------------------------------------------
template <typename T, int MS>
struct ShimExt {
    struct Args {
        const T* sh;  int64_t sh_sn;                         // (N|1, nS, nT), batch stride (0: shared)
        const T* shMap;  int64_t nS;                         // (N*nM, nS)
    };
    static Args args(const BzExt& x) { return {(const T*)x.sh, x.sh_sn, (const T*)x.shMap, x.nS}; }
    static constexpr int BATCH = shim_batch<T, MS>();
    struct Lane { T sm[MS]; };
    using Wave = ShimCP<T, MS>;
    struct Tau {};                                           // the channels' field needs nothing of the batch
    static __device__ __forceinline__ Lane lane(const Args& x, int64_t row)
    {
        Lane l;
        load_shim_map<T, MS>(x.shMap, row, (int)x.nS, l.sm);
        return l;
    }
    static __device__ __forceinline__ Wave wave(const Args& x, int64_t n, int64_t nT)
    {
        return shim_cp<T, MS>(x.sh, x.sh_sn, n, nT, (int)x.nS);
    }
    static __device__ __forceinline__ Tau batch(const Wave&, int64_t) { return {}; }
    static __device__ __forceinline__ Tau step(Tau, int) { return {}; }
    template <bool HB1>
    static __device__ __forceinline__ void field(T br, T bi, const PulseCP<T>& p, const Wave& c, const Lane& l, int64_t t, Tau,
                                                 const Spin<T>& sp, T& Bx, T& By, T& Bz)
    {
        field_shim<HB1, MS>(br, bi, p, c, t, sp, l.sm, Bx, By, Bz);
    }
};

// ---------------------------------------------------------------------------------------------
// K2shb: the adjoint w.r.t. Mi, rf, gr, sh.  K2b's persistent waves, checkpoints, prefetches, recompute and sweep with
// field_shim; the sums over the tile's spins in K2b-mc's layout, rows of the segment next to per-lane coefficient rows
// in LDS, every sum a dot product of the two:
//     rows  [rf_re | rf_im | gBz][step][lane]      (3 x 16 x 64, slot-swizzled as K2b's tile: red_idx)
//     coefficients [loc x y z | shMap 0..MS)[lane] (zero for lanes past nM and for channels past nS)
//     grad_gr[i][t] = sum_l loc_i[l] gBz[t][l]      grad_sh[k][t] = sum_l shMap[k][l] gBz[t][l]
// The two rf rows hold K2b's own per-lane expressions (b1r gBx + b1i gBy, b1r gBy - b1i gBx; gBx, gBy without a map)
// rather than raw gBx, gBy beside b1 coefficient rows: one transmit coil has one such pair, the tile is no larger
// for it (3 x 16 rows either way), their sums need no coefficient reads -- and they are K2b's bits by construction.
// So are grad_gr's: every sum here is formed in K2b's order, each product rounded on its own (no contraction, as
// K2b rounds it into its tile), four chains over the spins l = j mod 4 in ascending l, combined (p0 + p1) + (p2 + p3).
// Lane (step, j) = (lane >> 2, lane & 3) forms chain j of ALL the step's sums: its row reads are conflict-free by
// red_idx's swizzle (the 64 lanes of one read hit 64 different banks), its coefficient reads are 16 consecutive
// elements (the rows are stored chain-major: element l of a row at (l & 3) * 16 + (l >> 2)), the same address for the
// 16 lanes of a chain -- a broadcast.  Two butterfly adds leave the full sum in all four lanes of a step, bit for bit
// the same; lane j then updates the workspace rows 4 u + j of the capacity's order
//     [gr_x, gr_y, gr_z, sh_0 .. sh_{MS-1}, rf_re, rf_im]
// which map to the wave's workspace rows [gr_x, gr_y, gr_z, sh_0 .. sh_{nS-1}, rf_re, rf_im] of (P, N, 5 + nS, nT);
// channels past nS are not stored.  The old values are read at the start of the segment (at most ceil((5 + MS) / 4)
// per lane) and there is ONE explicit wait before the stores.  A channel's sum does not depend on the capacity.
// LDS: 12288 + (3 + MS) 256 B in fp32 -- 15104 B at capacity 8, two waves per SIMD.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct ShimBwdArgs : FusedBwdArgs<T> {                       // work: (P, N, 5 + nS, nT)
    const T* sh;  int64_t sh_sn;
    const T* shMap;  int64_t nS;
};

template <typename T, typename CT, bool RELAX, bool HB1, int MS>
__global__ __launch_bounds__(WAVE) void k_bloch_rfgr_shim_bwd(ShimBwdArgs<T> a)
{
    // NOT generic in SEG: the sums and the workspace update take their step from the lane as `lane >> 2` (64 lanes =
    // 16 steps x 4 chains) while raw[] and the workspace rows are sized from SEG.  With any other SEG lanes would index
    // steps past the segment (LDS reads past raw[], global stores past t0 + SEG), as in k_fused_mc_bwd.hpp
    static_assert(SEG * 4 == WAVE && SEG == 16,
                  "k_bloch_rfgr_shim_bwd derives the step from the lane as lane >> 2: SEG must be 16 (geom.hpp)");
    constexpr int NCF = 3 + MS;                              // coefficient rows
    constexpr int NQ = 5 + MS;                               // sums per step, in the capacity's order
    constexpr int NU = (NQ + 3) / 4;                         // of which a lane stores at most NU
    __shared__ __attribute__((aligned(16))) T raw[3 * SEG * RED_PITCH];
    __shared__ __attribute__((aligned(16))) T cfs[NCF * WAVE];
    const int lane = threadIdx.x;
    const int64_t wv = blockIdx.x, n = blockIdx.y;
    const int64_t nT = a.nT, rows = a.N * a.nM;
    const int nS = (int)a.nS;
    const int64_t ntiles = (a.nM + WAVE - 1) / WAVE;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    const ShimCP<T, MS> sc = shim_cp<T, MS>(a.sh, a.sh_sn, n, nT, nS);
    T* wsrow = a.work + ((wv * a.N + n) * (5 + nS)) * nT;
    const int st_w = lane >> 2, j_w = lane & 3;
    // the lane's workspace rows: capacity row q = 4 u + j -> row q (gr, the real channels) or q - MS + nS (rf)
    // (negative: none -- a channel past nS, or past the capacity's rows)
    int64_t wo[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int q = 4 * u + j_w;
        const bool on = q < 3 + nS || (q >= 3 + MS && q < NQ);
        wo[u] = on ? (int64_t)(q < 3 + MS ? q : q - MS + nS) * nT + st_w : -1;
    }
    const int cmine = j_w * (WAVE / 4) + st_w;               // where element `lane` of a coefficient row lives (chain-major)
    bool first = true;

    for (int64_t tile = wv; tile < ntiles; tile += a.P) {
        bool valid;
        const int64_t s = lane_spin(tile, lane, a.nM, valid);
        const int64_t row = n * a.nM + s;
        const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
        const Spin<T> sp = load_spin<T>(a.in, n, s, row);
        T sm[MS];
        load_shim_map<T, MS>(a.shMap, row, nS, sm);
        T br, bi;
        load_b1<HB1>(a.in.b1, row, br, bi);
        const T vmask = valid ? T(1) : T(0);
        // (the barrier that ended the previous tile's last segment has released the coefficients)
        cfs[0 * WAVE + cmine] = sp.lx * vmask;
        cfs[1 * WAVE + cmine] = sp.ly * vmask;
        cfs[2 * WAVE + cmine] = sp.lz * vmask;
#pragma unroll
        for (int c = 0; c < MS; ++c) cfs[(3 + c) * WAVE + cmine] = sm[c] * vmask;
        T hx = a.gMo[row * 3] * vmask, hy = a.gMo[row * 3 + 1] * vmask, hz = a.gMo[row * 3 + 2] * vmask;
        adj_begin<RELAX, T, CT>(k, hx, hy, hz);

        // (the checkpoint and the old workspace values are fetched a segment ahead: ck_before, k_fused_bwd_common.hpp)
        const int64_t nseg = nT / SEG;
        T cx = T(0), cy = T(0), cz = T(0);
        if (nseg > 0) { const T* ck = ck_before(a.Mck, nseg, rows, row); cx = ck[0]; cy = ck[1]; cz = ck[2]; }
        for (int64_t seg = nseg - 1; seg >= 0; --seg) {
            const int64_t t0 = seg * SEG;
            T mx = cx, my = cy, mz = cz;
            if (seg > 0) { const T* ck = ck_before(a.Mck, seg, rows, row); cx = ck[0]; cy = ck[1]; cz = ck[2]; }
            T old[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) old[u] = (!first && wo[u] >= 0) ? wsrow[wo[u] + t0] : T(0);
            auto field = [&](int64_t t, T& Bx, T& By, T& Bz) {
                field_shim<HB1, MS>(br, bi, pc, sc, t, sp, sm, Bx, By, Bz);
            };
            // 1. forward recompute, keeping the state before each step
            SegStates<T> h;
            seg_recompute<RELAX>(k, t0, mx, my, mz, field, h);
            // 2. adjoint sweep, the step's three rows to LDS
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
                    T g0, g1, g2;
                    rot_apply_adj<RELAX, T, CT>(k, ra[j], h.M0[st], h.M1[st], h.M2[st], hx, hy, hz, g0, g1, g2);
                    raw[red_idx(0 * SEG + st, lane)] = HB1 ? br * g0 + bi * g1 : g0;
                    raw[red_idx(1 * SEG + st, lane)] = HB1 ? br * g1 - bi * g0 : g1;
                    raw[red_idx(2 * SEG + st, lane)] = g2;   // lanes past nM: an exact zero (zero cotangent)
                }
            }
            __syncthreads();
            // 3. chain j_w of the 5 + MS sums of step st_w, in K2b's order
            {
#pragma clang fp contract(off)
                T pr = T(0), pi = T(0), pq[NCF];
#pragma unroll
                for (int c = 0; c < NCF; ++c) pq[c] = T(0);
                const T* cf = cfs + j_w * SEG;
#pragma unroll 4
                for (int i = 0; i < WAVE / 4; ++i) {
                    const int l = 4 * i + j_w;
                    pr += raw[red_idx(0 * SEG + st_w, l)];
                    pi += raw[red_idx(1 * SEG + st_w, l)];
                    const T z = raw[red_idx(2 * SEG + st_w, l)];
#pragma unroll
                    for (int c = 0; c < NCF; ++c) { const T x = cf[c * WAVE + i] * z; pq[c] += x; }
                }
                // lanes (st, 0), (st, 1): p0 + p1; (st, 2), (st, 3): p2 + p3; then (p0 + p1) + (p2 + p3) in all four
                T all[4 * NU];
#pragma unroll
                for (int c = 0; c < NCF; ++c) all[c] = pq[c];
                all[NCF] = pr; all[NCF + 1] = pi;
#pragma unroll
                for (int q = NQ; q < 4 * NU; ++q) all[q] = T(0);
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    all[q] += __shfl_xor(all[q], 1);
                    all[q] += __shfl_xor(all[q], 2);
                }
                // one wait for the old workspace values (requested at the start of the segment), not one per store
                __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0) (gfx9 encoding; expcnt / lgkmcnt untouched)
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    // the four candidates pinned in registers (no instruction): a choice among elements of `all` itself is
                    // turned into an index into it, and the array then lives in a private segment
                    T a0 = all[4 * u], a1 = all[4 * u + 1], a2 = all[4 * u + 2], a3 = all[4 * u + 3];
                    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
                    const T v = (j_w & 2) ? ((j_w & 1) ? a3 : a2) : ((j_w & 1) ? a1 : a0);
                    if (wo[u] >= 0) wsrow[wo[u] + t0] = old[u] + v;     // old = 0 on the wave's first tile
                }
            }
            __syncthreads();
        }
        adj_end<RELAX, T, CT>(k, hx, hy, hz);
        if (valid && a.gMi) { a.gMi[row * 3] = hx; a.gMi[row * 3 + 1] = hy; a.gMi[row * 3 + 2] = hz; }
        first = false;
    }
}

// The request is K2b's plain one with the lead buffer (N, 3 + nS, nT) in ggr's place; the second pass is K2b's with
// nG = 3 + nS leading quantities
template <int MS, typename T, typename CT>
int launch_k2shb(const AdjointReq& r, const PulseOps& in, hipStream_t st)
{
    return fused_bwd_launch<T>(r, k2b_waves(r.nM), st, [&](dim3 grid) {
        ShimBwdArgs<T> a;
        static_cast<FusedBwdArgs<T>&>(a) = fused_bwd_args<T>(r, in, grid.x);
        a.sh = (const T*)r.ext.sh; a.sh_sn = r.ext.sh_sn; a.shMap = (const T*)r.ext.shMap; a.nS = r.ext.nS;
#define MRPHY_K2SHB(RX_, HB_) \
    hipLaunchKernelGGL((k_bloch_rfgr_shim_bwd<T, CT, RX_, HB_, MS>), grid, dim3(WAVE), 0, st, a)
        if (in.b1) { if (in.E1.p) MRPHY_K2SHB(true, true);  else MRPHY_K2SHB(false, true); }
        else       { if (in.E1.p) MRPHY_K2SHB(true, false); else MRPHY_K2SHB(false, false); }   // no b1 map: Bxy = rf
#undef MRPHY_K2SHB
    }, 3 + (int)r.ext.nS);
}

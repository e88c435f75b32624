// k_fused_moving.hpp -- K2v / K2vb: K2 and K2b (mode 0) for spins that move at constant velocity, one transmit coil
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_ext_fwd.hpp"

// =============================================================================================
// A spin that is at loc when step 0 begins and moves by w = vel dt per step sees, during step t of a call that starts
// at step0, the gradient at its midpoint position (exact for a piecewise-constant gradient)
//     pos_t = loc + w (step0 + t + 1/2),      Bz_t = gr_t . pos_t + df / gamma;
// Bxy is K2's (a b1 map is sampled at loc).  The lane holds w next to loc and forms pos_t by ONE FMA per component in
// closed form at every step -- never a running sum -- so the forward, the adjoint's recompute and sweep, and a pulse
// chained over several calls through step0 all see the same bits, and w == 0 gives loc, i.e. K2's / K2b's bits.
// pos_t goes to field_z in loc's place; nothing else in the step differs from K2 / K2b, whose helpers these kernels are
// built on (load_consts, pulse_cp, rot_prepare / rot_apply, seg_recompute, rot_prepare_adj_given / rot_apply_adj,
// adj_begin / adj_end, red_idx, fused_bwd_launch / launch_p2).
// =============================================================================================
template <typename T> struct Motion { T wx, wy, wz; };       // vel dt: the displacement per step

template <typename T>
__device__ __forceinline__ Motion<T> load_motion(const T* vdt, int64_t row)
{
    return {vdt[row * 3], vdt[row * 3 + 1], vdt[row * 3 + 2]};
}

// step0 + t + 1/2 in the data type (wave-uniform).  Exact: the float types are called with step0 + nT < 2^23 (abi.hip
// refuses anything else), where n + 1/2 has no rounding and n fits an int; fp64 converts the 64-bit count
template <typename T>
__device__ __forceinline__ T step_mid(int64_t n)
{
    if constexpr (sizeof(T) == 4) return T((int)n) + T(0.5);
    else return T(n) + T(0.5);
}

template <typename T>
__device__ __forceinline__ void moving_pos(const Spin<T>& sp, const Motion<T>& w, T tau, T& px, T& py, T& pz)
{
    px = fma_(w.wx, tau, sp.lx); py = fma_(w.wy, tau, sp.ly); pz = fma_(w.wz, tau, sp.lz);
}

// field_1coil (k_fused_common.hpp) with the spin at its position of the step, tau = step0 + t + 1/2
template <bool HB1, typename T>
__device__ __forceinline__ void field_moving(T br, T bi, const PulseCP<T>& p, int64_t t, T tau, const Spin<T>& sp,
                                             const Motion<T>& w, T& Bx, T& By, T& Bz)
{
    Bx = T(0); By = T(0);
    if (HB1) field_xy_acc<T>(br, bi, p.rfr[t], p.rfi[t], Bx, By);
    else     { Bx = p.rfr[t]; By = p.rfi[t]; }               // no b1 map: Bxy = rf (as K0)
    T px, py, pz;
    moving_pos(sp, w, tau, px, py, pz);
    Bz = field_z<T>(p.gx[t], p.gy[t], p.gz[t], px, py, pz, sp.delta);
}

// ---------------------------------------------------------------------------------------------
// K2v: the forward -- the frame of k_fused_ext_fwd.hpp with K2's step batches (8 steps, 4 in fp64).  The batch's tau is
// converted once; the steps add their (compile-time) offset, which is exact.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct MovingExt {
    struct Args { const T* vdt;  int64_t step0; };            // (N*nM, 3); steps played before this call
    static Args args(const BzExt& x) { return {(const T*)x.vdt, x.step0}; }
    static constexpr int BATCH = sizeof(T) == 8 ? 4 : 8;     // as K2's one-coil builds
    using Lane = Motion<T>;
    using Wave = int64_t;                                    // step0
    using Tau = T;
    static __device__ __forceinline__ Lane lane(const Args& x, int64_t row) { return load_motion<T>(x.vdt, row); }
    static __device__ __forceinline__ Wave wave(const Args& x, int64_t, int64_t) { return x.step0; }
    static __device__ __forceinline__ T batch(Wave step0, int64_t t) { return step_mid<T>(step0 + t); }
    static __device__ __forceinline__ T step(T tb, int j) { return tb + T(j); }
    template <bool HB1>
    static __device__ __forceinline__ void field(T br, T bi, const PulseCP<T>& p, Wave, const Lane& w, int64_t t, T tau,
                                                 const Spin<T>& sp, T& Bx, T& By, T& Bz)
    {
        field_moving<HB1>(br, bi, p, t, tau, sp, w, Bx, By, Bz);
    }
};

// ---------------------------------------------------------------------------------------------
// K2vb: the adjoint w.r.t. Mi, rf, gr -- K2b's mode 0 (k_fused_bwd.hpp) with the moving field in the recompute and the
// sweep.  The same persistent waves (k2b_waves), checkpoints, prefetches, reduction tile (20480 B of LDS), two-pass row
// sums into the wave's own workspace row (P, N, 5, nT) and second pass; no atomics, every sum in a fixed order.  The
// three gradient rows of a step are pos_t * dL/dBz_t with pos_t re-formed by the forward's FMA; the rf rows are K2b's.
// Lanes past nM start from a zero cotangent, so everything they add is an exact zero (their pos_t is finite: they hold
// a copy of the last valid spin).
// ---------------------------------------------------------------------------------------------
template <typename T>
struct MovingBwdArgs : FusedBwdArgs<T> {
    const T* vdt;  int64_t step0;
};

template <typename T, typename CT, bool RELAX, bool HB1>
__global__ __launch_bounds__(WAVE) void k_bloch_rfgr_moving_bwd(MovingBwdArgs<T> a)
{
    __shared__ __attribute__((aligned(16))) T red[5 * SEG * RED_PITCH];
    const int lane = threadIdx.x;
    const int64_t wv = blockIdx.x, n = blockIdx.y;
    const int64_t nT = a.nT, rows = a.N * a.nM, step0 = a.step0;
    const int64_t ntiles = (a.nM + WAVE - 1) / WAVE;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    T* wsrow = a.work + ((wv * a.N + n) * 5) * nT;
    bool first = true;

    for (int64_t tile = wv; tile < ntiles; tile += a.P) {
        bool valid;
        const int64_t s = lane_spin(tile, lane, a.nM, valid);
        const int64_t row = n * a.nM + s;
        const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
        const Spin<T> sp = load_spin<T>(a.in, n, s, row);
        const Motion<T> w = load_motion<T>(a.vdt, row);
        T br, bi;
        load_b1<HB1>(a.in.b1, row, br, bi);
        const T vmask = valid ? T(1) : T(0);
        T hx = a.gMo[row * 3] * vmask, hy = a.gMo[row * 3 + 1] * vmask, hz = a.gMo[row * 3 + 2] * vmask;
        adj_begin<RELAX, T, CT>(k, hx, hy, hz);

        // (the checkpoint and the old workspace values are fetched a segment ahead: ck_before, k_fused_bwd_common.hpp)
        const int64_t nseg = nT / SEG;
        T cx = T(0), cy = T(0), cz = T(0);
        if (nseg > 0) { const T* ck = ck_before(a.Mck, nseg, rows, row); cx = ck[0]; cy = ck[1]; cz = ck[2]; }
        const int r1 = WAVE + (lane >> 2);                   // rows 64..79: four lanes per row, one chain each
        for (int64_t seg = nseg - 1; seg >= 0; --seg) {
            const int64_t t0 = seg * SEG;
            T mx = cx, my = cy, mz = cz;
            if (seg > 0) { const T* ck = ck_before(a.Mck, seg, rows, row); cx = ck[0]; cy = ck[1]; cz = ck[2]; }
            T* dst0 = wsrow + (lane / SEG) * nT + t0 + (lane % SEG);
            T* dst1 = wsrow + (r1 / SEG) * nT + t0 + (r1 % SEG);
            T old0 = T(0), old1 = T(0);
            if (!first) { old0 = *dst0; old1 = *dst1; }
            // the segment's tau, converted once; the steps add their compile-time offset (exact)
            const T tb = step_mid<T>(step0 + t0);
            // Each 4-step batch of the sweep takes tau from a copy of tb the compiler cannot see through (no instruction
            // beyond a move): otherwise it recognises the recompute's sixteen positions in the sweep and keeps all 48
            // values alive across the segment -- 260-274 VGPRs in fp32, a private segment in fp64
            T tbs = tb;
            auto field_at = [&](T base, int64_t t, T& Bx, T& By, T& Bz) {
                field_moving<HB1>(br, bi, pc, t, base + T((int)(t - t0)), sp, w, Bx, By, Bz);
            };
            auto field = [&](int64_t t, T& Bx, T& By, T& Bz) { field_at(tb, t, Bx, By, Bz); };
            // 1. forward recompute, keeping the state before each step
            SegStates<T> h;
            seg_recompute<RELAX>(k, t0, mx, my, mz, field, h);
            // 2. adjoint sweep, contributions to LDS
#pragma unroll
            for (int sb = SEG / 4 - 1; sb >= 0; --sb) {
                T Bx[4], By[4], Bz[4];
                asm volatile("" : "+v"(tbs));
#pragma unroll
                for (int j = 0; j < 4; ++j) field_at(tbs, t0 + sb * 4 + j, Bx[j], By[j], Bz[j]);
                RotAdj<T> ra[4];
                const T S4[4] = {h.Sv[sb * 4], h.Sv[sb * 4 + 1], h.Sv[sb * 4 + 2], h.Sv[sb * 4 + 3]};
                const T C4[4] = {h.Cv[sb * 4], h.Cv[sb * 4 + 1], h.Cv[sb * 4 + 2], h.Cv[sb * 4 + 3]};
                rot_prepare_adj_given<T, CT, 4>(k, Bx, By, Bz, S4, C4, ra);
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    const int st = sb * 4 + j;
                    T g0, g1, g2;
                    rot_apply_adj<RELAX, T, CT>(k, ra[j], h.M0[st], h.M1[st], h.M2[st], hx, hy, hz, g0, g1, g2);
                    T px, py, pz;
                    moving_pos(sp, w, tbs + T(st), px, py, pz);
                    red[red_idx(0 * SEG + st, lane)] = px * g2;
                    red[red_idx(1 * SEG + st, lane)] = py * g2;
                    red[red_idx(2 * SEG + st, lane)] = pz * g2;
                    red[red_idx(3 * SEG + st, lane)] = HB1 ? br * g0 + bi * g1 : g0;
                    red[red_idx(4 * SEG + st, lane)] = HB1 ? br * g1 - bi * g0 : g1;
                }
            }
            __syncthreads();
            // 3. 80 row sums, as K2b: lanes 0..63 take rows 0..63, then lane (r, j) chain j of row 64 + r; ONE explicit
            // wait for the vector loads requested a segment ago
            __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0) (gfx9 encoding; expcnt / lgkmcnt untouched)
            {
                T p0 = T(0), p1 = T(0), p2 = T(0), p3 = T(0);      // 4 chains for ILP; fixed order
#pragma unroll
                for (int i = 0; i < WAVE; i += 4) {
                    const T* q = red + red_idx(lane, i);
                    p0 += q[0]; p1 += q[1]; p2 += q[2]; p3 += q[3];
                }
                *dst0 = old0 + ((p0 + p1) + (p2 + p3));            // old = 0 on the wave's first tile
            }
            static_assert(5 * SEG - WAVE == WAVE / 4, "second pass: 16 rows x 4 chains = one wave");
            {
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
        first = false;
    }
}

template <typename T, typename CT>
int launch_k2vb(const AdjointReq& r, const PulseOps& in, hipStream_t st)
{
    return fused_bwd_launch<T>(r, k2b_waves(r.nM), st, [&](dim3 grid) {
        MovingBwdArgs<T> a;
        static_cast<FusedBwdArgs<T>&>(a) = fused_bwd_args<T>(r, in, grid.x);
        a.vdt = (const T*)r.ext.vdt; a.step0 = r.ext.step0;
#define MRPHY_K2VB(RX_, HB_) \
    hipLaunchKernelGGL((k_bloch_rfgr_moving_bwd<T, CT, RX_, HB_>), grid, dim3(WAVE), 0, st, a)
        if (in.b1) { if (in.E1.p) MRPHY_K2VB(true, true);  else MRPHY_K2VB(false, true); }
        else       { if (in.E1.p) MRPHY_K2VB(true, false); else MRPHY_K2VB(false, false); }   // no b1 map: Bxy = rf
#undef MRPHY_K2VB
    });
}

// k_fused_common.hpp -- what the fused kernels of both directions share (K2, K2s, K2b, the pTx K2b): the lane's spin,
// the pulse pointers, the field of a step, the strided store of M, the reduction tile's index, the second pass over the
// workspace rows and the host side of a launch
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once

// The lane's spin.  One block = one wave = 64 spins of ONE batch entry n; lanes past nM take a copy of the last valid
// spin (valid = false: they compute, and store nothing).
__device__ __forceinline__ int64_t lane_spin(int64_t tile, int lane, int64_t nM, bool& valid)
{
    const int64_t s_ = tile * WAVE + lane;
    valid = s_ < nM;
    return valid ? s_ : nM - 1;
}

// what the field of a step needs of the spin (its step constants come from load_consts, k_common.hpp)
template <typename T> struct Spin { T lx, ly, lz, delta; };   // loc, df / gamma

template <typename T>
__device__ __forceinline__ Spin<T> load_spin(const PulseOpsT<T>& in, int64_t n, int64_t s, int64_t row)
{
    Spin<T> p;
    p.lx = in.loc[row * 3]; p.ly = in.loc[row * 3 + 1]; p.lz = in.loc[row * 3 + 2];
    p.delta = T(0);
    if (in.df.p) p.delta = bc_load<T>(in.df, n, s) / bc_load<T>(in.gam, n, s);
    return p;
}

// HB1 (one-coil builds): the coil has a b1 map.  Without one Bxy = rf (beffective.py:147-151): the
// build then skips the complex product -- 6 of the ~50 VALU instructions of a step; with b1 = (1, 0)
// the product returns rf bit for bit anyway, so results are unchanged.  A template parameter, not a
// run-time test: a wave-uniform branch in the field assembly broke the batching of the pulse's scalar
// loads (round 1: 6.6 -> 7.2 ms).
template <bool HB1, typename T>
__device__ __forceinline__ void load_b1(const T* b1, int64_t row, T& br, T& bi)
{
    br = T(1); bi = T(0);
    if (HB1 && b1) { br = b1[row * 2]; bi = b1[row * 2 + 1]; }
}

// The pulse is read-only for the whole launch and its addresses are wave-uniform: pointers into the
// CONSTANT address space make the loads scalar (s_load, batched) whatever else the loop does.  With
// plain global pointers the checkpoint-writing build could not prove that its stores leave the pulse
// alone and fetched the samples with vector loads + v_readfirstlane (K2 with checkpoints: 0.82 ms
// where the plain build's rate gives 0.60 at 64^3 x 2048).
template <typename T>
struct PulseCP {
    using CP = const T __attribute__((address_space(4)))*;
    CP rfr, rfi;                                          // [nT][nC]
    CP gx, gy, gz;                                        // [nT]
};

template <typename T>
__device__ __forceinline__ PulseCP<T> pulse_cp(const PulseOpsT<T>& in, int64_t n, int64_t nT, int64_t nC)
{
    using CP = typename PulseCP<T>::CP;
    PulseCP<T> p;
    p.rfr = (CP)(in.rf + n * in.rf_sn);
    p.rfi = p.rfr + nT * nC;
    p.gx = (CP)(in.gr + n * in.gr_sn);
    p.gy = p.gx + nT;
    p.gz = p.gy + nT;
    return p;
}

// The field of step t on the lane's spin, assembled exactly as K0 rounds it (B first, then g*B).
// One coil: its sample through scalar loads, the lane's b1 = (br, bi)
template <bool HB1, typename T>
__device__ __forceinline__ void field_1coil(T br, T bi, const PulseCP<T>& p, int64_t t, const Spin<T>& sp,
                                            T& Bx, T& By, T& Bz)
{
    Bx = T(0); By = T(0);
    if (HB1) field_xy_acc<T>(br, bi, p.rfr[t], p.rfi[t], Bx, By);
    else     { Bx = p.rfr[t]; By = p.rfi[t]; }               // no b1 map: Bxy = rf (as K0)
    Bz = field_z<T>(p.gx[t], p.gy[t], p.gz[t], sp.lx, sp.ly, sp.lz, sp.delta);
}

// MC coils in registers: the step's rf samples staged in LDS at q[c] and q[pitch + c], read as
// broadcasts, batched: no test in the loop; the coil sum is ONE ascending FMA chain whatever MC is
template <int MC, typename T>
__device__ __forceinline__ void field_staged(const T (&b1r)[MC], const T (&b1i)[MC], const T* q, int pitch,
                                             const PulseCP<T>& p, int64_t t, const Spin<T>& sp, T& Bx, T& By, T& Bz)
{
    Bx = T(0); By = T(0);
    const T* qr = q;
    const T* qi = qr + pitch;
#pragma unroll
    for (int c = 0; c < MC; ++c) field_xy_fma<T>(b1r[c], b1i[c], qr[c], qi[c], Bx, By);
    Bz = field_z<T>(p.gx[t], p.gy[t], p.gz[t], sp.lx, sp.ly, sp.lz, sp.delta);
}

// M after step t to the running destination dst if t is the step `next` of the stride, which then moves on by
// `every` -- checkpoints and strided records alike.  `t0 % every`, `t0 / every` on 64-bit run-time values were a
// software division on the scalar unit every 8 steps (round 3: +200 scalar instructions per 16 steps in the ISA of
// the checkpoint build)
template <typename T>
__device__ __forceinline__ void ck_store(int64_t t, bool valid, T mx, T my, T mz, T*& dst, int64_t pitch,
                                         int64_t& next, int64_t every)
{
    if (t == next) {                                          // wave-uniform
        if (valid) { dst[0] = mx; dst[1] = my; dst[2] = mz; }
        dst += pitch; next += every;
    }
}

// Reduction tile of K2b (80 rows) and K2s (32 rows) x 64 lanes, NO padding (K2b: 20480 B = exactly 1/8 of a CU's
// LDS, so 8 waves = 2 per SIMD are resident; with a padded pitch of 68 it was 21760 B -> 7 per CU, SIMD load
// 2:2:2:1).  Conflict-free row reads come from an XOR swizzle of the 16-B slot index instead:
// element (row, lane) lives in slot (lane/4) ^ (row & 15).
constexpr int RED_PITCH = WAVE;
// The swizzle is a bijection of the 16 slots of a row for ANY row count, so red_idx is correct for every SEG; it
// is conflict-free for the 16-row groups of SEG = 16 it was laid out for.
__device__ __forceinline__ int red_idx(int row, int l)
{
    return row * RED_PITCH + ((((l >> 2) ^ (row & 15)) << 2) | (l & 3));
}

// Pass 2: sum the P workspace rows (P, N, nQ, nT) per (n, quantity, t) in a fixed order.  Block = 32 time points
// x 8 row groups (group g takes rows g, g+8, ...: 128-B coalesced reads per row), then the eight
// partial sums are combined through LDS in group order -- deterministic, and nT/32 * 5 blocks
// instead of nT/256 * 5 (40 blocks at nT = 2048 took 0.45 ms for 73 MB).
constexpr int P2_T = 32, P2_G = 8;
// Where the sum of quantity q goes: the first nG quantities to lead (N, nG, nT), then (re, im) per coil to
// rf (N, 2, nT, nC).  K2b: grad_gr (nG = 3) and grad_rf; K2s: no lead, sig (N, 2, nRec) as one coil's rf.  Null: not wanted.
template <typename T> struct P2Dst { T* lead; int nG; T* rf; int nC; };

template <typename T>
__global__ __launch_bounds__(P2_T * P2_G) void k_bloch_rfgr_p2(const T* work, P2Dst<T> d, int64_t N, int64_t nT, int64_t P)
{
    __shared__ T part[P2_G][P2_T];
    const int tl = threadIdx.x % P2_T, g = threadIdx.x / P2_T;
    const int64_t t = (int64_t)blockIdx.x * P2_T + tl;
    const int64_t q = blockIdx.y, n = blockIdx.z;
    const int nQ = d.nG + 2 * d.nC;
    T acc = T(0);
    if (t < nT)
        for (int64_t w = g; w < P; w += P2_G) acc += work[((w * N + n) * nQ + q) * nT + t];
    part[g][tl] = acc;
    __syncthreads();
    if (g != 0 || t >= nT) return;
    T sum = part[0][tl];
#pragma unroll
    for (int i = 1; i < P2_G; ++i) sum += part[i][tl];
    if (q < d.nG) { if (d.lead) d.lead[(n * d.nG + q) * nT + t] = sum; }
    else if (d.rf) {
        const int64_t c = (q - d.nG) / 2, ri = (q - d.nG) % 2;
        d.rf[((n * 2 + ri) * nT + t) * d.nC + c] = sum;
    }
}

template <typename T>
int launch_p2(const void* work, void* lead, int nG, void* rf, int64_t nC, int64_t N, int64_t nT, int64_t P, hipStream_t st)
{
    const P2Dst<T> d = {(T*)lead, nG, (T*)rf, (int)nC};
    hipLaunchKernelGGL((k_bloch_rfgr_p2<T>), dim3((unsigned)((nT + P2_T - 1) / P2_T), (unsigned)(nG + 2 * nC), (unsigned)N),
                       dim3(P2_T * P2_G), 0, st, (const T*)work, d, N, nT, P);
    return launch_status();
}

// Host: the grid of a fused kernel -- gx one-wave blocks per batch entry.  False: nothing to launch, and rc is what
// the launcher returns: 0 for an empty problem (`elems` == 0), MRPHY_EINVAL for more batch entries than grid.y holds.
inline bool fused_grid(int64_t elems, int64_t gx, int64_t N, dim3& grid, int& rc)
{
    rc = elems == 0 ? 0 : MRPHY_EINVAL;
    if (elems == 0 || N > 65535) return false;
    grid = dim3((unsigned)gx, (unsigned)N);
    return true;
}

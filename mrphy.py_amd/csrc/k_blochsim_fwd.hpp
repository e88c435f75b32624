// k_blochsim_fwd.hpp -- K1 (blochsim forward): chunked and line-granular kernels
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_lines.hpp"     // the Beff line mover of the line-granular kernels

// =============================================================================================
// K1: blochsim forward, materialised Beff.
// =============================================================================================
template <typename T>
struct FwdArgs {
    const T* Mi;
    const T* Beff;
    T* Mo;
    HistParts hist;        // SAVE builds: where the magnetisation before each step goes (n_parts = 0: not wanted)
    Bc g, E1, E2;
    const void* E1m1;
    int64_t rows, nM, nT;
    int vec_ok;
    unsigned per_xcd;      // line kernels: > 0 -> block b works on spin tile (b % 8) * per_xcd + b / 8
};

template <typename T, typename CT, int TC, bool SAVE>
__global__ __launch_bounds__(WAVE) void k_bloch_fwd(FwdArgs<T> a)
{
    using TL = Tile<T, TC>;
    using V = typename TL::V;
    constexpr int VE = TL::VE;
    __shared__ __attribute__((aligned(16))) T tile[TL::ELEMS];

    const int lane = threadIdx.x;
    const auto [row0, r, valid, rc, n, s] = row_id((int64_t)blockIdx.x, lane, a.rows, a.nM);
    const SpinConst<T, CT> k = load_consts<T, CT>(a.g, a.E1, a.E2, a.E1m1, n, s);

    T mx = a.Mi[rc * 3 + 0], my = a.Mi[rc * 3 + 1], mz = a.Mi[rc * 3 + 2];
    const int64_t rowlen = 3 * a.nT;
    int64_t t = 0;

    T* hp = SAVE ? hist_tile_base<T>(a.hist, (int64_t)blockIdx.x, a.nT) + lane : nullptr;
    if (a.vec_ok) {
        const int64_t nfull = a.nT / TC;
        Stage<T, TC> st;
        if (nfull > 0) st = chunk_fetch<T, TC>(a.Beff, row0, a.rows, rowlen, 0, lane);
        T* myrow = tile + lane * TL::PITCH;
        for (int64_t c = 0; c < nfull; ++c) {
            __syncthreads();                         // tile free (previous chunk consumed)
            chunk_to_lds<T, TC>(tile, st, lane);
            __syncthreads();
            if (c + 1 < nfull)                       // next chunk flies while this one integrates
                st = chunk_fetch<T, TC>(a.Beff, row0, a.rows, rowlen, (c + 1) * TC, lane);
#pragma unroll 1
            for (int tt = 0; tt < TC; tt += VE) {    // VE steps = 3 vectors = 48 B per lane
                T bb[3 * VE];
                vec_unpack(*reinterpret_cast<const V*>(myrow + tt * 3), bb);
                vec_unpack(*reinterpret_cast<const V*>(myrow + tt * 3 + VE), bb + VE);
                vec_unpack(*reinterpret_cast<const V*>(myrow + tt * 3 + 2 * VE), bb + 2 * VE);
                T gBx[VE], gBy[VE], gBz[VE];
#pragma unroll
                for (int q = 0; q < VE; ++q) { gBx[q] = bb[3 * q]; gBy[q] = bb[3 * q + 1]; gBz[q] = bb[3 * q + 2]; }
                Rot<T> rr[VE];
                rot_prepare<T, CT, VE>(k, gBx, gBy, gBz, rr);
#pragma unroll
                for (int q = 0; q < VE; ++q) {
                    if (SAVE) hist_store<T>(hp, c * TC + tt + q, mx, my, mz);
                    if (k.relax) rot_apply<true, T, CT>(k, rr[q], mx, my, mz);
                    else         rot_apply<false, T, CT>(k, rr[q], mx, my, mz);
                }
            }
        }
        t = nfull * TC;
    }
    // tail steps and the unaligned-shape path: each lane reads its own samples directly
    const T* bp = a.Beff + rc * rowlen;
    for (; t < a.nT; ++t) {
        if (SAVE) hist_store<T>(hp, t, mx, my, mz);
        bloch_step<T, CT>(k, bp[t * 3], bp[t * 3 + 1], bp[t * 3 + 2], mx, my, mz);
    }
    if (valid) { a.Mo[r * 3] = mx; a.Mo[r * 3 + 1] = my; a.Mo[r * 3 + 2] = mz; }
}


// =============================================================================================
// K1, line-granular variant (the headline path): float data, no history, rows 128-B aligned
// (Beff base % 128 == 0 and nT % 32 == 0).
//
// The chunked kernel above fetches 16 steps = 192 B per spin per chunk, i.e. one and a half
// cache lines: measured with FETCH_SIZE it reads 1.22x the algorithmic bytes, because the shared
// half line has usually left L2 when the next chunk asks for it.  Here the unit of transfer is
// ONE 128-B line per spin ("piece" = 32 floats = 10 2/3 steps), moved by LineMover (k_lines.hpp: the
// wave-loads, the VGPR staging, the LDS tile).  A step needs 3 consecutive floats, so steps straddle
// piece boundaries; 3 pieces = 96 floats = 32 steps is the period: piece 0 holds steps 0-9 + 2 floats
// of step 10, piece 1 the rest of step 10, steps 11-20 + 1 float of step 21, piece 2 the rest of step
// 21 and steps 22-31.  The straddling floats travel in two carry registers.
// =============================================================================================
// NA steps whose samples start at float `first` of this lane's LDS row, optionally preceded by a
// straddling step whose leading floats arrive in registers.
// SAVE: record the magnetisation before each step at hist[t], t = th, th+1, ...
template <bool RELAX, bool SAVE, bool PIN, typename CT, int NA, typename T = float>
__device__ __forceinline__ void lines_steps(const SpinConst<T, CT>& k, const T* q,
                                            T* hp, int64_t th, T& mx, T& my, T& mz)
{
    T Bx[NA], By[NA], Bz[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) { Bx[j] = q[3 * j]; By[j] = q[3 * j + 1]; Bz[j] = q[3 * j + 2]; }
    Rot<T> r[NA];
    rot_prepare<T, CT, NA>(k, Bx, By, Bz, r);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        if (SAVE) hist_store<T>(hp, th + j, mx, my, mz);
        rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
    }
    if (PIN) pin_state(mx, my, mz);
}

// 1 straddling step (b0,b1,b2 given) + NA steps from q
template <bool RELAX, bool SAVE, bool PIN, typename CT, int NA, typename T = float>
__device__ __forceinline__ void lines_steps_carry(const SpinConst<T, CT>& k, T b0, T b1,
                                                  T b2, const T* q, T* hp, int64_t th,
                                                  T& mx, T& my, T& mz)
{
    T Bx[NA + 1], By[NA + 1], Bz[NA + 1];
    Bx[0] = b0; By[0] = b1; Bz[0] = b2;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        Bx[j + 1] = q[3 * j]; By[j + 1] = q[3 * j + 1]; Bz[j + 1] = q[3 * j + 2];
    }
    Rot<T> r[NA + 1];
    rot_prepare<T, CT, NA + 1>(k, Bx, By, Bz, r);
#pragma unroll
    for (int j = 0; j < NA + 1; ++j) {
        if (SAVE) hist_store<T>(hp, th + j, mx, my, mz);
        rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
    }
    if (PIN) pin_state(mx, my, mz);
}

// Bounded for 3 waves per SIMD.  SPLIT: sub-batches per piece (2: 5/6 steps prepared at once, 3: 3/4 steps --
// fewer live registers).
// (Tried: three pieces in flight per wave instead of one -- 96 prefetch VGPRs, 2 waves/SIMD -- no
// gain at any grid size.)
template <typename CT, bool RELAX, int SPLIT, bool SAVE, bool PIN>
__global__ __launch_bounds__(WAVE, 3) void k_bloch_fwd_lines(FwdArgs<float> a)
{
    using T = float;
    using LM = LineMover<T>;
    constexpr int PF = LM::PF;
    __shared__ __attribute__((aligned(16))) T tile[WAVE * LM::PITCH];

    const int lane = threadIdx.x;
    const int64_t tile_id = xcd_tile(a.per_xcd);
    if (tile_id * WAVE >= a.rows) return;
    const auto [row0, r, valid, rc, n, s] = row_id(tile_id, lane, a.rows, a.nM);
    const SpinConst<T, CT> k = load_consts<T, CT>(a.g, a.E1, a.E2, a.E1m1, n, s);
    T mx = a.Mi[rc * 3 + 0], my = a.Mi[rc * 3 + 1], mz = a.Mi[rc * 3 + 2];

    const int64_t rowlen = 3 * a.nT;                       // floats; multiple of 96
    const int64_t npieces = rowlen / PF;                   // multiple of 3
    const LM lm(a.Beff, tile, lane, row0, a.rows, a.nT);
    const T* my_ = tile + lane * LM::PITCH;
    typename LM::V st0[8];
    T* hp = SAVE ? hist_tile_base<T>(a.hist, tile_id, a.nT) + lane : nullptr;
#define LS(NA_, Q_, TH_) lines_steps<RELAX, SAVE, PIN, CT, NA_>(k, my_ + (Q_), hp, t0 + (TH_), mx, my, mz)
#define LC(NA_, B0_, B1_, B2_, Q_, TH_) \
    lines_steps_carry<RELAX, SAVE, PIN, CT, NA_>(k, B0_, B1_, B2_, my_ + (Q_), hp, t0 + (TH_), mx, my, mz)
    if (npieces > 0) { MRPHY_LINES_FETCH(lm, st0, 0) }
    T c0, c1;
    for (int64_t p = 0; p < npieces; p += 3) {
        const int64_t t0 = (p / 3) * 32;
        const bool more = p + 3 < npieces;
        // piece 0: steps 0..9 (floats 0..29), carry floats 30, 31
        MRPHY_LINES_STAGE(lm, st0)
        MRPHY_LINES_FETCH(lm, st0, p + 1)
        if (SPLIT == 2) { LS(5, 0, 0); LS(5, 15, 5); }
        else            { LS(4, 0, 0); LS(3, 12, 4); LS(3, 21, 7); }
        c0 = my_[30]; c1 = my_[31];
        // piece 1: step 10 = (c0, c1, f0); steps 11..20 from float 1; carry float 31
        MRPHY_LINES_STAGE(lm, st0)
        MRPHY_LINES_FETCH(lm, st0, p + 2)
        if (SPLIT == 2) { LC(5, c0, c1, my_[0], 1, 10); LS(5, 16, 16); }
        else            { LC(3, c0, c1, my_[0], 1, 10); LS(4, 10, 14); LS(3, 22, 18); }
        c0 = my_[31];
        // piece 2: step 21 = (c0, f0, f1); steps 22..31 from float 2
        MRPHY_LINES_STAGE(lm, st0)
        if (more) { MRPHY_LINES_FETCH(lm, st0, p + 3) }
        if (SPLIT == 2) { LC(5, c0, my_[0], my_[1], 2, 21); LS(5, 17, 27); }
        else            { LC(3, c0, my_[0], my_[1], 2, 21); LS(4, 11, 25); LS(3, 23, 29); }
    }
#undef LS
#undef LC
    if (valid) { a.Mo[r * 3] = mx; a.Mo[r * 3 + 1] = my; a.Mo[r * 3 + 2] = mz; }
}


// =============================================================================================
// K1, line-granular, DOUBLE precision (round 4): the reference's own tests run in fp64
// (tests/test_sims.py:16), and the chunked kernel above reads fp64 rows 192 B at a time -- one and a
// half lines, 1.22 x the algorithmic bytes, 4.1-4.5 TB/s.  Same scheme as k_bloch_fwd_lines with the
// numbers of an 8-byte element: a piece = one 128-B line per spin = 16 doubles = 5 1/3 steps, period
// 3 pieces = 48 doubles = 16 steps (rows 128-B aligned, nT % 16 == 0):
//     piece 0: steps 0-4 (doubles 0-14), double 15 carried;
//     piece 1: step 5 = (carry, d0, d1), steps 6-9 (doubles 2-13), doubles 14, 15 carried;
//     piece 2: step 10 = (carry, carry, d0), steps 11-15 (doubles 1-15).
// Batches of at most two steps (a Rot<double> is 10 VGPRs): 150-160 VGPRs, three waves per SIMD, no scratch.
// The mover is the same struct at sizeof(T) = 8: LDS tile 64 x (16 + 2) doubles = 9 KB.
// =============================================================================================
template <typename CT, bool RELAX, bool SAVE>
__global__ __launch_bounds__(WAVE, 3) void k_bloch_fwd_lines_f64(FwdArgs<double> a)
{
    using T = double;
    using LM = LineMover<T>;
    constexpr int PF = LM::PF;
    __shared__ __attribute__((aligned(16))) T tile[WAVE * LM::PITCH];

    const int lane = threadIdx.x;
    const int64_t tile_id = xcd_tile(a.per_xcd);
    if (tile_id * WAVE >= a.rows) return;
    const auto [row0, r, valid, rc, n, s] = row_id(tile_id, lane, a.rows, a.nM);
    const SpinConst<T, CT> k = load_consts<T, CT>(a.g, a.E1, a.E2, a.E1m1, n, s);
    T mx = a.Mi[rc * 3 + 0], my = a.Mi[rc * 3 + 1], mz = a.Mi[rc * 3 + 2];

    const int64_t rowlen = 3 * a.nT;                       // doubles; multiple of 48
    const int64_t npieces = rowlen / PF;                   // multiple of 3
    const LM lm(a.Beff, tile, lane, row0, a.rows, a.nT);
    const T* my_ = tile + lane * LM::PITCH;
    typename LM::V st0[8];
    T* hp = SAVE ? hist_tile_base<T>(a.hist, tile_id, a.nT) + lane : nullptr;
#define LS(NA_, Q_, TH_) lines_steps<RELAX, SAVE, true, CT, NA_, T>(k, my_ + (Q_), hp, t0 + (TH_), mx, my, mz)
#define LC(NA_, B0_, B1_, B2_, Q_, TH_) \
    lines_steps_carry<RELAX, SAVE, true, CT, NA_, T>(k, B0_, B1_, B2_, my_ + (Q_), hp, t0 + (TH_), mx, my, mz)
    if (npieces > 0) { MRPHY_LINES_FETCH(lm, st0, 0) }
    T c0, c1;
    for (int64_t p = 0; p < npieces; p += 3) {
        const int64_t t0 = (p / 3) * 16;
        const bool more = p + 3 < npieces;
        // piece 0: steps 0..4 (doubles 0..14), carry double 15
        MRPHY_LINES_STAGE(lm, st0)
        MRPHY_LINES_FETCH(lm, st0, p + 1)
        LS(2, 0, 0); LS(2, 6, 2); LS(1, 12, 4);
        c0 = my_[15];
        // piece 1: step 5 = (c0, d0, d1); steps 6..9 from double 2; carry doubles 14, 15
        MRPHY_LINES_STAGE(lm, st0)
        MRPHY_LINES_FETCH(lm, st0, p + 2)
        LC(1, c0, my_[0], my_[1], 2, 5); LS(2, 5, 7); LS(1, 11, 9);
        c0 = my_[14]; c1 = my_[15];
        // piece 2: step 10 = (c0, c1, d0); steps 11..15 from double 1
        MRPHY_LINES_STAGE(lm, st0)
        if (more) { MRPHY_LINES_FETCH(lm, st0, p + 3) }
        LC(1, c0, c1, my_[0], 1, 10); LS(2, 4, 12); LS(2, 10, 14);
    }
#undef LS
#undef LC
    if (valid) { a.Mo[r * 3] = mx; a.Mo[r * 3 + 1] = my; a.Mo[r * 3 + 2] = mz; }
}

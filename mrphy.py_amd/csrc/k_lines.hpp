// k_lines.hpp -- how a 64-spin tile of Beff travels HBM -> VGPRs -> LDS (-> HBM) in the line-granular K1 / K1h / K3
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once

// The unit of transfer is ONE 128-B line per spin, a "piece" of PF elements (LINE_ELEMS, geom.hpp):
//   * a piece of the tile is 8 wave-loads; load i, lane l fetches 16 B of row 8i + l/8 at byte 16*(l%8) of that
//     row's line: every wave-load covers 8 rows x one WHOLE line;
//   * the next piece waits in 8 16-B vectors per lane (the kernel's own local array: see Stage in k_common.hpp for
//     why it is not a member) while the current one is integrated;
//   * LDS tile 64 x PITCH elements = 9 KB, pitch 9 slots of 16 B (odd): lane = spin reads its row conflict-free;
//   * a step needs 3 consecutive elements, so steps straddle piece boundaries: 3 pieces = PF steps is the period.
template <typename T>
struct LineMover {
    using V = typename V16<T>::type;
    static constexpr int VE = V16<T>::N;                   // elements per 16-B vector
    static constexpr int PF = LINE_ELEMS<T>;               // elements per piece = one 128-B line
    static constexpr int PITCH = PF + VE;                  // 9 slots of 16 B
    static constexpr int PERIOD = PF;                      // steps per period of 3 pieces

    // wave-uniform base (SGPRs) + 32-bit per-lane offsets: loads and stores use the saddr+voffset form and need 8
    // VGPRs of addressing instead of 16 (host guarantees 64*rowlen*sizeof(T) < 2^32: lines_shape_ok)
    const T* __restrict__ base;
    // byte offset of load / store i = min(off0 + i * ostride, olim): two VGPRs instead of eight precomputed offsets.
    // Rows past the end of the last tile re-read its last valid row in the loads and are skipped by the stores.
    unsigned off0, ostride, olim;
    T* wr;                                                 // this lane's slot in the LDS tile, + i*8*PITCH per load
    int frow, lastrow;                                     // row of load 0; last valid row of this tile

    // (takes nT, not the row length: this function is simplified before it is inlined, and from an opaque row length the
    // stride 8 * rowlen * sizeof(T) becomes a shift of 3 nT instead of one multiplication of nT)
    __device__ __forceinline__ LineMover(const T* Beff, T* tile, int lane, int64_t row0, int64_t rows, int64_t nT)
    {
        const int64_t rowlen = 3 * nT;
        frow = lane >> 3;
        const int fcol = (lane & 7) * VE;
        wr = tile + frow * PITCH + fcol;
        base = Beff + row0 * rowlen;
        const int64_t last = rows - 1 - row0;              // last valid row of this tile
        ostride = (unsigned)(8 * rowlen * sizeof(T));
        off0 = (unsigned)(((frow < last ? frow : last) * rowlen + fcol) * sizeof(T));
        olim = (unsigned)(((last < 63 ? last : 63) * rowlen + fcol) * sizeof(T));
        lastrow = (int)(last < 63 ? last : 63);
    }
};

// fetch, stage and store are statement macros over a LineMover `lm`, the kernel's staged vectors `st` (8 of LM::V, a
// local array: see Stage in k_common.hpp) and the piece `p`.  Not member functions: a function is simplified and
// its loops unrolled before it is inlined, the kernel's own statements only with the kernel, and the step loops around
// them are then scheduled differently (other VGPR counts, other waits).
// (o0 is laundered through an empty asm per use, or the compiler hoists all eight offsets back into registers for the
// whole loop)
#define MRPHY_LINES_OFF(lm, o0, i) (min((o0) + (unsigned)(i) * (lm).ostride, (lm).olim))
// piece p: HBM -> st
#define MRPHY_LINES_FETCH(lm, st, p)                                                                                  \
    { unsigned o0 = (lm).off0; asm volatile("" : "+v"(o0));                                                           \
    _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                                     \
        (st)[i] = __builtin_nontemporal_load(reinterpret_cast<const typename decltype(lm)::V*>(                       \
            reinterpret_cast<const char*>((lm).base + (p) * (lm).PF) + MRPHY_LINES_OFF(lm, o0, i))); }
// st -> LDS tile, once every lane is done with the piece that is there
#define MRPHY_LINES_STAGE(lm, st)                                                                                     \
    __syncthreads();                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                                     \
        *reinterpret_cast<typename decltype(lm)::V*>((lm).wr + i * 8 * (lm).PITCH) = (st)[i];                         \
    __syncthreads();
// LDS tile -> piece p of the tile's rows at obase (the tile's first row; null: nothing is stored), as whole lines
#define MRPHY_LINES_STORE(lm, obase, p)                                                                               \
    if (obase) {                                                                                                      \
        __syncthreads();                                                                                              \
        unsigned o0 = (lm).off0; asm volatile("" : "+v"(o0));                                                         \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                               \
            const auto v = *reinterpret_cast<const typename decltype(lm)::V*>((lm).wr + i * 8 * (lm).PITCH);          \
            if ((lm).frow + 8 * i <= (lm).lastrow)                                                                    \
                __builtin_nontemporal_store(v, reinterpret_cast<typename decltype(lm)::V*>(                           \
                    reinterpret_cast<char*>((obase) + (p) * (lm).PF) + MRPHY_LINES_OFF(lm, o0, i)));                  \
        }                                                                                                             \
    }

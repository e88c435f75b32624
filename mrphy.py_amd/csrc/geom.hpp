// geom.hpp -- sizes and capacities that more than one translation unit must agree on: the kernels, their
// launchers (tu_*.hip) and the workspace / buffer-size queries of the C ABI (abi.hip) all read them here.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace mrphy {

constexpr int WAVE = 64;
constexpr int HIST_STEP = 3 * WAVE;               // history: elements per time step of one 64-spin tile
constexpr int AB_HIST_STEP = 12 * WAVE;           // beff2ab history: the 3x4 state per step and tile
// Line-granular K1 / K1h / K3 (k_lines.hpp): a piece = one LINE_BYTES line per spin = LINE_ELEMS<T> elements; three
// pieces = LINE_ELEMS<T> steps are one period, and a pulse must be whole periods (lines_shape_ok, host_common.hpp).
constexpr int LINE_BYTES = 128;
template <typename T> constexpr int LINE_ELEMS = LINE_BYTES / (int)sizeof(T);
constexpr int SEG = 16;                           // K2 / K2b: steps per checkpoint segment
// Generic in SEG: K2 (k_fused_fwd.hpp: only the checkpoint stride), the checkpoint / workspace size queries.
// NOT generic: k_bloch_rfgr_bwd_mc (step = lane >> 2, needs SEG * 4 == WAVE) and the reduction tile of both fused
// adjoints (red_idx).  Both carry a static_assert; change SEG only together with them.
constexpr int64_t K2B_MAX_WAVES = 256 * 8;        // K2b: resident waves, 8 per CU
constexpr int64_t SIG_MAX_WAVES = 256 * 16;       // K2s (signal forward): 8 / 16 KB of LDS per wave, 16 waves per CU as K2 runs
constexpr int SIG_MAX_RX_F32 = 8, SIG_MAX_RX_F64 = 8;   // receive coils per launch of the signal kernels
constexpr int K2B_MAXC = 8;                       // fused adjoint: largest coil capacity
constexpr int64_t K2B_MC_MAX_WAVES = 256 * 8;     // 18 KB of LDS per wave -> 8 per CU = 2 per SIMD
// K2ab-mc / K2abb-mc (k_ab_rfgr_mc.hpp): the largest coil capacity built (2, 4, 8) per data type, forward and adjoint
// alike; never above K2B_MAXC, whose workspace rows and persistent waves the adjoint shares
// (fp64 stops at 4: K2abb is at 443-464 VGPRs there, the capacity-8 adjoint would need a private segment)
constexpr int AB_MC_MAXC_F32 = 8, AB_MC_MAXC_F64 = 4;
constexpr int ab_mc_max_coils(size_t tsize) { return tsize == 8 ? AB_MC_MAXC_F64 : AB_MC_MAXC_F32; }
static_assert(AB_MC_MAXC_F32 <= K2B_MAXC && AB_MC_MAXC_F64 <= K2B_MAXC, "K2abb-mc takes K2b-mc's workspace");
// K2sh / K2shb (k_fused_shim.hpp): the largest channel capacity built (2, 4, 8) per data type, forward and adjoint alike
constexpr int SHIM_MAXS_F32 = 8, SHIM_MAXS_F64 = 8;
constexpr int shim_max_channels(size_t tsize) { return tsize == 8 ? SHIM_MAXS_F64 : SHIM_MAXS_F32; }
// K2j (k_fused_jvp.hpp): the largest direction capacity built (1, 2, 4) per data type
constexpr int JVP_MAXD_F32 = 4, JVP_MAXD_F64 = 4;
constexpr int jvp_max_dirs(size_t tsize) { return tsize == 8 ? JVP_MAXD_F64 : JVP_MAXD_F32; }
// Ksqj (k_ab_sequence_jvp.hpp): the largest direction capacity built (1, 2, 4) per data type
constexpr int SEQ_JVP_MAXD_F32 = 4, SEQ_JVP_MAXD_F64 = 4;
constexpr int seq_jvp_max_dirs(size_t tsize) { return tsize == 8 ? SEQ_JVP_MAXD_F64 : SEQ_JVP_MAXD_F32; }
constexpr int BWD_MAXC = 32;                      // K0 adjoint: largest coil capacity of the one-pass kernels

// broadcastable per-spin constant (see mrphy_hip.h): element (n, s) at p[n * sn + s * sm]
struct Bc {
    const void* p;
    int64_t sn, sm;
};

// The operands every member of the fused family (K2, K2b, K2s and their trajectory / multi-coil builds) takes: the
// pulse on the spins plus the step constants, in the order of include/mrphy_hip.h.  abi.hip packs an entry point's
// scalars into PulseOps = PulseOpsT<void> once; the launchers take it by value and the kernel argument structs embed
// PulseOpsT<T> -- the same bytes with the arrays of the data type typed -- at the place of these twelve fields.
template <typename T>
struct PulseOpsT {
    const T* rf;   int64_t rf_sn;     // (N, 2, nT, nC), batch stride
    const T* gr;   int64_t gr_sn;     // (N, 3, nT), batch stride
    const T* loc;                     // (N, nM, 3)
    Bc df, gam;                       // null df: no off-resonance
    const T* b1;                      // (N, nM, 2, nC) or null
    Bc g, E1, E2;
    const void* E1m1;                 // E1, E2, E1m1: all or none (no relaxation)
};
using PulseOps = PulseOpsT<void>;
static_assert(sizeof(PulseOps) == 176 && sizeof(PulseOpsT<float>) == 176 && sizeof(PulseOpsT<double>) == 176,
              "PulseOps: 7 pointers and strides of 8 bytes, 5 Bc of 24");
template <typename T>
inline PulseOpsT<T> typed(const PulseOps& o) { return __builtin_bit_cast(PulseOpsT<T>, o); }

// What a Bz-extended call carries besides PulseOps: the motion of K2v / K2vb or the field channels of K2sh / K2shb.  The
// fields of the other extension are null / 0.
struct BzExt {
    const void* vdt;   int64_t step0; // motion: (N, nM, 3), the displacement per step; the steps played before this call
    const void* sh;    int64_t sh_sn; // channels: the waveforms (N|1, nS, nT) and their batch stride (0: shared),
    const void* shMap; int64_t nS;    // the maps (N nM, nS)
};

// What a forward-mode call (K2j) carries besides PulseOps: D directions, each a set of tangents of the operands.  Dense
// tables of the data type with a leading direction axis; a null table is a zero tangent.
struct JvpTangents {
    int64_t D;
    const void *dMi, *drf, *dgr;      // (D, N, nM, 3)  (D, N, 2, nT)  (D, N, 3, nT)
    const void *dloc, *ddf, *db1;     // (D, N, nM, 3)  (D, N, nM)     (D, N, nM, 2)
    const void *dE1, *dE2, *dE1m1;    // (D, N, nM) each
};

// What a forward-mode call of the sequence (Ksqj) carries: the operands of mrphy_ab_sequence_fwd and D directions, each a
// set of tangents of them.  Per spin, dense tables of the data type with a leading direction axis: dA (D, P, rows, 9),
// dB (D, P, rows, 3), dMi (D, rows, 3), dT1, dT2, ddf (D, rows).  Block-uniform, fp64: dphase, drest (D, N|1, K) with the
// element stride *_sn between batch entries (0 broadcasts; a direction is (sn ? N : 1) K elements).  A null table is a
// zero tangent.
struct SeqJvpCall {
    const void *A, *B; int64_t P; const void* pulse;
    const void* rs; int64_t rs_sn;
    Bc T1, T2, df;
    const void* Mi; int64_t Mi_sn, Mi_sm;
    const void* cs; int64_t cs_sn;
    int64_t D;
    const void *dA, *dB, *dMi, *dT1, *dT2, *ddf;
    const void* dphase; int64_t dphase_sn;
    const void* drest;  int64_t drest_sn;
    void* Mt;                         // (K, rows, 3) or null: not wanted
    void* dMt;                        // (D, K, rows, 3)
    int64_t N, nM, K;
};

// Everything an adjoint call of the fused family (K2b, its trajectory, signal, MAPS, CONSTS, multi-coil, moving and shim
// builds) carries besides PulseOps.  Each adjoint entry point of abi.hip packs it once; the validators, the launchers and
// the kernel argument structs take it from there on.  A null pointer is "not given" (a cotangent) or "not wanted" (an
// output).  The shim builds return grad_sh next to grad_gr: their ggr is the lead buffer (N, 3 + nS, nT).
struct AdjointReq {
    const void* Mck;                  // (nT/SEG, N*nM, 3): the forward's checkpoints
    const void* gMo;                  // cotangents: grad_Mo (N, nM, 3) ...
    const void* gMt; int64_t every;   // ... or grad_Mt (nRec, N, nM, 3), a record every `every` steps;
    const void* rx; int64_t nRx;      // the signal's receive map (N, nM, 2, nRx) with
    const void* gsig;                 // grad_sig (N, 2, nRec, nRx)
    void *gMi, *grf, *ggr;            // outputs: (N, nM, 3), (N, 2, nT, nC), (N, 3, nT)
    void *gloc, *gBz, *gb1, *gC;      // per-spin outputs: (N, nM, 3), (N, nM), (N, nM, 2), (N, nM, 4)
    void* work;
    int64_t N, nM, nT, nC;
    BzExt ext;                        // the builds MOVING and SHIM2 / 4 / 8 (internal.hpp) only
};

inline int64_t hist_tiles(int64_t N, int64_t nM) { return (N * nM + WAVE - 1) / WAVE; }
inline int64_t hist_elems(int64_t N, int64_t nM, int64_t nT)
{
    return hist_tiles(N, nM) * nT * HIST_STEP;
}

// The history of K1h / K3 (ABI 5) as 1..HIST_MAX_PARTS separately allocated parts: the 64-spin tiles are dealt to the
// parts in blocks (tile -> part tile / tiles_per_part) or round-robin (tile -> part tile % n_parts), a tile's
// nT * HIST_STEP elements are contiguous inside its part.  One launch then writes (K1h) / reads (K3) every part at the
// same time: a write stream spread over two separately allocated blocks runs in the fast placement mode where ONE
// block of the same total size usually does not.  Passed to the kernels by value (kernarg).
constexpr int HIST_MAX_PARTS = 8;
struct HistParts {
    void* p[HIST_MAX_PARTS];
    uint32_t tiles_per_part;          // every part holds this many tiles (the last one may use fewer)
    int32_t n_parts;                  // 0: no history wanted
    int32_t interleaved;              // 0: blocks of tiles_per_part consecutive tiles; 1: round-robin
};
inline int64_t hist_tiles_per_part(int64_t N, int64_t nM, int64_t n_parts)
{
    return n_parts > 0 ? (hist_tiles(N, nM) + n_parts - 1) / n_parts : 0;
}
inline HistParts hist_one_part(const void* p, int64_t N, int64_t nM)
{
    HistParts h = {};
    h.p[0] = const_cast<void*>(p);
    h.n_parts = p ? 1 : 0;
    h.tiles_per_part = (uint32_t)hist_tiles(N, nM);
    return h;
}

inline int64_t k2b_waves(int64_t nM)
{
    const int64_t tiles = (nM + WAVE - 1) / WAVE;
    return tiles < K2B_MAX_WAVES ? tiles : K2B_MAX_WAVES;
}

// K2s: persistent waves of the signal forward, and the records it takes at stride `every`
inline int64_t sig_waves(int64_t nM)
{
    const int64_t tiles = (nM + WAVE - 1) / WAVE;
    return tiles < SIG_MAX_WAVES ? tiles : SIG_MAX_WAVES;
}
inline int64_t sig_records(int64_t nT, int64_t every) { return nT / every + (nT % every != 0); }
// K2s / K2bs: the most receive coils one launch takes for a data type of `tsize` bytes -- the largest coil capacity the
// kernels are built at (1, 2, 4, 8), forward and adjoint alike (DESIGN.md section 3 has the register readings)
constexpr int sig_max_rx(size_t tsize) { return tsize == 8 ? SIG_MAX_RX_F64 : SIG_MAX_RX_F32; }

// Ktrs / Ktrsb (k_train_signal.hpp): the signal of a K-repetition train.  One wave per block, persistent over the
// 64-spin tiles w, w + P, ... with P = trs_waves(nM) partial rows whatever nM: 17 KB of LDS per wave -> 9 per CU fit,
// 8 are asked for.  TRS_SEG repetitions per checkpoint segment of the adjoint; TRS_ROWS rows of the forward's tile.
constexpr int TRS_SEG = 8;
constexpr int TRS_ROWS = 32;
constexpr int64_t TRS_MAX_WAVES = 256 * 8;
constexpr int TRS_MAX_RX_F32 = 8, TRS_MAX_RX_F64 = 8;   // receive coils per launch (capacities 1, 2, 4, 8)
constexpr int trs_max_rx(size_t tsize) { return tsize == 8 ? TRS_MAX_RX_F64 : TRS_MAX_RX_F32; }
inline int64_t trs_waves(int64_t nM)
{
    const int64_t tiles = (nM + WAVE - 1) / WAVE;
    return tiles < TRS_MAX_WAVES ? tiles : TRS_MAX_WAVES;
}
inline int64_t trs_segments(int64_t K) { return (K + TRS_SEG - 1) / TRS_SEG; }
// workspace of one launch: P partial rows of (N, rows, K) fp64 sums -- rows = 2 nRx (forward), 1 (the adjoint's phase)
inline size_t trs_workspace(int64_t N, int64_t nM, int64_t K, int64_t rows)
{
    return (size_t)(trs_waves(nM) * N * rows * K) * sizeof(double);
}

inline int64_t k2b_mc_waves(int64_t nM)
{
    const int64_t tiles = (nM + WAVE - 1) / WAVE;
    return tiles < K2B_MC_MAX_WAVES ? tiles : K2B_MC_MAX_WAVES;
}

// coil capacity of the one-pass K0 adjoint for nC coils: 8 / 16 / 32, or 0 = the generic passes
// (no b1 map, or more than BWD_MAXC coils).  Used by the launcher AND the workspace query.
// Round 4: more than BWD_MAXC coils run the same pass over blocks of BWD_MAXC coils (every coil's sums are
// independent of the others', so nothing is carried between blocks: grad_Beff is read once per block).
inline int bwd_capacity(int64_t nC, bool has_b1)
{
    if (nC < 2 || !has_b1) return 0;
    return nC <= 8 ? 8 : (nC <= 16 ? 16 : 32);
}
// padded coil count of the SGPR pass (k_rfgr2beff_bwd_sgpr) for nC coils, 0 as above
inline int bwd_padded_coils(int64_t nC, bool has_b1)
{
    if (!bwd_capacity(nC, has_b1)) return 0;
    if (nC > BWD_MAXC) return BWD_MAXC;               // blocks of 32 (the last one padded to its own count)
    return nC <= 4 ? 4 : (nC <= 8 ? 8 : (nC <= 12 ? 12 : (nC <= 16 ? 16 : (nC <= 24 ? 24 : 32))));
}

inline int64_t bwd_spin_groups(int64_t nM);
// Workspace of the multi-coil K0 adjoint (2..BWD_MAXC coils): [partial sums (nSG, N, 3 + 2 nC, nT) |
// packed coefficient rows (N nM, 2 MC + 4)], the second part on a 256-byte boundary.
inline size_t bwd_pack_offset(size_t ts, int64_t N, int64_t nM, int64_t nT, int64_t nC)
{
    const size_t sums = (size_t)(bwd_spin_groups(nM) * N * (3 + 2 * nC) * nT) * ts;
    return (sums + 255) / 256 * 256;
}
inline int64_t bwd_spin_groups(int64_t nM)
{
    int64_t g = (nM + 255) / 256;
    if (g < 1) g = 1;
    if (g > 256) g = 256;
    return g;
}

}  // namespace mrphy

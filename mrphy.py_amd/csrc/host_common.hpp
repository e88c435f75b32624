// host_common.hpp -- what every translation unit of libmrphy_hip.so starts with: the HIP runtime, the C ABI
// header, the shared geometry, the step math, the common device fragment (k_common.hpp, inside this
// unit's anonymous namespace: kernels have internal linkage, every unit carries its own code object)
// and the host-side helpers of the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>

#include "../../include/mrphy_hip.h"
#include "geom.hpp"
#include "bloch_math.hpp"
#include "internal.hpp"

using namespace mrphy;

namespace {
#include "k_common.hpp"

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

inline int launch_status()
{
    hipError_t e = hipGetLastError();
    return (int)e;
}

inline size_t tsize(int dtype) { return dtype == MRPHY_F64 ? 8 : 4; }
inline size_t csize(int dtype) { return (dtype == MRPHY_F32 || dtype == MRPHY_F32P) ? 4 : 8; }

// steps per chunk of the chunked kernels.  fp32: 16 steps = 192 B per row.  fp64 forward: 8 steps =
// 192 B per row as well -- with 16 (384 B, 24 staging vectors = 96 VGPRs per lane) the fp64 forward
// builds need 354 VGPRs = ONE wave per SIMD; with 8, 244 = two (same-box A/B at 64^3 x 1024, round 3:
// K1 1.55 -> 1.42 ms, K1h 2.49 -> 2.40 ms).  The fp64 adjoint stays at 16: with 8 it got slower
// (3.92 -> 4.51 ms; 356 VGPRs either way is one wave per SIMD, and the smaller chunk doubles the
// barriers).  Putting the fp64 large-angle path (ocml sincos) behind a real call to shrink the
// kernels was tried too: the call's register convention spilled the HOT path (fused K2 0.78 -> 2.58 ms).
template <typename T> constexpr int TC_FWD = sizeof(T) == 8 ? 8 : 16;
template <typename T> constexpr int TC_BWD = 16;

inline int check_common(int dtype, int64_t N, int64_t nM, int64_t nT)
{
    if (dtype != MRPHY_F32 && dtype != MRPHY_F64 && dtype != MRPHY_F32_C64 &&
        dtype != MRPHY_F32P && dtype != MRPHY_F32P_C64)
        return MRPHY_EINVAL;
    if (N < 0 || nM < 0 || nT < 0) return MRPHY_EINVAL;
    return 0;
}

// What the line-granular kernels need (k_lines.hpp; the constants are geom.hpp's): rows on whole lines, whole periods
// of LINE_ELEMS<T> steps, and a tile of WAVE rows within the 32-bit byte offsets of the mover.
template <typename T>
inline bool lines_shape_ok(const void* Beff, int64_t nT)
{
    return aligned_to(Beff, LINE_BYTES) && nT > 0 && (nT % LINE_ELEMS<T> == 0) &&
           ((int64_t)(WAVE * 3 * sizeof(T)) * nT < (int64_t)4294967295);
}

// XCD-contiguous tile order (xcd_tile, k_common.hpp): the grid padded to 8 equal shares; returns the share
inline unsigned xcd_pad(dim3& grid)
{
    const unsigned per_xcd = (grid.x + 7) / 8;
    grid.x = per_xcd * 8;
    return per_xcd;
}

}  // namespace

// dtype code -> (T, CT); a unit instantiates its launchers for the codes in MRPHY_DT_MASK (bit = code)
#ifndef MRPHY_DT_MASK
#define MRPHY_DT_MASK 0x1f
#endif
#if MRPHY_DT_MASK & 1
#define MRPHY_IF_F32(X) X(float, float)
#else
#define MRPHY_IF_F32(X)
#endif
#if MRPHY_DT_MASK & 2
#define MRPHY_IF_F64(X) X(double, double)
#else
#define MRPHY_IF_F64(X)
#endif
#if MRPHY_DT_MASK & 4
#define MRPHY_IF_F32_C64(X) X(float, double)
#else
#define MRPHY_IF_F32_C64(X)
#endif
#if MRPHY_DT_MASK & 8
#define MRPHY_IF_F32P(X) X(float, prec_f32)
#else
#define MRPHY_IF_F32P(X)
#endif
#if MRPHY_DT_MASK & 16
#define MRPHY_IF_F32P_C64(X) X(float, prec_f64)
#else
#define MRPHY_IF_F32P_C64(X)
#endif
#define MRPHY_FOR_DTYPES(X) MRPHY_IF_F32(X) MRPHY_IF_F64(X) MRPHY_IF_F32_C64(X) MRPHY_IF_F32P(X) MRPHY_IF_F32P_C64(X)
// the units whose kernels have a data type only (K0 and its adjoint): bits 0 and 1
#define MRPHY_FOR_DATA_TYPES(X) MRPHY_IF_F32(X) MRPHY_IF_F64(X)

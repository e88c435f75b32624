// k_ab_steady.hpp -- the steady state of a periodic pulse from Hargreaves' A, B, and its adjoint
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once

// =============================================================================================
// One period = a rest of duration `rest` (free precession, exactly k_freeprec of k_aux.hpp), then the pulse
// M_after = A M_before + B.  With
//     F = diag(E2r, E2r, E1r) Rz(phi),   phi = -2 pi df rest,   E1r = exp(-rest/T1),   E2r = exp(-rest/T2),
//     f = (0, 0, -expm1(-rest/T1))                                            (M- = F M + f: the rest)
// the state right after the pulse solves
//     (I - A F) Mss = A f + B.
// One thread per spin.  Whatever the data type, ALL arithmetic is fp64 -- the rest constants, the products and the
// solve -- and the outputs are rounded once: the kernel runs once per spin, not once per step, and Mss already carries
// A's rounding amplified by the condition number of I - A F (about 1 / (1 - E1r)); the solve adds nothing to it.
// The solve is the cofactor form, K = cof(I - A F), (I - A F)^-1 = K^T / det with ONE division: no pivot search, no
// dynamically indexed array, nothing in scratch.  A singular system (no relaxation anywhere: det == 0) gives
// non-finite output; nothing on the host looks at det.
//
// Adjoint, for a cotangent g of Mss (recomputing Mss from A, B and the constants; nothing else was saved):
//     lambda = (I - A F)^-T g = K g / det       (the same cofactors, not transposed)
//     M- = F Mss + f,   mu = A^T lambda
//     grad_B = lambda,   grad_A[i][j] = lambda_i M-_j
//     grad_consts = [d rest, d T1, d T2, d df] = the formulas of k_freeprec_gc (k_aux.hpp) at Mi := Mss, gMo := mu.
// rest == null: no rest period, F = I, f = 0, Mss = (I - A)^-1 B.
// =============================================================================================
struct SteadyArgs {
    const void* A; const void* B;         // (rows, 3, 3), (rows, 3)
    const void* g;                        // (rows, 3): the cotangent of Mss (adjoint only)
    const void* rest; int64_t rest_sn;    // (N|1,); null: no rest period
    Bc T1, T2, df;                        // T1.p == null: no relaxation in the rest; df.p == null: no precession
    void* Mss;                            // (rows, 3) (forward only)
    void* gA; void* gB; void* gC;         // (rows, 3, 3), (rows, 3), (rows, 4); each may be null (adjoint only)
    int64_t rows, nM;
};

// what both kernels form per spin
struct SteadySpin {
    double a[9];                          // A, row-major
    double rest, df, t1, t2;              // the constants as loaded (1 for an absent T)
    double c, s, e1, e2, f3;              // cos phi, sin phi, E1r, E2r, -expm1(-rest/T1)
    double k[9];                          // cofactors of I - A F, row-major
    double rdet;                          // 1 / det(I - A F)
    double m[3];                          // Mss
};

template <typename T>
__device__ __forceinline__ SteadySpin steady_spin(const SteadyArgs& q, int64_t r)
{
    SteadySpin v;
    const int64_t n = r / q.nM, sidx = r % q.nM;
    const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
    const T* pb = reinterpret_cast<const T*>(q.B) + r * 3;
#pragma unroll
    for (int i = 0; i < 9; ++i) v.a[i] = double(pa[i]);
    const double b0 = double(pb[0]), b1 = double(pb[1]), b2 = double(pb[2]);
    v.rest = 0.0; v.df = 0.0; v.t1 = 1.0; v.t2 = 1.0;
    v.c = 1.0; v.s = 0.0; v.e1 = 1.0; v.e2 = 1.0; v.f3 = 0.0;
    if (q.rest) {
        v.rest = double(reinterpret_cast<const T*>(q.rest)[n * q.rest_sn]);
        if (q.df.p) {
            v.df = double(bc_load<T>(q.df, n, sidx));
            sincos(-6.283185307179586476925 * v.df * v.rest, &v.s, &v.c);
        }
        if (q.T1.p) {
            v.t1 = double(bc_load<T>(q.T1, n, sidx));
            v.t2 = double(bc_load<T>(q.T2, n, sidx));
            const double a1 = -v.rest / v.t1;
            v.e1 = exp(a1); v.f3 = -expm1(a1); v.e2 = exp(-v.rest / v.t2);
        }
    }
    // C = I - A F,   F = [[e2 c, -e2 s, 0], [e2 s, e2 c, 0], [0, 0, e1]]
    const double fc = v.e2 * v.c, fs = v.e2 * v.s;
    double c[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[3 * i]     = -(v.a[3 * i] * fc + v.a[3 * i + 1] * fs);
        c[3 * i + 1] = -(v.a[3 * i + 1] * fc - v.a[3 * i] * fs);
        c[3 * i + 2] = -(v.a[3 * i + 2] * v.e1);
    }
    c[0] += 1.0; c[4] += 1.0; c[8] += 1.0;
    v.k[0] = c[4] * c[8] - c[5] * c[7];
    v.k[1] = c[5] * c[6] - c[3] * c[8];
    v.k[2] = c[3] * c[7] - c[4] * c[6];
    v.k[3] = c[2] * c[7] - c[1] * c[8];
    v.k[4] = c[0] * c[8] - c[2] * c[6];
    v.k[5] = c[1] * c[6] - c[0] * c[7];
    v.k[6] = c[1] * c[5] - c[2] * c[4];
    v.k[7] = c[2] * c[3] - c[0] * c[5];
    v.k[8] = c[0] * c[4] - c[1] * c[3];
    v.rdet = 1.0 / (c[0] * v.k[0] + c[1] * v.k[1] + c[2] * v.k[2]);
    // rhs = A f + B;   Mss = K^T rhs / det
    const double r0 = v.a[2] * v.f3 + b0, r1 = v.a[5] * v.f3 + b1, r2 = v.a[8] * v.f3 + b2;
#pragma unroll
    for (int j = 0; j < 3; ++j) v.m[j] = (v.k[j] * r0 + v.k[3 + j] * r1 + v.k[6 + j] * r2) * v.rdet;
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void k_ab_steadystate_fwd(SteadyArgs q)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= q.rows) return;
    const SteadySpin v = steady_spin<T>(q, r);
    T* o = reinterpret_cast<T*>(q.Mss) + r * 3;
    o[0] = T(v.m[0]); o[1] = T(v.m[1]); o[2] = T(v.m[2]);
}

template <typename T>
__global__ __launch_bounds__(256) void k_ab_steadystate_bwd(SteadyArgs q)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= q.rows) return;
    const SteadySpin v = steady_spin<T>(q, r);
    const T* pg = reinterpret_cast<const T*>(q.g) + r * 3;
    const double g0 = double(pg[0]), g1 = double(pg[1]), g2 = double(pg[2]);
    double l[3];                                                   // lambda = K g / det
#pragma unroll
    for (int i = 0; i < 3; ++i) l[i] = (v.k[3 * i] * g0 + v.k[3 * i + 1] * g1 + v.k[3 * i + 2] * g2) * v.rdet;
    const double x = v.m[0], y = v.m[1], z = v.m[2];
    const double rx = v.c * x - v.s * y, ry = v.s * x + v.c * y;   // rotated, before relaxation
    if (q.gB) {
        T* o = reinterpret_cast<T*>(q.gB) + r * 3;
        o[0] = T(l[0]); o[1] = T(l[1]); o[2] = T(l[2]);
    }
    if (q.gA) {
        const double p0 = rx * v.e2, p1 = ry * v.e2, p2 = z * v.e1 + v.f3;      // M- = F Mss + f
        T* o = reinterpret_cast<T*>(q.gA) + r * 9;
#pragma unroll
        for (int i = 0; i < 3; ++i) { o[3 * i] = T(l[i] * p0); o[3 * i + 1] = T(l[i] * p1); o[3 * i + 2] = T(l[i] * p2); }
    }
    if (q.gC) {
        // mu = A^T lambda, then k_freeprec_gc's formulas with (x, y, z) = Mss and the cotangent mu
        const double ux = v.a[0] * l[0] + v.a[3] * l[1] + v.a[6] * l[2];
        const double uy = v.a[1] * l[0] + v.a[4] * l[1] + v.a[7] * l[2];
        const double uz = v.a[2] * l[0] + v.a[5] * l[1] + v.a[8] * l[2];
        const bool relax = q.rest && q.T1.p, prec = q.rest && q.df.p;
        const double twopi = 6.283185307179586476925;
        const double dphi = prec ? v.e2 * (uy * rx - ux * ry) : 0.0;
        const double dE2 = relax ? ux * rx + uy * ry : 0.0;
        const double dE1 = relax ? uz * (z - 1.0) : 0.0;
        const double da1 = dE1 * v.e1, da2 = dE2 * v.e2;                       // dL/da_i, a_i = -rest / T_i
        T* o = reinterpret_cast<T*>(q.gC) + r * 4;
        o[0] = T(-twopi * v.df * dphi - da1 / v.t1 - da2 / v.t2);
        o[1] = T(da1 * v.rest / (v.t1 * v.t1));
        o[2] = T(da2 * v.rest / (v.t2 * v.t2));
        o[3] = T(-twopi * v.rest * dphi);
    }
}

// k_ab_train.hpp -- the transient of a pulse repeated K times from Hargreaves' A, B, and its adjoint (Ktr / Ktrb)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once

// =============================================================================================
// Per spin, from M_0 = Mi, for k = 0 .. K-1:
//     M-      = F M_k + f                        the rest, exactly as k_ab_steady.hpp forms it:
//                                                F = diag(E2r, E2r, E1r) Rz(-2 pi df rest), f = (0, 0, -expm1(-rest/T1))
//     M_{k+1} = Rz(phi_k) [ A Rz(-phi_k) M- + B ]   the pulse played with RF phase phi_k
// and record k is M_{k+1}, the state right after pulse k, stored time-major: Mt (K, rows, 3) -- 12 B (fp64: 24 B) per
// lane and repetition, a wave's 64 records contiguous.
// One thread per spin, blockIdx.y = the batch entry n, so that the phase table cs (N|1, K, 2) = (cos phi, sin phi) in
// fp64 is read at block-uniform addresses through the constant address space (scalar loads, no sincos in the loop).
// Whatever the data type, ALL arithmetic is fp64 and the carried state stays fp64 between repetitions; each record is
// rounded once on its store.  The rest constants (exp, expm1, sincos) are formed once per spin before the loop.
//
// Adjoint, for the cotangents G_k of the records, walking k downwards from h = 0.  It reads M_{k+1} and M_k from the
// forward's own output (M_0 = Mi): nothing else was saved and nothing is recomputed forward.
//     lambda = h + G_k,   u = Rz(-phi_k) lambda,   p = Rz(-phi_k) M-  with  M- = F M_k + f
//     grad_B += u,   grad_A += u p^T,   gM- = Rz(phi_k) A^T u
//     dL/dphi_k (this spin) = (lambda_y M_x - lambda_x M_y) at M_{k+1}  -  (gM-_y M-_x - gM-_x M-_y)
//     the rest's constants: the formulas of k_freeprec_gc (k_aux.hpp) at Mi := M_k, gMo := gM-, summed over k
//     h = F^T gM-                                   and at the end grad_Mi = h.
// Record k-2 and cotangent k-1 are requested one repetition ahead of their use.  Every sum is lane-private and runs in
// a fixed order: no LDS, no workspace, no atomics, no second pass; the same inputs give the same bits.
// =============================================================================================
struct TrainArgs {
    const void* A; const void* B;         // (rows, 3, 3), (rows, 3)
    const void* g;                        // (K, rows, 3): the cotangents of the records (adjoint only)
    const void* rest; int64_t rest_sn;    // (N|1,); null: no rest period
    Bc T1, T2, df;                        // T1.p == null: no relaxation in the rest; df.p == null: no precession
    const void* Mi; int64_t Mi_sn, Mi_sm; // (N|1, nM|1, 3), element strides; null: (0, 0, 1)
    const double* cs; int64_t cs_sn;      // (N|1, K, 2) fp64: cos phi_k, sin phi_k; null: phi = 0
    void* Mt;                             // (K, rows, 3): written by the forward, read by the adjoint
    void* gA; void* gB; void* gC;         // (rows, 3, 3), (rows, 3), (rows, 4); each may be null (adjoint only)
    void* gMi; void* gphi;                // (rows, 3), (K, rows); each may be null (adjoint only)
    int64_t rows, nM, K;
};

typedef const double __attribute__((address_space(4)))* TrainCP;

// what both kernels form per spin before their loop
struct TrainSpin {
    double rest, df, t1, t2;              // the constants as loaded (1 for an absent T)
    double c, s, e1, e2, f3;              // cos, sin of -2 pi df rest; E1r, E2r, -expm1(-rest/T1)
    double m0, m1, m2;                    // Mi
};

template <typename T>
__device__ __forceinline__ TrainSpin train_spin(const TrainArgs& q, int64_t n, int64_t sidx)
{
    TrainSpin v;
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
    v.m0 = 0.0; v.m1 = 0.0; v.m2 = 1.0;
    if (q.Mi) {
        const T* pm = reinterpret_cast<const T*>(q.Mi) + n * q.Mi_sn + sidx * q.Mi_sm;
        v.m0 = double(pm[0]); v.m1 = double(pm[1]); v.m2 = double(pm[2]);
    }
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void k_ab_train_fwd(TrainArgs q)
{
    const int64_t sidx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sidx >= q.nM) return;
    const int64_t n = blockIdx.y, r = n * q.nM + sidx;
    const TrainSpin v = train_spin<T>(q, n, sidx);
    const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
    const T* pb = reinterpret_cast<const T*>(q.B) + r * 3;
    const double a0 = double(pa[0]), a1 = double(pa[1]), a2 = double(pa[2]), a3 = double(pa[3]), a4 = double(pa[4]),
                 a5 = double(pa[5]), a6 = double(pa[6]), a7 = double(pa[7]), a8 = double(pa[8]);
    const double b0 = double(pb[0]), b1 = double(pb[1]), b2 = double(pb[2]);
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    T* o = reinterpret_cast<T*>(q.Mt) + r * 3;
    const int64_t pitch = q.rows * 3;
    double mx = v.m0, my = v.m1, mz = v.m2;
    for (int64_t k = 0; k < q.K; ++k) {
        double cp = 1.0, sp = 0.0;
        if (cs) { cp = cs[2 * k]; sp = cs[2 * k + 1]; }
        const double rx = v.c * mx - v.s * my, ry = v.s * mx + v.c * my;
        const double px = rx * v.e2, py = ry * v.e2, pz = mz * v.e1 + v.f3;          // M- = F M + f
        const double qx = cp * px + sp * py, qy = cp * py - sp * px;                 // Rz(-phi) M-
        const double tx = a0 * qx + a1 * qy + a2 * pz + b0;
        const double ty = a3 * qx + a4 * qy + a5 * pz + b1;
        mz = a6 * qx + a7 * qy + a8 * pz + b2;
        mx = cp * tx - sp * ty; my = sp * tx + cp * ty;                              // Rz(phi) (A . + B)
        o[0] = T(mx); o[1] = T(my); o[2] = T(mz);
        o += pitch;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ab_train_bwd(TrainArgs q)
{
    const int64_t sidx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sidx >= q.nM) return;
    const int64_t n = blockIdx.y, r = n * q.nM + sidx;
    const TrainSpin v = train_spin<T>(q, n, sidx);
    const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
    const double a0 = double(pa[0]), a1 = double(pa[1]), a2 = double(pa[2]), a3 = double(pa[3]), a4 = double(pa[4]),
                 a5 = double(pa[5]), a6 = double(pa[6]), a7 = double(pa[7]), a8 = double(pa[8]);
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    const int64_t pitch = q.rows * 3;
    const T* rec = reinterpret_cast<const T*>(q.Mt) + r * 3;
    const T* cot = reinterpret_cast<const T*>(q.g) + r * 3;
    T* gphi = q.gphi ? reinterpret_cast<T*>(q.gphi) + r : nullptr;
    const bool relax = q.rest && q.T1.p, prec = q.rest && q.df.p;

    double gA0 = 0, gA1 = 0, gA2 = 0, gA3 = 0, gA4 = 0, gA5 = 0, gA6 = 0, gA7 = 0, gA8 = 0;
    double gB0 = 0, gB1 = 0, gB2 = 0;
    double sphi = 0, sa1 = 0, sa2 = 0;             // sums of dL/dphi_rest, dL/da1, dL/da2 (a_i = -rest / T_i)
    double hx = 0, hy = 0, hz = 0;

    // record K-1 (M_{k+1} of the first repetition walked), record K-2 (its M_k) and cotangent K-1
    const int64_t K = q.K;
    const T* pc = rec + (K - 1) * pitch;
    double cx = double(pc[0]), cy = double(pc[1]);
    double px_ = v.m0, py_ = v.m1, pz_ = v.m2;
    if (K >= 2) { const T* pp = rec + (K - 2) * pitch; px_ = double(pp[0]); py_ = double(pp[1]); pz_ = double(pp[2]); }
    const T* pg = cot + (K - 1) * pitch;
    double gx = double(pg[0]), gy = double(pg[1]), gz = double(pg[2]);

    for (int64_t k = K - 1; k >= 0; --k) {
        // one repetition ahead: record k-2 and cotangent k-1 (indices clamped: the loads stay inside the buffers)
        const int64_t kr = k >= 2 ? k - 2 : 0, kg = k >= 1 ? k - 1 : 0;
        const T* nr = rec + kr * pitch;
        const T* ng = cot + kg * pitch;
        const T nrx = nr[0], nry = nr[1], nrz = nr[2];
        const T ngx = ng[0], ngy = ng[1], ngz = ng[2];

        double cp = 1.0, sp = 0.0;
        if (cs) { cp = cs[2 * k]; sp = cs[2 * k + 1]; }
        const double lx = hx + gx, ly = hy + gy, lz = hz + gz;                       // lambda
        const double ux = cp * lx + sp * ly, uy = cp * ly - sp * lx, uz = lz;        // u = Rz(-phi) lambda
        const double rx = v.c * px_ - v.s * py_, ry = v.s * px_ + v.c * py_;         // M_k rotated, before relaxation
        const double mmx = rx * v.e2, mmy = ry * v.e2, mmz = pz_ * v.e1 + v.f3;      // M- = F M_k + f
        const double qx = cp * mmx + sp * mmy, qy = cp * mmy - sp * mmx, qz = mmz;   // p = Rz(-phi) M-
        gB0 += ux; gB1 += uy; gB2 += uz;
        gA0 += ux * qx; gA1 += ux * qy; gA2 += ux * qz;
        gA3 += uy * qx; gA4 += uy * qy; gA5 += uy * qz;
        gA6 += uz * qx; gA7 += uz * qy; gA8 += uz * qz;
        const double wx = a0 * ux + a3 * uy + a6 * uz;                               // A^T u
        const double wy = a1 * ux + a4 * uy + a7 * uz;
        const double wz = a2 * ux + a5 * uy + a8 * uz;
        const double mx = cp * wx - sp * wy, my = sp * wx + cp * wy, mz = wz;        // gM- = Rz(phi) A^T u
        if (gphi) gphi[k * q.rows] = T((ly * cx - lx * cy) - (my * mmx - mx * mmy));
        // k_freeprec_gc's formulas with (x, y, z) = M_k and the cotangent gM-
        sphi += prec ? v.e2 * (my * rx - mx * ry) : 0.0;
        sa2 += relax ? (mx * rx + my * ry) * v.e2 : 0.0;
        sa1 += relax ? mz * (pz_ - 1.0) * v.e1 : 0.0;
        // h = F^T gM-
        hx = v.e2 * (v.c * mx + v.s * my); hy = v.e2 * (v.c * my - v.s * mx); hz = v.e1 * mz;

        cx = px_; cy = py_;
        const bool first = k < 2;                                                    // record k-2 does not exist: Mi
        px_ = first ? v.m0 : double(nrx); py_ = first ? v.m1 : double(nry); pz_ = first ? v.m2 : double(nrz);
        gx = double(ngx); gy = double(ngy); gz = double(ngz);
    }
    if (q.gB) {
        T* o = reinterpret_cast<T*>(q.gB) + r * 3;
        o[0] = T(gB0); o[1] = T(gB1); o[2] = T(gB2);
    }
    if (q.gA) {
        T* o = reinterpret_cast<T*>(q.gA) + r * 9;
        o[0] = T(gA0); o[1] = T(gA1); o[2] = T(gA2); o[3] = T(gA3); o[4] = T(gA4); o[5] = T(gA5);
        o[6] = T(gA6); o[7] = T(gA7); o[8] = T(gA8);
    }
    if (q.gC) {
        const double twopi = 6.283185307179586476925;
        T* o = reinterpret_cast<T*>(q.gC) + r * 4;
        o[0] = T(-twopi * v.df * sphi - sa1 / v.t1 - sa2 / v.t2);
        o[1] = T(sa1 * v.rest / (v.t1 * v.t1));
        o[2] = T(sa2 * v.rest / (v.t2 * v.t2));
        o[3] = T(-twopi * v.rest * sphi);
    }
    if (q.gMi) {
        T* o = reinterpret_cast<T*>(q.gMi) + r * 3;
        o[0] = T(hx); o[1] = T(hy); o[2] = T(hz);
    }
}

// Host: what the entry points of Ktr / Ktrb and of Ktrs / Ktrsb (tu_train_signal.hip) check alike, in the order of
// tu_ab_steady.hip's steady_check: dtype and sizes, the empty problem (0), null pointers and the operand rules,
// alignment.  `empty` is set for a problem without records.
inline int train_check(int dtype, const void* A, const void* B, const void* rest, const void* T1, const void* T2,
                       const void* df, const void* Mi, const void* cs, int64_t N, int64_t nM, int64_t K, bool& empty)
{
    empty = false;
    if ((dtype != MRPHY_F32 && dtype != MRPHY_F64) || N < 0 || nM < 0 || K < 0) return MRPHY_EINVAL;
    if (N * nM * K == 0) { empty = true; return 0; }
    if (N > 65535 || (nM + 255) / 256 > (int64_t)0x7fffffff) return MRPHY_EINVAL;   // blockIdx.y = n, as K0 / K2
    if (!A || !B) return MRPHY_EINVAL;
    if (!rest && (T1 || T2 || df)) return MRPHY_EINVAL;               // no rest period: nothing to relax or precess in
    if ((T1 == nullptr) != (T2 == nullptr)) return MRPHY_EINVAL;      // both or neither
    const size_t ts = tsize(dtype);
    if (!aligned_to(A, ts) || !aligned_to(B, ts) || !aligned_to(rest, ts) || !aligned_to(T1, ts) ||
        !aligned_to(T2, ts) || !aligned_to(df, ts) || !aligned_to(Mi, ts) || !aligned_to(cs, sizeof(double)))
        return MRPHY_EALIGN;
    return 0;
}

// the operands A .. cs and the sizes, as every entry point of Ktr / Ktrb and Ktrs / Ktrsb passes them on
inline void train_fill(TrainArgs& q, const void* A, const void* B, const void* rest, int64_t rest_sn, Bc T1, Bc T2, Bc df,
                       const void* Mi, int64_t Mi_sn, int64_t Mi_sm, const void* cs, int64_t cs_sn, int64_t N,
                       int64_t nM, int64_t K)
{
    q.A = A; q.B = B; q.rest = rest; q.rest_sn = rest_sn;
    q.T1 = T1; q.T2 = T2; q.df = df;
    q.Mi = Mi; q.Mi_sn = Mi_sn; q.Mi_sm = Mi_sm; q.cs = reinterpret_cast<const double*>(cs); q.cs_sn = cs_sn;
    q.rows = N * nM; q.nM = nM; q.K = K;
}

// k_sequence_steady.hpp -- the steady state of a scheduled period: Ksq's K repetitions (a pulse of a bank and a rest per
// repetition) composed into one affine map per spin and solved for its fixed point, and the first half of its adjoint
// (Ksqp / Ksqpl)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp, k_ab_train.hpp (TrainSpin,
// TrainCP), k_train_signal.hpp (train_rep) and k_ab_sequence.hpp (SeqArgs, SeqIP, seq_spin, seq_rest, seq_load_a).
// Not a standalone header.
#pragma once

// =============================================================================================
// Ksqp: repetition k of the period is Ksq's affine map (k_ab_sequence.hpp),
//     M-  = F_k M + f_k,   M' = Rz(phi_k) [ A_p Rz(-phi_k) M- + B_p ],  p = pulse_k,
// and the K of them compose to Phi(M) = Abar M + bbar.  Ksq's grid and operands: one thread per spin, 256 threads,
// blockIdx.y = the batch entry n, the tables pulse, cs, rs through scalar loads, A_p, B_p reloaded when pulse_k changes,
// seq_rest re-formed when the BITS of rest_k change.  The lane carries FOUR fp64 columns through train_rep, one refresh
// per repetition for all four: the affine column from 0 (it ends as bbar), and the three columns of I through the linear
// part alone -- train_rep with f3 = 0 and B = 0 -- which end as the columns of Abar; nothing is obtained as a
// difference.  Then (I - Abar) Mss = bbar in Kss's cofactor form (k_ab_steady.hpp: K = cof(I - Abar),
// (I - Abar)^-1 = K^T / det, ONE division, no pivot search, no indexed array), all fp64, Mss rounded once into the data
// type.  Mss is the state right after the LAST repetition of the period = the state before the rest of repetition 0:
// Kss's convention and record K-1 of Ksq started there.  A singular system (det == 0) gives non-finite values, as Kss.
// Two optional outputs, for the adjoint:
//     per (12, rows) fp64: Abar row-major in slots 0 .. 8, bbar in 9 .. 11, slot i of a wave's 64 lanes contiguous (the
//         layout of the bank workspace);
//     ck (ceil(K/S), rows, 3) fp64, S = TRS_SEG: the state before repetitions 0, S, 2S, ... of the period started at
//         the UNROUNDED fp64 Mss -- Ksqs's checkpoints, what Ksqsb's sweep reads -- written by a second walk of one
//         column in the same kernel, which stops at the last checkpoint.
// Both walks are one rolled loop (the second walk is the iterations K .. K + klast), so that the refreshes -- seq_rest's
// sincos / exp / expm1 among them -- are inlined once.  No LDS, no private segment.
//
// Ksqpl: one thread per spin, lambda = (I - Abar)^-T g = K g / det from per (the same cofactors, not transposed), fp64,
// rounded once into the data type: the cotangent of Mlast that Ksqsb's sweep (k_sequence_signal.hpp) starts from.  With
// no signal cotangent that sweep, run from ck, yields (dPhi/dtheta)^T lambda at M = Mss for every operand theta of the
// period: the gradient of the steady state.
// =============================================================================================
struct SeqSteadyArgs {
    SeqArgs s;                      // A .. cs, rows, nM, K as Ksq takes them; Mi null; g, Mt and the gradients unused
    void* Mss;                      // (rows, 3) of the data type
    double* per;                    // (12, rows) fp64: Abar row-major, then bbar; null: not wanted
    double* ck;                     // (ceil(K/S), rows, 3) fp64; null: not wanted
    const void* g;                  // Ksqpl: (rows, 3), the cotangent of Mss
    void* lam;                      // Ksqpl: (rows, 3) of the data type
};

// K = cof(C) row-major and 1 / det(C), as steady_spin (k_ab_steady.hpp) forms them: C^-1 = K^T / det, C^-T = K / det
__device__ __forceinline__ void sqp_cofactors(double c0, double c1, double c2, double c3, double c4, double c5, double c6,
                                              double c7, double c8, double& k0, double& k1, double& k2, double& k3,
                                              double& k4, double& k5, double& k6, double& k7, double& k8, double& rdet)
{
    k0 = c4 * c8 - c5 * c7;
    k1 = c5 * c6 - c3 * c8;
    k2 = c3 * c7 - c4 * c6;
    k3 = c2 * c7 - c1 * c8;
    k4 = c0 * c8 - c2 * c6;
    k5 = c1 * c6 - c0 * c7;
    k6 = c1 * c5 - c2 * c4;
    k7 = c2 * c3 - c0 * c5;
    k8 = c0 * c4 - c1 * c3;
    rdet = 1.0 / (c0 * k0 + c1 * k1 + c2 * k2);
}

template <typename T>
__global__ __launch_bounds__(256) void k_sequence_steady_fwd(SeqSteadyArgs a)
{
    const SeqArgs& q = a.s;
    const int64_t sidx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sidx >= q.nM) return;
    const int64_t n = blockIdx.y, r = n * q.nM + sidx, K = q.K;
    TrainSpin v = seq_spin<T>(q, n, sidx);
    const bool prec = q.rs && q.df.p, relax = q.rs && q.T1.p;
    const SeqIP pl = (SeqIP)q.pulse;
    const TrainCP rs = (TrainCP)(q.rs ? q.rs + n * q.rs_sn : nullptr);
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0, b0 = 0, b1 = 0, b2 = 0;
    int32_t pcur = -1;
    long long rbits = 0;
    bool rok = false;                                       // v holds the constants of the rest with the bits rbits
    double mx = 0.0, my = 0.0, mz = 0.0;                     // the affine column; in the second walk: the state
    double xx = 1.0, xy = 0.0, xz = 0.0;                     // Abar e_x
    double yx = 0.0, yy = 1.0, yz = 0.0;                     // Abar e_y
    double zx = 0.0, zy = 0.0, zz = 1.0;                     // Abar e_z
    // the second walk ends at the last checkpoint, klast = the largest multiple of S below K
    const int64_t klast = ((K - 1) / TRS_SEG) * TRS_SEG;
    const int64_t total = a.ck ? K + klast : K;
    int64_t ck_next = TRS_SEG, ck_row = 0;                   // block-uniform: the lane keeps no checkpoint pointer

    for (int64_t kk = 0; kk <= total; ++kk) {
        if (kk == K) {                                       // block-uniform: the period is composed
            // C = I - Abar (row i, column j = component i of Abar e_j), K = cof(C), Mss = K^T bbar / det
            double k0, k1, k2, k3, k4, k5, k6, k7, k8, rdet;
            sqp_cofactors(1.0 - xx, -yx, -zx, -xy, 1.0 - yy, -zy, -xz, -yz, 1.0 - zz, k0, k1, k2, k3, k4, k5, k6, k7, k8,
                          rdet);
            if (a.per) {
                double* o = a.per + r;
                const int64_t R = q.rows;
                o[0] = xx; o[R] = yx; o[2 * R] = zx; o[3 * R] = xy; o[4 * R] = yy; o[5 * R] = zy;
                o[6 * R] = xz; o[7 * R] = yz; o[8 * R] = zz; o[9 * R] = mx; o[10 * R] = my; o[11 * R] = mz;
            }
            const double s0 = (k0 * mx + k3 * my + k6 * mz) * rdet;
            const double s1 = (k1 * mx + k4 * my + k7 * mz) * rdet;
            const double s2 = (k2 * mx + k5 * my + k8 * mz) * rdet;
            T* o = reinterpret_cast<T*>(a.Mss) + r * 3;
            o[0] = T(s0); o[1] = T(s1); o[2] = T(s2);
            mx = s0; my = s1; mz = s2;
            if (a.ck) { double* c = a.ck + r * 3; c[0] = mx; c[1] = my; c[2] = mz; ck_row = q.rows; }
        }
        if (kk == total) break;
        const bool second = kk >= K;                         // block-uniform
        const int64_t k = second ? kk - K : kk;
        const int32_t p = pl ? pl[k] : 0;
        if (p != pcur) {                                     // block-uniform
            const int64_t pr = (int64_t)p * q.rows + r;      // formed per reload: the lane keeps no pointer into the bank
            seq_load_a(reinterpret_cast<const T*>(q.A) + pr * 9, a0, a1, a2, a3, a4, a5, a6, a7, a8);
            const T* b = reinterpret_cast<const T*>(q.B) + pr * 3;
            b0 = double(b[0]); b1 = double(b[1]); b2 = double(b[2]);
            pcur = p;
        }
        if (rs) {
            const double rk = rs[k];
            const long long bits = __double_as_longlong(rk);
            if (!rok || bits != rbits) { seq_rest(v, rk, prec, relax); rbits = bits; rok = true; }   // block-uniform
        }
        double cp = 1.0, sp = 0.0;
        if (cs) { cp = cs[2 * k]; sp = cs[2 * k + 1]; }
        train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, b0, b1, b2, cp, sp, mx, my, mz);
        if (!second) {
            const double f3 = v.f3;                          // the linear part: f = 0, B = 0
            v.f3 = 0.0;
            train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, 0.0, 0.0, 0.0, cp, sp, xx, xy, xz);
            train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, 0.0, 0.0, 0.0, cp, sp, yx, yy, yz);
            train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, 0.0, 0.0, 0.0, cp, sp, zx, zy, zz);
            v.f3 = f3;
        } else if (k + 1 == ck_next) {                       // block-uniform: the state before repetition ck_next
            double* c = a.ck + (ck_row + r) * 3;
            c[0] = mx; c[1] = my; c[2] = mz;
            ck_row += q.rows; ck_next += TRS_SEG;
        }
    }
}

// Ksqpl: lambda = (I - Abar)^-T g
template <typename T>
__global__ __launch_bounds__(256) void k_sequence_steady_lambda(SeqSteadyArgs a)
{
    const int64_t R = a.s.rows;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const double* p = a.per + r;
    double k0, k1, k2, k3, k4, k5, k6, k7, k8, rdet;
    sqp_cofactors(1.0 - p[0], -p[R], -p[2 * R], -p[3 * R], 1.0 - p[4 * R], -p[5 * R], -p[6 * R], -p[7 * R],
                  1.0 - p[8 * R], k0, k1, k2, k3, k4, k5, k6, k7, k8, rdet);
    const T* pg = reinterpret_cast<const T*>(a.g) + r * 3;
    const double g0 = double(pg[0]), g1 = double(pg[1]), g2 = double(pg[2]);
    T* o = reinterpret_cast<T*>(a.lam) + r * 3;
    o[0] = T((k0 * g0 + k1 * g1 + k2 * g2) * rdet);
    o[1] = T((k3 * g0 + k4 * g1 + k5 * g2) * rdet);
    o[2] = T((k6 * g0 + k7 * g1 + k8 * g2) * rdet);
}

// k_ab_sequence_jvp.hpp -- Ksqj: Ksq's records and their forward-mode tangents along up to MD directions
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp, k_ab_train.hpp,
// k_train_signal.hpp (train_rep) and k_ab_sequence.hpp (SeqArgs, seq_spin, seq_rest, seq_load_a, seq_fill).  Not a
// standalone header.
#pragma once

// =============================================================================================
// Ksqj: Ksq's frame (one thread per spin, 256 threads, blockIdx.y = the batch entry; pulse, cs, rs through scalar loads;
// A_p, B_p reloaded when pulse_k changes and the rest's constants re-formed when the bits of rest_k change, both uniform
// over the block) carrying, beside the state M, its derivative along up to MD directions.  A direction d is a set of
// tangents of the operands, each optional (null: zero): per spin dA (D, P, rows, 9), dB (D, P, rows, 3), dMi (D, rows, 3),
// dT1, dT2, ddf (D, rows) of the data type; block-uniform dphase, drest (D, N|1, K) fp64 through the constant address
// space.  The primal repetition is train_rep, called as Ksq calls it: Mt is Ksq's, bit for bit.
//
// Per repetition and direction, in fp64 (train_rep's names; m = the state before the repetition, M' the new one):
//     th' = -2 pi (df' rest_k + df rest'_k)       c' = -s th'     s' = c th'
//     e1' = e1 (rest_k T1'/T1^2 - rest'_k/T1)     f3' = -e1'      e2' = e2 (rest_k T2'/T2^2 - rest'_k/T2)
//     r'  = (c m'x - s m'y + c' mx - s' my,  c m'y + s m'x + c' my + s' mx)
//     p'  = (r'x e2 + rx e2',  r'y e2 + ry e2',  m'z e1 + mz e1' + f3')
//     q'  = (cp p'x + sp p'y + phi' qy,  cp p'y - sp p'x - phi' qx)
//     t'  = A_p (q'x, q'y, p'z) + A'_p (qx, qy, pz) + B'_p
//     M'' = (cp t'x - sp t'y - phi' M'y,  sp t'x + cp t'y + phi' M'x,  t'z)
// No transcendental function is called for a tangent: c', s', e1', e2', f3' are products of the primal's constants, formed
// per repetition (rest'_k may change while the bits of rest_k do not).  Every product holds exactly one tangent factor,
// contraction is off and every fused multiply-add is written out: a direction scaled by a power of two or negated scales
// or negates its records exactly, the zero direction gives zeros, and the arithmetic of direction d does not depend on MD
// or on what rides along.  rest_k / T^2 and 1 / T are primal numbers re-formed with the rest's constants.
// Registers: a direction keeps its state (3 fp64) and, in the DATA TYPE, dT1, dT2, ddf and the 12 numbers of A'_p, B'_p of
// the current run (widened where they are used -- exact), reloaded with A_p, B_p: an entry never played is never read.
// No LDS, no atomics, no private segment; each record is rounded once on its store; the same inputs give the same bits.
// =============================================================================================
struct SeqJvpArgs {
    int64_t D;                                            // directions given, 1 <= D <= MD
    const void *dA, *dB, *dMi, *dT1, *dT2, *ddf;
    const double* dphase; int64_t dphase_sn, dphase_sd;   // element strides over the batch entry and the direction
    const double* drest;  int64_t drest_sn, drest_sd;
    void* dMt;                                            // (D, K, rows, 3)
};

template <typename T, int MD>
__global__ __launch_bounds__(256) void k_ab_sequence_jvp(SeqArgs q, SeqJvpArgs j)
{
#pragma clang fp contract(off)
    const int64_t sidx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sidx >= q.nM) return;
    const int64_t n = blockIdx.y, r = n * q.nM + sidx;
    TrainSpin v = seq_spin<T>(q, n, sidx);
    const bool prec = q.rs && q.df.p, relax = q.rs && q.T1.p;
    const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
    const T* pb = reinterpret_cast<const T*>(q.B) + r * 3;
    const SeqIP pl = (SeqIP)q.pulse;
    const TrainCP rs = (TrainCP)(q.rs ? q.rs + n * q.rs_sn : nullptr);
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    T* o = q.Mt ? reinterpret_cast<T*>(q.Mt) + r * 3 : nullptr;
    T* od = reinterpret_cast<T*>(j.dMt) + r * 3;
    const int64_t pitch = q.rows * 3, dpitch = q.K * pitch;
    const double twopi = 6.283185307179586476925;
    // whether any direction moves the rest's constants (block-uniform)
    const bool restg = q.rs && (j.dT1 || j.dT2 || j.ddf || j.drest);

    double dmx[MD], dmy[MD], dmz[MD];
    T dt1[MD], dt2[MD], ddf[MD], da[MD][9], db[MD][3];
    TrainCP dr[MD], dp[MD];
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        const bool on = d < j.D;                          // block-uniform, as every test of a table's pointer
        const int64_t rd = d * q.rows + r;
        dmx[d] = dmy[d] = dmz[d] = 0.0;
        if (on && j.dMi) {
            const T* pm = reinterpret_cast<const T*>(j.dMi) + rd * 3;
            dmx[d] = double(pm[0]); dmy[d] = double(pm[1]); dmz[d] = double(pm[2]);
        }
        dt1[d] = dt2[d] = ddf[d] = T(0);
        if (on && j.dT1) dt1[d] = reinterpret_cast<const T*>(j.dT1)[rd];
        if (on && j.dT2) dt2[d] = reinterpret_cast<const T*>(j.dT2)[rd];
        if (on && j.ddf) ddf[d] = reinterpret_cast<const T*>(j.ddf)[rd];
#pragma unroll
        for (int i = 0; i < 9; ++i) da[d][i] = T(0);
#pragma unroll
        for (int i = 0; i < 3; ++i) db[d][i] = T(0);
        dr[d] = (TrainCP)(on && j.drest ? j.drest + d * j.drest_sd + n * j.drest_sn : nullptr);
        dp[d] = (TrainCP)(on && j.dphase ? j.dphase + d * j.dphase_sd + n * j.dphase_sn : nullptr);
    }

    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0, b0 = 0, b1 = 0, b2 = 0;
    double ka1 = 0, kb1 = 0, ka2 = 0, kb2 = 0;            // rest / T1^2, 1 / T1, rest / T2^2, 1 / T2 (0 without relaxation)
    int32_t pcur = -1;
    long long rbits = 0;
    double mx = v.m0, my = v.m1, mz = v.m2;
    for (int64_t k = 0; k < q.K; ++k) {
        const int32_t p = pl ? pl[k] : 0;
        if (p != pcur) {                                     // block-uniform
            seq_load_a(pa + (int64_t)p * q.rows * 9, a0, a1, a2, a3, a4, a5, a6, a7, a8);
            const T* b = pb + (int64_t)p * q.rows * 3;
            b0 = double(b[0]); b1 = double(b[1]); b2 = double(b[2]);
#pragma unroll
            for (int d = 0; d < MD; ++d) {
                if (d < j.D && j.dA) {
                    const T* t = reinterpret_cast<const T*>(j.dA) + ((d * q.P + p) * q.rows + r) * 9;
#pragma unroll
                    for (int i = 0; i < 9; ++i) da[d][i] = t[i];
                }
                if (d < j.D && j.dB) {
                    const T* t = reinterpret_cast<const T*>(j.dB) + ((d * q.P + p) * q.rows + r) * 3;
#pragma unroll
                    for (int i = 0; i < 3; ++i) db[d][i] = t[i];
                }
            }
            pcur = p;
        }
        if (rs) {
            const double rk = rs[k];
            const long long bits = __double_as_longlong(rk);
            if (k == 0 || bits != rbits) {                   // block-uniform
                seq_rest(v, rk, prec, relax);
                if (relax && restg) {
                    kb1 = 1.0 / v.t1; kb2 = 1.0 / v.t2;
                    ka1 = v.rest / (v.t1 * v.t1); ka2 = v.rest / (v.t2 * v.t2);
                }
                rbits = bits;
            }
        }
        double cp = 1.0, sp = 0.0;
        if (cs) { cp = cs[2 * k]; sp = cs[2 * k + 1]; }
        const double ox = mx, oy = my, oz = mz;              // the state before the repetition
        train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, b0, b1, b2, cp, sp, mx, my, mz);
        if (o) { o[0] = T(mx); o[1] = T(my); o[2] = T(mz); o += pitch; }
        // the primal's intermediates, train_rep's expressions
        const double rx = fma(v.c, ox, -(v.s * oy)), ry = fma(v.c, oy, v.s * ox);
        const double px = rx * v.e2, py = ry * v.e2, pz = fma(oz, v.e1, v.f3);
        const double qx = fma(sp, py, cp * px), qy = fma(cp, py, -(sp * px));
#pragma unroll
        for (int d = 0; d < MD; ++d) {
            if (d < j.D) {                                   // block-uniform
                const double drk = dr[d] ? dr[d][k] : 0.0, dph = dp[d] ? dp[d][k] : 0.0;
                double dc = 0.0, ds = 0.0, de1 = 0.0, de2 = 0.0;
                if (restg) {
                    const double thd = -twopi * fma(double(ddf[d]), v.rest, v.df * drk);
                    dc = -(v.s * thd); ds = v.c * thd;
                    de1 = v.e1 * fma(ka1, double(dt1[d]), -(kb1 * drk));
                    de2 = v.e2 * fma(ka2, double(dt2[d]), -(kb2 * drk));
                }
                const double drx = fma(v.c, dmx[d], fma(-v.s, dmy[d], fma(dc, ox, -(ds * oy))));
                const double dry = fma(v.c, dmy[d], fma(v.s, dmx[d], fma(dc, oy, ds * ox)));
                const double dpx = fma(drx, v.e2, rx * de2), dpy = fma(dry, v.e2, ry * de2);
                const double dpz = fma(dmz[d], v.e1, fma(oz, de1, -de1));
                const double dqx = fma(cp, dpx, fma(sp, dpy, dph * qy));
                const double dqy = fma(cp, dpy, fma(-sp, dpx, -(dph * qx)));
                const double tx = fma(a0, dqx, fma(a1, dqy, fma(a2, dpz, fma(double(da[d][0]), qx,
                                  fma(double(da[d][1]), qy, fma(double(da[d][2]), pz, double(db[d][0])))))));
                const double ty = fma(a3, dqx, fma(a4, dqy, fma(a5, dpz, fma(double(da[d][3]), qx,
                                  fma(double(da[d][4]), qy, fma(double(da[d][5]), pz, double(db[d][1])))))));
                const double tz = fma(a6, dqx, fma(a7, dqy, fma(a8, dpz, fma(double(da[d][6]), qx,
                                  fma(double(da[d][7]), qy, fma(double(da[d][8]), pz, double(db[d][2])))))));
                dmx[d] = fma(cp, tx, fma(-sp, ty, -(dph * my)));
                dmy[d] = fma(sp, tx, fma(cp, ty, dph * mx));
                dmz[d] = tz;
                T* w = od + d * dpitch;
                w[0] = T(dmx[d]); w[1] = T(dmy[d]); w[2] = T(dmz[d]);
            }
        }
        od += pitch;
    }
}

// Host: the launch at capacity MD of a call that mrphy_ab_sequence_jvp_fwd has checked
template <int MD, typename T>
int launch_seq_jvp(const SeqJvpCall& c, hipStream_t st)
{
    if (c.D < 1 || c.D > MD) return MRPHY_EINVAL;
    SeqArgs q{};
    seq_fill(q, c.A, c.B, c.P, c.pulse, c.rs, c.rs_sn, c.T1, c.T2, c.df, c.Mi, c.Mi_sn, c.Mi_sm, c.cs, c.cs_sn, c.N, c.nM,
             c.K);
    q.Mt = c.Mt;
    SeqJvpArgs j{};
    j.D = c.D;
    j.dA = c.dA; j.dB = c.dB; j.dMi = c.dMi; j.dT1 = c.dT1; j.dT2 = c.dT2; j.ddf = c.ddf;
    j.dphase = reinterpret_cast<const double*>(c.dphase); j.dphase_sn = c.dphase_sn;
    j.dphase_sd = (c.dphase_sn ? c.N : 1) * c.K;
    j.drest = reinterpret_cast<const double*>(c.drest); j.drest_sn = c.drest_sn;
    j.drest_sd = (c.drest_sn ? c.N : 1) * c.K;
    j.dMt = c.dMt;
    const dim3 grid((unsigned)((c.nM + 255) / 256), (unsigned)c.N);
    hipLaunchKernelGGL((k_ab_sequence_jvp<T, MD>), grid, dim3(256), 0, st, q, j);
    return launch_status();
}

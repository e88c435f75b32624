// k_ab_sequence.hpp -- a train whose repetitions each play one pulse of a bank after a rest of their own, from
// Hargreaves' A, B, and its adjoint (Ksq / Ksqb)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp, k_ab_train.hpp (TrainSpin,
// TrainCP, train_check) and k_train_signal.hpp (train_rep).  Not a standalone header.
#pragma once

// =============================================================================================
// Ksq: Ktr's recursion (k_ab_train.hpp) with a schedule.  Per spin, from M_0 = Mi, for k = 0 .. K-1:
//     M-      = F_k M_k + f_k                                  the rest of duration rest_k, formed as train_spin forms it
//     M_{k+1} = Rz(phi_k) [ A_p Rz(-phi_k) M- + B_p ],  p = pulse_k    entry p of the bank A (P, rows, 3, 3), B (P, rows, 3)
// and record k is M_{k+1}, stored time-major: Mt (K, rows, 3).  One thread per spin, blockIdx.y = the batch entry n, 256
// threads, as Ktr.  Three block-uniform tables come through the constant address space (scalar loads): the int32
// pulse (K,), the fp64 cs (N|1, K, 2) = (cos phi, sin phi) and the fp64 rs (N|1, K), the rest durations -- the operand
// rounded to the data type and widened, the number Ktr's double(T) sees.  The lane reloads its 12 numbers of A_p, B_p
// when pulse_k differs from pulse_{k-1}, and re-forms c, s, e1, e2, f3 (seq_rest: train_spin's sincos / exp / expm1 on
// the same products) when the BITS of rest_k differ from those of rest_{k-1}; both conditions are uniform over the
// block, and a run of equal repetitions costs what Ktr's loop costs.  The repetition itself is train_rep: the state has
// Ktr's bits.  All arithmetic fp64, the state carried in fp64, each record rounded once on its store.
//
// Ksqb: Ktrb's sweep down the repetitions, the states read from Mt itself (M_0 = Mi), record k-2 and cotangent k-1
// requested one repetition ahead at clamped indices; A_{pulse_k} and the constants of rest_k refreshed by the same two
// uniform conditions (against repetition k+1, the one walked before).  Per repetition, with Ktrb's names,
//     dphi_k = e2 (gM-_y rx - gM-_x ry),   da2_k = (gM-_x rx + gM-_y ry) e2,   da1_k = gM-_z (M_k,z - 1) e1
//     grad_rest (K, rows)[k] = -2 pi df dphi_k - da1_k / T1 - da2_k / T2        per spin, Ktrb's dL/d rest not summed
//     grad_consts (rows, 3)  = [ sum_k da1_k rest_k / T1^2,  sum_k da2_k rest_k / T2^2,  -2 pi sum_k rest_k dphi_k ]
// grad_phase (K, rows) and grad_Mi as Ktrb.  The 12 fp64 accumulators of grad_A, grad_B belong to the bank entry of the
// current run: when pulse_k changes they are added into the lane's OWN slots of the fp64 workspace (P, 12, rows) --
// read-modify-write on memory no other lane touches, no atomics, a fixed order -- and cleared; the workspace is cleared
// by the entry point beforehand.  (P, 12, rows): slot (p, i) of a wave's 64 lanes is 512 contiguous bytes; (P, rows, 12)
// would put the lanes 96 B apart, 12 partial lines per access.  A second pass (k_ab_sequence_p2) rounds once into the
// data type and thereby writes zeros for the entries never played.  The same inputs give the same bits.
// Registers: the fp64 sincos / exp / expm1 of seq_rest are inlined into loops that hold the rest of the state, so Ksq
// needs 118 - 120 VGPRs (Ktr 46 - 48: both four waves per SIMD or more) and Ksqb, with its 12 accumulators, A and the
// sweep's state live across them, 176 (fp32) / 182 (fp64) where Ktrb needs 126 - 128: two waves per SIMD instead of
// four.  No LDS, no private segment (a call out of line would cost one: 112 B per lane).  A build that holds no pointer
// per lane, refreshes before the loads ahead and reads Mi again reaches 166 / 168 and three waves, and was SLOWER on
// the device (fp32 0.56 against 0.49 ms at 64^3 x 256 without a schedule): the sweep is bound by its loads' latency and
// the addresses formed per use cost more than the third wave hides.
// =============================================================================================
struct SeqArgs {
    const void* A; const void* B;         // (P, rows, 3, 3), (P, rows, 3)
    const int32_t* pulse; int64_t P;      // (K,) int32; null: all zeros (P == 1)
    const double* rs; int64_t rs_sn;      // (N|1, K) fp64; null: no rest period
    const void* g;                        // (K, rows, 3): the cotangents of the records (adjoint only)
    Bc T1, T2, df;
    const void* Mi; int64_t Mi_sn, Mi_sm;
    const double* cs; int64_t cs_sn;
    void* Mt;
    void* gC; void* grest; void* gMi; void* gphi;   // (rows, 3), (K, rows), (rows, 3), (K, rows); each may be null
    double* work;                         // (P, 12, rows) fp64; null: neither grad_A nor grad_B is wanted
    int64_t rows, nM, K;
};

typedef const int32_t __attribute__((address_space(4)))* SeqIP;

// what train_spin loads of the spin, without a rest: the constants of a rest of duration 0
template <typename T>
__device__ __forceinline__ TrainSpin seq_spin(const SeqArgs& q, int64_t n, int64_t sidx)
{
    TrainSpin v;
    v.rest = 0.0; v.df = 0.0; v.t1 = 1.0; v.t2 = 1.0;
    v.c = 1.0; v.s = 0.0; v.e1 = 1.0; v.e2 = 1.0; v.f3 = 0.0;
    if (q.rs) {
        if (q.df.p) v.df = double(bc_load<T>(q.df, n, sidx));
        if (q.T1.p) { v.t1 = double(bc_load<T>(q.T1, n, sidx)); v.t2 = double(bc_load<T>(q.T2, n, sidx)); }
    }
    v.m0 = 0.0; v.m1 = 0.0; v.m2 = 1.0;
    if (q.Mi) {
        const T* pm = reinterpret_cast<const T*>(q.Mi) + n * q.Mi_sn + sidx * q.Mi_sm;
        v.m0 = double(pm[0]); v.m1 = double(pm[1]); v.m2 = double(pm[2]);
    }
    return v;
}

// c, s, e1, e2, f3 of a rest of duration `rest`: train_spin's expressions
__device__ __forceinline__ void seq_rest(TrainSpin& v, double rest, bool prec, bool relax)
{
    v.rest = rest;
    if (prec) sincos(-6.283185307179586476925 * v.df * v.rest, &v.s, &v.c);
    if (relax) {
        const double a1 = -v.rest / v.t1;
        v.e1 = exp(a1); v.f3 = -expm1(a1); v.e2 = exp(-v.rest / v.t2);
    }
}

template <typename T>
__device__ __forceinline__ void seq_load_a(const T* pa, double& a0, double& a1, double& a2, double& a3, double& a4,
                                           double& a5, double& a6, double& a7, double& a8)
{
    a0 = double(pa[0]); a1 = double(pa[1]); a2 = double(pa[2]); a3 = double(pa[3]); a4 = double(pa[4]);
    a5 = double(pa[5]); a6 = double(pa[6]); a7 = double(pa[7]); a8 = double(pa[8]);
}

template <typename T>
__global__ __launch_bounds__(256) void k_ab_sequence_fwd(SeqArgs q)
{
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
    T* o = reinterpret_cast<T*>(q.Mt) + r * 3;
    const int64_t pitch = q.rows * 3;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0, b0 = 0, b1 = 0, b2 = 0;
    int32_t pcur = -1;
    long long rbits = 0;
    double mx = v.m0, my = v.m1, mz = v.m2;
    for (int64_t k = 0; k < q.K; ++k) {
        const int32_t p = pl ? pl[k] : 0;
        if (p != pcur) {                                     // block-uniform
            seq_load_a(pa + (int64_t)p * q.rows * 9, a0, a1, a2, a3, a4, a5, a6, a7, a8);
            const T* b = pb + (int64_t)p * q.rows * 3;
            b0 = double(b[0]); b1 = double(b[1]); b2 = double(b[2]);
            pcur = p;
        }
        if (rs) {
            const double rk = rs[k];
            const long long bits = __double_as_longlong(rk);
            if (k == 0 || bits != rbits) { seq_rest(v, rk, prec, relax); rbits = bits; }   // block-uniform
        }
        double cp = 1.0, sp = 0.0;
        if (cs) { cp = cs[2 * k]; sp = cs[2 * k + 1]; }
        train_rep(v, a0, a1, a2, a3, a4, a5, a6, a7, a8, b0, b1, b2, cp, sp, mx, my, mz);
        o[0] = T(mx); o[1] = T(my); o[2] = T(mz);
        o += pitch;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ab_sequence_bwd(SeqArgs q)
{
    const int64_t sidx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (sidx >= q.nM) return;
    const int64_t n = blockIdx.y, r = n * q.nM + sidx;
    TrainSpin v = seq_spin<T>(q, n, sidx);
    const bool prec = q.rs && q.df.p, relax = q.rs && q.T1.p;
    const T* pa = reinterpret_cast<const T*>(q.A) + r * 9;
    const SeqIP pl = (SeqIP)q.pulse;
    const TrainCP rs = (TrainCP)(q.rs ? q.rs + n * q.rs_sn : nullptr);
    const TrainCP cs = (TrainCP)(q.cs ? q.cs + n * q.cs_sn : nullptr);
    const int64_t pitch = q.rows * 3;
    const T* rec = reinterpret_cast<const T*>(q.Mt) + r * 3;
    const T* cot = reinterpret_cast<const T*>(q.g) + r * 3;
    T* gphi = q.gphi ? reinterpret_cast<T*>(q.gphi) + r : nullptr;
    T* grest = q.grest ? reinterpret_cast<T*>(q.grest) + r : nullptr;
    double* wk = q.work ? q.work + r : nullptr;
    const double twopi = 6.283185307179586476925;

    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0;
    double gA0 = 0, gA1 = 0, gA2 = 0, gA3 = 0, gA4 = 0, gA5 = 0, gA6 = 0, gA7 = 0, gA8 = 0;
    double gB0 = 0, gB1 = 0, gB2 = 0;
    double sphi = 0, sa1 = 0, sa2 = 0;             // sums of rest_k dphi_k, rest_k da1_k, rest_k da2_k
    double hx = 0, hy = 0, hz = 0;
    int32_t pcur = -1;
    long long rbits = 0;

    // add the accumulators into the lane's slots of bank entry pcur and clear them
    auto flush = [&]() {
        double* w = wk + (int64_t)pcur * 12 * q.rows;
        const int64_t R = q.rows;
        w[0] += gA0; w[R] += gA1; w[2 * R] += gA2; w[3 * R] += gA3; w[4 * R] += gA4; w[5 * R] += gA5;
        w[6 * R] += gA6; w[7 * R] += gA7; w[8 * R] += gA8; w[9 * R] += gB0; w[10 * R] += gB1; w[11 * R] += gB2;
        gA0 = gA1 = gA2 = gA3 = gA4 = gA5 = gA6 = gA7 = gA8 = 0.0;
        gB0 = gB1 = gB2 = 0.0;
    };

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

        const int32_t p = pl ? pl[k] : 0;
        if (p != pcur) {                                     // block-uniform
            if (wk && pcur >= 0) flush();
            seq_load_a(pa + (int64_t)p * q.rows * 9, a0, a1, a2, a3, a4, a5, a6, a7, a8);
            pcur = p;
        }
        if (rs) {
            const double rk = rs[k];
            const long long bits = __double_as_longlong(rk);
            if (k == K - 1 || bits != rbits) { seq_rest(v, rk, prec, relax); rbits = bits; }   // block-uniform
        }
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
        // k_freeprec_gc's formulas with (x, y, z) = M_k and the cotangent gM-, per repetition
        const double dphi = prec ? v.e2 * (my * rx - mx * ry) : 0.0;
        const double da2 = relax ? (mx * rx + my * ry) * v.e2 : 0.0;
        const double da1 = relax ? mz * (pz_ - 1.0) * v.e1 : 0.0;
        if (grest) grest[k * q.rows] = T(-twopi * v.df * dphi - da1 / v.t1 - da2 / v.t2);
        sphi += v.rest * dphi; sa1 += v.rest * da1; sa2 += v.rest * da2;
        // h = F^T gM-
        hx = v.e2 * (v.c * mx + v.s * my); hy = v.e2 * (v.c * my - v.s * mx); hz = v.e1 * mz;

        cx = px_; cy = py_;
        const bool first = k < 2;                                                    // record k-2 does not exist: Mi
        px_ = first ? v.m0 : double(nrx); py_ = first ? v.m1 : double(nry); pz_ = first ? v.m2 : double(nrz);
        gx = double(ngx); gy = double(ngy); gz = double(ngz);
    }
    if (wk) flush();
    if (q.gC) {
        T* o = reinterpret_cast<T*>(q.gC) + r * 3;
        o[0] = T(sa1 / (v.t1 * v.t1));
        o[1] = T(sa2 / (v.t2 * v.t2));
        o[2] = T(-twopi * sphi);
    }
    if (q.gMi) {
        T* o = reinterpret_cast<T*>(q.gMi) + r * 3;
        o[0] = T(hx); o[1] = T(hy); o[2] = T(hz);
    }
}

// Pass 2: the workspace (P, 12, rows) fp64 rounded once into grad_A (P, rows, 3, 3) and grad_B (P, rows, 3); one
// thread per (entry, row), reads lane-contiguous per slot.  Either output may be null.
template <typename T>
__global__ __launch_bounds__(256) void k_ab_sequence_p2(const double* work, T* gA, T* gB, int64_t rows)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int64_t p = blockIdx.y;
    const double* w = work + p * 12 * rows + r;
    if (gA) {
        T* o = gA + (p * rows + r) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) o[i] = T(w[i * rows]);
    }
    if (gB) {
        T* o = gB + (p * rows + r) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = T(w[(9 + i) * rows]);
    }
}

// Host: what the entry points of Ksq / Ksqb, Ksqs / Ksqsb (tu_sequence_signal.hip) and Ksqp (tu_sequence_steady.hip)
// check alike, in train_check's order: dtype and sizes (P among them), the empty problem (0), null pointers and the
// operand rules; `align` is what train_check found of misaligned pointers, to be returned after the caller's own null
// checks.  `period`: the steady state's rules -- Mi is null, only a problem without spins is empty, and a period needs a
// repetition.
inline int seq_check(int dtype, const void* A, const void* B, int64_t P, const void* pulse, const void* rs,
                     const void* T1, const void* T2, const void* df, const void* Mi, const void* cs, int64_t N,
                     int64_t nM, int64_t K, bool period, bool& empty, int& align)
{
    align = 0;
    const int e = train_check(dtype, A, B, rs, T1, T2, df, Mi, cs, N, nM, K, empty);
    if (e == MRPHY_EINVAL || P < 1 || P > 65535) return MRPHY_EINVAL;           // blockIdx.y = p in the bank's second pass
    if (period) empty = N * nM == 0;
    if (empty) return 0;
    if (period && K < 1) return MRPHY_EINVAL;                                   // a period needs a repetition
    if (!pulse && P > 1) return MRPHY_EINVAL;
    align = (e || !aligned_to(rs, sizeof(double)) || !aligned_to(pulse, sizeof(int32_t))) ? MRPHY_EALIGN : 0;
    return 0;
}

// the operands A .. cs and the sizes, as every entry point of the sequence family passes them on
inline void seq_fill(SeqArgs& q, const void* A, const void* B, int64_t P, const void* pulse, const void* rs,
                     int64_t rs_sn, Bc T1, Bc T2, Bc df, const void* Mi, int64_t Mi_sn, int64_t Mi_sm, const void* cs,
                     int64_t cs_sn, int64_t N, int64_t nM, int64_t K)
{
    q.A = A; q.B = B; q.P = P; q.pulse = reinterpret_cast<const int32_t*>(pulse);
    q.rs = reinterpret_cast<const double*>(rs); q.rs_sn = rs_sn;
    q.T1 = T1; q.T2 = T2; q.df = df;
    q.Mi = Mi; q.Mi_sn = Mi_sn; q.Mi_sm = Mi_sm; q.cs = reinterpret_cast<const double*>(cs); q.cs_sn = cs_sn;
    q.rows = N * nM; q.nM = nM; q.K = K;
}

// the fp64 workspace (P, 12, rows) of the bank's gradients
inline size_t seq_bank_bytes(int64_t P, int64_t N, int64_t nM) { return (size_t)P * 12 * (size_t)(N * nM) * sizeof(double); }

// the bank's second pass: the workspace rounded once into grad_A, grad_B (either may be null).  A template (W is double)
// only so that a unit which never calls it -- tu_sequence_steady.hip -- does not instantiate the two kernels.
template <typename W>
int seq_launch_bank_p2(int dtype, const W* work, void* grad_A, void* grad_B, int64_t rows, int64_t P, hipStream_t st)
{
    const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)P);
    if (dtype == MRPHY_F32)
        hipLaunchKernelGGL((k_ab_sequence_p2<float>), grid, dim3(256), 0, st, work, (float*)grad_A, (float*)grad_B, rows);
    else
        hipLaunchKernelGGL((k_ab_sequence_p2<double>), grid, dim3(256), 0, st, work, (double*)grad_A, (double*)grad_B, rows);
    return launch_status();
}

// k_rfgr2beff_bwd.hpp -- adjoint of K0 (rfgr2beff) to rf, gr
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once

// ---------------------------------------------------------------------------------------------
// Adjoint of K0 w.r.t. rf, gr: deterministic two-pass reduction over spins.
// Pass 1: block (time tile, spin group, batch*coil): thread = one time point, loops over the
// group's spins in order; partial sums -> work[(sg, n, 5, nC', nT)].  Pass 2: fixed-order sum.
// Rows of `work` per (sg, n): [gr_x, gr_y, gr_z, rf_r[c]..., rf_i[c]...].
// ---------------------------------------------------------------------------------------------
constexpr int BWD_GROUP = 256;        // spins per LDS sub-block of the K0-adjoint pass 1

template <typename T>
struct BeffBwdArgs {
    const T* gB;      // (N, nM, nT, 3)
    const T* loc;     // (N, nM, 3)
    const T* b1;      // (N, nM, 2, nC) or null
    T* work;          // (nSG, N, 3 + 2 nC, nT)
    T* grf;           // (N, 2, nT, nC) or null
    T* ggr;           // (N, 3, nT) or null
    int64_t N, nM, nT, nC, nSG, spins_per_group;
};

// Pass 1, single-coil fast path.  Thread = VW consecutive elements e = 3t + c of the (t, xyz) axis
// (one 16-B load per spin, fully coalesced), three running sums per element over the group's spins:
//   c = 0 or 1 (gBx / gBy):  (b1r*g, b1i*g, 0)          c = 2 (gBz):  (lx*g, ly*g, lz*g)
// written to work[(sg, n, k, e)], k = 0..2.  Pass 2 combines them per time point:
//   grad_gr[i][t] = A_i(t,2);  grad_rf_re[t] = A_0(t,0) + A_1(t,1);  grad_rf_im[t] = A_0(t,1) - A_1(t,0)
template <typename T, int VW>
__global__ __launch_bounds__(256) void k_rfgr2beff_bwd_p1v(BeffBwdArgs<T> a)
{
    const int64_t L = 3 * a.nT;
    const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VW;
    const int64_t sg = blockIdx.y, n = blockIdx.z;
    const int64_t s0 = sg * a.spins_per_group;
    const int64_t s1 = (s0 + a.spins_per_group < a.nM) ? s0 + a.spins_per_group : a.nM;
    // the per-spin operands go through LDS, BWD_GROUP spins at a time, so that the row loop has
    // nothing but the gB stream in it and can keep U loads in flight per thread
    __shared__ T sp[BWD_GROUP][8];                     // lx, ly, lz, b1r, b1i
    const bool active = e0 < L;
    const bool fullv = e0 + VW <= L;                   // else: this thread straddles the row end
    bool isz[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) isz[j] = ((e0 + j) % 3) == 2;
    T acc0[VW], acc1[VW], acc2[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) acc0[j] = acc1[j] = acc2[j] = T(0);
    constexpr int U = 8;
    auto accumulate = [&](const T* q, const T* g) {
        const T lx = q[0], ly = q[1], lz = q[2], br = q[3], bi = q[4];
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            acc0[j] += (isz[j] ? lx : br) * g[j];
            acc1[j] += (isz[j] ? ly : bi) * g[j];
            acc2[j] += (isz[j] ? lz : T(0)) * g[j];
        }
    };
    for (int64_t sb = s0; sb < s1; sb += BWD_GROUP) {
        const int64_t cnt = (s1 - sb < BWD_GROUP) ? s1 - sb : BWD_GROUP;
        __syncthreads();                               // previous sub-block consumed
        for (int64_t i = threadIdx.x; i < cnt; i += 256) {
            const int64_t row = n * a.nM + sb + i;
            sp[i][0] = a.loc[row * 3]; sp[i][1] = a.loc[row * 3 + 1]; sp[i][2] = a.loc[row * 3 + 2];
            sp[i][3] = a.b1 ? a.b1[row * 2] : T(1);
            sp[i][4] = a.b1 ? a.b1[row * 2 + 1] : T(0);
        }
        __syncthreads();
        if (!active) continue;
        const T* src0 = a.gB + (n * a.nM + sb) * L + e0;
        int64_t i = 0;
        if (VW == V16<T>::N && fullv) {
            for (; i + U <= cnt; i += U) {             // U rows' loads issued before the first use
                typename V16<T>::type v[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    v[u] = __builtin_nontemporal_load(
                        reinterpret_cast<const typename V16<T>::utype*>(src0 + (i + u) * L));
#pragma unroll
                for (int u = 0; u < U; ++u) {          // same order as a plain loop: same sums
                    T g[VW];
                    vec_unpack(v[u], g);
                    accumulate(sp[i + u], g);
                }
            }
        }
        for (; i < cnt; ++i) {
            T g[VW];
            const T* src = src0 + i * L;
            if (VW == V16<T>::N && fullv) {
                vec_unpack(__builtin_nontemporal_load(
                               reinterpret_cast<const typename V16<T>::utype*>(src)), g);
            } else {
#pragma unroll
                for (int j = 0; j < VW; ++j) g[j] = (e0 + j < L) ? src[j] : T(0);
            }
            accumulate(sp[i], g);
        }
    }
    if (!active) return;
    T* w = a.work + ((sg * a.N + n) * 3) * L;
#pragma unroll
    for (int j = 0; j < VW; ++j)
        if (e0 + j < L) { w[e0 + j] = acc0[j]; w[L + e0 + j] = acc1[j]; w[2 * L + e0 + j] = acc2[j]; }
}

template <typename T>
__global__ __launch_bounds__(256) void k_rfgr2beff_bwd_p2v(BeffBwdArgs<T> a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = blockIdx.z;
    if (t >= a.nT) return;
    const int64_t L = 3 * a.nT;
    T A[3][3];                                         // A[k][c]
#pragma unroll
    for (int kk = 0; kk < 3; ++kk)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[kk][c] = T(0);
    for (int64_t sg = 0; sg < a.nSG; ++sg) {           // fixed order: deterministic
        const T* w = a.work + ((sg * a.N + n) * 3) * L + 3 * t;
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
#pragma unroll
            for (int c = 0; c < 3; ++c) A[kk][c] += w[kk * L + c];
    }
    if (a.ggr) {
        a.ggr[(n * 3 + 0) * a.nT + t] = A[0][2];
        a.ggr[(n * 3 + 1) * a.nT + t] = A[1][2];
        a.ggr[(n * 3 + 2) * a.nT + t] = A[2][2];
    }
    if (a.grf) {                                        // nC == 1
        a.grf[(n * 2 + 0) * a.nT + t] = A[0][0] + A[1][1];
        a.grf[(n * 2 + 1) * a.nT + t] = A[0][1] - A[1][0];
    }
}

// NE consecutive elements, element-aligned, non-temporal, in the widest pieces (16 B, 8 B, one element):
// a 3- or 6-element vector type would not do -- clang widens a 3-vector load to 4 elements, which at the
// last time point of the last row reads past the tensor
template <typename T, int NE>
struct ElemRun { T v[NE]; };
template <typename T, int NE>
__device__ __forceinline__ ElemRun<T, NE> load_run_nt(const T* p)
{
    ElemRun<T, NE> r;
    constexpr int VE = V16<T>::N;
    constexpr int NV = NE / VE;
#pragma unroll
    for (int v = 0; v < NV; ++v)
        vec_unpack(__builtin_nontemporal_load(reinterpret_cast<const typename V16<T>::utype*>(p + v * VE)), r.v + v * VE);
    constexpr int E1 = NV * VE;
    if constexpr (sizeof(T) == 4 && NE - E1 >= 2) {
        const f32x2 h = __builtin_nontemporal_load(reinterpret_cast<const f32x2_u*>(p + E1));
        r.v[E1] = T(h.x); r.v[E1 + 1] = T(h.y);
#pragma unroll
        for (int e = E1 + 2; e < NE; ++e) r.v[e] = __builtin_nontemporal_load(p + e);
    } else {
#pragma unroll
        for (int e = E1; e < NE; ++e) r.v[e] = __builtin_nontemporal_load(p + e);
    }
    return r;
}

// =============================================================================================
// K0 adjoint for parallel transmit (2..32 coils with a b1 map; more coils in blocks of 32), round 3: a thread
// owns a whole TIME POINT and keeps exactly the sums its gradient has, 2 MC for grad_rf (re, im per coil) and 3
// for grad_gr:
//     gRe[c] += b1r[c] gBx + b1i[c] gBy      gIm[c] += b1r[c] gBy - b1i[c] gBx      gG[i] += loc[i] gBz
// 4 MC + 3 FMAs per time point (round 2's element-per-thread pass ran 6 MC, and read its coefficients from LDS).
// A row's b1 and loc are wave-uniform, so they belong in SGPRs: a v_fmac whose source is an SGPR runs at the
// full rate, one with a DPP source (the first version of this pass) at HALF the rate (round 3:
// profiles/r03_valu_operand_rates.txt; v_mov_dpp or v_readlane in front of plain FMAs cost 14-19 cycles each).
// A small pre-pass (k_pack_coefs) writes them once, zero-padded, to pk[row][2 MC + 4] =
// [b1r 0..MC-1 | b1i 0..MC-1 | loc x y z, 0] in the workspace; the main pass reads a row with scalar
// loads (constant address space: s_load_dwordx16, batched, all in bounds thanks to the padding) and
// every FMA takes its coefficient straight from an SGPR.  No LDS, no barriers, no inline asm.  The
// capacities are fine-grained (4, 8, 12, 16, 24, 32: no LDS or register tile depends on them here), so
// a coil count pays for at most a third more coils than it has.  (Skipping the coil groups beyond nC
// with wave-uniform branches inside ONE 32-coil build was tried first: the compiler sinks the scalar
// loads into the branches, three exposed scalar-load round trips per row.)  Output: work[(sg, n, 3 + 2 nC, nT)]
// -- the layout of the generic pass 2, which sums the spin groups in fixed order: deterministic, no atomics.
// =============================================================================================
template <typename T>
struct PackArgs {
    const T* b1; const T* loc; T* pk;
    int64_t rows, nC; int MC;
    int64_t c0, nCtot;      // this block of coils: c0 .. c0 + nC - 1 of nCtot (round 4: coil counts above 32 in blocks)
};
template <typename T>
__global__ __launch_bounds__(256) void k_pack_coefs(PackArgs<T> a)
{
    const int PW = 2 * a.MC + 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.rows * PW) return;
    const int64_t r = i / PW;
    const int k = (int)(i - r * PW);
    const int part = k >= a.MC, c = k - part * a.MC;
    T v = T(0);
    if (k < 2 * a.MC) { if (c < a.nC) v = a.b1[r * 2 * a.nCtot + part * a.nCtot + a.c0 + c]; }
    else if (k < 2 * a.MC + 3) v = a.loc[r * 3 + (k - 2 * a.MC)];
    a.pk[i] = v;
}

template <typename T>
struct BeffBwdPkArgs {
    const T* gB;      // (N, nM, nT, 3)
    const T* pk;      // (N nM, 2 MC + 4): packed coefficient rows
    T* work;          // (nSG, N, 3 + 2 nCtot, nT)
    int64_t N, nM, nT, nC, spins_per_group;
    int K, rowR, rowI;    // workspace rows per (spin group, n): K = 3 + 2 nCtot; this block's coil c -> rows rowR + c
                          // (= 3 + c0 + c) and rowI + c (= 3 + nCtot + c0 + c); rowR == 3 also writes grad_gr's rows
};

template <typename T, int MC>
__global__ __launch_bounds__(256, 2) void k_rfgr2beff_bwd_sgpr(BeffBwdPkArgs<T> a)
{
    // U rows' gB loads are issued together, ahead of the arithmetic on them.  (Requesting the NEXT group
    // before computing this one -- a register double buffer -- was slower at every coil count: the
    // compiler splits and scatters the loads through the group, 0.61 -> 1.04 ms at 2 coils; U = 8: no gain.)
    // TP time points per thread (two, to halve the scalar loads: no gain)
    constexpr int TP = 1, NE = 3 * TP, PW = 2 * MC + 4, U = 4, H = MC / 2;
    static_assert(MC % 2 == 0, "coil pairs");
    using gvec = ElemRun<T, NE>;
    using CP = const T __attribute__((address_space(4)))*;
    typedef T V2 __attribute__((ext_vector_type(2)));   // a coil PAIR: v_pk_fma_f32 for float
    const int64_t L = 3 * a.nT, nT = a.nT;             // the launcher guarantees nT >= TP
    const int64_t t0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * TP;
    const int64_t sg = blockIdx.y, n = blockIdx.z;
    const int64_t s0 = sg * a.spins_per_group;
    const int64_t s1 = (s0 + a.spins_per_group < a.nM) ? s0 + a.spins_per_group : a.nM;
    const int nC = (int)a.nC;
    // a thread at or beyond the row end re-reads the row's last TP time points (slot q = time point
    // tr + q) and stores only its own
    const int64_t tr = (t0 + TP <= nT) ? t0 : nT - TP;
    V2 aR[TP][H], aI[TP][H];
    T aG[TP][3];
#pragma unroll
    for (int j = 0; j < TP; ++j) {
#pragma unroll
        for (int k = 0; k < H; ++k) aR[j][k] = aI[j][k] = V2{T(0), T(0)};
        aG[j][0] = aG[j][1] = aG[j][2] = T(0);
    }
    const int64_t cnt = s1 - s0;
    const T* src0 = a.gB + (n * a.nM + s0) * L + 3 * tr;
    CP pk0 = (CP)(a.pk + (n * a.nM + s0) * PW);
    for (int64_t i = 0; i < cnt; i += U) {
        gvec g[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t ir = (i + u < cnt) ? i + u : cnt - 1;
            g[u] = load_run_nt<T, NE>(src0 + ir * L);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // no branch in here (it would sink the U loads above into the rows that use them): a row past
            // the group's end re-reads the last row, against zeroed gB
            const bool on = i + u < cnt;
            CP q = pk0 + (on ? i + u : cnt - 1) * PW;
            T cf[PW];
#pragma unroll
            for (int k = 0; k < PW; ++k) cf[k] = q[k];  // scalar loads, all issued before the first FMA
#pragma unroll
            for (int e = 0; e < NE; ++e) g[u].v[e] = on ? g[u].v[e] : T(0);
#pragma unroll
            for (int j = 0; j < TP; ++j) {
                const T gx = g[u].v[3 * j], gy = g[u].v[3 * j + 1], gz = g[u].v[3 * j + 2];
                const V2 gx2 = {gx, gx}, gy2 = {gy, gy}, ngx2 = {-gx, -gx};
#pragma unroll
                for (int k = 0; k < H; ++k) {
                    const V2 br = {cf[2 * k], cf[2 * k + 1]}, bi = {cf[MC + 2 * k], cf[MC + 2 * k + 1]};
                    aR[j][k] = __builtin_elementwise_fma(bi, gy2, __builtin_elementwise_fma(br, gx2, aR[j][k]));
                    aI[j][k] = __builtin_elementwise_fma(bi, ngx2, __builtin_elementwise_fma(br, gy2, aI[j][k]));
                }
                aG[j][0] = fma_(cf[2 * MC], gz, aG[j][0]);
                aG[j][1] = fma_(cf[2 * MC + 1], gz, aG[j][1]);
                aG[j][2] = fma_(cf[2 * MC + 2], gz, aG[j][2]);
            }
        }
    }
    T* w = a.work + ((sg * a.N + n) * a.K) * nT;
#pragma unroll
    for (int q = 0; q < TP; ++q) {
        const int64_t t = tr + q;
        if (t < t0) continue;                           // a tail thread's re-read time points: not its own
        if (a.rowR == 3) { w[0 * nT + t] = aG[q][0]; w[1 * nT + t] = aG[q][1]; w[2 * nT + t] = aG[q][2]; }
#pragma unroll
        for (int c = 0; c < MC; ++c)
            if (c < nC) {
                w[(a.rowR + c) * nT + t] = (c & 1) ? aR[q][c / 2].y : aR[q][c / 2].x;
                w[(a.rowI + c) * nT + t] = (c & 1) ? aI[q][c / 2].y : aI[q][c / 2].x;
            }
    }
}

// Pass 1, any coil count (one block column per coil; strided scalar loads).
template <typename T>
__global__ __launch_bounds__(256) void k_rfgr2beff_bwd_p1(BeffBwdArgs<T> a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t sg = blockIdx.y;
    const int64_t n = blockIdx.z / (a.nC + 1);
    const int64_t part = blockIdx.z % (a.nC + 1);     // 0: gradients, 1..nC: coil part-1
    if (t >= a.nT) return;
    const int64_t s0 = sg * a.spins_per_group;
    const int64_t s1 = (s0 + a.spins_per_group < a.nM) ? s0 + a.spins_per_group : a.nM;
    const int64_t K = 3 + 2 * a.nC;
    T* w = a.work + ((sg * a.N + n) * K) * a.nT;
    if (part == 0) {
        T ax = T(0), ay = T(0), az = T(0);
        for (int64_t s = s0; s < s1; ++s) {
            const int64_t row = n * a.nM + s;
            const T gz = a.gB[(row * a.nT + t) * 3 + 2];
            ax += a.loc[row * 3] * gz;
            ay += a.loc[row * 3 + 1] * gz;
            az += a.loc[row * 3 + 2] * gz;
        }
        w[0 * a.nT + t] = ax; w[1 * a.nT + t] = ay; w[2 * a.nT + t] = az;
    } else {
        const int64_t c = part - 1;
        T ar = T(0), ai = T(0);
        for (int64_t s = s0; s < s1; ++s) {
            const int64_t row = n * a.nM + s;
            const T gx = a.gB[(row * a.nT + t) * 3], gy = a.gB[(row * a.nT + t) * 3 + 1];
            T br = T(1), bi = T(0);
            if (a.b1) { br = a.b1[(row * 2) * a.nC + c]; bi = a.b1[(row * 2 + 1) * a.nC + c]; }
            ar += br * gx + bi * gy;
            ai += br * gy - bi * gx;
        }
        w[(3 + c) * a.nT + t] = ar;
        w[(3 + a.nC + c) * a.nT + t] = ai;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_rfgr2beff_bwd_p2(BeffBwdArgs<T> a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t kk = blockIdx.y;       // row of the (3 + 2 nC) partial rows
    const int64_t n = blockIdx.z;
    if (t >= a.nT) return;
    const int64_t K = 3 + 2 * a.nC;
    T acc = T(0);
    for (int64_t sg = 0; sg < a.nSG; ++sg) acc += a.work[((sg * a.N + n) * K + kk) * a.nT + t];
    if (kk < 3) {
        if (a.ggr) a.ggr[(n * 3 + kk) * a.nT + t] = acc;
    } else if (a.grf) {
        const int64_t c = (kk - 3) % a.nC, ri = (kk - 3) / a.nC;
        a.grf[((n * 2 + ri) * a.nT + t) * a.nC + c] = acc;
    }
}


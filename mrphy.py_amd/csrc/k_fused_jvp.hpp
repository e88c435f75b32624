// k_fused_jvp.hpp -- K2j (fused rf,gr -> Mo and its forward-mode tangents dMo, one transmit coil)
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_common.hpp"

// =============================================================================================
// K2j: K2's frame (one block = one wave = 64 spins of ONE batch entry; lane_spin, load_consts, pulse_cp, step batches,
// then a per-step tail) carrying, beside the magnetisation m, its directional derivatives along up to MD directions.
// A direction d is a set of tangents of the operands -- dMi, drf, dgr, dloc, ddf, db1, dE1, dE2, dE1m1, each a dense
// table with a leading direction axis, each optional (null: zero) -- and dMo[d] is the derivative of Mo along it.
//
// One step (bloch_math.hpp: b = g B, x = b.b, w = b x m, v = b x w, u = m - S w + C v, m' = (E2 ux, E2 uy, E1 uz - E1m1)):
//     Bx' + i By' = b1 rf' + b1' rf           Bz' = gr'.loc + gr.loc' + df'/gamma
//     b' = g B'      x' = 2 b.b'      S'(x) x',  C'(x) x'
//     w' = b' x m + b x m'       v' = b' x w + b x w'
//     u' = m' - (S'x') w - S w' + (C'x') v + C v'
//     m'_next = (E2 u'x + E2' ux,  E2 u'y + E2' uy,  E1 u'z + E1' uz - E1m1')
// Every line is linear in the tangent quantities, and every product below holds exactly one tangent factor: a direction
// scaled by a power of two or negated scales or negates dMo[d] exactly, and the zero direction gives zeros.
//
// The primal goes through K2's own field (field_1coil) and step (rot_prepare_adj forms the S, C of rot_prepare bit for
// bit -- K2b relies on the same -- beside the S'(x), C'(x) the tangent needs: the polynomials on [0, pi^2], the closed
// forms beyond; rot_apply): Mo is K2's, bit for bit.  b, S, C, S', C', w, v, u of a step are formed once and shared by
// all directions; a direction keeps 12 values in registers (m' 3, loc' 3, df'/gamma 1, b1' 2, E' 3).  The pulse-side
// tangents drf[d][t], dgr[d][t] are wave-uniform: scalar loads through constant-address-space pointers, and there is no
// store inside the step loop, as in plain K2.  A null drf / dgr -- or a direction of the capacity beyond D -- reads the
// primal pulse instead and clears the loaded bits under a wave-uniform mask: no branch in the loop, no memory of zeros
// needed.  (The compiler folds the AND into a select and issues it on the vector unit: one v_cndmask_b32, mostly with a
// v_mov_b32 of the scalar sample, per sample -- 5 + 5 of the ~74 VALU instructions a direction costs per step.)
// The arithmetic of direction d is the same whatever MD is and whatever the other directions hold.
// No checkpoints, no LDS, no second pass.
// =============================================================================================
template <typename T>
struct JvpArgs {
    const T* Mi;
    PulseOpsT<T> in;
    int64_t D;                                            // directions given, 1 <= D <= MD
    const T *dMi, *drf, *dgr;                             // (D, N, nM, 3)  (D, N, 2, nT)  (D, N, 3, nT)
    const T *dloc, *ddf, *db1;                            // (D, N, nM, 3)  (D, N, nM)     (D, N, nM, 2)
    const T *dE1, *dE2, *dE1m1;                           // (D, N, nM) each
    T* Mo;                                                // (N, nM, 3) or null
    T* dMo;                                               // (D, N, nM, 3)
    int64_t N, nM, nT;
};

// steps per batch: the pulse samples of a batch are 5 (1 + MD) scalars per step, twice the registers in fp64
template <typename T, int MD>
constexpr int jvp_batch() { return sizeof(T) == 8 ? (MD == 4 ? 1 : 2) : (MD == 4 ? 2 : 4); }

template <typename T> struct JvpBits;
template <> struct JvpBits<float>  { using type = uint32_t; };
template <> struct JvpBits<double> { using type = uint64_t; };
// a wave-uniform sample under a wave-uniform mask (all ones: kept; zero: +0.0): a select, not a multiplication (0 * inf)
template <typename T>
__device__ __forceinline__ T jvp_keep(T v, typename JvpBits<T>::type mask)
{
    using U = typename JvpBits<T>::type;
    return __builtin_bit_cast(T, (U)(__builtin_bit_cast(U, v) & mask));
}

// what a lane keeps per direction
template <typename T, int MD>
struct JvpLane {
    T mx[MD], my[MD], mz[MD];                             // m'
    T lx[MD], ly[MD], lz[MD], delta[MD];                  // loc', df'/gamma
    T br[MD], bi[MD];                                     // b1'
    T e1[MD], e2[MD], e1m1[MD];                           // E1', E2', E1m1'
};
// what the wave keeps per direction: the rows of the pulse tangents (rf: re at [t], im at [nT + t]; gr: x, y, z at
// [t], [nT + t], [2 nT + t]) and their masks
template <typename T, int MD>
struct JvpWave {
    using CP = typename PulseCP<T>::CP;
    using U = typename JvpBits<T>::type;
    CP rf[MD], gr[MD];
    U krf[MD], kgr[MD];
};

// NS steps from t0: the primal's batch as K2 runs it, and per step the tangents of every direction before m moves on
template <int NS, bool RELAX, bool HB1, int MD, typename T, typename CT>
__device__ __forceinline__ void jvp_steps(const SpinConst<T, CT>& k, const Spin<T>& sp, T br, T bi, const PulseCP<T>& pc,
                                          const JvpWave<T, MD>& w_, int64_t t0, int64_t nT, T e1, T e2, T& mx, T& my, T& mz,
                                          JvpLane<T, MD>& l)
{
#pragma clang fp contract(off)
    T Bx[NS], By[NS], Bz[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) field_1coil<HB1>(br, bi, pc, t0 + j, sp, Bx[j], By[j], Bz[j]);
    RotAdj<T> r[NS];
    rot_prepare_adj<T, CT, NS>(k, Bx, By, Bz, r);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int64_t t = t0 + j;
        const RotAdj<T>& q = r[j];
        // the primal's w, v and rotated state u, as rot_apply forms them (the precise step's `s`)
        T wx, wy, wz, vx, vy, vz;
        cross_(q.bx, q.by, q.bz, mx, my, mz, wx, wy, wz);
        cross_(q.bx, q.by, q.bz, wx, wy, wz, vx, vy, vz);
        const T ux = fma_(q.C, vx, fma_(-q.S, wx, mx));
        const T uy = fma_(q.C, vy, fma_(-q.S, wy, my));
        const T uz = fma_(q.C, vz, fma_(-q.S, wz, mz));
        const T rr = pc.rfr[t], ri = pc.rfi[t], gx = pc.gx[t], gy = pc.gy[t], gz = pc.gz[t];
#pragma unroll
        for (int d = 0; d < MD; ++d) {
            const T drr = jvp_keep<T>(w_.rf[d][t], w_.krf[d]), dri = jvp_keep<T>(w_.rf[d][nT + t], w_.krf[d]);
            const T dgx = jvp_keep<T>(w_.gr[d][t], w_.kgr[d]), dgy = jvp_keep<T>(w_.gr[d][nT + t], w_.kgr[d]),
                    dgz = jvp_keep<T>(w_.gr[d][2 * nT + t], w_.kgr[d]);
            T dBx = drr, dBy = dri;                          // no b1 map: b1 = (1, 0), b1' = 0
            if (HB1) {
                dBx = fma_(br, drr, fma_(-bi, dri, fma_(l.br[d], rr, -(l.bi[d] * ri))));
                dBy = fma_(br, dri, fma_(bi, drr, fma_(l.br[d], ri, l.bi[d] * rr)));
            }
            const T dBz = fma_(dgz, sp.lz, fma_(dgy, sp.ly, fma_(dgx, sp.lx,
                          fma_(gz, l.lz[d], fma_(gy, l.ly[d], fma_(gx, l.lx[d], l.delta[d]))))));
            T dbx, dby, dbz;
            scale_b<T, CT>(k, dBx, dBy, dBz, dbx, dby, dbz);
            const T dx = T(2) * dot_(q.bx, q.by, q.bz, dbx, dby, dbz);
            const T dS = q.dS * dx, dC = q.dC * dx;
            const T pmx = l.mx[d], pmy = l.my[d], pmz = l.mz[d];
            // w' = b' x m + b x m'
            const T dwx = fma_(q.by, pmz, fma_(-q.bz, pmy, fma_(dby, mz, -(dbz * my))));
            const T dwy = fma_(q.bz, pmx, fma_(-q.bx, pmz, fma_(dbz, mx, -(dbx * mz))));
            const T dwz = fma_(q.bx, pmy, fma_(-q.by, pmx, fma_(dbx, my, -(dby * mx))));
            // v' = b' x w + b x w'
            const T dvx = fma_(q.by, dwz, fma_(-q.bz, dwy, fma_(dby, wz, -(dbz * wy))));
            const T dvy = fma_(q.bz, dwx, fma_(-q.bx, dwz, fma_(dbz, wx, -(dbx * wz))));
            const T dvz = fma_(q.bx, dwy, fma_(-q.by, dwx, fma_(dbx, wy, -(dby * wx))));
            // u' = m' - S' w - S w' + C' v + C v'
            const T dux = fma_(q.C, dvx, fma_(dC, vx, fma_(-q.S, dwx, fma_(-dS, wx, pmx))));
            const T duy = fma_(q.C, dvy, fma_(dC, vy, fma_(-q.S, dwy, fma_(-dS, wy, pmy))));
            const T duz = fma_(q.C, dvz, fma_(dC, vz, fma_(-q.S, dwz, fma_(-dS, wz, pmz))));
            if (RELAX) {
                l.mx[d] = fma_(e2, dux, l.e2[d] * ux);
                l.my[d] = fma_(e2, duy, l.e2[d] * uy);
                l.mz[d] = fma_(e1, duz, fma_(l.e1[d], uz, -l.e1m1[d]));
            } else {
                l.mx[d] = dux; l.my[d] = duy; l.mz[d] = duz;
            }
        }
        const Rot<T> rp = {q.bx, q.by, q.bz, q.S, q.C};
        rot_apply<RELAX, T, CT>(k, rp, mx, my, mz);
    }
}

template <typename T, typename CT, bool RELAX, bool HB1, int MD>
__global__ __launch_bounds__(WAVE) void k_bloch_rfgr_jvp(JvpArgs<T> a)
{
    constexpr int NS = jvp_batch<T, MD>();
    using CP = typename PulseCP<T>::CP;
    using U = typename JvpBits<T>::type;
    const int lane = threadIdx.x;
    const int64_t n = blockIdx.y;
    bool valid;
    const int64_t s = lane_spin(blockIdx.x, lane, a.nM, valid);
    const int64_t row = n * a.nM + s;
    const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
    T mx = a.Mi[row * 3], my = a.Mi[row * 3 + 1], mz = a.Mi[row * 3 + 2];
    const Spin<T> sp = load_spin<T>(a.in, n, s, row);
    T br, bi;
    load_b1<HB1>(a.in.b1, row, br, bi);
    const T e1 = T(k.e1), e2 = T(k.e2);                   // the tangent's arithmetic is the data type's

    const int64_t nT = a.nT, rows = a.N * a.nM;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    JvpLane<T, MD> l;
    JvpWave<T, MD> w;
#pragma unroll
    for (int d = 0; d < MD; ++d) {
        const bool on = d < a.D;                          // wave-uniform, as every test of a table's pointer below
        const int64_t r = d * rows + row;
        l.mx[d] = l.my[d] = l.mz[d] = T(0);
        if (on && a.dMi) { l.mx[d] = a.dMi[r * 3]; l.my[d] = a.dMi[r * 3 + 1]; l.mz[d] = a.dMi[r * 3 + 2]; }
        l.lx[d] = l.ly[d] = l.lz[d] = T(0);
        if (on && a.dloc) { l.lx[d] = a.dloc[r * 3]; l.ly[d] = a.dloc[r * 3 + 1]; l.lz[d] = a.dloc[r * 3 + 2]; }
        l.delta[d] = T(0);
        if (on && a.ddf) l.delta[d] = a.ddf[r] / bc_load<T>(a.in.gam, n, s);
        l.br[d] = l.bi[d] = T(0);
        if (HB1 && on && a.db1) { l.br[d] = a.db1[r * 2]; l.bi[d] = a.db1[r * 2 + 1]; }
        l.e1[d] = l.e2[d] = l.e1m1[d] = T(0);
        if (RELAX && on) {
            if (a.dE1) l.e1[d] = a.dE1[r];
            if (a.dE2) l.e2[d] = a.dE2[r];
            if (a.dE1m1) l.e1m1[d] = a.dE1m1[r];
        }
        const bool hrf = on && a.drf, hgr = on && a.dgr;
        w.rf[d] = hrf ? (CP)(a.drf + (d * a.N + n) * 2 * nT) : pc.rfr;
        w.gr[d] = hgr ? (CP)(a.dgr + (d * a.N + n) * 3 * nT) : pc.gx;
        w.krf[d] = hrf ? ~U(0) : U(0);
        w.kgr[d] = hgr ? ~U(0) : U(0);
    }

    int64_t t0 = 0;
    for (; t0 + NS <= nT; t0 += NS) jvp_steps<NS, RELAX, HB1, MD, T, CT>(k, sp, br, bi, pc, w, t0, nT, e1, e2, mx, my, mz, l);
    for (; t0 < nT; ++t0) jvp_steps<1, RELAX, HB1, MD, T, CT>(k, sp, br, bi, pc, w, t0, nT, e1, e2, mx, my, mz, l);   // nT % NS tail
    if (!valid) return;
    if (a.Mo) { a.Mo[row * 3] = mx; a.Mo[row * 3 + 1] = my; a.Mo[row * 3 + 2] = mz; }
#pragma unroll
    for (int d = 0; d < MD; ++d)
        if (d < a.D) {
            T* o = a.dMo + (d * rows + row) * 3;
            o[0] = l.mx[d]; o[1] = l.my[d]; o[2] = l.mz[d];
        }
}

// Host: the launch of the build RELAX x HB1 at capacity MD.  Runs at nT == 0 too (Mo = Mi, dMo = dMi or zeros), as K2
template <int MD, typename T, typename CT>
int launch_jvp(const void* Mi, const PulseOps& in, const JvpTangents& tg, void* Mo, void* dMo, int64_t N, int64_t nM,
               int64_t nT, hipStream_t st)
{
    JvpArgs<T> a;
    a.Mi = (const T*)Mi; a.in = typed<T>(in); a.D = tg.D;
    a.dMi = (const T*)tg.dMi; a.drf = (const T*)tg.drf; a.dgr = (const T*)tg.dgr;
    a.dloc = (const T*)tg.dloc; a.ddf = (const T*)tg.ddf; a.db1 = (const T*)tg.db1;
    a.dE1 = (const T*)tg.dE1; a.dE2 = (const T*)tg.dE2; a.dE1m1 = (const T*)tg.dE1m1;
    a.Mo = (T*)Mo; a.dMo = (T*)dMo;
    a.N = N; a.nM = nM; a.nT = nT;
    if (tg.D < 1 || tg.D > MD) return MRPHY_EINVAL;
    dim3 grid;
    int rc;
    if (!fused_grid(N * nM, (nM + WAVE - 1) / WAVE, N, grid, rc)) return rc;
#define MRPHY_K2J(RX_, HB_) hipLaunchKernelGGL((k_bloch_rfgr_jvp<T, CT, RX_, HB_, MD>), grid, dim3(WAVE), 0, st, a)
    const bool rx = (a.in.E1.p != nullptr);
    if (rx) { if (a.in.b1) MRPHY_K2J(true, true); else MRPHY_K2J(true, false); }
    else    { if (a.in.b1) MRPHY_K2J(false, true); else MRPHY_K2J(false, false); }
#undef MRPHY_K2J
    return launch_status();
}

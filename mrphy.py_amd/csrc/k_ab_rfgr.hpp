// k_ab_rfgr.hpp -- K2ab (fused rf,gr -> Hargreaves' A, B) and its adjoint K2abb, one transmit coil
// Fragment: included INSIDE a translation unit's anonymous namespace, after host_common.hpp (HIP runtime,
// include/mrphy_hip.h, geom.hpp, bloch_math.hpp, k_common.hpp).  Not a standalone header.
#pragma once
#include "k_fused_bwd_common.hpp"

// =============================================================================================
// K2ab: beff2ab (beffective.py:40-104) of rfgr2beff (beffective.py:107-168) without Beff in HBM.  K2's frame -- one
// block = one wave = 64 spins of ONE batch entry, the pulse through scalar loads, the field assembled as K0 rounds it
// (field_1coil) -- carrying the four columns of [I | 0] as k_beff2ab does: per step ONE field and ONE rot_prepare, then
// rot_apply on the three A columns with a zero offset (`kl`) and on the B column with the real one.  So A, B are
// k_beff2ab(K0(.)) bit for bit, and column j of A is K2(e_j) with a zero offset.
// Without relaxation (RELAX == false: E1, E2, E1m1 null) the B column is not stepped: the step map is then linear, B stays
// the exact zero it started as, and so do its checkpoints and its part in the adjoint.
// CK: checkpoints of the four columns every ck_every steps, ABck (nCk, 4, N*nM, 3): plane j of checkpoint c is column j
// before step c * ck_every -- per column the 768 contiguous bytes per wave of K2's Mck.
// =============================================================================================
template <typename T>
struct AbFusedArgs {
    PulseOpsT<T> in;
    T* A;                  // (N*nM, 3, 3): A[r][i][j], i = xyz component, j = column
    T* B;                  // (N*nM, 3)
    T* ABck;  int64_t ck_every;
    int64_t N, nM, nT;
};

template <bool RELAX> constexpr int AB_COLS = RELAX ? 4 : 3;      // the columns that are stepped

template <typename T, typename CT, bool CK, bool RELAX, bool HB1>
__global__ __launch_bounds__(WAVE) void k_ab_rfgr_fwd(AbFusedArgs<T> a)
{
    constexpr int NS = sizeof(T) == 8 ? 4 : 8;              // steps per batch, as K2's one-coil builds
    constexpr int NCOL = AB_COLS<RELAX>;
    const int lane = threadIdx.x;
    const int64_t n = blockIdx.y;
    bool valid;
    const int64_t s = lane_spin(blockIdx.x, lane, a.nM, valid);
    const int64_t row = n * a.nM + s;
    const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
    SpinConst<T, CT> kl = k;
    kl.e1m1 = typename CTr<CT>::reg(0);                     // the A columns: linear part only
    const Spin<T> sp = load_spin<T>(a.in, n, s, row);
    T br, bi;
    load_b1<HB1>(a.in.b1, row, br, bi);

    const int64_t nT = a.nT;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    const int64_t rows = a.N * a.nM;
    T cx[4] = {T(1), T(0), T(0), T(0)}, cy[4] = {T(0), T(1), T(0), T(0)}, cz[4] = {T(0), T(0), T(1), T(0)};

    // one step of the columns that are stepped
    auto apply = [&](const Rot<T>& r) {
#pragma unroll
        for (int j = 0; j < 3; ++j) rot_apply<RELAX, T, CT>(kl, r, cx[j], cy[j], cz[j]);
        if constexpr (RELAX) rot_apply<RELAX, T, CT>(k, r, cx[3], cy[3], cz[3]);
    };
    // the four columns before step t to the running checkpoint if t is the step `next` (ck_store, four planes)
    int64_t ck_next = 0;
    T* ckp = CK ? a.ABck + row * 3 : nullptr;
    const int64_t ck_pitch = rows * 3;
    auto checkpoint = [&](int64_t t) {
        if (t == ck_next) {                                 // wave-uniform
            if (valid) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    T* q = ckp + j * ck_pitch;
                    q[0] = cx[j]; q[1] = cy[j]; q[2] = cz[j];
                }
            }
            ckp += 4 * ck_pitch; ck_next += a.ck_every;
        }
    };

    // (the checkpoint build awaits the prologue's vector loads before the loop, as K2's does: k_fused_fwd.hpp)
    if (CK) __builtin_amdgcn_s_waitcnt(0x0F70);             // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
    int64_t t0 = 0;
    for (; t0 + NS <= nT; t0 += NS) {
        if (CK) checkpoint(t0);
        T Bx[NS], By[NS], Bz[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) field_1coil<HB1>(br, bi, pc, t0 + j, sp, Bx[j], By[j], Bz[j]);
        Rot<T> r[NS];
        rot_prepare<T, CT, NS>(k, Bx, By, Bz, r);
#pragma unroll
        for (int j = 0; j < NS; ++j) apply(r[j]);
    }
    for (; t0 < nT; ++t0) {                                 // nT % NS tail
        if (CK) checkpoint(t0);
        T Bx[1], By[1], Bz[1];
        field_1coil<HB1>(br, bi, pc, t0, sp, Bx[0], By[0], Bz[0]);
        Rot<T> r[1];
        rot_prepare<T, CT, 1>(k, Bx, By, Bz, r);
        apply(r[0]);
    }
    if (valid) {
        T* A = a.A + row * 9;
#pragma unroll
        for (int j = 0; j < 3; ++j) { A[j] = cx[j]; A[3 + j] = cy[j]; A[6 + j] = cz[j]; }
        a.B[row * 3] = cx[3]; a.B[row * 3 + 1] = cy[3]; a.B[row * 3 + 2] = cz[3];
    }
}

// Host: the build for the checkpoint, relaxation and b1 modes of the arguments.  Runs at nT == 0 too (A = I, B = 0).
template <typename T, typename CT>
int launch_k2ab(const PulseOps& in, void* A, void* B, void* ABck, int64_t ck_every, int64_t N, int64_t nM, int64_t nT,
                hipStream_t st)
{
    AbFusedArgs<T> a;
    a.in = typed<T>(in); a.A = (T*)A; a.B = (T*)B; a.ABck = (T*)ABck; a.ck_every = ck_every > 0 ? ck_every : 1;
    a.N = N; a.nM = nM; a.nT = nT;
    dim3 grid;
    int rc;
    if (!fused_grid(N * nM, (nM + WAVE - 1) / WAVE, N, grid, rc)) return rc;
#define MRPHY_K2AB(CK_, RX_, HB_) \
    hipLaunchKernelGGL((k_ab_rfgr_fwd<T, CT, CK_, RX_, HB_>), grid, dim3(WAVE), 0, st, a)
#define MRPHY_K2AB_B1(CK_, RX_) \
    do { if (in.b1) MRPHY_K2AB(CK_, RX_, true); else MRPHY_K2AB(CK_, RX_, false); } while (0)
    const bool ck = (ABck != nullptr), rx = (in.E1.p != nullptr);
    if (ck) { if (rx) MRPHY_K2AB_B1(true, true); else MRPHY_K2AB_B1(true, false); }
    else    { if (rx) MRPHY_K2AB_B1(false, true); else MRPHY_K2AB_B1(false, false); }
#undef MRPHY_K2AB_B1
#undef MRPHY_K2AB
    return launch_status();
}

// =============================================================================================
// K2abb: adjoint of K2ab -- grad_A, grad_B -> grad_rf, grad_gr without Beff, history or grad_Beff in HBM.  K2b's frame
// and reduction, unchanged: persistent waves, the 5 x SEG LDS transpose-sum, a workspace row per wave, the second pass
// (k_fused_bwd_common.hpp).  The four columns share a step's field, S and C but not its registers: SegStates is one
// column's recomputed segment.  So within a segment the columns run one after another, in a loop that is NOT unrolled
// (the sweep is K2b's code once, not four times):
//   1. column j's SEG pre-step states are recomputed from its checkpoint; S and C are formed during column 0 and
//      taken from there by the others (b = g B is re-formed: one rounding, the same bits);
//   2. column j is swept with its own carried adjoint state.  The loop always works on the carried state in slot 0
//      and rotates the slots at its end (registers cannot be indexed by a run-time j);
//   3. the step's dL/dB is summed over the columns in the lane's own slots of the reduction tile, rows (0..2) SEG + st,
//      in the fixed order ((c0 + c1) + c2) + c3 -- lane-private, so no barrier between columns;
//   4. once per segment the sums become the five contributions K2b forms (loc g2; b1 x (g0, g1)), then the row sums.
// The relaxation offset is an additive constant: it enters the recompute of the B column only and not the adjoint.
// No adj_end: nothing is returned per spin.  Without relaxation the B column is skipped (its states are exact zeros,
// and every dL/dB it would form is linear in them).
//
// MAPS (tu_ab_rfgr_maps_bwd.hip): the gradients w.r.t. the lane's own loc, df / gamma and b1 besides, as K2b's MAPS
// builds form them (k_fused_bwd.hpp) -- step 4 holds the column-summed (g0, g1, g2) = dL/dB of the segment's 16 steps,
// and sums them over TIME there: partials per segment (steps ascending), added to lane-private running sums once per
// segment (segments descending), reset per tile, stored per spin under `valid`.  No LDS beyond the reduction tile, no
// workspace, no second pass, a fixed order of summation; the sweep is untouched.
// CONSTS (tu_ab_rfgr_consts_bwd.hip): the gradients w.r.t. the lane's own step constants besides, gC = [dL/dg, dL/dE1,
// dL/dE2, dL/dE1m1], by K2b's CONSTS arithmetic (rot_apply_adj_consts): dL/dg, dL/dE1, dL/dE2 summed over every stepped
// column, dL/dE1m1 over the B column alone -- the A columns run without the offset.  The segment's partials are carried
// through the column loop; in the precise fp32 mode all four columns carry t = E h (adj_begin on each), and one
// adj_const_finish per tile divides the E out.  Without relaxation gC[1..3] are exact zeros, as K2b's.  The CONSTS
// build forms the MAPS sums as well (the MAPS build's bits); each of gloc, gBz, gb1, gC may be null.
// Everything the plain build computes is computed by the same expressions in all three.
// =============================================================================================
template <typename T>
struct AbFusedBwdArgs {
    const T* ABck;                   // (nT/SEG, 4, N*nM, 3)
    PulseOpsT<T> in;
    const T* gA;                     // (N*nM, 3, 3) or null (= 0)
    const T* gB;                     // (N*nM, 3) or null (= 0)
    T* work;                         // (P, N, 5, nT)
    int64_t N, nM, nT, P;
};
template <typename T>
struct AbFusedBwdMapsArgs : AbFusedBwdArgs<T> {
    T* gloc;                         // (N, nM, 3): dL/dloc
    T* gBz;                          // (N, nM): dL/d(df / gamma)
    T* gb1;                          // (N, nM, 2): dL/db1; builds with a b1 map only
};
template <typename T>
struct AbFusedBwdConstsArgs : AbFusedBwdMapsArgs<T> {
    T* gC;                           // (N, nM, 4): [dL/dg, dL/dE1, dL/dE2, dL/dE1m1], g = gamma 2 pi dt
};
template <typename T, bool MAPS, bool CONSTS>
using AbFusedBwdKArgsT = std::conditional_t<CONSTS, AbFusedBwdConstsArgs<T>,
                                            std::conditional_t<MAPS, AbFusedBwdMapsArgs<T>, AbFusedBwdArgs<T>>>;

// seg_recompute (k_fused_bwd_common.hpp) with the rotations' S, C either formed and kept in h (GIVEN == false) or taken
// from h (GIVEN == true): Rot is scale_b's b and those S, C, which is what rot_prepare leaves in it
template <bool RELAX, bool GIVEN, typename T, typename CT, typename F>
__device__ __forceinline__ void ab_seg_recompute(const SpinConst<T, CT>& k, int64_t t0, T& mx, T& my, T& mz, F&& field,
                                                 SegStates<T>& h)
{
#pragma unroll
    for (int sb = 0; sb < SEG / 4; ++sb) {
        T Bx[4], By[4], Bz[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) field(t0 + sb * 4 + j, Bx[j], By[j], Bz[j]);
        Rot<T> r[4];
        if constexpr (GIVEN) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                scale_b<T, CT>(k, Bx[j], By[j], Bz[j], r[j].bx, r[j].by, r[j].bz);
                r[j].S = h.Sv[sb * 4 + j]; r[j].C = h.Cv[sb * 4 + j];
            }
        } else {
            rot_prepare<T, CT, 4>(k, Bx, By, Bz, r);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int st = sb * 4 + j;
            h.M0[st] = mx; h.M1[st] = my; h.M2[st] = mz;
            if constexpr (!GIVEN) { h.Sv[st] = r[j].S; h.Cv[st] = r[j].C; }
            rot_apply<RELAX, T, CT>(k, r[j], mx, my, mz);
        }
    }
}

// (the fp32 MAPS / CONSTS builds are bound to two waves per SIMD, K2b's occupancy: a build that outgrows 256 VGPRs then
// spills, which tools/kregs.py --scratch and the suite's scratch test name, instead of halving the occupancy unseen)
template <typename T, typename CT, bool RELAX, bool HB1, bool MAPS = false, bool CONSTS = false>
__global__ __launch_bounds__(WAVE, ((MAPS || CONSTS) && sizeof(T) == 4 ? 2 : 1))
void k_ab_rfgr_bwd(AbFusedBwdKArgsT<T, MAPS, CONSTS> a)
{
    static_assert(!(MAPS && CONSTS), "the CONSTS build forms the map sums itself");
    constexpr bool MSUM = MAPS || CONSTS;                   // the sums over time of dL/dB
    constexpr int NCOL = AB_COLS<RELAX>;
    using R = typename CTr<CT>::reg;
    __shared__ __attribute__((aligned(16))) T red[5 * SEG * RED_PITCH];
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, n = blockIdx.y;
    const int64_t nT = a.nT, rows = a.N * a.nM;
    const int64_t ntiles = (a.nM + WAVE - 1) / WAVE;
    const PulseCP<T> pc = pulse_cp<T>(a.in, n, nT, 1);
    T* wsrow = a.work + ((w * a.N + n) * 5) * nT;
    bool first = true;

    for (int64_t tile = w; tile < ntiles; tile += a.P) {
        bool valid;
        const int64_t s = lane_spin(tile, lane, a.nM, valid);
        const int64_t row = n * a.nM + s;
        const SpinConst<T, CT> k = load_consts<T, CT>(a.in.g, a.in.E1, a.in.E2, a.in.E1m1, n, s);
        const Spin<T> sp = load_spin<T>(a.in, n, s, row);
        T br, bi;
        load_b1<HB1>(a.in.b1, row, br, bi);
        // lanes past nM start from a zero cotangent, as in K2b: everything they form stays an exact zero
        const T vmask = valid ? T(1) : T(0);
        T hx[4], hy[4], hz[4];                              // the carried adjoint state of column j: dL/d(column j)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            hx[j] = a.gA ? a.gA[row * 9 + j] * vmask : T(0);
            hy[j] = a.gA ? a.gA[row * 9 + 3 + j] * vmask : T(0);
            hz[j] = a.gA ? a.gA[row * 9 + 6 + j] * vmask : T(0);
        }
        hx[3] = a.gB ? a.gB[row * 3] * vmask : T(0);
        hy[3] = a.gB ? a.gB[row * 3 + 1] * vmask : T(0);
        hz[3] = a.gB ? a.gB[row * 3 + 2] * vmask : T(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) adj_begin<RELAX, T, CT>(k, hx[j], hy[j], hz[j]);
        // MAPS / CONSTS: the running sums over time, reset per tile (unused, and compiled away, in the plain build)
        T aZ = T(0), aL[3] = {T(0), T(0), T(0)}, aBr = T(0), aBi = T(0);
        T aC[4] = {T(0), T(0), T(0), T(0)};

        // The checkpoints are visited segments descending, columns ascending; each is requested one column ahead of
        // its use (the first column of a segment during the last column of the segment before).
        const int64_t nseg = nT / SEG;
        const int64_t plane = rows * 3;
        const T* ckq = a.ABck + ((nseg - 1) * 4 * rows + row) * 3;       // (formed, not dereferenced, at nseg == 0)
        T cx = T(0), cy = T(0), cz = T(0);
        if (nseg > 0) { cx = ckq[0]; cy = ckq[1]; cz = ckq[2]; }
        const int r1 = WAVE + (lane >> 2);                  // rows 64..79 of the row sums: four lanes per row
        for (int64_t seg = nseg - 1; seg >= 0; --seg) {
            const int64_t t0 = seg * SEG;
            T* dst0 = wsrow + (lane / SEG) * nT + t0 + (lane % SEG);
            T* dst1 = wsrow + (r1 / SEG) * nT + t0 + (r1 % SEG);
            T old0 = T(0), old1 = T(0);
            if (!first) { old0 = *dst0; old1 = *dst1; }
            SegStates<T> h;
            T pC[4] = {T(0), T(0), T(0), T(0)};             // CONSTS: this segment's partial sums, over its columns
#pragma unroll 1
            for (int j = 0; j < NCOL; ++j) {
                T mx = cx, my = cy, mz = cz;
                const bool last = j == NCOL - 1;
                ckq += last ? -(4 + NCOL - 1) * plane : plane;      // the next column; after the last: (seg - 1, 0)
                if (!last || seg > 0) { cx = ckq[0]; cy = ckq[1]; cz = ckq[2]; }
                // 1. forward recompute, keeping the state before each step; the offset acts on the B column only
                SpinConst<T, CT> kc = k;
                kc.e1m1 = j == 3 ? k.e1m1 : R(0);
                // Only S and C are carried from one column to the next.  The lane's operands of the field and of
                // b = g B are pinned per column (no instruction is emitted): left to itself the compiler hoists b, x,
                // dS, dC of all SEG steps out of this loop -- 96 registers more, one wave per SIMD where K2b runs two
                Spin<T> spc = sp;
                T brc = br, bic = bi;
                asm volatile("" : "+v"(spc.lx), "+v"(spc.ly), "+v"(spc.lz), "+v"(spc.delta), "+v"(brc), "+v"(bic),
                                  "+v"(kc.g));
                auto field = [&](int64_t t, T& Bx, T& By, T& Bz) { field_1coil<HB1>(brc, bic, pc, t, spc, Bx, By, Bz); };
                if (j == 0) ab_seg_recompute<RELAX, false>(kc, t0, mx, my, mz, field, h);
                else        ab_seg_recompute<RELAX, true>(kc, t0, mx, my, mz, field, h);
                // 2. adjoint sweep of this column, 3. its dL/dB added to the columns before it
#pragma unroll
                for (int sb = SEG / 4 - 1; sb >= 0; --sb) {
                    T Bx[4], By[4], Bz[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) field(t0 + sb * 4 + q, Bx[q], By[q], Bz[q]);
                    RotAdj<T> ra[4];
                    const T S4[4] = {h.Sv[sb * 4], h.Sv[sb * 4 + 1], h.Sv[sb * 4 + 2], h.Sv[sb * 4 + 3]};
                    const T C4[4] = {h.Cv[sb * 4], h.Cv[sb * 4 + 1], h.Cv[sb * 4 + 2], h.Cv[sb * 4 + 3]};
                    rot_prepare_adj_given<T, CT, 4>(kc, Bx, By, Bz, S4, C4, ra);
#pragma unroll
                    for (int q = 3; q >= 0; --q) {
                        const int st = sb * 4 + q;
                        T g0, g1, g2;
                        if constexpr (CONSTS) {
                            // dL/dg wants the step's unscaled field: assembled again here (the same expressions, the
                            // same bits) from operands pinned per step, or the batch's Bx, By, Bz stay alive through
                            // its four steps -- twelve registers at the sweep's peak, which the fp32 builds do not have
                            // at two waves per SIMD.  The offset's gradient comes from the B column only (wave-uniform).
                            asm volatile("" : "+v"(spc.lx), "+v"(spc.ly), "+v"(spc.lz), "+v"(spc.delta), "+v"(brc),
                                              "+v"(bic));
                            T fx, fy, fz;
                            field(t0 + st, fx, fy, fz);
                            rot_apply_adj_consts<RELAX, T, CT>(kc, ra[q], fx, fy, fz, h.M0[st], h.M1[st], h.M2[st],
                                                               hx[0], hy[0], hz[0], g0, g1, g2, pC, j == 3);
                        } else
                            rot_apply_adj<RELAX, T, CT>(kc, ra[q], h.M0[st], h.M1[st], h.M2[st], hx[0], hy[0], hz[0],
                                                        g0, g1, g2);
                        T* q0 = red + red_idx(0 * SEG + st, lane);
                        T* q1 = red + red_idx(1 * SEG + st, lane);
                        T* q2 = red + red_idx(2 * SEG + st, lane);
                        if (j != 0) { g0 = *q0 + g0; g1 = *q1 + g1; g2 = *q2 + g2; }      // wave-uniform
                        *q0 = g0; *q1 = g1; *q2 = g2;
                    }
                }
                // the next column's carried state into slot 0, this one's to the back
                const T tx = hx[0], ty = hy[0], tz = hz[0];
#pragma unroll
                for (int i = 0; i + 1 < NCOL; ++i) { hx[i] = hx[i + 1]; hy[i] = hy[i + 1]; hz[i] = hz[i + 1]; }
                hx[NCOL - 1] = tx; hy[NCOL - 1] = ty; hz[NCOL - 1] = tz;
            }
            // 4. the five contributions of each step from the columns' sum, as K2b forms them from one column's
            T pZ = T(0), pL[3] = {T(0), T(0), T(0)}, pBr = T(0), pBi = T(0);      // MAPS: this segment's partial sums
#pragma unroll
            for (int st = 0; st < SEG; ++st) {
                const T g0 = red[red_idx(0 * SEG + st, lane)], g1 = red[red_idx(1 * SEG + st, lane)],
                        g2 = red[red_idx(2 * SEG + st, lane)];
                if constexpr (MSUM) {
                    // the step's pulse sample: wave-uniform scalars, as the sweep's `field` read them
                    const int64_t t = t0 + st;
                    pZ += g2;
                    pL[0] += g2 * pc.gx[t]; pL[1] += g2 * pc.gy[t]; pL[2] += g2 * pc.gz[t];
                    if constexpr (HB1) {
                        const T rr = pc.rfr[t], ri = pc.rfi[t];
                        pBr += g0 * rr + g1 * ri;
                        pBi += g1 * rr - g0 * ri;
                    }
                }
                red[red_idx(0 * SEG + st, lane)] = sp.lx * g2;
                red[red_idx(1 * SEG + st, lane)] = sp.ly * g2;
                red[red_idx(2 * SEG + st, lane)] = sp.lz * g2;
                red[red_idx(3 * SEG + st, lane)] = HB1 ? br * g0 + bi * g1 : g0;
                red[red_idx(4 * SEG + st, lane)] = HB1 ? br * g1 - bi * g0 : g1;
                // (the pulse samples a batch of steps at a time, as the sweep takes them: requested all at once, the 80
                // scalars of a segment do not fit the scalar registers in fp64)
                if constexpr (MSUM)
                    if (st % 4 == 3) __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (CONSTS) {
#pragma unroll
                for (int i = 0; i < 4; ++i) aC[i] += pC[i];
            }
            if constexpr (MSUM) {
                aZ += pZ; aL[0] += pL[0]; aL[1] += pL[1]; aL[2] += pL[2];
                if constexpr (HB1) { aBr += pBr; aBi += pBi; }
            }
            __syncthreads();
            // 80 row sums, K2b's: lanes 0..63 take rows 0..63, then lane (r, j) chain j of row 64 + r; ONE explicit wait
            // for the vector loads requested above (k_fused_bwd.hpp says why)
            __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0) (gfx9 encoding; expcnt / lgkmcnt untouched)
            {
                T p0 = T(0), p1 = T(0), p2 = T(0), p3 = T(0);
#pragma unroll
                for (int i = 0; i < WAVE; i += 4) {
                    const T* q = red + red_idx(lane, i);
                    p0 += q[0]; p1 += q[1]; p2 += q[2]; p3 += q[3];
                }
                *dst0 = old0 + ((p0 + p1) + (p2 + p3));
            }
            static_assert(5 * SEG - WAVE == WAVE / 4, "second pass: 16 rows x 4 chains = one wave");
            {
                const int c = lane & 3;
                T p = T(0);
#pragma unroll
                for (int i = 0; i < WAVE; i += 4) p += red[red_idx(r1, i) + c];
                p += __shfl_xor(p, 1);
                p += __shfl_xor(p, 2);
                if (c == 0) *dst1 = old1 + p;
            }
            __syncthreads();
        }
        if constexpr (CONSTS) {
            adj_const_finish<T, CT>(k, aC);                 // the precise fp32 mode carried t = E h: E divided out once
            if (valid && a.gC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) a.gC[row * 4 + i] = aC[i];
            }
        }
        if constexpr (MSUM) {
            // once per spin; each output optional.  gBz is dL/d(df / gamma): the division by gamma and the folds to
            // the operands' own shapes are the host's
            if (valid && a.gloc) { a.gloc[row * 3] = aL[0]; a.gloc[row * 3 + 1] = aL[1]; a.gloc[row * 3 + 2] = aL[2]; }
            if (valid && a.gBz) a.gBz[row] = aZ;
            if constexpr (HB1)
                if (valid && a.gb1) { a.gb1[row * 2] = aBr; a.gb1[row * 2 + 1] = aBi; }
        }
        first = false;
    }
}

// the per-spin outputs of the MAPS and CONSTS builds, each may be null; the plain build takes none
struct AbSpinGrads { void *gloc = nullptr, *gBz = nullptr, *gb1 = nullptr, *gC = nullptr; };

// Host: K2abb on k2b_waves persistent waves per batch entry, then the second pass into grad_gr / grad_rf
template <typename T, typename CT, bool MAPS = false, bool CONSTS = false>
int launch_k2abb(const void* ABck, const PulseOps& in, const void* gA, const void* gB, void* grf, void* ggr, void* work,
                 int64_t N, int64_t nM, int64_t nT, hipStream_t st, const AbSpinGrads& sg = {})
{
    dim3 grid;
    int e;
    if (!fused_grid(N * nM * nT, k2b_waves(nM), N, grid, e)) return e;
    AbFusedBwdKArgsT<T, MAPS, CONSTS> a;
    a.ABck = (const T*)ABck; a.in = typed<T>(in); a.gA = (const T*)gA; a.gB = (const T*)gB; a.work = (T*)work;
    a.N = N; a.nM = nM; a.nT = nT; a.P = grid.x;
    if constexpr (MAPS || CONSTS) { a.gloc = (T*)sg.gloc; a.gBz = (T*)sg.gBz; a.gb1 = (T*)sg.gb1; }
    if constexpr (CONSTS) a.gC = (T*)sg.gC;
#define MRPHY_K2ABB(RX_, HB_) \
    hipLaunchKernelGGL((k_ab_rfgr_bwd<T, CT, RX_, HB_, MAPS, CONSTS>), grid, dim3(WAVE), 0, st, a)
    if (in.b1) { if (in.E1.p) MRPHY_K2ABB(true, true);  else MRPHY_K2ABB(false, true); }
    else       { if (in.E1.p) MRPHY_K2ABB(true, false); else MRPHY_K2ABB(false, false); }
#undef MRPHY_K2ABB
    e = launch_status();
    if (e || !(grf || ggr)) return e;
    return launch_p2<T>(work, ggr, 3, grf, 1, N, nT, grid.x, st);
}

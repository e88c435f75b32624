/* mrphy_hip.h -- C ABI of libmrphy_hip.so, the MI355X (gfx950) Bloch-simulation hot path.
 *
 * This is the drop-in boundary for ONE path of tianrluo/MRphy.py (reference v0.2.0):
 *
 *     mrphy.beffective.rfgr2beff   (reference mrphy/beffective.py:107-168)
 *     mrphy.sims.blochsim          (reference mrphy/sims.py:272-315; BlochSim.forward :32-132,
 *                                   BlochSim.backward :135-269)
 *     mrphy.slowsims.blochsim_1step(reference mrphy/slowsims.py:15-54)
 *
 * plus, in the order of SURVEY.md section 8(f), the callers and helpers either side of it:
 * sims.freeprec (sims.py:318-458), Pulse.interpT linear (mobjs.py:177-220), SpinArray.extract /
 * embed and SpinCube._update_loc_ (mobjs.py:512-553, 815-839), beffective.beff2ab and
 * slowsims.blochsim_ab (beffective.py:40-104, slowsims.py:117-131); and the fused rf,gr -> Mo
 * kernel with its adjoint (one transmit coil, or 2..8 with a b1 map), which is what
 * SpinArray.applypulse composes (mobjs.py:435-446).
 *
 * The reference has no FFI of its own (it is pure Python over ATen); the entry points below are
 * what a ctypes binding for those functions binds to.  INTEGRATION.md shows the reference-side
 * stub.  Conventions:
 *
 *   - plain pointers + sizes only; every pointer is a DEVICE address (hipMalloc'ed / a torch
 *     tensor's data_ptr()), never dereferenced on the host;
 *   - the library allocates nothing, keeps no state and is re-entrant (autograd calls the
 *     backward entry points from another thread); scratch space is passed in by the caller;
 *   - `stream` is a hipStream_t (0 = the null stream); launches are asynchronous, no host sync;
 *   - return value: 0 on success, otherwise a hipError_t value (mrphy_error_string() renders
 *     it) or one of the negative MRPHY_E* codes for argument errors caught on the host;
 *   - "spins" are rows r = n*nM + s of the compact layout (N batches x nM spins);
 *   - a *broadcastable per-spin constant* is passed as (ptr, stride_n, stride_m) in ELEMENTS:
 *     element (n, s) lives at ptr[n*stride_n + s*stride_m]; stride 0 broadcasts.  This covers
 *     the reference's "() | (N|1, nM|1)" shapes and torch's stride-0 expanded views
 *     (mobjs.SpinArray keeps T1_/T2_/gamma_ that way) without materialising them.
 *
 * dtype codes: data type T of M / Beff / rf / gr / loc and constant type CT of the
 * host-computed constants (gamma*2*pi*dt, E1, E2, E1-1):
 */
#ifndef MRPHY_HIP_H
#define MRPHY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* History of the contract.  A caller should check mrphy_abi_version() == MRPHY_ABI_VERSION.
 *   1  round 1: dtype codes 0..2.
 *   2  round 2-3: dtype codes 3 and 4 (precise fp32 step) accepted by every integrating entry
 *      point; mrphy_rfgr2beff_bwd_workspace sizes the one-pass layout for 2..32 coils (round 3:
 *      partial sums + packed per-spin coefficient rows; callers that ask the query see no change);
 *      mrphy_rfgr2beff_bwd returns MRPHY_EINVAL for nC >= 2 without a b1 map; under codes 3 / 4 the
 *      adjoint entry points (blochsim_bwd, blochsim_rfgr_*bwd, beff2ab_bwd) carry the adjoint state
 *      with the compensated update as well (round 3) -- same arguments, different (better) bits.
 *      No environment variable changes what the library runs (the development knobs of rounds 1-6
 *      lived in a separate development build, since retired).
 *   3  round 4: mrphy_freeprec_bwd_consts and mrphy_beff2ab_bwd_consts (gradients w.r.t. the constants that the
 *      reference's autograd supplies through slowsims.freeprec and beffective.beff2ab); the gamma*2*pi*dt column of
 *      mrphy_blochsim_bwd_consts is finite for spins with gamma*2*pi*dt == 0 (it was 0/0); nothing else changed.
 *      Domain of the adjoint entry points under codes 3 / 4 (since ABI 2): E1 and E2 must be non-zero -- the sweep
 *      carries E h and divides by E once at the end, as the reference's adjoint divides at every step
 *      (sims.py:174-177); an E that underflowed to 0 (T < dt/100 in fp32) yields NaN gradients.  The Python layer
 *      raises for such constants; a direct caller uses codes 0 / 2 for them.
 *   4  round 4: mrphy_rfgr2beff_st -- mrphy_rfgr2beff with the cache policy of its stores chosen by the caller
 *      (MRPHY_STORE_*); mrphy_rfgr2beff is that call with MRPHY_STORE_AUTO.  Same bits under every policy.
 *   5  round 6: the history of the blochsim forward / adjoint may live in 1..8 separately allocated parts
 *      (mrphy_blochsim_hist_part_bytes, mrphy_blochsim_fwd_parts, mrphy_blochsim_bwd_parts); the single-pointer entry
 *      points are the one-part case, unchanged.  RCCL helpers for a ctypes-only multi-GPU consumer
 *      live in a library of their own beside this one (include/mrphy_comm.h, libmrphy_comm.so).  Same bits.
 *      Added later under the same version, changing no existing call: mrphy_blochsim_rfgr_traj_fwd,
 *      mrphy_blochsim_rfgr_traj_bwd, mrphy_blochsim_rfgr_mc_traj_bwd (the magnetisation trajectory of K2);
 *      mrphy_signal_rfgr_fwd_workspace, mrphy_signal_rfgr_fwd, mrphy_signal_rfgr_bwd (the received signal of K2:
 *      the transverse magnetisation summed over the spins, sample by sample); mrphy_signal_rfgr_max_rx,
 *      mrphy_signal_rfgr_mrx_fwd_workspace, mrphy_signal_rfgr_mrx_fwd, mrphy_signal_rfgr_mrx_bwd (the same for the coils
 *      of a receive array from ONE simulation per launch); mrphy_blochsim_rfgr_maps_bwd (K2b / K2bt of one transmit
 *      coil, which also returns the gradients w.r.t. loc, df and b1); mrphy_blochsim_rfgr_consts_bwd,
 *      mrphy_signal_rfgr_consts_bwd (the same adjoints, which also return the gradients w.r.t. the step constants
 *      g = gamma 2 pi dt, E1, E2, E1m1 per spin); mrphy_ab_rfgr_fwd, mrphy_ab_rfgr_bwd (Hargreaves' A, B of a pulse
 *      from rf and gr without Beff in memory, and the adjoint w.r.t. the pulse); mrphy_ab_rfgr_maps_bwd,
 *      mrphy_ab_rfgr_consts_bwd (that adjoint, which also returns the gradients w.r.t. loc, df and b1 -- and w.r.t. the
 *      step constants -- per spin); mrphy_ab_steadystate_fwd,
 *      mrphy_ab_steadystate_bwd (the steady state of a periodic pulse from A, B and a rest period, and its adjoint);
 *      mrphy_ab_rfgr_mc_max_coils, mrphy_ab_rfgr_mc_bwd_workspace, mrphy_ab_rfgr_mc_fwd, mrphy_ab_rfgr_mc_bwd (A, B and
 *      the adjoint w.r.t. the pulse under parallel transmit, 2 .. 8 coils with their b1 map); mrphy_ab_train_fwd,
 *      mrphy_ab_train_bwd (the transient of a pulse repeated K times with an RF phase per repetition, and its adjoint);
 *      mrphy_train_signal_ck_every, mrphy_train_signal_max_rx, mrphy_train_signal_workspace, mrphy_train_signal_fwd,
 *      mrphy_train_signal_bwd (the received signal of that transient: the transverse magnetisation of its records summed
 *      over the spins, for up to 8 receive coils per launch, and its adjoint); mrphy_ab_sequence_bwd_workspace,
 *      mrphy_ab_sequence_fwd, mrphy_ab_sequence_bwd (that transient with a pulse of a bank and a rest duration per
 *      repetition, and its adjoint); mrphy_sequence_signal_workspace, mrphy_sequence_signal_bank_workspace,
 *      mrphy_sequence_signal_fwd, mrphy_sequence_signal_bwd (the received signal of that sequence, and its adjoint);
 *      mrphy_sequence_steadystate_fwd, mrphy_sequence_steadystate_bwd (the steady state of that sequence played as one
 *      period, and its adjoint); mrphy_blochsim_rfgr_moving_fwd, mrphy_blochsim_rfgr_moving_bwd (K2 / K2b for spins that
 *      move at constant velocity); mrphy_blochsim_rfgr_shim_max_channels, mrphy_blochsim_rfgr_shim_bwd_workspace,
 *      mrphy_blochsim_rfgr_shim_fwd, mrphy_blochsim_rfgr_shim_bwd (K2 / K2b with extra Bz field channels, and the adjoint
 *      w.r.t. their waveforms); mrphy_blochsim_rfgr_jvp_max_dirs, mrphy_blochsim_rfgr_jvp_fwd (K2 with the forward-mode
 *      tangents of Mo along up to 4 directions per launch); mrphy_ab_sequence_jvp_max_dirs, mrphy_ab_sequence_jvp_fwd
 *      (the sequence's records with their forward-mode tangents along up to 4 directions per launch). */
#define MRPHY_ABI_VERSION 5

#define MRPHY_F32      0  /* T = float,  CT = float                                          */
#define MRPHY_F64      1  /* T = double, CT = double                                         */
#define MRPHY_F32_C64  2  /* T = float,  CT = double: the reference's behaviour when fp32 data
                             meets its fp64 default constants (sims.py:62-64,74-77 promote)  */
#define MRPHY_F32P     3  /* as MRPHY_F32 with the PRECISE fp32 step: S = sin(phi)/phi and
                             C = (1-cos(phi))/phi^2 evaluated in fp64 and rounded once, rounding
                             errors of the update and of the relaxation product carried (FMA
                             error-free transformations).  128^3 x 4096, phi <= 2.6 rad per step:
                             4.8e-6 relative L2 from exact arithmetic (MRPHY_F32: 2.0e-5, the
                             reference's own fp32 runs 2.6e-5); ~1.8x the arithmetic per step.
                             Accepted wherever MRPHY_F32 is by the entry points that integrate
                             (blochsim_fwd/_bwd/_1step, blochsim_rfgr_*, beff2ab).  The adjoint
                             sweeps take the same treatment (round 3): they carry t = E h, whose
                             recursion t <- E R^T t has the forward step's shape, through the same
                             compensated update with the same once-rounded S, C.  64^3 x 2048
                             (BASELINE configs[4]), all spins, against fp64 differentiation of
                             the same function: grad_M0 4.0e-6, grad_rf 2.9e-7, grad_gr 1.8e-6
                             (MRPHY_F32: 1.24e-5, 4.0e-6, 1.26e-5)                            */
#define MRPHY_F32P_C64 4  /* as MRPHY_F32_C64 with the precise step                          */

#define MRPHY_EINVAL  (-1)  /* bad argument (null pointer, negative size, unknown dtype)     */
#define MRPHY_EALIGN  (-2)  /* a pointer is not aligned to its element size                  */
#define MRPHY_ENOSPC  (-3)  /* workspace too small                                           */

/* Library identity / diagnostics. */
int         mrphy_abi_version(void);
const char* mrphy_error_string(int code);
/* Compiled offload architecture, e.g. "gfx950". */
const char* mrphy_arch(void);

/* Diagnostic (no reference counterpart): out[b] = id (0..7) of the XCD that workgroup b of a 1-D
 * grid of `nblocks` one-wave workgroups ran on (HW_REG_XCC_ID).  The kernels that write large
 * tensors give every XCD a contiguous share of the output by assuming that blocks b and b + 8
 * share an XCD; bench.py records whether the process really got that dealing. */
int mrphy_debug_xcc_map(int32_t* out, int64_t nblocks, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K0  rfgr2beff -- replaces mrphy.beffective.rfgr2beff (beffective.py:107-168).
 *
 *   beff[n,s,t,0] = sum_c b1[n,s,0,c]*rf[n,0,t,c] - b1[n,s,1,c]*rf[n,1,t,c]
 *   beff[n,s,t,1] = sum_c b1[n,s,0,c]*rf[n,1,t,c] + b1[n,s,1,c]*rf[n,0,t,c]
 *   beff[n,s,t,2] = loc[n,s,:] . gr[n,:,t] + df[n,s]/gamma[n,s]
 *
 *   rf   (N|1, 2, nT, nC) contiguous, batch stride rf_sn elements (0 broadcasts the pulse)
 *   gr   (N|1, 3, nT)     contiguous, batch stride gr_sn
 *   loc  (N, nM, 3)       contiguous
 *   df, gamma             broadcastable per-spin constants; df may be NULL (no off-resonance)
 *   b1   (N, nM, 2, nC)   contiguous, or NULL: then nC must be 1 and Bx,By = rf (the host sums
 *                          a multi-coil rf over coils first, beffective.py:148-149)
 *   beff (N, nM, nT, 3)   contiguous output
 * Any nC: up to 64 coils (32 in fp64) in one launch; beyond, in blocks of that many coils whose launches
 * continue the ascending FMA chains of Bx, By from the values stored by the launch before (one extra read +
 * write pass over beff per block; the same bits as a single chain).
 * ------------------------------------------------------------------------------------------- */
int mrphy_rfgr2beff(int dtype,
                    const void* rf, int64_t rf_sn,
                    const void* gr, int64_t gr_sn,
                    const void* loc,
                    const void* df, int64_t df_sn, int64_t df_sm,
                    const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                    const void* b1,
                    void* beff,
                    int64_t N, int64_t nM, int64_t nT, int64_t nC,
                    void* stream);

/* The same with the cache policy of the Beff stores chosen by the caller (ABI 4).  What the stores leave in the
 * 256-MB memory-side cache decides how fast the kernel that reads Beff next starts (DESIGN.md "K1 right behind
 * K0"), what the writer pays for each encoding depends on the box and the block, and nothing a process can read
 * tells which: a caller that owns the block can time both (mrphy_amd.workspace.BeffArena does).
 *   MRPHY_STORE_AUTO   what mrphy_rfgr2beff does: SC1NT below 8 GB of Beff, NT from there up (round 5)
 *   MRPHY_STORE_PLAIN  cached stores
 *   MRPHY_STORE_NT     the non-temporal hint
 *   MRPHY_STORE_SC1NT  agent-scope write-through + non-temporal (16-byte stores; narrower ones take NT)
 * Any other value: MRPHY_EINVAL.  The results do not depend on the policy. */
#define MRPHY_STORE_AUTO  (-1)
#define MRPHY_STORE_PLAIN 0
#define MRPHY_STORE_NT    1
#define MRPHY_STORE_SC1NT 2
int mrphy_rfgr2beff_st(int dtype,
                       const void* rf, int64_t rf_sn,
                       const void* gr, int64_t gr_sn,
                       const void* loc,
                       const void* df, int64_t df_sn, int64_t df_sm,
                       const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                       const void* b1,
                       void* beff,
                       int64_t N, int64_t nM, int64_t nT, int64_t nC,
                       int store_policy,
                       void* stream);

/* Adjoint of K0 w.r.t. rf and gr (what autograd derives from beffective.py:137,160-165):
 *
 *   grad_gr[n,i,t]   = sum_s loc[n,s,i] * gB[n,s,t,2]
 *   grad_rf[n,0,t,c] = sum_s b1[n,s,0,c]*gB[n,s,t,0] + b1[n,s,1,c]*gB[n,s,t,1]
 *   grad_rf[n,1,t,c] = sum_s b1[n,s,0,c]*gB[n,s,t,1] - b1[n,s,1,c]*gB[n,s,t,0]
 *
 * Outputs are per-batch (N, 2, nT, nC) / (N, 3, nT); a broadcast pulse is reduced over n by the
 * caller.  Deterministic two-pass reduction over spins (fixed order, no float atomics).
 * `work` must hold mrphy_rfgr2beff_bwd_workspace(...) bytes.  b1 == NULL requires nC == 1, as in
 * mrphy_rfgr2beff (MRPHY_EINVAL otherwise).  With a map, 2..32 coils take ONE pass over grad_beff
 * (a thread owns a time point and its 2 nC + 3 running sums; the spins' b1 and loc, packed and
 * zero-padded into the tail of `work` by a pre-pass, reach the FMAs as scalar operands); more coils
 * take nC + 1 passes.  The workspace size depends on the path: always ask the query.
 */
size_t mrphy_rfgr2beff_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t nC);
int mrphy_rfgr2beff_bwd(int dtype,
                        const void* grad_beff,
                        const void* loc,
                        const void* b1,
                        void* grad_rf, void* grad_gr,
                        void* work, size_t work_bytes,
                        int64_t N, int64_t nM, int64_t nT, int64_t nC,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * K1  blochsim forward -- replaces mrphy.sims.BlochSim.forward (sims.py:32-132) with the
 * wrapper logic of sims.blochsim (sims.py:305-313) done by the caller.
 *
 * Per step t, with bt = g*Beff[n,s,t,:]  (g = gamma*2*pi*dt, computed by the host in the
 * reference's dtype, sims.py:62):
 *     rotate M about bt by -|bt| (Rodrigues, sims.py:100-121), then, if E1 != NULL,
 *     M <- (E2*Mx, E2*My, E1*Mz - E1m1)                           (sims.py:74-77,124)
 *
 *   Mi    (N, nM, 3)       contiguous, not modified
 *   Beff  (N, nM, nT, 3)   contiguous, not modified
 *   g, E1, E2, E1m1        broadcastable per-spin constants of type CT; E1==E2==E1m1==NULL
 *                          disables relaxation (reference T1=T2=None); E1m1 shares E1's strides
 *   Mo    (N, nM, 3)       contiguous output, final magnetisation
 *   Mpre                   optional (NULL = not wanted) history buffer of
 *                          mrphy_blochsim_hist_bytes() bytes: the magnetisation BEFORE each step,
 *                          the only history mrphy_blochsim_bwd needs (12 B per spin-step; the
 *                          reference keeps 40, sims.py:84-88).  Its layout is internal to the
 *                          library (per 64-spin tile, structure of arrays): pass it back to
 *                          mrphy_blochsim_bwd unchanged.
 * ------------------------------------------------------------------------------------------- */
size_t mrphy_blochsim_hist_bytes(int dtype, int64_t N, int64_t nM, int64_t nT);
int mrphy_blochsim_fwd(int dtype,
                       const void* Mi, const void* Beff,
                       const void* g,  int64_t g_sn,  int64_t g_sm,
                       const void* E1, int64_t E1_sn, int64_t E1_sm,
                       const void* E2, int64_t E2_sn, int64_t E2_sm,
                       const void* E1m1,
                       void* Mo, void* Mpre,
                       int64_t N, int64_t nM, int64_t nT,
                       void* stream);

/* K1h with the history in parts (ABI 5) -- the same forward; the history (sims.py:84-88) goes to `n_parts`
 * (1..MRPHY_HIST_MAX_PARTS) SEPARATELY ALLOCATED buffers of mrphy_blochsim_hist_part_bytes() bytes each instead of
 * one buffer.  Why: the rate at which a kernel can stream writes into a block depends on where the driver put the
 * block's physical pages (0.62 or 0.75 of HBM peak for K1h); a write stream spread over two
 * blocks from different allocations runs in the fast mode where one block of the same total size usually does not.
 * The history is internal to the library, so nothing forces it to be one allocation.
 *
 *   hist_parts   HOST array of n_parts device pointers (read during the call only); NULL or n_parts = 0: no history
 *   layout       how the 64-spin tiles are dealt to the parts:
 *                  MRPHY_HIST_BLOCKED      tile t -> part t / ceil(tiles / n_parts): with the XCD-contiguous block
 *                                          order of K1h / K3 every part is written by its own group of XCDs
 *                  MRPHY_HIST_INTERLEAVED  tile t -> part t % n_parts
 *                pass the same parts, in the same order, with the same layout to mrphy_blochsim_bwd_parts.
 * Results are bit-identical to mrphy_blochsim_fwd / _bwd (the kernels are the same; only a tile's base address differs).
 */
#define MRPHY_HIST_MAX_PARTS 8
#define MRPHY_HIST_BLOCKED      0
#define MRPHY_HIST_INTERLEAVED  1
size_t mrphy_blochsim_hist_part_bytes(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t n_parts);
int mrphy_blochsim_fwd_parts(int dtype,
                             const void* Mi, const void* Beff,
                             const void* g,  int64_t g_sn,  int64_t g_sm,
                             const void* E1, int64_t E1_sn, int64_t E1_sm,
                             const void* E2, int64_t E2_sn, int64_t E2_sm,
                             const void* E1m1,
                             void* Mo,
                             void* const* hist_parts, int64_t n_parts, int layout,
                             int64_t N, int64_t nM, int64_t nT,
                             void* stream);

/* K3 reading a history in parts: mrphy_blochsim_bwd (grad_consts = NULL) or mrphy_blochsim_bwd_consts
 * (grad_consts (N, nM, 4)) -- see below -- over the parts mrphy_blochsim_fwd_parts filled. */
int mrphy_blochsim_bwd_parts(int dtype,
                             const void* const* hist_parts, int64_t n_parts, int layout,
                             const void* Beff,
                             const void* g,  int64_t g_sn,  int64_t g_sm,
                             const void* E1, int64_t E1_sn, int64_t E1_sm,
                             const void* E2, int64_t E2_sn, int64_t E2_sm,
                             const void* grad_Mo,
                             void* grad_Mi, void* grad_Beff, void* grad_consts,
                             int64_t N, int64_t nM, int64_t nT,
                             void* stream);

/* K3  blochsim backward -- replaces mrphy.sims.BlochSim.backward (sims.py:135-269).
 *
 *   grad_Mo   (N, nM, 3)      contiguous
 *   grad_Mi   (N, nM, 3)      output, may be NULL
 *   grad_Beff (N, nM, nT, 3)  output, may be NULL; never aliases a saved tensor (the reference
 *                             overwrites its saved gamma*Beff, sims.py:239-264 -- not replicated)
 * Mpre is the history buffer mrphy_blochsim_fwd filled for the same (dtype, N, nM, nT).
 * E1m1 is not needed: the rotated, pre-relaxation magnetisation is recomputed from Mpre.
 */
int mrphy_blochsim_bwd(int dtype,
                       const void* Mpre, const void* Beff,
                       const void* g,  int64_t g_sn,  int64_t g_sm,
                       const void* E1, int64_t E1_sn, int64_t E1_sm,
                       const void* E2, int64_t E2_sn, int64_t E2_sm,
                       const void* grad_Mo,
                       void* grad_Mi, void* grad_Beff,
                       int64_t N, int64_t nM, int64_t nT,
                       void* stream);

/* As mrphy_blochsim_bwd, and in the same sweep the gradients w.r.t. the per-spin constants (round 3):
 *   grad_consts (N, nM, 4)  output: [dL/d(gamma*2*pi*dt), dL/dE1, dL/dE2, dL/d(E1-1)] per spin,
 *                           E1 and E1-1 treated as the two separate inputs they are.
 * The reference's slowsims.blochsim / blochsim_1step are plain differentiable torch ops
 * (slowsims.py:86-112, 42-51), so its callers get gradients w.r.t. T1, T2, gamma, dt; the host layer
 * chains these four to them (mrphy_amd.slowsims).  Without relaxation (E1 = E2 = NULL) only the first
 * entry is meaningful (the others are 0).  gamma*2*pi*dt must be non-zero.  Any shape / alignment
 * (the chunked adjoint kernel); about 25 more VALU operations per step than mrphy_blochsim_bwd.
 */
int mrphy_blochsim_bwd_consts(int dtype,
                              const void* Mpre, const void* Beff,
                              const void* g,  int64_t g_sn,  int64_t g_sm,
                              const void* E1, int64_t E1_sn, int64_t E1_sm,
                              const void* E2, int64_t E2_sn, int64_t E2_sm,
                              const void* grad_Mo,
                              void* grad_Mi, void* grad_Beff, void* grad_consts,
                              int64_t N, int64_t nM, int64_t nT,
                              void* stream);

/* blochsim_1step -- replaces mrphy.slowsims.blochsim_1step (slowsims.py:15-54): one step with
 * caller-supplied E1, E1-1, E2, gamma*2*pi*dt.  M (N,nM,3), b (N,nM,3) -> Mout (N,nM,3).
 * Mout may alias M (the reference mutates M in place on its all-zero-field branch).
 */
int mrphy_blochsim_1step(int dtype,
                         const void* M, const void* b,
                         const void* g,  int64_t g_sn,  int64_t g_sm,
                         const void* E1, int64_t E1_sn, int64_t E1_sm,
                         const void* E2, int64_t E2_sn, int64_t E2_sm,
                         const void* E1m1,
                         void* Mout,
                         int64_t N, int64_t nM,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2  fused rf,gr -> Mo: mrphy.mobjs.SpinArray.applypulse's back-to-back
 * rfgr2beff + blochsim (mobjs.py:435-446) without materialising Beff (N,nM,nT,3) in HBM.
 * Same operands as K0 and K1 together (`gamma` is the rfgr2beff one that divides df, `g` the
 * blochsim one).  Mck (nCk, N, nM, 3), nCk = ceil(nT/ck_every), receives the magnetisation
 * before steps 0, ck_every, 2*ck_every, ... when not NULL (checkpoints for an adjoint sweep;
 * ck_every must be a positive multiple of 8, the kernel's step batch).
 * Coils: register / LDS builds for 1, 2, 4, 8 (both precisions) and 16 ... 64 coils (float); more coils
 * than that run a generic build that re-reads rf and b1 from memory inside the coil loop (correct, two
 * orders of magnitude slower): call mrphy_rfgr2beff + mrphy_blochsim_fwd there, as the Python layer does.
 * ------------------------------------------------------------------------------------------- */
int mrphy_blochsim_rfgr_fwd(int dtype,
                            const void* Mi,
                            const void* rf, int64_t rf_sn,
                            const void* gr, int64_t gr_sn,
                            const void* loc,
                            const void* df, int64_t df_sn, int64_t df_sm,
                            const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                            const void* b1,
                            const void* g,  int64_t g_sn,  int64_t g_sm,
                            const void* E1, int64_t E1_sn, int64_t E1_sm,
                            const void* E2, int64_t E2_sn, int64_t E2_sm,
                            const void* E1m1,
                            void* Mo, void* Mck, int64_t ck_every,
                            int64_t N, int64_t nM, int64_t nT, int64_t nC,
                            void* stream);

/* K2b  adjoint of K2 (single-coil rf: rf (N|1, 2, nT, 1), b1 (N, nM, 2, 1) or NULL):
 *   grad_Mo (N,nM,3) -> grad_Mi (N,nM,3; may be NULL), grad_rf (N,2,nT), grad_gr (N,3,nT) (either may
 *   be NULL), per batch entry; a broadcast pulse is reduced over n by the caller.
 * Mck must be the checkpoints K2 wrote with ck_every = mrphy_blochsim_rfgr_ck_every(); nT must be a
 * multiple of it.  Each checkpoint segment is recomputed forward in registers, then swept
 * backwards; the reduction over spins is deterministic (per-wave partial rows in `work`, summed in
 * fixed order; no float atomics).  `work` must hold mrphy_blochsim_rfgr_bwd_workspace() bytes.
 */
int64_t mrphy_blochsim_rfgr_ck_every(void);
size_t mrphy_blochsim_rfgr_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT);
int mrphy_blochsim_rfgr_bwd(int dtype,
                            const void* Mck,
                            const void* rf, int64_t rf_sn,
                            const void* gr, int64_t gr_sn,
                            const void* loc,
                            const void* df, int64_t df_sn, int64_t df_sm,
                            const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                            const void* b1,
                            const void* g,  int64_t g_sn,  int64_t g_sm,
                            const void* E1, int64_t E1_sn, int64_t E1_sm,
                            const void* E2, int64_t E2_sn, int64_t E2_sm,
                            const void* E1m1,
                            const void* grad_Mo,
                            void* grad_Mi, void* grad_rf, void* grad_gr,
                            void* work, size_t work_bytes,
                            int64_t N, int64_t nM, int64_t nT,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * freeprec -- mrphy.sims.FreePrec forward / backward (sims.py:318-421; wrapper freeprec :424-458;
 * oracle form slowsims.py:134-174): precession by -2 pi df dur about z, then relaxation
 *     Mxy *= exp(-dur/T2),  Mz <- Mz exp(-dur/T1) - expm1(-dur/T1).
 *   Mi / Mo (N, nM, 3); dur (N|1,) with element stride dur_sn (0 broadcasts); T1, T2, df
 *   broadcastable per-spin constants of the DATA type; T1 == T2 == NULL: no relaxation;
 *   df == NULL: no precession.  The backward maps grad_Mo -> grad_Mi (the only input the
 *   reference differentiates, sims.py:321) and recomputes phi, E1, E2 instead of saving them.
 * ------------------------------------------------------------------------------------------- */
int mrphy_freeprec_fwd(int dtype, const void* Mi,
                       const void* dur, int64_t dur_sn,
                       const void* T1, int64_t T1_sn, int64_t T1_sm,
                       const void* T2, int64_t T2_sn, int64_t T2_sm,
                       const void* df, int64_t df_sn, int64_t df_sm,
                       void* Mo, int64_t N, int64_t nM, void* stream);
int mrphy_freeprec_bwd(int dtype, const void* grad_Mo,
                       const void* dur, int64_t dur_sn,
                       const void* T1, int64_t T1_sn, int64_t T1_sm,
                       const void* T2, int64_t T2_sn, int64_t T2_sm,
                       const void* df, int64_t df_sn, int64_t df_sm,
                       void* grad_Mi, int64_t N, int64_t nM, void* stream);

/* Gradients of freeprec w.r.t. its constants, per spin -- what autograd through the reference's plain torch ops
 * gives a caller of mrphy.slowsims.freeprec who differentiates w.r.t. dur, T1, T2, df (slowsims.py:151-174):
 *     grad_consts (N, nM, 4) = [dL/d dur, dL/d T1, dL/d T2, dL/d df]   (0 where the operand is NULL);
 * the caller sums each column over the axes its operand broadcasts along.  Mi is the INPUT magnetisation of the
 * forward call, grad_Mo the cotangent of its output. */
int mrphy_freeprec_bwd_consts(int dtype, const void* Mi, const void* grad_Mo,
                              const void* dur, int64_t dur_sn,
                              const void* T1, int64_t T1_sn, int64_t T1_sm,
                              const void* T2, int64_t T2_sn, int64_t T2_sm,
                              const void* df, int64_t df_sn, int64_t df_sm,
                              void* grad_consts, int64_t N, int64_t nM, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Linear time resampling of a pulse -- mrphy.mobjs.Pulse.interpT(kind='linear') (mobjs.py:177-220)
 * without the device -> host -> scipy -> device round trip.  `y` holds nch channels of nTo samples
 * (rf and gr rows), `out` nch x nTn.  The host supplies the grid (it depends on nTo, dt_old, dt_new
 * only): lo[j] = index of the left neighbour in the ZERO-PREPENDED source (mobjs.py:204-207; 0 means
 * the prepended sample), w[j] = t_new[j] - t[lo[j]], dx[j] = t[lo[j]+1] - t[lo[j]], fp64.
 * dir > 0: out = interp(y).  dir <= 0: the adjoint, `y` = grad wrt the resampled pulse (nch x nTn),
 * `out` = grad wrt the source (nch x nTo).  An empty result (nTn == 0: dt_new longer than the whole
 * pulse) has a zero adjoint: `out` is zeroed, `y` and the grid may then be NULL (here and in _select).
 * ------------------------------------------------------------------------------------------- */
int mrphy_pulse_interp_linear(int dtype, int dir, const void* y, void* out,
                              const void* lo, const void* w, const void* dx,
                              int64_t nch, int64_t nTo, int64_t nTn, void* stream);

/* The one-tap kinds of the same resampling -- mobjs.Pulse.interpT(kind=...) passes `kind` to
 * scipy.interpolate.interp1d (mobjs.py:201,214-215): 'nearest', 'nearest-up', 'previous', 'next',
 * 'zero'.  Each output sample is one sample of the zero-prepended source: sel[j] in [0, nTo]
 * (int32; 0 = the prepended zero, k >= 1 = y[., k - 1]), NON-DECREASING in j, computed by the host
 * for the grid (it depends on nTo, dt_old, dt_new and the kind only).  The caller guarantees the
 * range of sel; no arithmetic is done, so results equal the reference's bit for bit.
 * dir > 0: out (nch x nTn) = select(y (nch x nTo)).  dir <= 0: the adjoint, `y` = grad w.r.t. the
 * resampled pulse (nch x nTn), `out` = grad w.r.t. the source (nch x nTo), summed in j order. */
int mrphy_pulse_interp_select(int dtype, int dir, const void* y, void* out, const void* sel,
                              int64_t nch, int64_t nTo, int64_t nTn, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The two helpers mrphy.slowsims.blochsim_1step is written with in the reference.
 *
 * beff2uphi -- mrphy.beffective.beff2u\u03d5 (beffective.py:18-37):
 *     U = b / max(|b|, 1e-12),  Phi = -|b| * g          b (N,nM,3) -> U (N,nM,3), Phi (N,nM)
 * uphirot   -- mrphy.utils.u\u03d5rot (utils.py:333-359), Rodrigues rotation of nV vectors per row:
 *     Vo = cos(Phi) Vi + (1 - cos(Phi)) (U.Vi) U + sin(Phi) U x Vi
 *     U (rows,3), Phi (rows), Vi/Vo (rows, 3, nV) contiguous; Vo must not alias Vi.
 * ------------------------------------------------------------------------------------------- */
int mrphy_beff2uphi(int dtype, const void* b,
                    const void* g, int64_t g_sn, int64_t g_sm,
                    void* U, void* Phi, int64_t N, int64_t nM, void* stream);
int mrphy_uphirot(int dtype, const void* U, const void* Phi, const void* Vi, void* Vo,
                  int64_t rows, int64_t nV, void* stream);

/* Their adjoints.  The reference differentiates both through autograd over plain torch ops
 * (beffective.py:35-36: F.normalize + torch.norm; utils.py:351-357), which slowsims.blochsim_1step
 * -- the reference's implicit-Jacobian path -- relies on.
 *
 * beff2uphi_bwd: grad_U (N,nM,3) and grad_Phi (N,nM) (either may be NULL = zero) ->
 *     grad_b (N,nM,3) (NULL: skipped) and, if grad_g != NULL, the PER-SPIN gradient w.r.t. g,
 *     (N,nM), which the caller sums down to g's broadcast shape.
 * uphirot_bwd: grad_Vo (rows,3,nV) -> grad_U (rows,3), grad_Phi (rows) (summed over the nV
 *     vectors; U is treated as a free vector, as autograd does), grad_Vi (rows,3,nV); any output
 *     may be NULL. */
int mrphy_beff2uphi_bwd(int dtype, const void* b,
                        const void* g, int64_t g_sn, int64_t g_sm,
                        const void* grad_U, const void* grad_Phi, void* grad_b, void* grad_g,
                        int64_t N, int64_t nM, void* stream);
int mrphy_uphirot_bwd(int dtype, const void* U, const void* Phi, const void* Vi,
                      const void* grad_Vo, void* grad_U, void* grad_Phi, void* grad_Vi,
                      int64_t rows, int64_t nV, void* stream);

/* K2b for parallel transmit (nC = 1 .. mrphy_blochsim_rfgr_mc_max_coils() coils): as
 * mrphy_blochsim_rfgr_bwd, with rf (N|1, 2, nT, nC), b1 (N, nM, 2, nC) (required) and
 * grad_rf (N, 2, nT, nC).  The reference reaches these gradients through autograd over
 * rfgr2beff's complex coil sum (beffective.py:153-165) and BlochSim.backward (sims.py:135-269).
 * `work` must hold mrphy_blochsim_rfgr_mc_bwd_workspace() bytes.
 */
int64_t mrphy_blochsim_rfgr_mc_max_coils(void);
size_t mrphy_blochsim_rfgr_mc_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t nC);
int mrphy_blochsim_rfgr_mc_bwd(int dtype,
                               const void* Mck,
                               const void* rf, int64_t rf_sn,
                               const void* gr, int64_t gr_sn,
                               const void* loc,
                               const void* df, int64_t df_sn, int64_t df_sm,
                               const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                               const void* b1,
                               const void* g,  int64_t g_sn,  int64_t g_sm,
                               const void* E1, int64_t E1_sn, int64_t E1_sm,
                               const void* E2, int64_t E2_sn, int64_t E2_sm,
                               const void* E1m1,
                               const void* grad_Mo,
                               void* grad_Mi, void* grad_rf, void* grad_gr,
                               void* work, size_t work_bytes,
                               int64_t N, int64_t nM, int64_t nT, int64_t nC,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2t  trajectory of the fused simulation: K2 that also records M after steps
 *     e_j = min((j+1) * every, nT) - 1,   j = 0 .. nRec-1,   nRec = ceil(nT / every),
 * into Mt (nRec, N, nM, 3), time-major (record j is one (N, nM, 3) block: 768 B per wave and record, the
 * checkpoint layout).  The reference keeps the whole history Mhst (N, *Nd, nT, xyz) in BlochSim.forward and
 * returns only its last step (sims.py:83,131); every == 1 gives that history, and the last record is always Mo
 * bit for bit (a record is the state the step loop holds; nothing else changes).
 * Operands as mrphy_blochsim_rfgr_fwd; Mo may be NULL (it equals record nRec-1).  Mck / ck_every as there
 * (checkpoints for the adjoint below).  MRPHY_EINVAL: every < 1, Mt NULL, a coil count K2 rejects.
 * ------------------------------------------------------------------------------------------- */
int mrphy_blochsim_rfgr_traj_fwd(int dtype,
                                 const void* Mi,
                                 const void* rf, int64_t rf_sn,
                                 const void* gr, int64_t gr_sn,
                                 const void* loc,
                                 const void* df, int64_t df_sn, int64_t df_sm,
                                 const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                 const void* b1,
                                 const void* g,  int64_t g_sn,  int64_t g_sm,
                                 const void* E1, int64_t E1_sn, int64_t E1_sm,
                                 const void* E2, int64_t E2_sn, int64_t E2_sm,
                                 const void* E1m1,
                                 void* Mo, void* Mck, int64_t ck_every,
                                 void* Mt, int64_t every,
                                 int64_t N, int64_t nM, int64_t nT, int64_t nC,
                                 void* stream);

/* K2bt  adjoint of K2t: as mrphy_blochsim_rfgr_bwd / mrphy_blochsim_rfgr_mc_bwd, with grad_Mt (nRec, N, nM, 3)
 * (time-major, as Mt) in place of grad_Mo -- its last record is the cotangent of Mo.  The sweep adds grad_Mt[j]
 * to the adjoint state as it passes step e_j backwards: what the reference's autograd does with a loss on Mhst
 * (BlochSim.backward, sims.py:135-269, run once per recorded step).  Same checkpoints (nT a multiple of
 * mrphy_blochsim_rfgr_ck_every()), same workspace (mrphy_blochsim_rfgr_bwd_workspace /
 * mrphy_blochsim_rfgr_mc_bwd_workspace), same deterministic reduction.  MRPHY_EINVAL: every < 1, nT not a
 * whole number of segments, a coil count outside 1 .. mrphy_blochsim_rfgr_mc_max_coils() (mc); MRPHY_ENOSPC:
 * workspace too small. */
int mrphy_blochsim_rfgr_traj_bwd(int dtype,
                                 const void* Mck,
                                 const void* rf, int64_t rf_sn,
                                 const void* gr, int64_t gr_sn,
                                 const void* loc,
                                 const void* df, int64_t df_sn, int64_t df_sm,
                                 const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                 const void* b1,
                                 const void* g,  int64_t g_sn,  int64_t g_sm,
                                 const void* E1, int64_t E1_sn, int64_t E1_sm,
                                 const void* E2, int64_t E2_sn, int64_t E2_sm,
                                 const void* E1m1,
                                 const void* grad_Mt, int64_t every,
                                 void* grad_Mi, void* grad_rf, void* grad_gr,
                                 void* work, size_t work_bytes,
                                 int64_t N, int64_t nM, int64_t nT,
                                 void* stream);
/* K2b / K2bt with the gradients w.r.t. the spin-side operands (one transmit coil): mrphy_blochsim_rfgr_bwd (a null
 * grad_Mt; grad_Mo is read) or mrphy_blochsim_rfgr_traj_bwd (a null grad_Mo; grad_Mt and `every` are read), and in the
 * same sweep
 *     grad_loc (N, nM, 3)   dL/dloc[n,s,i]      = sum_t gBz[n,s,t] * gr[n,i,t]
 *     grad_Bz  (N, nM)      dL/d(df/gamma)[n,s] = sum_t gBz[n,s,t]        (the caller divides by gamma for dL/d df)
 *     grad_b1  (N, nM, 2)   dL/db1[n,s,0] = sum_t gBx*rf_re + gBy*rf_im,  dL/db1[n,s,1] = sum_t gBy*rf_re - gBx*rf_im
 * where (gBx, gBy, gBz)[n,s,t] is the dL/dBeff that the two-kernel route would have written to memory.  Each of the
 * three is optional (null: not wanted), as grad_Mi, grad_rf, grad_gr are -- which come out bit for bit as the entry
 * points above give them.  The sums over time are lane-private, in a fixed order (the 16 steps of a checkpoint segment,
 * then the segments, both descending): the same inputs give the same bits.  Same checkpoints, same workspace
 * (mrphy_blochsim_rfgr_bwd_workspace).  The entry point has no coil count: rf is (N|1, 2, nT, 1) and b1 (N, nM, 2) or
 * null, as for mrphy_blochsim_rfgr_bwd; parallel transmit has no such build.  MRPHY_EINVAL: what
 * mrphy_blochsim_rfgr_traj_bwd refuses (every < 1 with a grad_Mt, nT not a whole number of segments, null operands),
 * both or neither of grad_Mo and grad_Mt, a grad_b1 without a b1 map; MRPHY_ENOSPC: workspace too small.  An empty
 * problem is a success that writes nothing. */
int mrphy_blochsim_rfgr_maps_bwd(int dtype,
                                 const void* Mck,
                                 const void* rf, int64_t rf_sn,
                                 const void* gr, int64_t gr_sn,
                                 const void* loc,
                                 const void* df, int64_t df_sn, int64_t df_sm,
                                 const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                 const void* b1,
                                 const void* g,  int64_t g_sn,  int64_t g_sm,
                                 const void* E1, int64_t E1_sn, int64_t E1_sm,
                                 const void* E2, int64_t E2_sn, int64_t E2_sm,
                                 const void* E1m1,
                                 const void* grad_Mo, const void* grad_Mt, int64_t every,
                                 void* grad_Mi, void* grad_rf, void* grad_gr,
                                 void* grad_loc, void* grad_Bz, void* grad_b1,
                                 void* work, size_t work_bytes,
                                 int64_t N, int64_t nM, int64_t nT,
                                 void* stream);
/* mrphy_blochsim_rfgr_maps_bwd with the gradients w.r.t. the step constants besides, in the same sweep:
 *     grad_consts (N, nM, 4)   [dL/dg, dL/dE1, dL/dE2, dL/dE1m1][n,s],  g = gamma 2 pi dt
 * per spin, each the sum over the steps that mrphy_blochsim_bwd_consts forms on the two-kernel route (with u = R m the
 * rotated state of a step and h = dL/dm' the cotangent after it: dL/dE2 += hx ux + hy uy, dL/dE1 += hz uz,
 * dL/dE1m1 -= hz, dL/dg += dL/db . B), in the order of the map sums; without relaxation the last three are zeros.  The
 * caller folds them to its operands: dL/dE1 and dL/dE1m1 add for an E1m1 formed as E1 - 1.  grad_consts is optional like
 * the other outputs; every other output comes out bit for bit as mrphy_blochsim_rfgr_maps_bwd gives it.  Under codes
 * 3 / 4 E1 and E2 must be non-zero (see the history above).  Same checkpoints, workspace, refusals and empty-problem
 * rule as mrphy_blochsim_rfgr_maps_bwd. */
int mrphy_blochsim_rfgr_consts_bwd(int dtype,
                                   const void* Mck,
                                   const void* rf, int64_t rf_sn,
                                   const void* gr, int64_t gr_sn,
                                   const void* loc,
                                   const void* df, int64_t df_sn, int64_t df_sm,
                                   const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                   const void* b1,
                                   const void* g,  int64_t g_sn,  int64_t g_sm,
                                   const void* E1, int64_t E1_sn, int64_t E1_sm,
                                   const void* E2, int64_t E2_sn, int64_t E2_sm,
                                   const void* E1m1,
                                   const void* grad_Mo, const void* grad_Mt, int64_t every,
                                   void* grad_Mi, void* grad_rf, void* grad_gr,
                                   void* grad_loc, void* grad_Bz, void* grad_b1, void* grad_consts,
                                   void* work, size_t work_bytes,
                                   int64_t N, int64_t nM, int64_t nT,
                                   void* stream);
int mrphy_blochsim_rfgr_mc_traj_bwd(int dtype,
                                    const void* Mck,
                                    const void* rf, int64_t rf_sn,
                                    const void* gr, int64_t gr_sn,
                                    const void* loc,
                                    const void* df, int64_t df_sn, int64_t df_sm,
                                    const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                    const void* b1,
                                    const void* g,  int64_t g_sn,  int64_t g_sm,
                                    const void* E1, int64_t E1_sn, int64_t E1_sm,
                                    const void* E2, int64_t E2_sn, int64_t E2_sm,
                                    const void* E1m1,
                                    const void* grad_Mt, int64_t every,
                                    void* grad_Mi, void* grad_rf, void* grad_gr,
                                    void* work, size_t work_bytes,
                                    int64_t N, int64_t nM, int64_t nT, int64_t nC,
                                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2s  received signal of the fused simulation: K2 that, instead of keeping M, sums what a receive coil sees over the
 * spins of each batch entry at the trajectory's record steps
 *     e_j = min((j+1) * every, nT) - 1,   j = 0 .. nRec-1,   nRec = ceil(nT / every):
 *     sig[n, 0, j] = sum_s  rx_re[n,s] Mx[n,s] - rx_im[n,s] My[n,s]
 *     sig[n, 1, j] = sum_s  rx_re[n,s] My[n,s] + rx_im[n,s] Mx[n,s]           (M after step e_j)
 * -- the complex product of b1Map . rf in rfgr2beff (beffective.py:160-165), no conjugate.  sig (N, 2, nRec), the layout
 * of rf; rx (N, nM, 2), the layout of a one-coil b1, or NULL = (1, 0): the plain sums of Mx and My.  The reference has no
 * counterpart: it forms the history Mhst inside BlochSim.forward and drops it (sims.py:83,131); this is the sum over
 * the spins of what mrphy_blochsim_rfgr_traj_fwd records, without the records in memory.  The order of summation is
 * fixed (64 spins in LDS, a wave's tiles in its own workspace row, the rows in a second pass): the same inputs give the
 * same bits, no float atomics.
 * Operands and constants as mrphy_blochsim_rfgr_fwd, ONE transmit coil (nC == 1; b1 (N, nM, 2) or NULL).  Mo (N, nM, 3)
 * may be NULL; where given it is mrphy_blochsim_rfgr_fwd's bit for bit.  Mck / ck_every as there (checkpoints for the
 * adjoint below; Mck may be NULL).  Any nT.  `work` must hold mrphy_signal_rfgr_fwd_workspace() bytes.
 * MRPHY_EINVAL: every < 1, sig NULL, nC != 1, N > 65535, an unknown dtype; MRPHY_ENOSPC: workspace too small; an empty
 * problem (N nM nT == 0) returns 0 and touches nothing.
 * ------------------------------------------------------------------------------------------- */
size_t mrphy_signal_rfgr_fwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t every);
int mrphy_signal_rfgr_fwd(int dtype,
                          const void* Mi,
                          const void* rf, int64_t rf_sn,
                          const void* gr, int64_t gr_sn,
                          const void* loc,
                          const void* df, int64_t df_sn, int64_t df_sm,
                          const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                          const void* b1,
                          const void* g,  int64_t g_sn,  int64_t g_sm,
                          const void* E1, int64_t E1_sn, int64_t E1_sm,
                          const void* E2, int64_t E2_sn, int64_t E2_sm,
                          const void* E1m1,
                          const void* rx,
                          void* Mo, void* Mck, int64_t ck_every,
                          void* sig, int64_t every,
                          void* work, size_t work_bytes,
                          int64_t N, int64_t nM, int64_t nT, int64_t nC,
                          void* stream);

/* K2bs  adjoint of K2s: as mrphy_blochsim_rfgr_bwd, with the cotangents of BOTH outputs -- grad_Mo (N, nM, 3) and
 * grad_sig (N, 2, nRec); either may be NULL (= zero), not both.  The sweep starts from grad_Mo and, as it passes step e_j
 * backwards, adds the cotangent of sample j, the same for every spin up to its receive weight:
 *     (rx_re g0 + rx_im g1,  rx_re g1 - rx_im g0,  0),   g0, g1 = grad_sig[n, :, j]
 * -- what the reference's autograd would do with a loss on the spin sum of Mhst (BlochSim.backward, sims.py:135-269).
 * Without grad_sig it is mrphy_blochsim_rfgr_bwd.  Same checkpoints (nT a multiple of mrphy_blochsim_rfgr_ck_every()),
 * same workspace (mrphy_blochsim_rfgr_bwd_workspace), same deterministic reduction; no gradient w.r.t. rx.
 * MRPHY_EINVAL: every < 1, nT not a whole number of segments, both cotangents NULL, N > 65535, an unknown dtype;
 * MRPHY_ENOSPC: workspace too small. */
int mrphy_signal_rfgr_bwd(int dtype,
                          const void* Mck,
                          const void* rf, int64_t rf_sn,
                          const void* gr, int64_t gr_sn,
                          const void* loc,
                          const void* df, int64_t df_sn, int64_t df_sm,
                          const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                          const void* b1,
                          const void* g,  int64_t g_sn,  int64_t g_sm,
                          const void* E1, int64_t E1_sn, int64_t E1_sm,
                          const void* E2, int64_t E2_sn, int64_t E2_sm,
                          const void* E1m1,
                          const void* rx,
                          const void* grad_Mo, const void* grad_sig, int64_t every,
                          void* grad_Mi, void* grad_rf, void* grad_gr,
                          void* work, size_t work_bytes,
                          int64_t N, int64_t nM, int64_t nT,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2s, receive arrays  K2s for the nRx coils of a receive array in ONE launch: one simulation, every coil's samples
 * (the same kernel at a coil capacity of nRx or more; mrphy_signal_rfgr_fwd runs it at capacity 1).
 *     sig[n, 0, j, c] = sum_s  rx_re[n,s,c] Mx[n,s] - rx_im[n,s,c] My[n,s]
 *     sig[n, 1, j, c] = sum_s  rx_re[n,s,c] My[n,s] + rx_im[n,s,c] Mx[n,s]    (M after step e_j)
 * rx (N, nM, 2, nRx) contiguous, the layout of a multi-coil b1, required; sig (N, 2, nRec, nRx), the layout of a
 * multi-coil rf.  1 <= nRx <= mrphy_signal_rfgr_max_rx(dtype) (8 for every code; 0 for an unknown code): a caller with
 * more coils launches once per block of that many.  Every (record, coil) sum is formed on its own, in the lane, tile
 * and row order of K2s: sig[..., c] is bit for bit what mrphy_signal_rfgr_fwd returns for rx[..., c] alone, and Mo is
 * the same bits as well.  Everything else -- operands, ONE transmit coil, Mo, Mck / ck_every, any nT -- as
 * mrphy_signal_rfgr_fwd.  `work` must hold mrphy_signal_rfgr_mrx_fwd_workspace() bytes: sig_waves(nM) N 2 nRx nRec
 * elements, nRx times mrphy_signal_rfgr_fwd_workspace().
 * MRPHY_EINVAL: nRx < 1 or above the capacity, rx or sig NULL, every < 1, nC != 1, N > 65535, an unknown dtype;
 * MRPHY_ENOSPC: workspace too small; an empty problem (N nM nT == 0) returns 0 and touches nothing.
 * ------------------------------------------------------------------------------------------- */
int mrphy_signal_rfgr_max_rx(int dtype);
size_t mrphy_signal_rfgr_mrx_fwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t every, int64_t nRx);
int mrphy_signal_rfgr_mrx_fwd(int dtype,
                              const void* Mi,
                              const void* rf, int64_t rf_sn,
                              const void* gr, int64_t gr_sn,
                              const void* loc,
                              const void* df, int64_t df_sn, int64_t df_sm,
                              const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                              const void* b1,
                              const void* g,  int64_t g_sn,  int64_t g_sm,
                              const void* E1, int64_t E1_sn, int64_t E1_sm,
                              const void* E2, int64_t E2_sn, int64_t E2_sm,
                              const void* E1m1,
                              const void* rx, int64_t nRx,
                              void* Mo, void* Mck, int64_t ck_every,
                              void* sig, int64_t every,
                              void* work, size_t work_bytes,
                              int64_t N, int64_t nM, int64_t nT, int64_t nC,
                              void* stream);

/* K2bs, receive arrays  adjoint of the above: mrphy_signal_rfgr_bwd with rx (N, nM, 2, nRx) and
 * grad_sig (N, 2, nRec, nRx), in ONE sweep.  As it passes step e_j backwards the sweep adds the coils' cotangents of
 * sample j, summed in ascending c and injected once:
 *     (sum_c rx_re,c g0,c + rx_im,c g1,c,  sum_c rx_re,c g1,c - rx_im,c g0,c,  0),   g0,c, g1,c = grad_sig[n, :, j, c]
 * The gradients equal the sum of the one-coil calls' up to the association of that sum.  Without grad_sig it is
 * mrphy_blochsim_rfgr_bwd.  Checkpoints, workspace (mrphy_blochsim_rfgr_bwd_workspace) and reduction as
 * mrphy_signal_rfgr_bwd; no gradient w.r.t. rx.
 * MRPHY_EINVAL: nRx < 1 or above the capacity, rx NULL, every < 1, nT not a whole number of segments, both cotangents
 * NULL, N > 65535, an unknown dtype; MRPHY_ENOSPC: workspace too small; an empty problem returns 0. */
int mrphy_signal_rfgr_mrx_bwd(int dtype,
                              const void* Mck,
                              const void* rf, int64_t rf_sn,
                              const void* gr, int64_t gr_sn,
                              const void* loc,
                              const void* df, int64_t df_sn, int64_t df_sm,
                              const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                              const void* b1,
                              const void* g,  int64_t g_sn,  int64_t g_sm,
                              const void* E1, int64_t E1_sn, int64_t E1_sm,
                              const void* E2, int64_t E2_sn, int64_t E2_sm,
                              const void* E1m1,
                              const void* rx, int64_t nRx,
                              const void* grad_Mo, const void* grad_sig, int64_t every,
                              void* grad_Mi, void* grad_rf, void* grad_gr,
                              void* work, size_t work_bytes,
                              int64_t N, int64_t nM, int64_t nT,
                              void* stream);
/* mrphy_signal_rfgr_mrx_bwd with grad_consts (N, nM, 4) besides, as mrphy_blochsim_rfgr_consts_bwd returns it (optional);
 * 1 <= nRx <= mrphy_signal_rfgr_max_rx(dtype) -- a build for each of the capacities 1, 2, 4, 8 -- and for nRx == 1 rx
 * may be NULL, the (1, 0) of mrphy_signal_rfgr_bwd.  grad_Mi, grad_rf, grad_gr come out bit for bit as
 * mrphy_signal_rfgr_bwd (nRx == 1) and mrphy_signal_rfgr_mrx_bwd give them.  No gradient w.r.t. rx or the spin-side
 * maps.  Everything else, refusals included, as mrphy_signal_rfgr_mrx_bwd. */
int mrphy_signal_rfgr_consts_bwd(int dtype,
                                 const void* Mck,
                                 const void* rf, int64_t rf_sn,
                                 const void* gr, int64_t gr_sn,
                                 const void* loc,
                                 const void* df, int64_t df_sn, int64_t df_sm,
                                 const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                 const void* b1,
                                 const void* g,  int64_t g_sn,  int64_t g_sm,
                                 const void* E1, int64_t E1_sn, int64_t E1_sm,
                                 const void* E2, int64_t E2_sn, int64_t E2_sm,
                                 const void* E1m1,
                                 const void* rx, int64_t nRx,
                                 const void* grad_Mo, const void* grad_sig, int64_t every,
                                 void* grad_Mi, void* grad_rf, void* grad_gr, void* grad_consts,
                                 void* work, size_t work_bytes,
                                 int64_t N, int64_t nM, int64_t nT,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * the steps either side of the path in SpinArray.applypulse (mobjs.py:427-433,449).
 *
 * The reference gathers/scatters with a boolean mask (`v[mask]`, `out[mask] = v_`), which has to
 * count the mask on the host at every call.  Here the mask is turned ONCE into two int32 lists
 *     idx (nM)  -- voxel number (row-major over *Nd) of compact spin j
 *     inv (nV)  -- compact spin number of voxel p, or -1 outside the mask
 * (mrphy_amd.masks.MaskIndex builds them with torch) and the kernels move raw 4- or 8-byte
 * elements; K = number of trailing elements per voxel (3 for M/loc, 1 for maps, 2*nC for b1Map).
 *
 * mask_extract -- SpinArray.extract (mobjs.py:532-553):  out_[n, j, :] = v[n, idx[j], :]
 *     v (N, nV, K) -> out_ (N, nM, K)
 * mask_embed   -- SpinArray.embed (mobjs.py:512-530):    out[n, p, :] = v_[n, inv[p], :] inside
 *     the mask; outside it `fillbits` when fill = 1 (a fresh output: the reference fills NaN),
 *     untouched when fill = 0 (the reference's `out=` form).        v_ (N, nM, K) -> out (N, nV, K)
 * cube_loc     -- SpinCube._update_loc_ (mobjs.py:815-839), 3-D grids:
 *     loc_[n, j, i] = fov[n, i] * ((c_i - dim_i / 2) / dim_i) + ofst[n, i],  c = unravel(idx[j])
 *     fov, ofst (N, 3) -> loc_ (N, nM, 3); same three roundings as the reference's expression.
 * Limits: nV < 2^31, N <= 65535.
 * ------------------------------------------------------------------------------------------- */
int mrphy_mask_extract(int elem_bytes, const void* v, const int32_t* idx, void* out_, int64_t N,
                       int64_t nV, int64_t nM, int64_t K, void* stream);
int mrphy_mask_embed(int elem_bytes, const void* v_, const int32_t* inv, void* out, int64_t N,
                     int64_t nV, int64_t nM, int64_t K, int fill, uint64_t fillbits, void* stream);
int mrphy_cube_loc(int dtype, const int32_t* idx, const void* fov, const void* ofst, void* loc_,
                   int64_t N, int64_t nM, int64_t nx, int64_t ny, int64_t nz, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Hargreaves' A/B propagation (doi:10.1002/mrm.1170).
 *
 * beff2ab -- mrphy.beffective.beff2ab (beffective.py:40-104): the step map
 *     M -> relax(rotate(M, Beff[t]))  is affine; its composition over the pulse is  M -> A M + B.
 *     The kernel carries the four columns of [I | 0] through the nT steps with the arithmetic of
 *     mrphy_blochsim_fwd (the -(E1-1) offset acts on the B column only), so column j of A is
 *     bit-identical to blochsim(e_j) with a zero offset and B to blochsim(0).
 *     Beff (N,nM,nT,3); constants as for mrphy_blochsim_fwd but E1, E2, E1m1 are mandatory (the
 *     reference takes E1, E2 -- not T1, T2 -- and always relaxes; E1 = E2 = 1, E1m1 = 0 is "no
 *     relaxation");  A (N,nM,3,3) row-major A[i][j] (i = xyz of the result), B (N,nM,3).
 * blochsim_ab -- mrphy.slowsims.blochsim_ab (slowsims.py:117-131):  Mo = A M + B  per spin;
 *     rows = N*nM, M/Mo/B (rows,3), A (rows,3,3) contiguous.
 * blochsim_ab_bwd -- its adjoint: gM = A^T gMo (needs A), gA[i][j] = gMo_i M_j (needs M); either
 *     output may be NULL; the gradient w.r.t. B is gMo itself.
 * ------------------------------------------------------------------------------------------- */
int mrphy_beff2ab(int dtype, const void* Beff,
                  const void* g, int64_t g_sn, int64_t g_sm,
                  const void* E1, int64_t E1_sn, int64_t E1_sm,
                  const void* E2, int64_t E2_sn, int64_t E2_sm,
                  const void* E1m1, void* A, void* B,
                  int64_t N, int64_t nM, int64_t nT, void* stream);

/* beff2ab with its adjoint in ONE backward sweep over Beff (the reference differentiates its time
 * loop with autograd, beffective.py:88-100).  mrphy_beff2ab_save = mrphy_beff2ab that also records
 * the 3x4 state before every step in `hist` (opaque layout, mrphy_beff2ab_hist_bytes bytes: 48 B per
 * spin-step in fp32); mrphy_beff2ab_bwd turns grad_A (N,nM,3,3) / grad_B (N,nM,3) (either may be
 * NULL = zero) into grad_Beff (N,nM,nT,3): the four columns share each step's rotation, so Beff is
 * read once and grad_Beff written once, where four blochsim adjoints would read it four times,
 * write four gradients and add them up. */
size_t mrphy_beff2ab_hist_bytes(int dtype, int64_t N, int64_t nM, int64_t nT);
int mrphy_beff2ab_save(int dtype, const void* Beff,
                       const void* g, int64_t g_sn, int64_t g_sm,
                       const void* E1, int64_t E1_sn, int64_t E1_sm,
                       const void* E2, int64_t E2_sn, int64_t E2_sm,
                       const void* E1m1, void* A, void* B, void* hist,
                       int64_t N, int64_t nM, int64_t nT, void* stream);
int mrphy_beff2ab_bwd(int dtype, const void* hist, const void* Beff,
                      const void* g, int64_t g_sn, int64_t g_sm,
                      const void* E1, int64_t E1_sn, int64_t E1_sm,
                      const void* E2, int64_t E2_sn, int64_t E2_sm,
                      const void* grad_A, const void* grad_B, void* grad_Beff,
                      int64_t N, int64_t nM, int64_t nT, void* stream);

/* mrphy_beff2ab_bwd that also returns the gradients w.r.t. the per-spin constants, as the reference's autograd
 * through its time loop does for a caller who differentiates beff2ab w.r.t. E1, E2, gamma, dt (beffective.py:73-100):
 *     grad_consts (N, nM, 4) = [dL/d(gamma 2 pi dt), dL/dE1, dL/dE2, dL/d(E1-1)]
 * (the host chains them through its own expressions for those four, as for mrphy_blochsim_bwd_consts). */
int mrphy_beff2ab_bwd_consts(int dtype, const void* hist, const void* Beff,
                             const void* g, int64_t g_sn, int64_t g_sm,
                             const void* E1, int64_t E1_sn, int64_t E1_sm,
                             const void* E2, int64_t E2_sn, int64_t E2_sm,
                             const void* grad_A, const void* grad_B, void* grad_Beff,
                             void* grad_consts, int64_t N, int64_t nM, int64_t nT, void* stream);
/* ---------------------------------------------------------------------------------------------
 * K2ab  fused rf,gr -> A, B: mrphy.beffective.beff2ab (beffective.py:40-104) of mrphy.beffective.rfgr2beff
 * (beffective.py:107-168) without Beff (N,nM,nT,3) in HBM.  Operands and constants as mrphy_blochsim_rfgr_fwd, ONE
 * transmit coil (rf (N|1, 2, nT, 1), b1 (N, nM, 2) or NULL); E1 == E2 == E1m1 == NULL is "no relaxation": A is then a
 * pure rotation and B an exact zero.  A (N,nM,3,3), B (N,nM,3) as mrphy_beff2ab lays them out, and with the same
 * constants they are mrphy_beff2ab(mrphy_rfgr2beff(.)) bit for bit: one field and one rotation per step, applied to
 * the three A columns with a zero offset and to the B column with E1m1.  nT == 0 writes A = I, B = 0.
 * ABck (nCk, 4, N*nM, 3), nCk = ceil(nT/ck_every), may be NULL; otherwise plane j of checkpoint c receives column j
 * (j == 3: B) before step c*ck_every (ck_every a positive multiple of 8): plane j < 3 is the Mck that
 * mrphy_blochsim_rfgr_fwd writes for Mi = e_j with a zero E1m1, bit for bit.
 *
 * K2abb  its adjoint w.r.t. the pulse: grad_A (N,nM,3,3), grad_B (N,nM,3) (either may be NULL = zero) -> grad_rf
 * (N,2,nT), grad_gr (N,3,nT) (either may be NULL), per batch entry as mrphy_blochsim_rfgr_bwd returns them.  ABck must
 * be the checkpoints of mrphy_ab_rfgr_fwd with ck_every = mrphy_blochsim_rfgr_ck_every(), nT a multiple of it; `work`
 * holds mrphy_blochsim_rfgr_bwd_workspace() bytes.  Per segment the four columns are recomputed and swept one after
 * another (they share the step's rotation; S and C are formed once), their dL/dBeff summed in a fixed order, then
 * reduced over the spins as K2b reduces: deterministic, no Beff, no history, no grad_Beff in memory.  Under codes
 * 3 / 4 E1 and E2 must be non-zero, as for the other adjoints.
 * Both refuse with MRPHY_EINVAL, before anything is launched: an unknown dtype, a NULL required pointer, N > 65535;
 * the adjoint also nT not a multiple of the segment and a workspace shorter than the query's.  An empty problem
 * (N*nM == 0; the adjoint: N*nM*nT == 0) is a success that writes nothing.
 * ------------------------------------------------------------------------------------------- */
int mrphy_ab_rfgr_fwd(int dtype,
                      const void* rf, int64_t rf_sn,
                      const void* gr, int64_t gr_sn,
                      const void* loc,
                      const void* df, int64_t df_sn, int64_t df_sm,
                      const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                      const void* b1,
                      const void* g,  int64_t g_sn,  int64_t g_sm,
                      const void* E1, int64_t E1_sn, int64_t E1_sm,
                      const void* E2, int64_t E2_sn, int64_t E2_sm,
                      const void* E1m1,
                      void* A, void* B, void* ABck, int64_t ck_every,
                      int64_t N, int64_t nM, int64_t nT,
                      void* stream);
int mrphy_ab_rfgr_bwd(int dtype,
                      const void* ABck,
                      const void* rf, int64_t rf_sn,
                      const void* gr, int64_t gr_sn,
                      const void* loc,
                      const void* df, int64_t df_sn, int64_t df_sm,
                      const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                      const void* b1,
                      const void* g,  int64_t g_sn,  int64_t g_sm,
                      const void* E1, int64_t E1_sn, int64_t E1_sm,
                      const void* E2, int64_t E2_sn, int64_t E2_sm,
                      const void* E1m1,
                      const void* grad_A, const void* grad_B,
                      void* grad_rf, void* grad_gr,
                      void* work, size_t work_bytes,
                      int64_t N, int64_t nM, int64_t nT,
                      void* stream);
/* K2abb's MAPS and CONSTS builds: mrphy_ab_rfgr_bwd -- the same arguments, the same sweep, the same bits for grad_rf and
 * grad_gr -- which also returns, per spin, the gradients w.r.t. the spin-side operands, as
 * mrphy_blochsim_rfgr_maps_bwd / _consts_bwd return them for K2b: grad_loc (N,nM,3), grad_Bz (N,nM) = dL/d(df / gamma)
 * (the division by gamma is the caller's), grad_b1 (N,nM,2), and from the CONSTS build grad_consts (N,nM,4) =
 * [dL/dg, dL/dE1, dL/dE2, dL/dE1m1] of the step constants (g = gamma 2 pi dt; dL/dE1m1 comes from the B column alone, the
 * only one the offset acts on; without relaxation the last three are exact zeros).  Each of the per-spin outputs may
 * be NULL (not wanted); they are sums over time in a fixed order: the same inputs give the same bits.  No workspace
 * beyond mrphy_blochsim_rfgr_bwd_workspace().
 * Both refuse with MRPHY_EINVAL, before anything is launched, what mrphy_ab_rfgr_bwd refuses, and a grad_b1 without a
 * b1 map.  An empty problem (N*nM*nT == 0) is a success that writes nothing. */
int mrphy_ab_rfgr_maps_bwd(int dtype,
                           const void* ABck,
                           const void* rf, int64_t rf_sn,
                           const void* gr, int64_t gr_sn,
                           const void* loc,
                           const void* df, int64_t df_sn, int64_t df_sm,
                           const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                           const void* b1,
                           const void* g,  int64_t g_sn,  int64_t g_sm,
                           const void* E1, int64_t E1_sn, int64_t E1_sm,
                           const void* E2, int64_t E2_sn, int64_t E2_sm,
                           const void* E1m1,
                           const void* grad_A, const void* grad_B,
                           void* grad_rf, void* grad_gr,
                           void* grad_loc, void* grad_Bz, void* grad_b1,
                           void* work, size_t work_bytes,
                           int64_t N, int64_t nM, int64_t nT,
                           void* stream);
int mrphy_ab_rfgr_consts_bwd(int dtype,
                             const void* ABck,
                             const void* rf, int64_t rf_sn,
                             const void* gr, int64_t gr_sn,
                             const void* loc,
                             const void* df, int64_t df_sn, int64_t df_sm,
                             const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                             const void* b1,
                             const void* g,  int64_t g_sn,  int64_t g_sm,
                             const void* E1, int64_t E1_sn, int64_t E1_sm,
                             const void* E2, int64_t E2_sn, int64_t E2_sm,
                             const void* E1m1,
                             const void* grad_A, const void* grad_B,
                             void* grad_rf, void* grad_gr,
                             void* grad_loc, void* grad_Bz, void* grad_b1, void* grad_consts,
                             void* work, size_t work_bytes,
                             int64_t N, int64_t nM, int64_t nT,
                             void* stream);
/* K2ab-mc / K2abb-mc: mrphy_ab_rfgr_fwd / mrphy_ab_rfgr_bwd under parallel transmit -- rf (N|1, 2, nT, nC), b1 (N, nM, 2,
 * nC) required, 1 <= nC <= mrphy_ab_rfgr_mc_max_coils(dtype) (8 for the fp32 codes, 4 for MRPHY_F64, whose
 * capacity-8 adjoint would not fit the register file; 0 for an unknown code).  The field is the coil sum mrphy_rfgr2beff and mrphy_blochsim_rfgr_fwd form (one ascending FMA chain), so A, B
 * are mrphy_beff2ab(mrphy_rfgr2beff(.)) bit for bit and B is mrphy_blochsim_rfgr_fwd(Mi = 0)'s.  ABck as above.  The adjoint
 * returns grad_rf (N, 2, nT, nC) and grad_gr (N, 3, nT) (either may be NULL) from grad_A, grad_B (either may be NULL,
 * not both): K2abb's sweep over the four columns, then the per-coil reduction over the spins of
 * mrphy_blochsim_rfgr_mc_bwd -- deterministic.  `work` holds mrphy_ab_rfgr_mc_bwd_workspace() bytes, which IS
 * mrphy_blochsim_rfgr_mc_bwd_workspace(): the same rows [gr_x, gr_y, gr_z, (re, im) x nC] per persistent wave.
 * Both refuse, before anything is launched, with MRPHY_EINVAL what the one-coil entry points refuse, a coil count
 * outside 1 .. max_coils and a NULL b1; the adjoint also nT not a whole number of segments and both cotangents NULL, and
 * with MRPHY_ENOSPC a workspace shorter than the query's.  An empty problem (N*nM == 0; the adjoint: N*nM*nT == 0) is a
 * success that writes nothing; the forward at nT == 0 writes A = I, B = 0.  The gradients w.r.t. the spin-side operands
 * and the step constants have no parallel-transmit build. */
int mrphy_ab_rfgr_mc_max_coils(int dtype);
size_t mrphy_ab_rfgr_mc_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t nC);
int mrphy_ab_rfgr_mc_fwd(int dtype,
                         const void* rf, int64_t rf_sn,
                         const void* gr, int64_t gr_sn,
                         const void* loc,
                         const void* df, int64_t df_sn, int64_t df_sm,
                         const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                         const void* b1,
                         const void* g,  int64_t g_sn,  int64_t g_sm,
                         const void* E1, int64_t E1_sn, int64_t E1_sm,
                         const void* E2, int64_t E2_sn, int64_t E2_sm,
                         const void* E1m1,
                         void* A, void* B, void* ABck, int64_t ck_every,
                         int64_t N, int64_t nM, int64_t nT, int64_t nC,
                         void* stream);
int mrphy_ab_rfgr_mc_bwd(int dtype,
                         const void* ABck,
                         const void* rf, int64_t rf_sn,
                         const void* gr, int64_t gr_sn,
                         const void* loc,
                         const void* df, int64_t df_sn, int64_t df_sm,
                         const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                         const void* b1,
                         const void* g,  int64_t g_sn,  int64_t g_sm,
                         const void* E1, int64_t E1_sn, int64_t E1_sm,
                         const void* E2, int64_t E2_sn, int64_t E2_sm,
                         const void* E1m1,
                         const void* grad_A, const void* grad_B,
                         void* grad_rf, void* grad_gr,
                         void* work, size_t work_bytes,
                         int64_t N, int64_t nM, int64_t nT, int64_t nC,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kss  the steady state of a sequence that repeats every period: a rest of duration `rest` -- free precession exactly
 * as mrphy_freeprec_fwd defines it, M- = F M + f with F = diag(E2r, E2r, E1r) Rz(-2 pi df rest), E1r = exp(-rest/T1),
 * E2r = exp(-rest/T2), f = (0, 0, -expm1(-rest/T1)) -- then the pulse M_after = A M_before + B (Hargreaves' A, B of
 * mrphy_ab_rfgr_fwd or mrphy_beff2ab, or any product of them).  The state right after the pulse solves
 *     (I - A F) Mss = A f + B,
 * one thread per spin.  A (N,nM,3,3), B (N,nM,3) as mrphy_beff2ab lays them out; Mss (N,nM,3); rest (N|1,) with
 * element stride rest_sn (0 broadcasts), as `dur` of mrphy_freeprec_fwd; T1, T2, df broadcastable per-spin constants of
 * the DATA type (MRPHY_F32 or MRPHY_F64, the codes mrphy_freeprec_* accept).  rest == NULL is "no rest period":
 * F = I, f = 0, Mss = (I - A)^-1 B, and T1, T2, df must then be NULL too; with a rest, T1 and T2 are both given or
 * neither (no relaxation in the rest), df == NULL is no precession.
 * Whatever the data type, all arithmetic in the kernel is fp64 (the rest constants, the products, the solve) and the
 * outputs are rounded once: Mss carries the rounding of A amplified by the condition number of I - A F, about
 * 1 / (1 - E1r), and the kernel adds nothing to it.  The solve is the cofactor form with one division by the
 * determinant.  A singular system -- no relaxation in the pulse nor in the rest: det == 0 -- yields non-finite
 * output; nothing is synchronised with the host to detect it.
 *
 * Kssb  its adjoint, for the cotangent grad_Mss (N,nM,3); Mss is recomputed from A, B and the constants:
 *     lambda = (I - A F)^-T grad_Mss,   M- = F Mss + f,   mu = A^T lambda
 *     grad_B (N,nM,3) = lambda,   grad_A (N,nM,3,3) = lambda M-^T,
 *     grad_consts (N,nM,4) = [dL/d rest, dL/d T1, dL/d T2, dL/d df]  (0 where the operand is NULL): the per-spin
 *     formulas of mrphy_freeprec_bwd_consts at Mi := Mss, grad_Mo := mu; the caller sums each column over the axes its
 *     operand broadcasts along.
 * Each of grad_A, grad_B, grad_consts may be NULL, not all three.
 * Both refuse before anything is launched: MRPHY_EINVAL for an unknown dtype, a negative size, a NULL required
 * pointer or a breach of the operand rules above; MRPHY_EALIGN for a pointer not aligned to its element size.  An
 * empty problem (N*nM == 0) is a success that writes nothing, whatever the pointers are.
 * ------------------------------------------------------------------------------------------- */
int mrphy_ab_steadystate_fwd(int dtype, const void* A, const void* B,
                             const void* rest, int64_t rest_sn,
                             const void* T1, int64_t T1_sn, int64_t T1_sm,
                             const void* T2, int64_t T2_sn, int64_t T2_sm,
                             const void* df, int64_t df_sn, int64_t df_sm,
                             void* Mss, int64_t N, int64_t nM, void* stream);
int mrphy_ab_steadystate_bwd(int dtype, const void* A, const void* B, const void* grad_Mss,
                             const void* rest, int64_t rest_sn,
                             const void* T1, int64_t T1_sn, int64_t T1_sm,
                             const void* T2, int64_t T2_sn, int64_t T2_sm,
                             const void* df, int64_t df_sn, int64_t df_sm,
                             void* grad_A, void* grad_B, void* grad_consts,
                             int64_t N, int64_t nM, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ktr  the transient of the same sequence over its first K repetitions, the RF phase phi_k (rad) changing from one
 * to the next.  Per spin, from M_0 = Mi, for k = 0 .. K-1:
 *     M-      = F M_k + f                           the rest, F and f exactly as Kss forms them (above)
 *     M_{k+1} = Rz(phi_k) [ A Rz(-phi_k) M- + B ]   the pulse played with its rf multiplied by e^{i phi_k}
 * with Rz(phi) = [[c,-s,0],[s,c,0],[0,0,1]].  Record k is M_{k+1}, the state right after pulse k (as Mss of Kss), and
 * the records are stored TIME-MAJOR: Mt (K,N,nM,3).  A, B, rest, T1, T2, df and their rules as in Kss.  Mi (N|1,nM|1,3)
 * of the data type with ELEMENT strides Mi_sn, Mi_sm (0 broadcasts; xyz contiguous), NULL = (0,0,1).  cs (N|1,K,2):
 * cos phi_k, sin phi_k, ALWAYS fp64, contiguous over (K,2) with element stride cs_sn between batch entries
 * (0 broadcasts); NULL = all phases zero.  One thread per spin, blockIdx.y = the batch entry: N <= 65535.  Whatever the
 * data type, all arithmetic is fp64, the state carried from one repetition to the next stays fp64, and each record is
 * rounded once on its store.
 *
 * Ktrb  its adjoint, for the cotangents grad_Mt (K,N,nM,3) of the records.  It walks k downwards and reads M_{k+1} and
 * M_k from Mt, the forward's own output (M_0 = Mi): nothing else is saved, nothing is recomputed forward.  From h = 0:
 *     lambda = h + grad_Mt[k],   u = Rz(-phi_k) lambda,   p = Rz(-phi_k) M-,   M- = F M_k + f
 *     grad_B (N,nM,3) += u,   grad_A (N,nM,3,3) += u p^T,   gM- = Rz(phi_k) A^T u
 *     grad_phase (K,N,nM)[k] = (lambda_y M_x - lambda_x M_y) at M_{k+1} - (gM-_y M-_x - gM-_x M-_y)   PER SPIN: the
 *         caller sums over the spins that share a phase
 *     grad_consts (N,nM,4) = [dL/d rest, dL/d T1, dL/d T2, dL/d df] += the per-spin formulas of
 *         mrphy_freeprec_bwd_consts at Mi := M_k, grad_Mo := gM-  (0 where the operand is NULL)
 *     h = F^T gM-                                      and at the end grad_Mi (N,nM,3) = h.
 * Every sum is private to its thread and runs in a fixed order: no workspace, no atomics, the same bits every run.
 * Each of grad_A, grad_B, grad_consts, grad_Mi, grad_phase may be NULL, not all five.
 * Both refuse before anything is launched: MRPHY_EINVAL for an unknown dtype, a negative size, N > 65535, a NULL
 * required pointer (A, B, Mt, grad_Mt) or a breach of the operand rules of Kss; MRPHY_EALIGN for a pointer not aligned to
 * its element size (cs: 8).  An empty problem (N*nM*K == 0) is a success that writes nothing, whatever the pointers are.
 * ------------------------------------------------------------------------------------------- */
int mrphy_ab_train_fwd(int dtype, const void* A, const void* B,
                       const void* rest, int64_t rest_sn,
                       const void* T1, int64_t T1_sn, int64_t T1_sm,
                       const void* T2, int64_t T2_sn, int64_t T2_sm,
                       const void* df, int64_t df_sn, int64_t df_sm,
                       const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                       const void* cs, int64_t cs_sn,
                       void* Mt, int64_t N, int64_t nM, int64_t K, void* stream);
int mrphy_ab_train_bwd(int dtype, const void* A, const void* B, const void* grad_Mt,
                       const void* rest, int64_t rest_sn,
                       const void* T1, int64_t T1_sn, int64_t T1_sm,
                       const void* T2, int64_t T2_sn, int64_t T2_sm,
                       const void* df, int64_t df_sn, int64_t df_sm,
                       const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                       const void* cs, int64_t cs_sn, const void* Mt,
                       void* grad_A, void* grad_B, void* grad_consts, void* grad_Mi, void* grad_phase,
                       int64_t N, int64_t nM, int64_t K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ktrs  the signal of Ktr's train: the same recursion, operands and rules (A, B, rest, T1, T2, df, Mi, cs as
 * mrphy_ab_train_fwd takes them), the same fp64 arithmetic and therefore the same bits of the state, but instead of the
 * records what nRx receive coils see of them, summed over the spins of each batch entry:
 *     sig[n,0,k,c] = sum_s rx_re Mx - rx_im My,   sig[n,1,k,c] = sum_s rx_re My + rx_im Mx      at record k = M_{k+1}
 * with rx (N,nM,2,nRx) of the data type, contiguous (the product of mrphy_signal_rfgr_fwd, no conjugate); rx NULL means
 * weight (1,0) and needs nRx == 1.  1 <= nRx <= mrphy_train_signal_max_rx(dtype) (8 for both data types; 0 for another
 * code): builds at the capacities 1, 2, 4, 8, pad coils of weight zero; a caller with more coils runs blocks of that
 * many.  sig (N,2,K,nRx) of the data type.  Mlast (N,nM,3) of the data type, or NULL: the last record, the bits of
 * Mt[K-1] of mrphy_ab_train_fwd.  ck: NULL, or fp64 (ceil(K/S),N*nM,3) with S = mrphy_train_signal_ck_every(): the state
 * BEFORE repetitions 0, S, 2S, ... for the adjoint; with NULL nothing per spin is written besides Mlast.
 * One wave per 64 spins of one batch entry, persistent over the tiles w, w+P, ... with P = min(ceil(nM/64), 2048): per
 * repetition each lane's 2 nRx products (fp64) go into an LDS tile, a full tile is summed over the lanes in a fixed order
 * and added into the wave's OWN row of work (P,N,2 nRx,K) fp64; a second pass sums the P rows in fixed order and rounds
 * once into sig.  No atomics: the same inputs give the same bits, and coil c's samples are the bits of the one-coil
 * call.  work_bytes >= mrphy_train_signal_workspace(dtype,N,nM,K,rows) = P*N*rows*K*8 with rows = 2 nRx (the adjoint:
 * rows = 1, and only when grad_phase is wanted).
 *
 * Ktrsb  its adjoint, for the cotangents grad_sig -- REPACKED by the caller as an fp64 table (N,K,nRx,2), NULL = none --
 * and grad_Mlast (N,nM,3) of the data type, NULL = none; not both NULL.  Ktrb's sweep (mrphy_ab_train_bwd) from
 * h = grad_Mlast, with the cotangent of record k formed per spin as
 *     (sum_c rx_re g0 + rx_im g1,  sum_c rx_re g1 - rx_im g0,  0),   g = grad_sig[n,k,c,:],  in ascending c,
 * and M_k, M_{k+1} recomputed per segment of S repetitions from ck (required) instead of read from records.  grad_A,
 * grad_B, grad_Mi per spin as Ktrb writes them; grad_consts (N,nM,4) per spin with Ktrb's formulas but ALWAYS fp64 (the
 * caller sums it over the spins that share an operand -- every spin for rest -- and rounds once); grad_rx (N,nM,2,nRx):
 *     d/d rx_re = sum_k g0 Mx + g1 My,   d/d rx_im = sum_k g1 Mx - g0 My      at M_{k+1};
 * grad_phase (N,K) is SUMMED OVER THE SPINS of each batch entry inside the kernel (the forward's reduction with one row
 * per repetition, work (P,N,K) fp64, the same second pass).  Each output may be NULL, not all six.
 * Both refuse before anything is launched: what mrphy_ab_train_fwd refuses, with the same codes; MRPHY_EINVAL for a
 * coil count outside 1 .. the limit, a NULL rx with nRx != 1, a NULL sig, ck (adjoint) or a NULL work that is needed;
 * MRPHY_EALIGN for a pointer not aligned to its element size (ck, work, grad_sig, grad_consts, cs: 8); MRPHY_ENOSPC for a workspace
 * shorter than the query's.  An empty problem (N*nM*K == 0) is a success that writes nothing.
 * ------------------------------------------------------------------------------------------- */
int64_t mrphy_train_signal_ck_every(void);
int mrphy_train_signal_max_rx(int dtype);
size_t mrphy_train_signal_workspace(int dtype, int64_t N, int64_t nM, int64_t K, int64_t rows);
int mrphy_train_signal_fwd(int dtype, const void* A, const void* B,
                           const void* rest, int64_t rest_sn,
                           const void* T1, int64_t T1_sn, int64_t T1_sm,
                           const void* T2, int64_t T2_sn, int64_t T2_sm,
                           const void* df, int64_t df_sn, int64_t df_sm,
                           const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                           const void* cs, int64_t cs_sn,
                           const void* rx, int64_t nRx,
                           void* sig, void* Mlast, void* ck, void* work, size_t work_bytes,
                           int64_t N, int64_t nM, int64_t K, void* stream);
int mrphy_train_signal_bwd(int dtype, const void* A, const void* B, const void* grad_sig, const void* grad_Mlast,
                           const void* rest, int64_t rest_sn,
                           const void* T1, int64_t T1_sn, int64_t T1_sm,
                           const void* T2, int64_t T2_sn, int64_t T2_sm,
                           const void* df, int64_t df_sn, int64_t df_sm,
                           const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                           const void* cs, int64_t cs_sn,
                           const void* rx, int64_t nRx, const void* ck,
                           void* grad_A, void* grad_B, void* grad_consts, void* grad_Mi, void* grad_phase,
                           void* grad_rx, void* work, size_t work_bytes,
                           int64_t N, int64_t nM, int64_t K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ksq  Ktr's transient with a schedule: repetition k plays entry pulse_k of a bank of P >= 1 pulses after a rest of
 * its own duration rest_k.  Per spin, from M_0 = Mi, for k = 0 .. K-1:
 *     M-      = F_k M_k + f_k                                   F, f of Kss at the duration rest_k (0 is legal: no rest)
 *     M_{k+1} = Rz(phi_k) [ A_p Rz(-phi_k) M- + B_p ],  p = pulse_k
 * A (P,N,nM,3,3), B (P,N,nM,3) of the data type, contiguous, the bank axis leading.  pulse (K,): int32 on the device,
 * one schedule for all batch entries, NULL = all zeros (P == 1 only); 0 <= pulse_k < P is a PRECONDITION (the library
 * cannot read device memory on the host).  rs (N|1,K): the rest durations, ALWAYS fp64 -- the caller's operand rounded
 * to the data type and widened, the number Ktr sees --, contiguous over K with element stride rs_sn between batch
 * entries (0 broadcasts); NULL = no rest period (T1, T2, df must then be NULL).  T1 .. cs_sn, Mt (K,N,nM,3), the grid
 * and the arithmetic as mrphy_ab_train_fwd: the repetition is Ktr's, bit for bit; A_p, B_p are reloaded when pulse_k
 * changes and the rest's constants re-formed when the bits of rest_k change, both uniform over the block.
 *
 * Ksqb  its adjoint: Ktrb's sweep with the same two refreshes.  grad_A (P,N,nM,3,3), grad_B (P,N,nM,3): the whole bank,
 * exact zeros for an entry the schedule never plays; accumulated per run of equal pulse_k in registers and added into
 * the lane's own slots of work (P,12,N*nM) fp64 when pulse_k changes (no atomics, fixed order), rounded once by a second
 * pass.  work is needed when grad_A or grad_B is: work_bytes >= mrphy_ab_sequence_bwd_workspace(dtype,P,N,nM) =
 * P*12*N*nM*8; it is passed in uninitialised and cleared on the caller's stream.  grad_consts (N,nM,3) = [dL/d T1,
 * dL/d T2, dL/d df] summed over k with rest_k inside the sum; grad_rest (K,N,nM): Ktrb's dL/d rest per repetition and
 * PER SPIN (the caller sums over the spins, and over k for one duration); grad_Mi, grad_phase as Ktrb.  Each of the six
 * may be NULL, not all.
 * Both refuse before anything is launched, in the order of mrphy_ab_train_*: MRPHY_EINVAL for what those refuse (rs in
 * the place of rest), P < 1 or P > 65535, pulse == NULL with P > 1, a NULL work that is needed; MRPHY_EALIGN for a
 * misaligned pointer (rs, cs, work: 8; pulse: 4); MRPHY_ENOSPC for a workspace shorter than the query's.  An empty
 * problem (N*nM*K == 0) is a success that writes nothing.
 * ------------------------------------------------------------------------------------------- */
size_t mrphy_ab_sequence_bwd_workspace(int dtype, int64_t P, int64_t N, int64_t nM);
int mrphy_ab_sequence_fwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                          const void* rs, int64_t rs_sn,
                          const void* T1, int64_t T1_sn, int64_t T1_sm,
                          const void* T2, int64_t T2_sn, int64_t T2_sm,
                          const void* df, int64_t df_sn, int64_t df_sm,
                          const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                          const void* cs, int64_t cs_sn,
                          void* Mt, int64_t N, int64_t nM, int64_t K, void* stream);
int mrphy_ab_sequence_bwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse, const void* grad_Mt,
                          const void* rs, int64_t rs_sn,
                          const void* T1, int64_t T1_sn, int64_t T1_sm,
                          const void* T2, int64_t T2_sn, int64_t T2_sm,
                          const void* df, int64_t df_sn, int64_t df_sm,
                          const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                          const void* cs, int64_t cs_sn, const void* Mt,
                          void* grad_A, void* grad_B, void* grad_consts, void* grad_rest, void* grad_Mi,
                          void* grad_phase, void* work, size_t work_bytes,
                          int64_t N, int64_t nM, int64_t K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ksqj  Ksq with forward-mode tangents: Mt of mrphy_ab_sequence_fwd, bit for bit, and dMt (D,K,N,nM,3), time-major like
 * Mt, the derivative of every record along D directions.  A .. cs_sn exactly as mrphy_ab_sequence_fwd.  A direction is
 * a set of tangents of the operands, one dense contiguous table per operand with a leading direction axis:
 *     per spin, of the data type:   dA (D,P,N,nM,3,3)   dB (D,P,N,nM,3)   dMi (D,N,nM,3)   dT1, dT2, ddf (D,N,nM)
 *     block-uniform, ALWAYS fp64:   dphase (D,N|1,K) in rad   drest (D,N|1,K) in s
 * dphase and drest are contiguous over K with the element stride *_sn between batch entries (0 broadcasts: the table is
 * (D,1,K)).  Any of the eight may be NULL: a zero tangent.  A tangent of df may come without df (df counts as 0).
 * The primal repetition is Ksq's own; per repetition the tangents of cos, sin, E1, E2 of the rest are products of those
 * numbers (no transcendental function is called for a tangent), everything in fp64, each record rounded once on its
 * store.  The arithmetic of a direction does not depend on D or on the other directions: dMt[d] has the bits of the call
 * with that direction alone; a direction scaled by a power of two or negated scales or negates dMt[d] exactly; zero
 * tangents give zeros; dA, dB of an entry the schedule never plays are never read.  Mt may be NULL (not wanted).
 * mrphy_ab_sequence_jvp_max_dirs(dtype): the most directions one launch takes (the kernels are built at the capacities
 * 1, 2, 4; the smallest that holds D runs): 4; < 0 for a dtype code other than MRPHY_F32, MRPHY_F64.
 * Checks: those of mrphy_ab_sequence_fwd in its order, the empty problem (N*nM*K == 0) a success that looks at no pointer
 * and writes nothing; then MRPHY_EINVAL for D < 1 or D above the capacity, for dT1 or dT2 without T1, for ddf, drest,
 * dT1 or dT2 without rs, for a NULL dMt; MRPHY_EALIGN for a misaligned pointer (dphase, drest: 8).  Nothing is launched
 * after a refusal.  No atomics, no workspace; the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------- */
int mrphy_ab_sequence_jvp_max_dirs(int dtype);
int mrphy_ab_sequence_jvp_fwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                              const void* rs, int64_t rs_sn,
                              const void* T1, int64_t T1_sn, int64_t T1_sm,
                              const void* T2, int64_t T2_sn, int64_t T2_sm,
                              const void* df, int64_t df_sn, int64_t df_sm,
                              const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                              const void* cs, int64_t cs_sn,
                              int64_t D,
                              const void* dA, const void* dB, const void* dMi,
                              const void* dT1, const void* dT2, const void* ddf,
                              const void* dphase, int64_t dphase_sn,
                              const void* drest, int64_t drest_sn,
                              void* Mt, void* dMt, int64_t N, int64_t nM, int64_t K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ksqs the received signal of Ksq's sequence: the transverse magnetisation of its records summed over the spins per
 * repetition, for nRx receive coils, inside the kernel -- Ktrs's frame around Ksq's repetition.  A .. cs_sn exactly as
 * mrphy_ab_sequence_fwd (the bank, the int32 schedule, the fp64 rs), rx .. work_bytes exactly as
 * mrphy_train_signal_fwd: rx (N,nM,2,nRx) or NULL with nRx == 1, 1 <= nRx <= mrphy_train_signal_max_rx(dtype),
 * sig (N,2,K,nRx), Mlast (N,nM,3) or NULL, ck (ceil(K/S),N*nM,3) fp64 with S = mrphy_train_signal_ck_every() or NULL
 * (no adjoint wanted), work_bytes >= mrphy_sequence_signal_workspace(dtype,N,nM,K,2*nRx) = Pw*N*2*nRx*K*8 with
 * Pw = min(ceil(nM/64), 2048) persistent waves.  The state has Ksq's bits, a coil's samples those of a call with that
 * coil alone; without a schedule (P == 1, one duration) sig and Mlast are mrphy_train_signal_fwd's, bit for bit.
 *
 * Ksqsb  its adjoint: Ktrsb's sweep per segment of S repetitions, the segment's states recomputed from ck into LDS,
 * with Ksqb's refreshes.  grad_sig (N,K,nRx,2) fp64 and grad_Mlast (N,nM,3): either may be NULL, not both.
 * grad_A (P,N,nM,3,3), grad_B (P,N,nM,3): the whole bank through bank (P,12,N*nM) fp64, needed when either is wanted:
 * bank_bytes >= mrphy_sequence_signal_bank_workspace(dtype,P,N,nM) = P*12*N*nM*8, passed in uninitialised and cleared
 * on the caller's stream.  grad_consts (N,nM,3) FP64 = [dL/d T1, dL/d T2, dL/d df] per spin with rest_k inside the sum;
 * grad_phase (N,K) and grad_rest (N,K), both FP64: dL/d phi_k and dL/d rest_k summed over the spins inside the kernel
 * (the caller folds them over what shares the operand and rounds once); they need work_bytes >=
 * mrphy_sequence_signal_workspace(dtype,N,nM,K,nQ), nQ = how many of the two are wanted.  grad_Mi (N,nM,3),
 * grad_rx (N,nM,2,nRx) of the data type.  Each of the seven may be NULL, not all.
 * Both refuse before anything is launched: MRPHY_EINVAL for what mrphy_ab_sequence_* and mrphy_train_signal_* refuse
 * (the coil count, rx == NULL with nRx != 1, a NULL output, ck, work or bank that is needed); MRPHY_EALIGN for a
 * misaligned pointer (rs, cs, ck, work, bank, grad_sig, grad_consts, grad_phase, grad_rest: 8; pulse: 4);
 * MRPHY_ENOSPC for a workspace shorter than its query's.  0 <= pulse_k < P is a PRECONDITION as for Ksq.  An empty
 * problem (N*nM*K == 0) is a success that writes nothing, whatever the pointers.
 * ------------------------------------------------------------------------------------------- */
size_t mrphy_sequence_signal_workspace(int dtype, int64_t N, int64_t nM, int64_t K, int64_t rows);
size_t mrphy_sequence_signal_bank_workspace(int dtype, int64_t P, int64_t N, int64_t nM);
int mrphy_sequence_signal_fwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                              const void* rs, int64_t rs_sn,
                              const void* T1, int64_t T1_sn, int64_t T1_sm,
                              const void* T2, int64_t T2_sn, int64_t T2_sm,
                              const void* df, int64_t df_sn, int64_t df_sm,
                              const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                              const void* cs, int64_t cs_sn,
                              const void* rx, int64_t nRx, void* sig, void* Mlast, void* ck,
                              void* work, size_t work_bytes,
                              int64_t N, int64_t nM, int64_t K, void* stream);
int mrphy_sequence_signal_bwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                              const void* grad_sig, const void* grad_Mlast,
                              const void* rs, int64_t rs_sn,
                              const void* T1, int64_t T1_sn, int64_t T1_sm,
                              const void* T2, int64_t T2_sn, int64_t T2_sm,
                              const void* df, int64_t df_sn, int64_t df_sm,
                              const void* Mi, int64_t Mi_sn, int64_t Mi_sm,
                              const void* cs, int64_t cs_sn,
                              const void* rx, int64_t nRx, const void* ck,
                              void* grad_A, void* grad_B, void* grad_consts, void* grad_rest, void* grad_Mi,
                              void* grad_phase, void* grad_rx, void* work, size_t work_bytes,
                              void* bank, size_t bank_bytes,
                              int64_t N, int64_t nM, int64_t K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ksqp  the steady state of Ksq's K repetitions played as one period, over and over: per spin the K affine maps compose
 * to Phi(M) = Abar M + bbar, and Mss = (I - Abar)^-1 bbar is the state right after the LAST repetition of the period
 * (= the state before the rest of repetition 0; Kss's convention, record K-1 of Ksq started at Mss).  A .. df_sm and
 * cs, cs_sn exactly as mrphy_ab_sequence_fwd (the bank, the int32 schedule, the fp64 rs and cs); there is no Mi.  One
 * thread per spin carries four fp64 columns through Ksq's repetition (the affine column from 0 and the columns of I
 * through the linear part, nothing obtained as a difference), then solves in Kss's cofactor form, fp64, one division;
 * Mss (N,nM,3) is rounded once into the data type.  A singular period gives non-finite values, as Kss.  Two optional
 * outputs for the adjoint, both NULL when none is wanted: per (12,N*nM) fp64 = Abar row-major then bbar, slot-major;
 * ck (ceil(K/S),N*nM,3) fp64 with S = mrphy_train_signal_ck_every() = the state before repetitions 0, S, 2S, ... of the
 * period started at the unrounded Mss (a second walk of one column in the same launch).
 *
 * Ksqpl + Ksqsb  its adjoint for the cotangent grad_Mss (N,nM,3): a small kernel forms lambda = (I - Abar)^-T grad_Mss
 * from per into lam (N,nM,3) of the data type, scratch passed by the caller; then Ksqsb's sweep (the launcher of
 * mrphy_sequence_signal_bwd) runs from ck with no signal cotangent and lambda as the cotangent of the last state.  The
 * outputs are handed over exactly as mrphy_sequence_signal_bwd hands them over: grad_A (P,N,nM,3,3), grad_B (P,N,nM,3)
 * through bank (exact zeros for an entry never played), grad_consts (N,nM,3) FP64, grad_rest (N,K) and grad_phase (N,K)
 * FP64 summed over the spins inside the kernel; each may be NULL, not all.  work and bank are sized by
 * mrphy_sequence_signal_workspace(dtype,N,nM,K,nQ) and mrphy_sequence_signal_bank_workspace(dtype,P,N,nM).  No atomics;
 * the same inputs give the same bits.
 * Both refuse before anything is launched what mrphy_ab_sequence_* and mrphy_sequence_signal_* refuse, with the same
 * codes in the same order (MRPHY_EALIGN: rs, cs, per, ck, work, bank, grad_consts, grad_rest, grad_phase: 8; pulse: 4);
 * K < 1 with spins present is MRPHY_EINVAL: a period needs a repetition.  N*nM == 0 is a success that writes nothing.
 * ------------------------------------------------------------------------------------------- */
int mrphy_sequence_steadystate_fwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                                   const void* rs, int64_t rs_sn,
                                   const void* T1, int64_t T1_sn, int64_t T1_sm,
                                   const void* T2, int64_t T2_sn, int64_t T2_sm,
                                   const void* df, int64_t df_sn, int64_t df_sm,
                                   const void* cs, int64_t cs_sn,
                                   void* Mss, void* per, void* ck,
                                   int64_t N, int64_t nM, int64_t K, void* stream);
int mrphy_sequence_steadystate_bwd(int dtype, const void* A, const void* B, int64_t P, const void* pulse,
                                   const void* grad_Mss,
                                   const void* rs, int64_t rs_sn,
                                   const void* T1, int64_t T1_sn, int64_t T1_sm,
                                   const void* T2, int64_t T2_sn, int64_t T2_sm,
                                   const void* df, int64_t df_sn, int64_t df_sm,
                                   const void* cs, int64_t cs_sn,
                                   const void* per, const void* ck, void* lam,
                                   void* grad_A, void* grad_B, void* grad_consts, void* grad_rest, void* grad_phase,
                                   void* work, size_t work_bytes, void* bank, size_t bank_bytes,
                                   int64_t N, int64_t nM, int64_t K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2v / K2vb  K2 / K2b for spins that move at constant velocity (ONE transmit coil: nC == 1, b1 (N, nM, 2) or NULL).
 * A spin that is at loc when step 0 begins sees, during step t of this call, the gradient at its midpoint position
 *     pos_t = loc + vdt * (step0 + t + 1/2),      Bz_t = gr_t . pos_t + df / gamma,
 * vdt (N, nM, 3) = velocity * dt in cm per step, of the data type (formed and rounded once by the caller), step0 >= 0
 * the number of steps played before this call (a pulse chained over several calls gives the single call's bits).
 * Bxy is K2's: a b1 map is sampled at loc.  pos_t is one FMA per component in closed form, never a running sum, so the
 * forward, the adjoint's recompute and a chained call see the same bits; step0 + nT must stay below 2^23 in the
 * float types for step0 + t + 1/2 to be exact (the caller's check).  With vdt == 0 both are mrphy_blochsim_rfgr_fwd /
 * _bwd bit for bit.  Every other argument, the checkpoints, the workspace (mrphy_blochsim_rfgr_bwd_workspace), the
 * order of the checks and the return codes are those calls'; in addition a NULL vdt (with spins present), step0 < 0 and
 * nC != 1 are MRPHY_EINVAL before anything is launched.  grad_gr's rows are the sums over spins of pos_t * dL/dBz_t.
 * No atomics; the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------- */
int mrphy_blochsim_rfgr_moving_fwd(int dtype,
                                   const void* Mi,
                                   const void* rf, int64_t rf_sn,
                                   const void* gr, int64_t gr_sn,
                                   const void* loc,
                                   const void* df, int64_t df_sn, int64_t df_sm,
                                   const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                   const void* b1,
                                   const void* g,  int64_t g_sn,  int64_t g_sm,
                                   const void* E1, int64_t E1_sn, int64_t E1_sm,
                                   const void* E2, int64_t E2_sn, int64_t E2_sm,
                                   const void* E1m1,
                                   const void* vdt, int64_t step0,
                                   void* Mo, void* Mck, int64_t ck_every,
                                   int64_t N, int64_t nM, int64_t nT, int64_t nC,
                                   void* stream);
int mrphy_blochsim_rfgr_moving_bwd(int dtype,
                                   const void* Mck,
                                   const void* rf, int64_t rf_sn,
                                   const void* gr, int64_t gr_sn,
                                   const void* loc,
                                   const void* df, int64_t df_sn, int64_t df_sm,
                                   const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                   const void* b1,
                                   const void* g,  int64_t g_sn,  int64_t g_sm,
                                   const void* E1, int64_t E1_sn, int64_t E1_sm,
                                   const void* E2, int64_t E2_sn, int64_t E2_sm,
                                   const void* E1m1,
                                   const void* vdt, int64_t step0,
                                   const void* grad_Mo,
                                   void* grad_Mi, void* grad_rf, void* grad_gr,
                                   void* work, size_t work_bytes,
                                   int64_t N, int64_t nM, int64_t nT,
                                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2sh / K2shb  K2 / K2b with extra Bz field channels (ONE transmit coil: nC == 1, b1 (N, nM, 2) or NULL): fields whose
 * shape in space is not linear and whose amplitude changes during the pulse (shim arrays, higher-order and concomitant
 * terms, gradient nonlinearity, eddy currents, motion along given directions).  nS >= 1 channels, each a waveform times
 * a map,
 *     Bz_t = gr_t . loc + df / gamma + sum_k sh[k, t] shMap[k],
 * sh (N, nS, nT) of the data type with batch stride sh_sn (0: one waveform set shared by the batch, as rf_sn), in any
 * unit; shMap (N nM, nS) contiguous, of the data type, Gauss per that unit at each spin.  The sum is formed as K2's Bz
 * followed by one FMA per channel in ascending k -- by the forward, the adjoint's recompute and its sweep alike -- so
 * channels whose waveform or map is zero leave mrphy_blochsim_rfgr_fwd / _bwd's bits, and all-zero channels appended
 * after the real ones change no bit of any output, whichever capacity serves the call.  Both hold for finite waveforms
 * and maps, and up to the sign of a zero: 0 * inf is NaN, fma(s, 0, -0.0) is +0.0, and the channels between nS and the
 * capacity re-read the last real channel's waveform against a zero map.  Bxy is K2's.
 * mrphy_blochsim_rfgr_shim_max_channels(dtype): the most channels one launch takes (the kernels are built at the
 * capacities 2, 4, 8; the smallest that holds nS runs); 0 for an unknown dtype code, as the workspace query then is.
 * The adjoint returns grad_Mi (N, nM, 3), grad_rf (N, 2, nT, 1) and grad_lead (N, 3 + nS, nT): rows 0 .. 2 are grad_gr,
 * row 3 + k is grad_sh[k, t] = sum over the spins of shMap[k] dL/dBz_t; each may be NULL (not wanted).  Its workspace
 * is mrphy_blochsim_rfgr_shim_bwd_workspace(dtype, N, nM, nT, nS) bytes: (P, N, 5 + nS, nT) elements for the P persistent
 * waves of mrphy_blochsim_rfgr_bwd.  Every other argument and the checkpoints are mrphy_blochsim_rfgr_fwd / _bwd's.
 * Checks, in this order: dtype and sizes; the mode arguments -- nS < 1, nS above the capacity, nS nT >= 2^31, nC != 1, a
 * ck_every that is no multiple of 8 with Mck given, nT % 16 != 0 in the adjoint -- MRPHY_EINVAL on an empty problem too; the
 * empty problem (N nM == 0; the adjoint: N nM nT == 0) returns 0 and writes nothing; NULL sh or shMap or another
 * required pointer is MRPHY_EINVAL; a short workspace MRPHY_ENOSPC.  Nothing is launched after a refusal.
 * No atomics; the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------- */
int mrphy_blochsim_rfgr_shim_max_channels(int dtype);
size_t mrphy_blochsim_rfgr_shim_bwd_workspace(int dtype, int64_t N, int64_t nM, int64_t nT, int64_t nS);
int mrphy_blochsim_rfgr_shim_fwd(int dtype,
                                 const void* Mi,
                                 const void* rf, int64_t rf_sn,
                                 const void* gr, int64_t gr_sn,
                                 const void* loc,
                                 const void* df, int64_t df_sn, int64_t df_sm,
                                 const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                 const void* b1,
                                 const void* g,  int64_t g_sn,  int64_t g_sm,
                                 const void* E1, int64_t E1_sn, int64_t E1_sm,
                                 const void* E2, int64_t E2_sn, int64_t E2_sm,
                                 const void* E1m1,
                                 const void* sh, int64_t sh_sn, const void* shMap, int64_t nS,
                                 void* Mo, void* Mck, int64_t ck_every,
                                 int64_t N, int64_t nM, int64_t nT, int64_t nC,
                                 void* stream);
int mrphy_blochsim_rfgr_shim_bwd(int dtype,
                                 const void* Mck,
                                 const void* rf, int64_t rf_sn,
                                 const void* gr, int64_t gr_sn,
                                 const void* loc,
                                 const void* df, int64_t df_sn, int64_t df_sm,
                                 const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                 const void* b1,
                                 const void* g,  int64_t g_sn,  int64_t g_sm,
                                 const void* E1, int64_t E1_sn, int64_t E1_sm,
                                 const void* E2, int64_t E2_sn, int64_t E2_sm,
                                 const void* E1m1,
                                 const void* sh, int64_t sh_sn, const void* shMap, int64_t nS,
                                 const void* grad_Mo,
                                 void* grad_Mi, void* grad_rf, void* grad_lead,
                                 void* work, size_t work_bytes,
                                 int64_t N, int64_t nM, int64_t nT,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2j  K2 with forward-mode tangents (ONE transmit coil: nC == 1, b1 (N, nM, 2) or NULL): Mo of mrphy_blochsim_rfgr_fwd,
 * bit for bit, and dMo (D, N, nM, 3), the directional derivatives of Mo along D directions.  A direction is a set of
 * tangents of the operands, one dense contiguous table of the data type per operand with a leading direction axis:
 *     dMi (D, N, nM, 3)   drf (D, N, 2, nT)   dgr (D, N, 3, nT)
 *     dloc (D, N, nM, 3)  ddf (D, N, nM)      db1 (D, N, nM, 2)
 *     dE1, dE2, dE1m1 (D, N, nM)              (the tangents of the step constants E1, E2 and E1 - 1)
 * Any of them may be NULL: a zero tangent.  The field's tangent is
 *     Bx' + i By' = b1 rf' + b1' rf,   Bz' = gr' . loc + gr . loc' + df' / gamma
 * (the kernel forms ddf / gamma from the gamma operand, as the primal does); there are no tangents of g, gamma.
 * The primal step, its S(x), C(x) and their derivatives are formed once per step and shared by the directions, which a
 * lane keeps in registers; the tangent's arithmetic is plain FMAs in the data type under every dtype code.  The
 * arithmetic of a direction does not depend on D or on the other directions: dMo[d] has the bits of the call with that
 * direction alone; a direction scaled by a power of two or negated scales or negates dMo[d] exactly, zero tangents
 * give zeros.  Mo may be NULL (not wanted).
 * mrphy_blochsim_rfgr_jvp_max_dirs(dtype): the most directions one launch takes (the kernels are built at the
 * capacities 1, 2, 4; the smallest that holds D runs): 4; < 0 for an unknown dtype code.
 * Checks, in this order: dtype and sizes; the mode arguments -- D < 1, D above the capacity, nC != 1, db1 without b1, ddf
 * without gamma, dE1 / dE2 / dE1m1 without relaxation (E1 NULL) -- MRPHY_EINVAL on an empty problem too; the empty problem
 * (N nM == 0) returns 0 and writes nothing; NULL Mi, dMo, loc, g, and rf or gr with nT > 0, are MRPHY_EINVAL, as are the
 * operands mrphy_blochsim_rfgr_fwd refuses; N > 65535 is MRPHY_EINVAL.  Nothing is launched after a refusal.  nT == 0
 * with spins runs: Mo = Mi, dMo = dMi (zeros without one).  No atomics, no workspace; the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------- */
int mrphy_blochsim_rfgr_jvp_max_dirs(int dtype);
int mrphy_blochsim_rfgr_jvp_fwd(int dtype,
                                const void* Mi,
                                const void* rf, int64_t rf_sn,
                                const void* gr, int64_t gr_sn,
                                const void* loc,
                                const void* df, int64_t df_sn, int64_t df_sm,
                                const void* gamma, int64_t gamma_sn, int64_t gamma_sm,
                                const void* b1,
                                const void* g,  int64_t g_sn,  int64_t g_sm,
                                const void* E1, int64_t E1_sn, int64_t E1_sm,
                                const void* E2, int64_t E2_sn, int64_t E2_sm,
                                const void* E1m1,
                                int64_t D,
                                const void* dMi, const void* drf, const void* dgr,
                                const void* dloc, const void* ddf, const void* db1,
                                const void* dE1, const void* dE2, const void* dE1m1,
                                void* Mo, void* dMo,
                                int64_t N, int64_t nM, int64_t nT, int64_t nC,
                                void* stream);

int mrphy_blochsim_ab(int dtype, const void* M, const void* A, const void* B, void* Mo,
                      int64_t rows, void* stream);
int mrphy_blochsim_ab_bwd(int dtype, const void* M, const void* A, const void* gMo, void* gM,
                          void* gA, int64_t rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRPHY_HIP_H */

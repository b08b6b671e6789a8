// dadmm_fused.hip — fused K-iteration unfolded D-ADMM forward for gfx950 (MI355X).
//
// Reference semantics: unfolded_DLASSO.py:34-140 (DLASSO_unfolded.forward / compute_delta) and,
// for the GNN variant, the fixed clamps of gnn_dlasso_models_progressive.py:205-232.
//
// Design:
//   * one workgroup = BT = 16 problem instances ("samples") x all P agents x all K iterations;
//     y_k and U_k never leave the CU: they live in VGPRs (lane = one sample and 4 rows of one
//     16-row n-tile); y_k is mirrored into LDS as the B operand of the next gradient GEMM, and
//     delta_k = 2 L y_k is recomputed from the y rows the lane already holds;
//   * the primal gradient is factored, G_p = A_p^T (A_p y_p - b_p), as two f32 MFMA GEMMs with
//     the batch as the N dimension (v_mfma_f32_16x16x4_f32: exact f32, one fma per product):
//       GEMM1  R_p[64 x 16] = A_p[64 x n] . Y_p[n x 16] - b_p   (wave w: m-block w%4, agents
//                                                                 w/4, w/4+2, ...)
//       GEMM2  G_p[n x 16]  = A_p^T[n x 64] . R_p[64 x 16]       (wave w: n/8 rows, all agents)
//     A_p and A_p^T (the prepared operator, 64 KB each per agent at n = 256) stream from L2;
//   * the gradient assembly, clamps, primal update, the neighbour consensus delta = 2 L y (in the
//     reference's accumulation order) and the dual update run on the GEMM2 accumulators in
//     registers; each iterate is written to Y[k] exactly once, 16 B per lane.
//
// Reduction order (restated bit-for-bit by oracle/dadmm_oracle.c): every dot product is ONE fma
// chain. Within each block of 16 reduction indices the chain visits 0,4,8,12, 1,5,9,13, 2,6,10,14,
// 3,7,11,15 (4 MFMAs, each folding k = 4h + r for h = 0..3); blocks ascend; GEMM1's chain starts
// from -b, GEMM2's from +0. Everything else is evaluated operation by operation like the
// reference's torch eager ops (built with -ffp-contract=off: no fma outside the MFMA chains).
//
// Global memory goes through buffer descriptors: 32-bit per-lane offsets, and the hardware range
// check returns 0 for loads / drops stores of the samples past B in the last workgroup.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dadmm_internal.h"
#include "dadmm_consensus.h"
#include "dadmm_device.h"

#ifndef DADMM_FUSED_REC
#define DADMM_FUSED_REC 0
#endif
// Decisions measured at the headline shape (the A/B switches were removed in
// round 6 once their experiments closed):
//   * GEMM2's A^T operand through a per-wave LDS ring filled by LDS-DMA (buffer_load ... lds), six
//     quarter-chains (16 n-rows x 16 m, 1 KB per wave) deep, no VGPRs in flight (a 2-4 step
//     register ring, a 5-deep ring and inline-asm DMAs were no faster);
//   * GEMM2 as paired chains: an agent's T2 n-tiles run as T2 interleaved accumulator chains that
//     share the R_p operand, the agent's primal update under the next agent's MFMAs;
//   * GEMM1's A operand through a 3-step register ring (4 steps: no faster);
//   * LDS rows of Ylds / Rlds padded by 8 floats: a 16-lane ds_read_b128 group {j = 0-3, 12-15
//     at h} + {j = 4-11 at h + 1} hits distinct 16-B bank slots iff the row stride is 8 mod 64
//     floats (+8: 0.589-0.648 ms vs +4: 0.604-0.606 ms, profiles/r04/variants_r04c.txt);
//   * two workgroup barriers per iteration (per-agent-group LDS arrival counters: no faster), the
//     second half of the waves at raised priority, the deferred dual update's reads as
//     ds_read_b32 (b128 chunks removed the remaining bank conflicts but spilled: slower).

namespace dadmm {

// The paired-chain GEMM2's A^T ring, simulated at compile time: quarter q = (4 p + t) T2 + tt is
// A^T_p rows of n-tile tt, m-block t. PRE quarters are issued before the phase (under GEMM1's
// last step, across the barrier); each step (p, t) first issues every quarter up to q0 + QD - 1
// (q0 = (4 p + t) T2: reusing only slots of quarters read before the previous step's MFMAs),
// then waits for its T2 quarters; after the MFMAs of agent p >= 1 the primal update of agent
// p - 1 issues T2 * SPQ stores. younger[q] = the VMEM ops issued after quarter q's DMA and
// before its wait, i.e. the exact s_waitcnt vmcnt(younger[q]) that guarantees it has landed.
template <int P, int T2, int QD, int SPQ>
struct G2Plan {
    static constexpr int NQ = P * 4 * T2;
    static constexpr int PRE = QD < NQ ? QD : NQ;
    int younger[NQ];
    constexpr G2Plan() : younger{} {
        int pos[NQ] = {};
        int op = 0, issued = 0;
        for (; issued < PRE; ++issued) pos[issued] = op++;
        for (int p = 0; p < P; ++p) {
            for (int t = 0; t < 4; ++t) {
                const int q0 = (4 * p + t) * T2;
                const int lim = q0 + QD - 1 < NQ - 1 ? q0 + QD - 1 : NQ - 1;
                for (; issued <= lim; ++issued) pos[issued] = op++;
                for (int tt = 0; tt < T2; ++tt) younger[q0 + tt] = op - 1 - pos[q0 + tt];
            }
            if (p > 0) op += T2 * SPQ;
        }
    }
};

// GRAPH: GRAPH_SHARED (one graph, ascending adjacency), GRAPH_LANE (per-sample, ascending),
//        GRAPH_ORDERED (per-sample, explicit adjacency order).
//
// The body is specialised per wave half (HALF = w / 4) so that every GEMM1 tile index is a
// compile-time constant: waves 0-3 own agents 0, 2, 4, ... and waves 4-7 agents 1, 3, ... of
// m-block w % 4 (waves w and w + 4 share a SIMD under the observed dispatch order, so each SIMD
// carries P GEMM1 tiles). All operand rings are indexed at compile time (full unroll), so the
// compiler never copies registers between pipeline stages and its vmcnt/lgkmcnt waits are counted.
template <int P, int NT, int GRAPH, int WV, int HALF, bool REC>
__device__ __forceinline__ void fused_body(const FusedArgs& a, float* __restrict__ lds, const int w) {
    constexpr bool SHARED_GRAPH = GRAPH == GRAPH_SHARED;
    constexpr int WAVES = WV;                        // waves per workgroup (4 or 8)
    constexpr int AS = WAVES / 4;                    // GEMM1 agent stride: agents HALF + AS*i
    constexpr int MP = M_PAD;                        // padded m: 4 m-blocks of 16
    constexpr int NP = NT * 64;                      // padded n
    constexpr int NB = NP / 16;                      // 16-row n-tiles
    constexpr int T2 = (NB + WAVES - 1) / WAVES;     // GEMM2 n-tiles per wave
    constexpr int E = T2 * 4;                        // state elements per lane per agent
    constexpr int TH = (P - HALF + AS - 1) / AS;     // GEMM1 tiles of this wave: agents HALF + AS*i
    constexpr int THA = TH > 0 ? TH : 1;             // array extent (P = 1 leaves half 1 idle)
    constexpr int YS = NP + 8;            // LDS row strides (floats): the padding
    constexpr int RS = MP + 8;            //   breaks the power-of-two bank period
    // GEMM1 A-operand ring depth: one step in flight under the MFMAs of the current step. A
    // deeper ring for the small-state instantiations perturbs the register allocation of the
    // large ones compiled in the same module (MI355X_MICROARCH §5.4 rule 19): measured 65 VGPR
    // spills for P=5, n=256 with a conditional depth, 3 with a uniform depth of 2.
    constexpr int RING = 3;
    float* __restrict__ Ylds = lds;                  // [P][BT][YS]   y_k, n contiguous
    float* __restrict__ Rlds = lds + P * BT * YS;    // [P][BT][RS]   A y - b, m contiguous
    constexpr int QD = 6;                            // A^T ring depth (quarter-chains per wave)
    float* __restrict__ Qlds = Rlds + P * BT * RS;   // [WAVES][QD][256] A^T ring

    const int lane = threadIdx.x & 63;
    const int j = lane & 15;             // sample within the tile (MFMA column)
    const int h = lane >> 4;             // 4-row group within a 16-row tile
    const int s = blockIdx.x * BT + j;   // global sample index
    const bool sv = s < a.B;
    const int n = a.n, m = a.m, B = a.B;
    const int mb = w & 3;                // GEMM1 m-block of this wave
    const bool has_tiles = w * T2 < NB;  // GEMM2 rows of this wave (always when NB >= WAVES)

    // buffer descriptors (bounds = the tensor, so lanes past B read 0 and never store)
    const uint32_t state_bytes = (uint32_t)((size_t)B * P * n * 4);
    const rsrc_t rA = make_rsrc(a.A, (uint32_t)(P * MP * NP * 4));
    const rsrc_t rAt = make_rsrc(a.At, (uint32_t)(P * MP * NP * 4));

    // ---- graph data --------------------------------------------------------------------------
    uint32_t msk[P], ord[P];
    float dg[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (SHARED_GRAPH) {
            msk[p] = __builtin_amdgcn_readfirstlane((uint32_t)a.nbr[p]);   // kernel-uniform
            dg[p] = a.deg[p];
        } else {
            msk[p] = sv ? (uint32_t)a.nbr[(size_t)s * P + p] : 0u;
            dg[p] = sv ? a.deg[(size_t)s * P + p] : 0.0f;
        }
        ord[p] = (GRAPH == GRAPH_ORDERED && sv) ? a.nbr_order[(size_t)s * P + p] : 0u;
    }

    // ---- state: this wave owns n-tiles nb = w*T2 + tt; element e = 4*tt + r is row
    //      nb*16 + 4h + r. D holds delta_k = 2 L y_k (k = 0: the caller's d0). y_k itself is not
    //      held in registers: it lives in the LDS tile Ylds (GEMM1's B operand), from which the
    //      lane reads its own rows back when the updates need them (40 VGPRs freed at H). ------
    float U[P][E], D[P][E];
    bool bad_y = false;
    // the lane's rows of y (row e of agent p) in the LDS tile
    auto ylds_at = [&](int p, int e) -> float* {
        return Ylds + (p * BT + j) * YS + (w * T2 + e / 4) * 16 + 4 * h + (e & 3);
    };
    {
        const rsrc_t ry = make_rsrc(a.y0, state_bytes);
        const rsrc_t ru = make_rsrc(a.U0, state_bytes);
        const rsrc_t rd = make_rsrc(a.d0, state_bytes);
#pragma unroll
        for (int tt = 0; tt < T2; ++tt) {
            const int nb = w * T2 + tt;
            const int n0 = nb * 16 + 4 * h;
            const bool ok = has_tiles && n0 < n;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const uint32_t off = (uint32_t)(((s * P + p) * n + n0) * 4);
                f32x4 vy = {0, 0, 0, 0}, vu = {0, 0, 0, 0}, vd = {0, 0, 0, 0};
                if (ok) {
                    vy = bload4(ry, off, 0);
                    vu = bload4(ru, off, 0);
                    vd = bload4(rd, off, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    bad_y |= !finitef(vy[r]);
                    U[p][4 * tt + r] = vu[r];
                    D[p][4 * tt + r] = vd[r];
                }
                if (has_tiles) *(f32x4*)(Ylds + (p * BT + j) * YS + n0) = vy;
            }
        }
    }
    // -b for this wave's GEMM1 tiles (agent HALF + AS*i, rows m = 16*mb + 4h + r) seeds every
    // iteration's GEMM1 chains, held in registers (the LDS next to R holds the A^T ring)
    f32x4 bseed[THA];
#pragma unroll
    for (int i = 0; i < TH; ++i) {
        const int p = HALF + AS * i;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int mi = 16 * mb + 4 * h + r;
            v[r] = (sv && mi < m) ? -a.b[((size_t)s * P + p) * m + mi] : 0.0f;
        }
        bseed[i] = v;
    }

    // Reference guards at the top of an iteration (unfolded_DLASSO.py:55-61) can only fire at
    // k = 0: with finite y_k, U_k, hyp and no NaN gradient every later y_k, U_k is finite (all
    // terms are clamped), and a NaN gradient is flagged where it arises.
    uint32_t status = 0;
    {
        bool bad_u = false;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int e = 0; e < E; ++e) bad_u |= !finitef(U[p][e]);
        status |= (bad_y ? DADMM_STATUS_Y_NONFINITE : 0) | (bad_u ? DADMM_STATUS_U_NONFINITE : 0);
    }

    // A non-finite hyper-parameter makes y_next NaN (reference guard :102): flag it once for the
    // whole table (the bit only triggers the exact guarded recomputation of the batch)
    {
        bool bad_h = false;
        const int nh = a.K * a.hyp_rows * 4;
        for (int i = threadIdx.x; i < nh; i += WAVES * 64) bad_h |= !finitef(a.hyp[i]);
        status |= bad_h ? DADMM_STATUS_YNEXT_NAN : 0;
    }
    // the shared graph's edges as float 0/1 multipliers, mf[a][b] = (b in N(a)), a < b (uniform);
    // consensus_fma needs a symmetric adjacency: an asymmetric one (a directed graph's successor
    // lists) raises DADMM_STATUS_RECOMPUTE, which sends the batch through the exact guarded path
    float mf[P][P];
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int p = 0; p < P; ++p) mf[q][p] = 0.0f;
    if constexpr (SHARED_GRAPH) {
        bool asym = false;
#pragma unroll
        for (int q = 0; q < P; ++q)
#pragma unroll
            for (int p = q + 1; p < P; ++p) {
                const bool e1 = (msk[q] >> p) & 1u, e2 = (msk[p] >> q) & 1u;
                asym |= e1 != e2;
                mf[q][p] = e1 ? 1.0f : 0.0f;
            }
        status |= asym ? DADMM_STATUS_RECOMPUTE : 0;
    }

    // per-lane byte offsets into the operator and the output
    const uint32_t voffA = (uint32_t)(((16 * mb + j) * NP + 4 * h) * 4);   // + p*MP*NP*4 + 64*t
    const uint32_t voffAt = (uint32_t)((j * MP + 4 * h) * 4);             // + (p*NP+16nb)*MP*4 + 64*t
    const uint32_t voffY = (uint32_t)((s * P * n + 4 * h) * 4);           // + (p*n + nb*16)*4
    const float* brow = Ylds + j * YS + 4 * h;                            // + p*BT*YS + 16*t
    uint32_t voffAtw[T2];                                                 // rows of tile tt
#pragma unroll
    for (int tt = 0; tt < T2; ++tt) voffAtw[tt] = voffAt + (uint32_t)(16 * (w * T2 + tt) * MP * 4);
    // GEMM2 quarter q = 4 (p T2 + tt) + t: A^T_p rows of n-tile w T2 + tt, m-block t, DMA'd into
    // ring slot q % QD of this wave (lane-linear: lane l's 16 bytes at l * 16, which is exactly the
    // MFMA A-operand fragment lane l reads back)
    auto dma_quarter = [&](const uint32_t (&vAt)[T2], int q) {
        const int tt = q % T2, t = (q / T2) & 3, p = q / (4 * T2);   // see G2Plan
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rAt, (lds_void*)(Qlds + (w * QD + q % QD) * 256), 16,
                                                 vAt[tt] + 64 * t, (uint32_t)(p * NP * MP * 4), 0, 0);
    };

    // GEMM1 A-operand ring: slot t % RING holds A rows of step t (16 columns) for the TH tiles.
    // The first step of every iteration is issued before the previous iteration's last Y stores,
    // so it is not queued behind them (vmcnt counts loads and stores in order).
    f32x4 aring[RING][THA];
    // soffset carries the agent's 64-KB block, the instruction's immediate the 64-B step: no
    // per-(tile, step) address registers.
    uint32_t vA = voffA;                 // re-laundered every iteration (see fresh())
    auto load_a = [&](f32x4 (&slot)[THA], int t) {
#pragma unroll
        for (int i = 0; i < TH; ++i)
            slot[i] = bload4(rA, vA + 64 * t, (uint32_t)((HALF + AS * i) * MP * NP * 4));
    };
#pragma unroll
    for (int t = 0; t + 1 < RING; ++t) load_a(aring[t], t);
    if (HALF == 1) __builtin_amdgcn_s_setprio(1);   // the second-dispatched half loses arbitration
    __syncthreads();

    // dual update deferred from the previous iteration: delta_k = 2 L y_k for row e (all agents,
    // lane-local), GNN delta clamp, U_k = clamp(U_{k-1} + delta_k * eta_{k-1}) (:95-99)
    float et_prev[P];
    float vclip_prev = 0.0f;
#pragma unroll
    for (int p = 0; p < P; ++p) et_prev[p] = 0.0f;
    // GNN variant: delta clamped to +-20 (:229); the unfolded variant: +-inf (a no-op on finite d)
    const float dlim = a.variant != 0 ? GNN_DELTA_LIMIT : __builtin_inff();
    auto dual_update_row = [&](int e, const uint32_t (&mk)[P], bool live, const float* yrow = nullptr) {
        float yy[P][1], dd[P][1];
#pragma unroll
        for (int p = 0; p < P; ++p) yy[p][0] = yrow != nullptr ? yrow[p] : *ylds_at(p, e);   // y_{k+1}, row e
        if constexpr (GRAPH == GRAPH_SHARED)
            consensus_fma<P>(yy, dd, mf);
        else if constexpr (GRAPH == GRAPH_LANE)
            consensus_lane<P, 1>(yy, dd, mk);
        else
            consensus_ordered<P, 1>(yy, dd, mk, ord);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            // dual_elem's two atoms (the composite around the select compiles to other code)
            const float d = delta_clamp<Clamp::MED3>(dd[p][0], dlim);
            const float un = dual_u<Clamp::MED3>(U[p][e], d, et_prev[p], vclip_prev);
            // k = 0 keeps the caller's U0, delta0 (a select, not a branch: the row stays one
            // basic block, interleavable with the GEMM1 MFMAs)
            D[p][e] = live ? d : D[p][e];
            U[p][e] = live ? un : U[p][e];
        }
    };

    for (int k = 0; k < a.K; ++k) {
        vA = fresh(voffA);
        // shared graph: re-launder the (uniform) masks so the neighbour tests are evaluated in the
        // loop (s_bitcmp + branch) instead of being hoisted as P*P 64-bit condition registers
        uint32_t mk[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if constexpr (SHARED_GRAPH) mk[p] = fresh_s(msk[p]);
            else mk[p] = msk[p];
        }
        uint32_t vAt[T2];
#pragma unroll
        for (int tt = 0; tt < T2; ++tt) vAt[tt] = fresh(voffAtw[tt]);
        // seq_hyp(k) row(s): (alpha, tau, rho, eta) — kernel-uniform scalars
        float al[P], ta[P], rh[P], et[P];
#pragma unroll
        for (int p = 0; p < P; ++p) load_hyp_row(a, k, p, al[p], ta[p], rh[p], et[p]);
        float gclip, vclip;
        iter_clips(a.variant, k, gclip, vclip);
        const bool deferred = k > 0;

        // ---- GEMM1: R_p = A_p y_p - b_p for this wave's TH tiles, with the previous
        //      iteration's dual update interleaved (VALU under the MFMA chains) ------------------
        {
            f32x4 acc[THA];
#pragma unroll
            for (int i = 0; i < TH; ++i)
                acc[i] = bseed[i];
            f32x4 bring[2][THA];
#pragma unroll
            for (int i = 0; i < TH; ++i)
                bring[0][i] = *(const f32x4*)(brow + (HALF + AS * i) * BT * YS);
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                if (t + RING - 1 < NB) load_a(aring[(t + RING - 1) % RING], t + RING - 1);
                compiler_fence();
                if (t + 1 < NB) {
#pragma unroll
                    for (int i = 0; i < TH; ++i)
                        bring[(t + 1) & 1][i] =
                            *(const f32x4*)(brow + (HALF + AS * i) * BT * YS + 16 * (t + 1));
                }
                const f32x4(&av)[THA] = aring[t % RING];
                const f32x4(&bv)[THA] = bring[t & 1];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int i = 0; i < TH; ++i) acc[i] = mfma4(av[i][r], bv[i][r], acc[i]);
                // GEMM2's first quarters, in flight across the barrier
                if (t == NB - 1 && has_tiles) {
#pragma unroll
                    for (int q = 0; q < QD && q < P * T2 * 4; ++q) dma_quarter(vAt, q);
                }
                // rows e with e * NB / E == t
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((e * NB) / E == t && has_tiles) dual_update_row(e, mk, deferred);
            }
#pragma unroll
            for (int i = 0; i < TH; ++i)
                *(f32x4*)(Rlds + ((HALF + AS * i) * BT + j) * RS + 16 * mb + 4 * h) = acc[i];
        }
        __syncthreads();

        // ---- GEMM2 (G_p = A_p^T R_p) as a sequence of (agent, n-tile) chains of 16 MFMAs; the
        //      A^T rows of the next chain load one chain ahead, and each chain's gradient
        //      assembly + primal update runs under the next chain's MFMAs -------------------------
        if (has_tiles) {
            const rsrc_t rY = make_rsrc(a.Y + (size_t)k * B * P * n, state_bytes);
            // REC (training): the adjoint's trajectory, Grec[k] = pre-clamp gradient, Urec[k] = U_k
            const rsrc_t rG = make_rsrc(REC ? a.Grec + (size_t)k * B * P * n : a.Y, REC ? state_bytes : 0u);
            const rsrc_t rUr = make_rsrc(REC ? a.Urec + (size_t)k * B * P * n : a.Y, REC ? state_bytes : 0u);
            [[maybe_unused]] constexpr int NS = P * T2;      // chains: s = p*T2 + tt
            [[maybe_unused]] f32x4 g[2];
            f32x4 rv[MP / 16];
            bool bad_g = false;
            // primal update of (agent p, tile tt) from its G (:73-93); iterate to LDS and Y[k]
            auto primal_update = [&](int s2, const f32x4& gp) {
                const int p = s2 / T2, tt = s2 % T2;
                const int nb = w * T2 + tt;
                const int n0 = nb * 16 + 4 * h;
                f32x4 yn, grv, urv;
                const f32x4 yk = *(const f32x4*)(Ylds + (p * BT + j) * YS + n0);   // y_k, 4 rows
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = 4 * tt + r;
                    const float yv = yk[r];
                    // (its sign(y)*tau, exactly +-tau or +0, is branch-free: a nested ternary
                    // compiles to short divergent branches between the MFMAs)
                    const float gr = grad_assemble(gp[r], yv, U[p][e], D[p][e], ta[p], dg[p], rh[p]);
                    grv[r] = gr;
                    urv[r] = U[p][e];
                    bad_g |= (gr != gr);                            // :84 guard (flag only)
                    yn[r] = primal_elem<Clamp::MED3>(yv, gr, al[p], gclip, vclip);
                }
                *(f32x4*)(Ylds + (p * BT + j) * YS + n0) = yn;
                // Y[k][s][p][n0..n0+3]; rows past n go to an offset the range check drops
                bstore4<16>(yn, rY, n0 < n ? voffY + (uint32_t)((p * n + nb * 16) * 4) : 0x80000000u);
                if constexpr (REC) {
                    const uint32_t o = n0 < n ? voffY + (uint32_t)((p * n + nb * 16) * 4) : 0x80000000u;
                    bstore4<16>(grv, rG, o);
                    bstore4<16>(urv, rUr, o);
                }
            };
            // stores of one primal update (Y[k], and Grec / Urec when recording)
            constexpr int SPQ = REC ? 3 : 1;
            constexpr G2Plan<P, T2, QD, SPQ> plan{};
            f32x4 gp[2][T2];
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int p = i;
                compiler_fence();
#pragma unroll
                for (int t = 0; t < MP / 16; ++t)
                    rv[t] = *(const f32x4*)(Rlds + (p * BT + j) * RS + 4 * h + 16 * t);
                f32x4 gc[T2];
#pragma unroll
                for (int tt = 0; tt < T2; ++tt) gc[tt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int t = 0; t < MP / 16; ++t) {
                    const int q0 = (4 * i + t) * T2;
                    // every quarter up to q0 + QD - 1 (the slots of the quarters read before the
                    // previous step's MFMAs), then this step's waits (exact counts: G2Plan)
#pragma unroll
                    for (int x = q0 + QD - T2; x < q0 + QD; ++x)
                        if (q0 > 0 && x < G2Plan<P, T2, QD, SPQ>::NQ) dma_quarter(vAt, x);
                    f32x4 av[T2];
#pragma unroll
                    for (int tt = 0; tt < T2; ++tt) {
                        wait_vm<16>(plan.younger[q0 + tt]);
                        av[tt] = *(const f32x4*)(Qlds + (w * QD + (q0 + tt) % QD) * 256 + lane * 4);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int tt = 0; tt < T2; ++tt) gc[tt] = mfma4(av[tt][r], rv[t][r], gc[tt]);
                }
#pragma unroll
                for (int tt = 0; tt < T2; ++tt) gp[i & 1][tt] = gc[tt];
                if (i + 1 == P && k + 1 < a.K) {
                    // next iteration's first GEMM1 steps, after every ring wait (so no wait has
                    // to count them), before the last agent's Y stores
                    for (int t0 = 0; t0 + 1 < RING; ++t0) load_a(aring[t0], t0);
                }
                if (i > 0) {
#pragma unroll
                    for (int tt = 0; tt < T2; ++tt) primal_update((i - 1) * T2 + tt, gp[(i - 1) & 1][tt]);
                }
            }
#pragma unroll
            for (int tt = 0; tt < T2; ++tt) primal_update((P - 1) * T2 + tt, gp[(P - 1) & 1][tt]);
            status |= bad_g ? DADMM_STATUS_GRAD_NAN : 0;
        } else if (k + 1 < a.K) {
            for (int t0 = 0; t0 + 1 < RING; ++t0) load_a(aring[t0], t0);
        }
#pragma unroll
        for (int p = 0; p < P; ++p) et_prev[p] = et[p];
        vclip_prev = vclip;
        __syncthreads();
    }

    if (a.U_out != nullptr && has_tiles) {
        // the dual update of the last iteration (deferred like the others)
        uint32_t mk[P];
#pragma unroll
        for (int p = 0; p < P; ++p) mk[p] = msk[p];
        if (a.K > 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) dual_update_row(e, mk, true);
        }
        const rsrc_t rU = make_rsrc(a.U_out, state_bytes);
#pragma unroll
        for (int tt = 0; tt < T2; ++tt) {
            const int n0 = (w * T2 + tt) * 16 + 4 * h;
            if (n0 < n) {
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const f32x4 v = {U[p][4 * tt], U[p][4 * tt + 1], U[p][4 * tt + 2], U[p][4 * tt + 3]};
                    bstore4(v, rU, (uint32_t)(((s * P + p) * n + n0) * 4), 0);
                }
            }
        }
    }
    if (a.status != nullptr) {
        // lanes past B carry zero state and never set a bit; one atomic per wave
        uint32_t wst = status;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) wst |= __shfl_xor(wst, off);
        if (lane == 0 && wst) atomicOr((unsigned int*)a.status, wst);
    }
}

template <int P, int NT, int GRAPH, int WV, bool REC>
__global__ __launch_bounds__(WV * 64) void fused_forward_kernel(FusedArgs a) {
    constexpr int NP = NT * 64;
    // Ylds + Rlds + the waves' A^T rings
    __shared__ __attribute__((aligned(16))) float lds[P * BT * ((NP + 8) + (M_PAD + 8)) + WV * 6 * 256];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave id, in an SGPR
    static_assert(WV == 8, "8 waves per workgroup (2 per SIMD; 4 and 16 measured slower, DESIGN.md §4.1)");
    if (w < 4)
        fused_body<P, NT, GRAPH, 8, 0, REC>(a, lds, w);
    else
        fused_body<P, NT, GRAPH, 8, 1, REC>(a, lds, w);
}

// ----------------------------------------------------------------------------------------------
template <int P, int NT, int GRAPH>
static hipError_t launch_fused(const FusedArgs& a, hipStream_t stream) {
    const int grid = (a.B + BT - 1) / BT;
    hipLaunchKernelGGL((fused_forward_kernel<P, NT, GRAPH, FUSED_WAVES, DADMM_FUSED_REC != 0>), dim3(grid),
                       dim3(FUSED_WAVES * 64), 0, stream, a);
    return hipGetLastError();
}

template <int P, int NT>
static fused_fn_ptr pick_graph(int graph) {
    switch (graph) {
        case GRAPH_SHARED: return &launch_fused<P, NT, GRAPH_SHARED>;
        case GRAPH_LANE: return &launch_fused<P, NT, GRAPH_LANE>;
        case GRAPH_ORDERED: return &launch_fused<P, NT, GRAPH_ORDERED>;
        default: return nullptr;
    }
}

// Instantiated shapes: P = 1..6, n_pad = 64 * NT with NT in {1, 2, 4} (NT = 4 only for P <= 5:
// the register budget of 2 waves per SIMD), m_pad = 64.
template <int P>
static fused_fn_ptr pick_nt(int nt, int graph) {
    if (nt == 1) return pick_graph<P, 1>(graph);
    if (nt == 2) return pick_graph<P, 2>(graph);
    if constexpr (P <= 5) {
        if (nt == 4) return pick_graph<P, 4>(graph);
    }
    return nullptr;
}


// This file is compiled twice (csrc/Makefile): DADMM_FUSED_REC = 0 defines find_fused (inference),
// DADMM_FUSED_REC = 1 defines find_fused_rec (training: also records Grec / Urec).
#if DADMM_FUSED_REC
fused_fn_ptr find_fused_rec(int P, int nt, int graph) {
#else
fused_fn_ptr find_fused(int P, int nt, int graph) {
#endif
    switch (P) {
        case 1: return pick_nt<1>(nt, graph);
        case 2: return pick_nt<2>(nt, graph);
        case 3: return pick_nt<3>(nt, graph);
        case 4: return pick_nt<4>(nt, graph);
        case 5: return pick_nt<5>(nt, graph);
        case 6: return pick_nt<6>(nt, graph);
        default: return nullptr;
    }
}

}  // namespace dadmm

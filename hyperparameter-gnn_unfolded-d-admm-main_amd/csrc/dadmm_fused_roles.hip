// dadmm_fused_roles.hip — the fused K-iteration forward with the workgroup's waves split into a
// matrix role and an update role, for the shared-graph, non-recording
// instantiations at n_pad = 256 (P = 1..5, m <= 64).
//
// Same problem decomposition and the same bits as dadmm_fused.hip (one workgroup = 16 samples x all
// agents x all K iterations; every dot product the same single fma chain; every element operation
// through the same grad_assemble / primal_elem / dual_elem of dadmm_device.h). What differs is who
// runs what:
//   * waves 0-3 (one per SIMD) issue only MFMAs, their operand loads and the accumulator stores:
//       GEMM1  R_p = A_p y_p - b_p   wave w: m-block w of every agent, agents interleaved;
//       GEMM2  G_p = A_p^T R_p       wave w: n-tiles 4w..4w+3 of every agent as four interleaved
//                                    chains sharing the R_p operand; G_p goes to the LDS tile
//                                    Glds[p & 1];
//     A / A^T fragments stream from L2 through ONE compile-time-indexed register ring that runs
//     through the whole iteration (GEMM2 of agents 0..P-1, then GEMM1 of the next iteration) and
//     wraps into the next one: RD fragments of lead, no LDS ring, no LDS-DMA. With RES = 1 the
//     GEMM1 operand of one agent (RA: rows 16 w..16 w + 15 of A_RA, 64 VGPRs the kernel's
//     allocation leaves this role anyway) is loaded once per launch and stays in registers for all
//     K iterations; the stream carries the other agents only;
//   * waves 4-7 (their SIMD partners) hold U and delta (wave u: n-tiles 4u..4u+3 of every agent,
//     16 rows per lane and agent) and do everything else: the gradient assembly, clamps and primal
//     update from Glds / Ylds, the Y[k] store, the consensus and the dual update, the input and
//     hyper-parameter guards, U_out and the status word.
// Synchronisation is workgroup barriers only, P + 2 per iteration, the same count on every path of
// both roles:
//   stage s = 0..P-1   matrix: GEMM2 of agent s          update: primal update of agent s - 1
//   stage P            matrix: GEMM1(k+1), agents < G1A  update: primal update of agent P - 1
//   stage P + 1        matrix: GEMM1(k+1), the others    update: consensus and dual update
// (agent P - 1's y_{k+1} is complete only after stage P, so it is always in the second group).
// The resident agent's GEMM1 chain runs in its group's stage like the others, interleaved with
// them step by step: same operands, same order, same seed, so the same bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dadmm_internal.h"
#include "dadmm_consensus.h"
#include "dadmm_device.h"

namespace dadmm {

template <int P, int RES>
struct Roles {
    static constexpr int NP = 256;              // padded n (NT = 4)
    static constexpr int NB = NP / 16;          // 16-row n-tiles
    static constexpr int MP = M_PAD;
    static constexpr int YS = NP + 8;           // LDS row strides (floats), 8 mod 64: see dadmm_fused.hip
    static constexpr int RS = MP + 8;
    static constexpr int GS = NP + 8;
    // operand ring depth (fragments of 4 VGPRs; must divide 16 P and NF). Streamed only, at P = 5:
    // 20 measured 1 % under 16 at the headline shape; 40 spills beside the update role's 227
    // registers. With the resident block NF = 32 P - 16, so 16 for every P
    static constexpr int RD = (P == 5 && RES == 0) ? 20 : 16;
    static constexpr int G1A = (P - 1) / 2;     // GEMM1 agents of stage P (agents 0..G1A-1)
    static constexpr int G1B = P - G1A;         // GEMM1 agents of stage P + 1
    // the resident agent (RES = 1). Agent 0 puts the block in stage P where there is one (P >= 3):
    // at P = 5 that stage then streams agent 1 alone, 16 fragments, which the ring already holds
    // when the stage begins, and stage P + 1 streams its three agents beside the consensus as
    // before. Measured at the headline shape against the streamed form: agent 0
    // -0.031 ms; agent G1A (two streamed agents in either stage) and agent P - 1 -0.003 ms
    static constexpr int RA = 0;
    static constexpr int SA = G1A - (RES && RA < G1A ? 1 : 0);    // streamed GEMM1 agents of stage P
    static constexpr int SB = G1B - (RES && RA >= G1A ? 1 : 0);   // ... of stage P + 1
    static constexpr int NF = 32 * P - 16 * RES;                  // fragments per wave and iteration
    static constexpr int LDS_FLOATS = P * BT * YS + P * BT * RS + 2 * BT * GS;
    static_assert(RES == 0 || RES == 1, "one resident block or none");
    static_assert(RA >= 0 && RA < P, "the resident agent");
    static_assert(NF == 16 * (P + SA + SB), "the stream: GEMM2 of every agent, GEMM1 of the streamed ones");
    static_assert(NF % RD == 0, "ring slots must line up where the stream wraps");
    static_assert((16 * P) % RD == 0, "ring slots must line up at the GEMM2 / GEMM1 boundary");
};

template <int V>
using ic = std::integral_constant<int, V>;

// ---- matrix role: waves 0-3 ----------------------------------------------------------------------
// The instruction scheduler may not move anything across this point: it keeps every operand load
// where the ring issues it (RD fragments ahead of its MFMAs; left alone it sinks the loads to their
// uses) and a stage's MFMAs and accumulator stores on their side of the stage's barrier.
__device__ __forceinline__ void pin() { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ void stage_barrier() {
    pin();
    __syncthreads();
    pin();
}

template <int P, int RES>
__device__ __forceinline__ void roles_matrix(const FusedArgs& a, float* __restrict__ lds, const int w) {
    using C = Roles<P, RES>;
    constexpr int NP = C::NP, NB = C::NB, MP = C::MP, YS = C::YS, RS = C::RS, GS = C::GS;
    constexpr int RD = C::RD, NF = C::NF, G1A = C::G1A, G1B = C::G1B, RA = C::RA, SA = C::SA, SB = C::SB;
    float* __restrict__ Ylds = lds;                  // [P][BT][YS]   y_k, n contiguous
    float* __restrict__ Rlds = lds + P * BT * YS;    // [P][BT][RS]   A y - b, m contiguous
    float* __restrict__ Glds = Rlds + P * BT * RS;   // [2][BT][GS]   G_p, n contiguous (agent parity)

    const int lane = threadIdx.x & 63;
    const int j = lane & 15;             // sample within the tile (MFMA column)
    const int h = lane >> 4;             // 4-row group within a 16-row tile
    const int s = blockIdx.x * BT + j;   // global sample index
    const bool sv = s < a.B;
    const int m = a.m;

    const rsrc_t rA = make_rsrc(a.A, (uint32_t)(P * MP * NP * 4));
    const rsrc_t rAt = make_rsrc(a.At, (uint32_t)(P * MP * NP * 4));

    // -b for m-block w of every agent (rows 16 w + 4 h + r) seeds every iteration's GEMM1 chains
    f32x4 bseed[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int mi = 16 * w + 4 * h + r;
            v[r] = (sv && mi < m) ? -a.b[((size_t)s * P + p) * m + mi] : 0.0f;
        }
        bseed[p] = v;
    }

    // per-lane byte offsets into the operator
    const uint32_t voffA = (uint32_t)(((16 * w + j) * NP + 4 * h) * 4);        // + p*MP*NP*4 + 64*t
    const uint32_t voffAt = (uint32_t)(((64 * w + j) * MP + 4 * h) * 4);       // + (p*NP + 16 tt)*MP*4 + 64*t
    const float* brow = Ylds + j * YS + 4 * h;                                 // + p*BT*YS + 16*t
    uint32_t vA = voffA, vAt = voffAt;   // re-laundered every iteration (see fresh())

    // The iteration's fragment stream, in consumption order:
    //   i <  16 P:  GEMM2, agent i / 16, m-block (i % 16) / 4, n-tile 4 w + i % 4;
    //   then GEMM1 of the streamed agents of 0..G1A-1 (step t, the group's c-th streamed agent:
    //   t * SA + c), then of those of G1A..P-1 (t * SB + c); the resident agent has no fragment here.
    // Fragment i lives in ring slot i % RD; fragment i + RD is issued right behind the MFMAs that
    // read fragment i. soffset carries the agent's (and the n-tile's) block, the immediate the
    // 64-B step.
    f32x4 ring[RD];
    auto frag_load = [&](int i) {
        if (i < 16 * P) {
            const int p = i / 16, t = (i % 16) / 4, tt = i % 4;
            ring[i % RD] = bload4(rAt, vAt + 64 * t, (uint32_t)((p * NP + 16 * tt) * MP * 4));
        } else {
            int ii = i - 16 * P, p, t;
            if (ii < 16 * SA) {
                t = ii / (SA > 0 ? SA : 1);
                p = ii % (SA > 0 ? SA : 1);
                if (RES && RA < G1A && p >= RA) ++p;
            } else {
                ii -= 16 * SA;
                t = ii / (SB > 0 ? SB : 1);
                p = G1A + ii % (SB > 0 ? SB : 1);
                if (RES && RA >= G1A && p >= RA) ++p;
            }
            ring[i % RD] = bload4(rA, vA + 64 * t, (uint32_t)(p * MP * NP * 4));
        }
    };

    // the resident block: agent RA's 16 GEMM1 fragments of this wave, at the offsets the ring would
    // load them from. Loaded here, once per launch, and read by every iteration's GEMM1
    f32x4 res[RES ? NB : 1];
    if constexpr (RES) {
#pragma unroll
        for (int t = 0; t < NB; ++t) res[t] = bload4(rA, voffA + 64 * t, (uint32_t)(RA * MP * NP * 4));
    }

    // GEMM1 of agents P0..P0+CNT-1 (interleaved chains); the streamed ones' fragments from stream
    // position BASE, the resident agent's from res
    auto gemm1 = [&](auto p0_, auto cnt_, auto base_) {
        constexpr int P0 = decltype(p0_)::value, CNT = decltype(cnt_)::value, BASE = decltype(base_)::value;
        constexpr bool HAS = RES && RA >= P0 && RA < P0 + CNT;   // the resident agent is in this group
        constexpr int S = CNT - (HAS ? 1 : 0);                   // streamed chains
        // chain i's place among the group's streamed chains
        auto sidx = [](int i) { return i - ((HAS && P0 + i > RA) ? 1 : 0); };
        if constexpr (CNT > 0) {
            f32x4 acc[CNT];
            f32x4 bring[2][CNT];
#pragma unroll
            for (int i = 0; i < CNT; ++i) {
                acc[i] = bseed[P0 + i];
                bring[0][i] = *(const f32x4*)(brow + (P0 + i) * BT * YS);
            }
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                if (t + 1 < NB) {
#pragma unroll
                    for (int i = 0; i < CNT; ++i)
                        bring[(t + 1) & 1][i] = *(const f32x4*)(brow + (P0 + i) * BT * YS + 16 * (t + 1));
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int i = 0; i < CNT; ++i) {
                        const float av = (HAS && P0 + i == RA) ? res[t][r] : ring[(BASE + t * S + sidx(i)) % RD][r];
                        acc[i] = mfma4(av, bring[t & 1][i][r], acc[i]);
                    }
#pragma unroll
                for (int i = 0; i < S; ++i) frag_load((BASE + t * S + i + RD) % NF);
                pin();
            }
#pragma unroll
            for (int i = 0; i < CNT; ++i)
                *(f32x4*)(Rlds + ((P0 + i) * BT + j) * RS + 16 * w + 4 * h) = acc[i];
        }
    };

    // GEMM2 of agent p: four n-tile chains over the shared R_p operand; R_{p+1} is read a stage ahead
    f32x4 rvb[2][MP / 16];
    auto load_r = [&](int p) {
#pragma unroll
        for (int t = 0; t < MP / 16; ++t)
            rvb[p & 1][t] = *(const f32x4*)(Rlds + (p * BT + j) * RS + 4 * h + 16 * t);
    };
    auto gemm2 = [&](auto p_) {
        constexpr int p = decltype(p_)::value;
        if constexpr (p + 1 < P) load_r(p + 1);
        f32x4 gc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) gc[tt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < MP / 16; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
                    gc[tt] = mfma4(ring[(16 * p + 4 * t + tt) % RD][r], rvb[p & 1][t][r], gc[tt]);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) frag_load((16 * p + 4 * t + tt + RD) % NF);
            pin();
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
            *(f32x4*)(Glds + ((p & 1) * BT + j) * GS + 16 * (4 * w + tt) + 4 * h) = gc[tt];
    };
    auto gemm2_all = [&](auto self, auto p_) -> void {
        constexpr int p = decltype(p_)::value;
        if constexpr (p < P) {
            gemm2(p_);
            stage_barrier();
            self(self, ic<p + 1>{});
        }
    };

    // the ring's first RD fragments: the head of GEMM1, running on into GEMM2 where fewer than RD
    // GEMM1 fragments are streamed
#pragma unroll
    for (int i = 0; i < RD; ++i) frag_load((16 * P + i) % NF);
    __syncthreads();                     // y_0 in Ylds

    gemm1(ic<0>{}, ic<G1A>{}, ic<16 * P>{});
    gemm1(ic<G1A>{}, ic<G1B>{}, ic<16 * P + 16 * SA>{});
    stage_barrier();                     // R(0)

    for (int k = 0; k < a.K; ++k) {
        vA = fresh(voffA);
        vAt = fresh(voffAt);
        load_r(0);
        gemm2_all(gemm2_all, ic<0>{});   // stages 0..P-1, a barrier after each
        if (k + 1 < a.K) {
            gemm1(ic<0>{}, ic<G1A>{}, ic<16 * P>{});
            stage_barrier();             // stage P
            gemm1(ic<G1A>{}, ic<G1B>{}, ic<16 * P + 16 * SA>{});
            stage_barrier();             // stage P + 1
        } else {
            __syncthreads();
            __syncthreads();
        }
    }
}

// ---- update role: waves 4-7 (u = wave - 4) --------------------------------------------------------
// EVAL (the evaluation forward, fused_roles_eval_kernel; ev is its EvalArgs, unused otherwise): the
// same update, and beside it the iterate's squared error against the label. A lane needs the same
// 16 label rows for every agent and iteration: it parks them in an LDS tile [BT][YS] behind the
// forward's tiles (written and read by that lane alone: no barrier), sums (y_{k+1} - x)^2 over its
// P * 16 elements in one fp32 accumulator in the fixed order p, tt, r, and the wave's sum goes to
// ev->partial[k][4 blockIdx.x + u]. Of the iterates only y_K is stored (a.Y is y_final [B][P][n]).
template <int P, bool EVAL = false>
__device__ __forceinline__ void roles_update(const FusedArgs& a, float* __restrict__ lds, const int u,
                                             const EvalArgs* ev = nullptr) {
    using C = Roles<P, 0>;               // (the LDS layout: the same with and without the resident block)
    constexpr int NP = C::NP, MP = C::MP, YS = C::YS, RS = C::RS, GS = C::GS;
    constexpr int T2 = 4;                // n-tiles of this wave: 4 u + tt
    constexpr int E = T2 * 4;            // state elements per lane per agent
    float* __restrict__ Ylds = lds;
    float* __restrict__ Glds = lds + P * BT * YS + P * BT * RS;
    float* __restrict__ Llds = Glds + 2 * BT * GS;   // EVAL: [BT][YS] the label rows
    (void)NP; (void)MP; (void)Llds;

    const int lane = threadIdx.x & 63;
    const int j = lane & 15;
    const int h = lane >> 4;
    const int s = blockIdx.x * BT + j;
    const int n = a.n, B = a.B;
    const uint32_t state_bytes = (uint32_t)((size_t)B * P * n * 4);

    // ---- graph data (shared graph: kernel-uniform) -------------------------------------------------
    uint32_t msk[P];
    float dg[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        msk[p] = __builtin_amdgcn_readfirstlane((uint32_t)a.nbr[p]);
        dg[p] = a.deg[p];
    }

    // ---- state: element e = 4 tt + r is row 16 (4 u + tt) + 4 h + r; y_k lives in Ylds ---------------
    float U[P][E], D[P][E];
    // the largest |y0| and |U0| bit patterns: at or above +inf's iff a value is not finite (one
    // running register each, folded in as the loads land, instead of a compare per element)
    uint32_t ymag = 0, umag = 0;
    {
        const rsrc_t ry = make_rsrc(a.y0, state_bytes);
        const rsrc_t ru = make_rsrc(a.U0, state_bytes);
        const rsrc_t rd = make_rsrc(a.d0, state_bytes);
#pragma unroll
        for (int tt = 0; tt < T2; ++tt) {
            const int nb = u * T2 + tt;
            const int n0 = nb * 16 + 4 * h;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                // rows past n (and samples past B) read 0: an offset the range check rejects
                const uint32_t off = n0 < n ? (uint32_t)(((s * P + p) * n + n0) * 4) : 0x80000000u;
                const f32x4 vy = bload4(ry, off, 0);
                const f32x4 vu = bload4(ru, off, 0);
                const f32x4 vd = bload4(rd, off, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ymag = max(ymag, __float_as_uint(vy[r]) & 0x7fffffffu);
                    umag = max(umag, __float_as_uint(vu[r]) & 0x7fffffffu);
                    U[p][4 * tt + r] = vu[r];
                    D[p][4 * tt + r] = vd[r];
                }
                *(f32x4*)(Ylds + (p * BT + j) * YS + n0) = vy;
            }
            ymag = fresh(ymag);
            umag = fresh(umag);
            compiler_fence();            // one tile's loads in flight at a time (register budget)
        }
    }
    if constexpr (EVAL) {
        // label [B][n]: rows past n and samples past B read 0, as the state above (there y stays 0
        // too, so they add exactly 0). Its largest magnitude bits flag a non-finite label as
        // dadmm_loss.hip's partial_kernel does
        const rsrc_t rl = make_rsrc(ev->label, (uint32_t)((size_t)B * n * 4));
        uint32_t lmag = 0;
#pragma unroll
        for (int tt = 0; tt < T2; ++tt) {
            const int n0 = (u * T2 + tt) * 16 + 4 * h;
            const f32x4 vx = bload4(rl, n0 < n ? (uint32_t)((s * n + n0) * 4) : 0x80000000u, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) lmag = max(lmag, __float_as_uint(vx[r]) & 0x7fffffffu);
            *(f32x4*)(Llds + j * YS + n0) = vx;
        }
        if (__ballot(lmag >= 0x7f800000u) != 0 && lane == 0) atomicOr((unsigned int*)ev->loss_flags, 1u);
    }
    __syncthreads();                     // y_0 in Ylds: the matrix waves start GEMM1(0)

    // dadmm_fused.hip's guards, restated ("The element update"): the y_0 / U_0
    // magnitudes, the hyper-parameter table over the update role's 256 threads, the shared graph's
    // asymmetry (DADMM_STATUS_GRAD_NAN in the loop)
    uint32_t status = (ymag >= 0x7f800000u ? DADMM_STATUS_Y_NONFINITE : 0) |
                      (umag >= 0x7f800000u ? DADMM_STATUS_U_NONFINITE : 0);
    {
        bool bad_h = false;
        const int nh = a.K * a.hyp_rows * 4;
        for (int i = threadIdx.x - 256; i < nh; i += 256) bad_h |= !finitef(a.hyp[i]);
        status |= bad_h ? DADMM_STATUS_YNEXT_NAN : 0;
    }
    // consensus_fma's multiplier table, each multiplier through readfirstlane: provably uniform, so
    // it is held in an SGPR
    float mf[P][P];
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int p = 0; p < P; ++p) mf[q][p] = 0.0f;
    {
        bool asym = false;
#pragma unroll
        for (int q = 0; q < P; ++q)
#pragma unroll
            for (int p = q + 1; p < P; ++p) {
                const bool e1 = (msk[q] >> p) & 1u, e2 = (msk[p] >> q) & 1u;
                asym |= e1 != e2;
                mf[q][p] = __uint_as_float(__builtin_amdgcn_readfirstlane(e1 ? 0x3f800000u : 0u));
            }
        status |= asym ? DADMM_STATUS_RECOMPUTE : 0;
    }
    const uint32_t voffY = (uint32_t)((s * P * n + 4 * h) * 4);           // + (p*n + nb*16)*4
    const float dlim = a.variant != 0 ? GNN_DELTA_LIMIT : __builtin_inff();
    __syncthreads();                     // R(0)

    for (int k = 0; k < a.K; ++k) {
        float al[P], ta[P], rh[P], et[P];
#pragma unroll
        for (int p = 0; p < P; ++p) load_hyp_row(a, k, p, al[p], ta[p], rh[p], et[p]);
        float gclip, vclip;
        iter_clips(a.variant, k, gclip, vclip);
        // EVAL: one iterate; before the last iteration the range check drops every store
        const rsrc_t rY = EVAL ? make_rsrc(a.Y, k + 1 == a.K ? state_bytes : 0u)
                               : make_rsrc(a.Y + (size_t)k * B * P * n, state_bytes);
        const uint32_t vY = fresh(voffY);
        // the largest |gradient| bit pattern seen: above +inf's iff some gradient was NaN (one
        // running register instead of a compare per row that the compiler keeps the rows alive for)
        uint32_t gmag = 0;
        float acc = 0.0f;                // EVAL: the lane's sum of (y_{k+1} - label)^2
        (void)acc;
        __syncthreads();                 // stage 0: G_0 is being computed

        // primal update of agent p from its G (unfolded_DLASSO.py:73-93); iterate to LDS and Y[k]
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const float* __restrict__ Gp = Glds + ((p & 1) * BT + j) * GS;
            // the next tile's G and y_k rows are read under the current tile's arithmetic
            f32x4 gpb[2], ykb[2];
            gpb[0] = *(const f32x4*)(Gp + u * T2 * 16 + 4 * h);
            ykb[0] = *(const f32x4*)(Ylds + (p * BT + j) * YS + u * T2 * 16 + 4 * h);
#pragma unroll
            for (int tt = 0; tt < T2; ++tt) {
                const int nb = u * T2 + tt;
                const int n0 = nb * 16 + 4 * h;
                if (tt + 1 < T2) {
                    gpb[(tt + 1) & 1] = *(const f32x4*)(Gp + n0 + 16);
                    ykb[(tt + 1) & 1] = *(const f32x4*)(Ylds + (p * BT + j) * YS + n0 + 16);
                }
                compiler_fence();
                const f32x4 gp = gpb[tt & 1];
                const f32x4 yk = ykb[tt & 1];   // y_k, 4 rows
                f32x4 yn, xl;
                if constexpr (EVAL) xl = *(const f32x4*)(Llds + j * YS + n0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = 4 * tt + r;
                    const float yv = yk[r];
                    const float gr = grad_assemble(gp[r], yv, U[p][e], D[p][e], ta[p], dg[p], rh[p]);
                    gmag = max(gmag, __float_as_uint(gr) & 0x7fffffffu);   // :84 guard (flag only)
                    yn[r] = primal_elem<Clamp::MED3>(yv, gr, al[p], gclip, vclip);
                    if constexpr (EVAL) {
                        const float d = yn[r] - xl[r];
                        acc += d * d;
                    }
                }
                gmag = fresh(gmag);      // folded here, not sunk to the loop's end with every row alive
                *(f32x4*)(Ylds + (p * BT + j) * YS + n0) = yn;
                // Y[k][s][p][n0..n0+3]; rows past n go to an offset the range check drops
                // (the range check sees the lane's offset only: the sample's, which decides; the
                // uniform (agent, tile) part rides in soffset instead of P * T2 hoisted registers)
                bstore4<16>(yn, rY, n0 < n ? vY : 0x80000000u, (uint32_t)((p * n + nb * 16) * 4));
            }
            __syncthreads();             // stages 1..P
        }
        status |= gmag > 0x7f800000u ? DADMM_STATUS_GRAD_NAN : 0;
        if constexpr (EVAL) {
            const float wsum = wave_sum_dpp(acc);
            if (lane == 0) ev->partial[(size_t)k * (gridDim.x * 4) + blockIdx.x * 4 + u] = wsum;
        }

        // delta_{k+1} = 2 L y_{k+1} for the lane's rows (all agents, lane-local), GNN delta clamp,
        // U_{k+1} = clamp(U_k + delta_{k+1} * eta_k) (:95-99). After the last iteration only U_out
        // needs them.
        if (k + 1 < a.K || a.U_out != nullptr) {
#pragma unroll
            for (int tt = 0; tt < T2; ++tt) {
                const int n0 = (u * T2 + tt) * 16 + 4 * h;
                compiler_fence();        // one tile's rows in flight at a time (register budget)
                f32x4 yv[P];
#pragma unroll
                for (int p = 0; p < P; ++p) yv[p] = *(const f32x4*)(Ylds + (p * BT + j) * YS + n0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = 4 * tt + r;
                    float yy[P][1], dd[P][1];
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        // one row at a time: a row's inputs wait for the previous row's last result
                        // (four rows interleaved hold 4 x P (P - 1) / 2 differences: past the budget)
                        float y = yv[p][r];
                        if (e > 0) asm volatile("" : "+v"(y) : "v"(U[P - 1][e - 1]));
                        yy[p][0] = y;
                    }
                    consensus_fma<P>(yy, dd, mf);
#pragma unroll
                    for (int p = 0; p < P; ++p)
                        dual_elem<Clamp::MED3>(dd[p][0], et[p], dlim, vclip, U[p][e], D[p][e]);
                }
            }
        }
        __syncthreads();                 // stage P + 1
    }

    if (a.U_out != nullptr) {
        const rsrc_t rU = make_rsrc(a.U_out, state_bytes);
#pragma unroll
        for (int tt = 0; tt < T2; ++tt) {
            const int n0 = (u * T2 + tt) * 16 + 4 * h;
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

// This file is compiled twice (csrc/Makefile), like dadmm_fused.hip: as it stands for the forward's
// kernels, and with DADMM_ROLES_EVAL=1 for the evaluation forward's alone, so that the forward's
// compile unit is the same with and without the evaluation kernels beside it.
#ifndef DADMM_ROLES_EVAL
#define DADMM_ROLES_EVAL 0
#endif

#if !DADMM_ROLES_EVAL
template <int P, int RES>
__global__ __launch_bounds__(FUSED_WAVES * 64) void fused_roles_kernel(FusedArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[Roles<P, RES>::LDS_FLOATS];
    static_assert(FUSED_WAVES == 8, "one matrix wave and one update wave per SIMD");
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave id, in an SGPR
    if (w < 4)
        roles_matrix<P, RES>(a, lds, w);
    else
        roles_update<P>(a, lds, w - 4);
}

template <int P, int RES>
static hipError_t launch_roles(const FusedArgs& a, hipStream_t stream) {
    const int grid = (a.B + BT - 1) / BT;
    hipLaunchKernelGGL((fused_roles_kernel<P, RES>), dim3(grid), dim3(FUSED_WAVES * 64), 0, stream, a);
    return hipGetLastError();
}

// Instantiated shapes: P = 1..5, n_pad = 256, one shared graph, no recording; nullptr otherwise.
// resident: with one agent's GEMM1 operand held in registers (RES = 1), or every fragment streamed.
fused_fn_ptr find_fused_roles(int P, int nt, int graph, bool resident) {
    if (nt != 4 || graph != GRAPH_SHARED) return nullptr;
    switch (P) {
        case 1: return resident ? &launch_roles<1, 1> : &launch_roles<1, 0>;
        case 2: return resident ? &launch_roles<2, 1> : &launch_roles<2, 0>;
        case 3: return resident ? &launch_roles<3, 1> : &launch_roles<3, 0>;
        case 4: return resident ? &launch_roles<4, 1> : &launch_roles<4, 0>;
        case 5: return resident ? &launch_roles<5, 1> : &launch_roles<5, 0>;
        default: return nullptr;
    }
}

#else   // DADMM_ROLES_EVAL
// The evaluation forward: the resident form's matrix role unchanged, the update
// role with EVAL and its label tile behind the forward's LDS tiles
template <int P>
__global__ __launch_bounds__(FUSED_WAVES * 64) void fused_roles_eval_kernel(EvalArgs e) {
    __shared__ __attribute__((aligned(16))) float lds[Roles<P, 1>::LDS_FLOATS + BT * Roles<P, 1>::YS];
    static_assert(sizeof(lds) <= 160 * 1024, "the label tile beside the forward's tiles");
    static_assert(FUSED_WAVES == 8, "one matrix wave and one update wave per SIMD");
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w < 4)
        roles_matrix<P, 1>(e.f, lds, w);
    else
        roles_update<P, true>(e.f, lds, w - 4, &e);
}

template <int P>
static hipError_t launch_roles_eval(const EvalArgs& e, hipStream_t stream) {
    const int grid = (e.f.B + BT - 1) / BT;
    hipLaunchKernelGGL((fused_roles_eval_kernel<P>), dim3(grid), dim3(FUSED_WAVES * 64), 0, stream, e);
    return hipGetLastError();
}

// The shapes of the resident role-split form; nullptr otherwise.
eval_fn_ptr find_fused_roles_eval(int P, int nt, int graph) {
    if (nt != 4 || graph != GRAPH_SHARED) return nullptr;
    switch (P) {
        case 1: return &launch_roles_eval<1>;
        case 2: return &launch_roles_eval<2>;
        case 3: return &launch_roles_eval<3>;
        case 4: return &launch_roles_eval<4>;
        case 5: return &launch_roles_eval<5>;
        default: return nullptr;
    }
}
#endif

}  // namespace dadmm

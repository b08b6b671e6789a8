// dadmm_device.h — the device-only primitives of the kernel translation units, each stated once:
// vector / resource / address-space types, MFMA and buffer-memory wrappers, the clamps and guards,
// the compiler-opacity helpers, the guard-flag atomics, the XCD swizzle, the wave reductions, the
// reference's per-iteration clip schedule, the element update it feeds and that update's adjoint.
// Everything is __forceinline__: no symbol is emitted.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dadmm_internal.h"

namespace dadmm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef __attribute__((address_space(3))) void lds_void;
// The hyper-parameter table through the scalar cache (s_load): it is read-only for the whole
// launch, so a constant-address-space view lets the uniform per-iteration reads bypass the vector
// memory queue (no vmcnt wait at the top of an iteration)
typedef const __attribute__((address_space(4))) float cfloat;

// v_mfma_f32_16x16x4_f32: exact f32, one fma per product
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// ---- buffer memory: 32-bit per-lane offsets; the hardware range check returns 0 for loads and
// drops stores past `bytes` ----------------------------------------------------------------------
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
// the same for a size_t extent that may pass 4 GB: saturates (the offsets used stay below it)
__device__ __forceinline__ rsrc_t make_rsrc_sat(const void* base, size_t bytes) {
    const uint32_t nb = bytes > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)nb, 0x00020000);
}
// AUX, the cache policy: 16 = sc1 (write-through store / L1-bypassing load), 2 = nt.
// The fused kernel's iterate stream Y (K*B*P*n*4 bytes, 524 MB at the headline shape) is written
// once and never re-read by the kernel; its cache policy decides whether it evicts the operator
// A / A^T that every workgroup re-reads from L2 each iteration: it is stored with sc1.
template <int AUX = 0>
__device__ __forceinline__ f32x4 bload4(rsrc_t r, uint32_t voff, uint32_t soff = 0) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ void bstore4(f32x4 v, rsrc_t r, uint32_t voff, uint32_t soff = 0) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), r, voff, soff, AUX);
}
// s_waitcnt vmcnt(n), n < CAP; any n >= CAP waits for vmcnt(CAP), the caller's own cap (it
// over-waits: safe). For a compile-time n the switch folds once the loops are unrolled; a runtime
// n (the wait counts of dadmm_hyper.hip's DMA ring depend on the wave) keeps the ladder.
template <int CAP>
__device__ __forceinline__ void wait_vm(int n) {
    static_assert(CAP >= 1 && CAP <= 16, "the ladder below has cases 0..15");
#define DADMM_WAIT_VM(i)                                          \
    case i:                                                       \
        if (i < CAP) {                                            \
            asm volatile("s_waitcnt vmcnt(" #i ")" ::: "memory"); \
            break;                                                \
        }                                                         \
        [[fallthrough]];
    switch (n) {
        DADMM_WAIT_VM(0) DADMM_WAIT_VM(1) DADMM_WAIT_VM(2) DADMM_WAIT_VM(3)
        DADMM_WAIT_VM(4) DADMM_WAIT_VM(5) DADMM_WAIT_VM(6) DADMM_WAIT_VM(7)
        DADMM_WAIT_VM(8) DADMM_WAIT_VM(9) DADMM_WAIT_VM(10) DADMM_WAIT_VM(11)
        DADMM_WAIT_VM(12) DADMM_WAIT_VM(13) DADMM_WAIT_VM(14) DADMM_WAIT_VM(15)
        default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CAP) : "memory"); break;
    }
#undef DADMM_WAIT_VM
}

// ---- clamps and guards -------------------------------------------------------------------------
// torch.clamp(x, lo, hi) == min(max(x, lo), hi) for every non-NaN x. A NaN never needs to be
// propagated by the fused kernels: they flag (status bits) every case in which a NaN would reach
// one of the reference's guards, and the caller then re-runs the batch through the guarded path.
__device__ __forceinline__ float tclamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
// tclamp as one v_med3_f32: equal to min(max(x, lo), hi) for every non-NaN x when lo <= hi
// (-0 stays -0: the median of {lo, -0, hi}); NaN cases are flagged like tclamp's
__device__ __forceinline__ float mclamp(float x, float lo, float hi) {
    return __builtin_amdgcn_fmed3f(x, lo, hi);
}
// torch.clamp as the guarded paths need it: NaN propagates, +-inf saturate
__device__ __forceinline__ float clamp_t(float x, float lo, float hi) {
    return x != x ? x : fminf(fmaxf(x, lo), hi);
}
// the clamp passes the gradient (the adjoints' masks)
__device__ __forceinline__ bool inside(float x, float lo, float hi) { return x >= lo && x <= hi; }
__device__ __forceinline__ bool finitef(float x) { return __builtin_isfinite(x); }
__device__ __forceinline__ bool finite4(f32x4 v) {
    return finitef(v[0]) && finitef(v[1]) && finitef(v[2]) && finitef(v[3]);
}

// sign(y) * t exactly as torch's eager ops give it (sign(+-0) = sign(NaN) = 0, so +0 there, else
// +-t), without branches: the sign bit of y moved onto t, then one select. (The nested-ternary
// form compiles to divergent branches, ~11 instructions per element in the middle of the MFMA
// chains.)
__device__ __forceinline__ float sign_times(float y, float t) {
    const float st = __uint_as_float(__float_as_uint(t) ^ (__float_as_uint(y) & 0x80000000u));
    return __builtin_fabsf(y) > 0.0f ? st : 0.0f;
}

// The reference's per-iteration clip schedule, the single statement of it on the device side
// (oracle/dadmm_oracle.c and dadmm_cpu.py keep independent restatements on purpose): gclip bounds
// the primal gradient, vclip the iterate and the dual variable. The fused paths and the guarded
// stepwise path that re-runs a flagged batch must agree on it bit-for-bit.
__device__ __forceinline__ void iter_clips(int variant, int k, float& gclip, float& vclip) {
    if (variant == 0) {
        gclip = fmaxf(1.0f, 30.0f - (float)k);          // unfolded_DLASSO.py:80
        vclip = fmaxf(10.0f, 200.0f - (float)(k * 3));  // unfolded_DLASSO.py:92
    } else {
        gclip = 10.0f;                                   // gnn_dlasso_models_progressive.py:212
        vclip = 100.0f;                                  // :224, :232
    }
}
// GNN variant only: delta = clamp(delta, -20, 20) (gnn_dlasso_models_progressive.py:229)
constexpr float GNN_DELTA_LIMIT = 20.0f;

// ---- the D-ADMM element update -------------------------------------------------------------------
// One iteration's arithmetic on one element of (y, U, delta), the single statement of it on the
// device side for every forward kernel (like iter_clips, restated independently by the oracle and
// dadmm_cpu.py). Each kernel family keeps its clamp: MED3 = mclamp (the on-chip forwards: fused,
// role-split, column-split), MINMAX = tclamp (tiled, stream), NANPROP = clamp_t (the guarded
// stepwise and GNN paths). The guards (NaN / finite checks), the recording of the trajectory and
// the masking of lanes differ by design and stay with the kernels.
enum class Clamp { MED3, MINMAX, NANPROP };
template <Clamp C>
__device__ __forceinline__ float clampf(float x, float lo, float hi) {
    if constexpr (C == Clamp::MED3) return mclamp(x, lo, hi);
    else if constexpr (C == Clamp::MINMAX) return tclamp(x, lo, hi);
    else return clamp_t(x, lo, hi);
}
// grad = (AtAy - Atb) + sign(y)*tau + U*deg + delta*rho, left to right, one rounding per operation
// (unfolded_DLASSO.py:73-77); g = the factored gradient A^T (A y - b)
__device__ __forceinline__ float grad_assemble(float g, float y, float u, float d, float tau, float deg,
                                               float rho) {
    g = g + sign_times(y, tau);
    g = g + u * deg;
    return g + d * rho;
}
template <Clamp C>
__device__ __forceinline__ float grad_clamp(float gr, float gclip) {                 // :80-81
    return clampf<C>(gr, -gclip, gclip);
}
// y_next = clamp(y - alpha * grad, +-vclip), grad already clamped (:89, :92-93)
template <Clamp C>
__device__ __forceinline__ float primal_y(float y, float alpha, float g_clamped, float vclip) {
    return clampf<C>(y - alpha * g_clamped, -vclip, vclip);
}
// the gradient clamp and the primal update in one place (:80-93)
template <Clamp C>
__device__ __forceinline__ float primal_elem(float y, float gr, float alpha, float gclip, float vclip) {
    return primal_y<C>(y, alpha, grad_clamp<C>(gr, gclip), vclip);
}
// GNN variant: delta = clamp(delta, +-dlim) (gnn_dlasso_models_progressive.py:229); the unfolded
// variant passes dlim = +inf (a no-op on finite delta) or skips the call
template <Clamp C>
__device__ __forceinline__ float delta_clamp(float cons, float dlim) {
    return clampf<C>(cons, -dlim, dlim);
}
// U_next = clamp(U + delta * eta, +-vclip) (:98-99)
template <Clamp C>
__device__ __forceinline__ float dual_u(float u, float d, float eta, float vclip) {
    return clampf<C>(u + d * eta, -vclip, vclip);
}
// the dual update from the consensus sum cons = 2 L y (:95-99)
template <Clamp C>
__device__ __forceinline__ void dual_elem(float cons, float eta, float dlim, float vclip, float& U,
                                          float& D) {
    const float d = delta_clamp<C>(cons, dlim);
    U = dual_u<C>(U, d, eta, vclip);
    D = d;
}

// ---- the adjoint of the element update -----------------------------------------------------------
// What torch autograd makes of the lines above (sign() has zero derivative, a clamp passes the
// gradient where lo <= x <= hi), for the any-shape adjoint (dadmm_adjoint.hip) and the GNN step
// backward (dadmm_gnn.hip); the masks re-evaluate the forward's own float ops, so the caller
// passes the forward's clamp. (The fused adjoint, dadmm_backward.hip, keeps its own statement.)
// Dual update (:95-99), from the raw consensus sum cons = 2 L y_{k+1}, the recorded U_k, eta and
// the incoming U_bar: d = the delta the forward used (GNN variant: clamped, and md = that clamp
// passes the gradient, gnn_dlasso_models_progressive.py:229), wb = U_bar through the dual clamp,
// pe = the eta partial, wbe = wb * eta, the dual update's own term of d_bar: the caller adds what
// else reaches delta_{k+1} and applies md.
struct DualAdj {
    float d, wb, pe, wbe;
    bool md;
};
template <Clamp C>
__device__ __forceinline__ DualAdj dual_adj(float cons, float u, float eta, float ubar, bool gnn, float vclip) {
    DualAdj r;
    r.md = !gnn || inside(cons, -GNN_DELTA_LIMIT, GNN_DELTA_LIMIT);
    r.d = gnn ? delta_clamp<C>(cons, GNN_DELTA_LIMIT) : cons;
    r.wb = inside(u + r.d * eta, -vclip, vclip) ? ubar : 0.0f;
    r.pe = r.wb * r.d;
    r.wbe = r.wb * eta;
    return r;
}
// Primal update and gradient clamp (:73-93), from y_k, the pre-clamp gradient gr, g = its clamp as
// the forward took it, the incoming y_bar and delta_k: zb = y_bar through the value clamp, grb =
// the adjoint of gr, and the alpha, tau and rho partials
struct PrimalAdj {
    float zb, grb, pa, pt, pr;
};
__device__ __forceinline__ PrimalAdj primal_adj(float y, float gr, float g, float alpha, float ybar, float dk,
                                                float gclip, float vclip) {
    PrimalAdj r;
    r.zb = inside(y - alpha * g, -vclip, vclip) ? ybar : 0.0f;
    r.pa = -r.zb * g;
    r.grb = inside(gr, -gclip, gclip) ? -alpha * r.zb : 0.0f;
    r.pt = r.grb * sign_times(y, 1.0f);
    r.pr = r.grb * dk;
    return r;
}

// ---- compiler opacity --------------------------------------------------------------------------
// A per-iteration opaque copy of a loop-invariant offset: keeps `base + constant` inside the loop
// so instruction selection folds the constant into the load's immediate offset instead of LICM
// hoisting one register per constant out of the loop.
__device__ __forceinline__ uint32_t fresh(uint32_t x) {
    asm volatile("" : "=v"(x) : "0"(x));
    return x;
}
// The same for a wave-uniform value (the adjoint: keeps the shared graph's neighbour tests inside
// the loop, s_bitcmp + branch, instead of P*P hoisted 64-bit condition registers)
__device__ __forceinline__ uint32_t fresh_s(uint32_t x) {
    asm volatile("" : "=s"(x) : "0"(x));
    return x;
}
// Compiler-only memory barrier: bounds how far the scheduler hoists operand loads (register budget).
__device__ __forceinline__ void compiler_fence() { asm volatile("" ::: "memory"); }

// ---- guard-flag words (the stepwise and GNN per-iteration paths) -------------------------------
__device__ __forceinline__ int flag_ld(const int32_t* f) {
    return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one atomic per wave (called with every lane of the wave active)
__device__ __forceinline__ void flag_or(int32_t* f, bool v) {
    if (__ballot(v) != 0 && (threadIdx.x & 63) == 0)
        __hip_atomic_fetch_or(f, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the hyper-parameter table of the on-chip forwards (fused, role-split, column-split) --------
// seq_hyp(k) row p: (alpha, tau, rho, eta), kernel-uniform scalars through the scalar cache
// hyp [K][H][4]: the row of agent p (H = 1: one row for all agents), and where seq_hyp(k)'s starts
__device__ __forceinline__ int hyp_agent_row(int H, int p) { return H == 1 ? 0 : p; }
__device__ __forceinline__ size_t hyp_index(int k, int H, int p) {
    return ((size_t)k * H + hyp_agent_row(H, p)) * 4;
}
__device__ __forceinline__ void load_hyp_row(const FusedArgs& a, int k, int p, float& al, float& ta,
                                             float& rh, float& et) {
    const cfloat* hp = (const cfloat*)a.hyp + hyp_index(k, a.hyp_rows, p);
    al = hp[0]; ta = hp[1]; rh = hp[2]; et = hp[3];
}

// XCD-aware block order: the dispatcher deals blocks round-robin over the 8 XCDs, each with its
// own L2; block bid of a grid of G gets work item xcd_swizzle(bid, G) so that consecutive items
// land on blocks of one XCD. The tiled forward: the P workgroups of one sample tile (the neighbour
// tiles a workgroup reads for delta are its siblings' own tiles, hot in that L2); the
// hypernetwork GEMMs: the column tiles of one row tile, which read the same input rows; wgrad: the
// k-tiles of one n-tile, which read the same dZ columns.
__device__ __forceinline__ int xcd_swizzle(int bid, int G) {
    constexpr int NX = 8;
    const int xcd = bid % NX, i = bid / NX, q = G / NX, r = G % NX;
    return xcd < r ? xcd * (q + 1) + i : r * (q + 1) + (xcd - r) * q + i;
}

// ---- wave reductions ---------------------------------------------------------------------------
// Sum of v over the wave's 64 lanes, in a fixed order, on DPP moves (quad perms, half-row and row
// mirrors: every lane ends with its 16-lane row's sum) and four readlanes: no LDS round trips (a
// __shfl_xor butterfly is six ds_bpermute round trips). Deterministic; the association differs
// from the butterfly's (f32 rounding). Uniform result.
template <int CTRL>
__device__ __forceinline__ float dpp_mov_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = v + dpp_mov_f32<0xB1>(v);    // quad_perm [1,0,3,2]
    v = v + dpp_mov_f32<0x4E>(v);    // quad_perm [2,3,0,1]: every lane holds its quad's sum
    v = v + dpp_mov_f32<0x141>(v);   // row_half_mirror: its 8-lane group's
    v = v + dpp_mov_f32<0x140>(v);   // row_mirror: its 16-lane row's
    const auto lane_v = [&](int l) {
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
    };
    return (lane_v(0) + lane_v(16)) + (lane_v(32) + lane_v(48));
}
// Sum of v over each 16-lane row, in every lane of the row (the first four steps above).
__device__ __forceinline__ float row16_sum_dpp(float v) {
    v = v + dpp_mov_f32<0xB1>(v);
    v = v + dpp_mov_f32<0x4E>(v);
    v = v + dpp_mov_f32<0x141>(v);
    return v + dpp_mov_f32<0x140>(v);
}
// The LayerNorm row sums (rownorm forward / backward and the hypernetwork tail kernel's copies of
// them, which must reduce identically): wave_sum_dpp.
__device__ __forceinline__ float ln_row_sum(float v) {
    return wave_sum_dpp(v);
}

}  // namespace dadmm

// dadmm_hyper_net.cpp — host orchestration of one training-mode hypernetwork call of
// DLASSO_GNNHyp3_Progressive (gnn_dlasso_models_progressive.py:165-196 with :52-72 in train mode)
// and of its backward, as ONE C-ABI call each: the 13 forward launches and ~35 backward launches
// of an iteration are issued from here instead of one Python / ctypes round trip each
// (dadmm_hip.hyper_ops, VERDICT r2 weak #6: the train step was host-bound on ~2,700 launches).
//
// Forward, per iteration (B samples of P nodes, rows = B P):
//   x_i = Dropout(BN_batch(leaky(A_hat (x_{i-1} W_i^T) + b_i)))   5 x dadmm_hyper_gcn_train
//   e   = LayerNorm(x_5)                                          dadmm_hyper_rownorm
//   d_j = LReLU(LN(Dropout(d_{j-1} D_j^T + c_j)))                 3 x dadmm_hyper_linear_ln_train
//   z   = d_3 fc^T + f; hyp = head(z)                             dadmm_hyper_head_train
// Backward: the same stages reversed; the parameter gradients are accumulated IN PLACE into the
// caller's buffers (dadmm_hyper_wgrad / dadmm_hyper_colsum: G += ...), the input gradients run as
// dadmm_hyper_linear with the caller's transposed weights. Everything is enqueued on `stream`;
// nothing here allocates or synchronises.

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dadmm.h"
#include "dadmm_internal.h"

namespace {

constexpr float LEAKY = 0.01f;   // F.leaky_relu's default slope (reference :52-68)

inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

struct Work {   // carve of the caller's work buffer (dadmm_hyper_train_work_bytes)
    float* dz;      // [B][4H]
    float* dx[2];   // [rows][max width] ping-pong
    float* dv;      // [B][max decoder width]
    float* part;    // max(3 B N, rownorm partials)
    float* wscr;    // dadmm_hyper_wgrad split partials
    float* lscr;    // dadmm_hyper_linear_ln_train split-K partials
};

int max_width(const dadmm_hyper_net* net) {
    int w = 2 * net->n;
    for (int i = 0; i < 5; ++i) w = w > net->width[i] ? w : net->width[i];
    return w;
}

size_t layout(const dadmm_hyper_net* net, int B, Work* w, char* base) {
    const int P = net->P, rows = B * P;
    const int mw = max_width(net);
    int md = net->dec_width[0];
    for (int j = 1; j < 3; ++j) md = md > net->dec_width[j] ? md : net->dec_width[j];
    size_t part = (size_t)3 * B * (mw > md ? mw : md);
    const size_t rn1 = dadmm_hyper_rownorm_bwd_part_bytes(rows, net->width[4]) / 4;
    part = part > rn1 ? part : rn1;
    for (int j = 0; j < 3; ++j) {
        const size_t r = dadmm_hyper_rownorm_bwd_part_bytes(B, net->dec_width[j]) / 4;
        part = part > r ? part : r;
    }
    // scratch: the largest split partials of any weight gradient; of any decoder linear
    size_t scr = 0, lscr = 0;
    int kin = 2 * net->n;
    for (int i = 0; i < 5; ++i) {
        const size_t s = dadmm_hyper_wgrad_scratch_bytes(rows, net->width[i], kin);
        scr = scr > s ? scr : s;
        kin = net->width[i];
    }
    int din = P * net->width[4];
    for (int j = 0; j < 3; ++j) {
        size_t s = dadmm_hyper_wgrad_scratch_bytes(B, net->dec_width[j], din);
        scr = scr > s ? scr : s;
        s = dadmm_hyper_linear_ln_scratch_bytes(B, din, net->dec_width[j]);
        lscr = lscr > s ? lscr : s;
        din = net->dec_width[j];
    }
    {
        const size_t s = dadmm_hyper_wgrad_scratch_bytes(B, 4 * net->H, din);
        scr = scr > s ? scr : s;
    }
    const size_t sizes[7] = {up16(scr + 16), up16(4 * (size_t)B * 4 * net->H), up16(4 * (size_t)rows * mw),
                             up16(4 * (size_t)rows * mw), up16(4 * (size_t)B * md), up16(4 * part), up16(lscr + 16)};
    size_t off = 0;
    float** slots[7] = {&w->wscr, &w->dz, &w->dx[0], &w->dx[1], &w->dv, &w->part, &w->lscr};
    for (int i = 0; i < 7; ++i) {
        if (base) *slots[i] = (float*)(base + off);
        off += sizes[i];
    }
    return off;
}

int check_net(const dadmm_hyper_net* net, int B) {
    if (!net || B < 0 || net->P < 2 || net->P > 64 || net->n < 1 || net->ld < net->n || net->H < 1)
        return DADMM_EINVAL;
    for (int i = 0; i < 5; ++i)
        if (net->width[i] < 4 || (net->width[i] & 3) || !net->conv_w[i] || !net->conv_b[i] || !net->bn_w[i] ||
            !net->bn_b[i])
            return DADMM_EINVAL;
    for (int j = 0; j < 3; ++j)
        if (net->dec_width[j] < 4 || (net->dec_width[j] & 3) || !net->dec_w[j] || !net->dec_b[j] ||
            !net->ln_w[j] || !net->ln_b[j])
            return DADMM_EINVAL;
    if (net->bn_eval)
        for (int i = 0; i < 5; ++i)
            if (!net->bn_rm[i] || !net->bn_rv[i]) return DADMM_EINVAL;
    if (!net->norm_w || !net->norm_b || !net->fc_w || !net->fc_b) return DADMM_EINVAL;
    return DADMM_OK;
}

// Deferred parameter gradients (dadmm_hyper_train_backward_deferred / dadmm_hyper_train_wgrad):
// the per-iteration gradient operands in one block of `dsave`, floats, 4-aligned slices
struct DSave {
    float* dz;          // [B][4H] head gradient (fc's dZ)
    float* dv[3];       // [B][dec_width_j] decoder blocks' dZ
    float* pdec[3];     // decoder LayerNorm partials (dadmm_hyper_rownorm_bwd_part_bytes)
    float* pnorm;       // encoder LayerNorm partials
    float* dZ[5];       // [B P][width_i] GCN layers' dZ
    float* pgcn[5];     // [3][B][width_i] GCN BatchNorm / bias partials
};
inline size_t up4(size_t f) { return (f + 3) & ~(size_t)3; }
size_t dsave_layout(const dadmm_hyper_net* net, int B, DSave* d, float* base) {
    const int P = net->P, rows = B * P;
    size_t off = 0;
    auto take = [&](float** slot, size_t floats) {
        if (base) *slot = base + off;
        off += up4(floats);
    };
    take(&d->dz, (size_t)B * 4 * net->H);
    for (int j = 0; j < 3; ++j) {
        take(&d->dv[j], (size_t)B * net->dec_width[j]);
        take(&d->pdec[j], dadmm_hyper_rownorm_bwd_part_bytes(B, net->dec_width[j]) / 4);
    }
    take(&d->pnorm, dadmm_hyper_rownorm_bwd_part_bytes(rows, net->width[4]) / 4);
    for (int i = 0; i < 5; ++i) {
        take(&d->dZ[i], (size_t)rows * net->width[i]);
        take(&d->pgcn[i], (size_t)3 * B * net->width[i]);
    }
    return off;
}

// Whether a GCN layer's block backward runs in the epilogue of the input-gradient GEMM above it.
// It pays while that GEMM's grid leaves the chip idle (~2 workgroups per CU: B = 256, the step is
// launch-bound, 9.31 -> 9.10 ms); on full grids the longer epilogue and its LDS cost more than the
// launch saved (B = 4096: 49.6 -> 50.5 ms, profiles/r05/gcn_bwd_fuse_r05m.txt).
// DADMM_GCNBWD_FUSE=0 / =1 in the environment: never / always (A/B timing, the bit-identity test).
bool gcn_bwd_fused(int B, int P, int Kin) {
    const char* e = getenv("DADMM_GCNBWD_FUSE");
    if (e != nullptr && (e[0] == '0' || e[0] == '1')) return e[0] == '1';
    const long st = P <= 32 ? 32 / P : 1;
    const long tiles = (B + st - 1) / st * ((Kin + 63) / 64);
    return tiles < 480;
}

// The decoder tail (blocks 2, 3, fc, head) as one launch each way (dadmm_hyper_tail.hip), where
// its results are the separate launches' bits: the separate path would not split K of blocks 2 and 3
// (dadmm_hyper_linear_ln_train's split-K), and the tiles fit LDS. By default only from B = 2048:
// at B = 256 its 16 workgroups walk the stages' memory round trips one after another (27 + 33.5 us
// per iteration, as long as the ten launches it replaces: 8.62-8.69 vs 8.48-8.54 ms per train step),
// at B = 4096 it is 0.1-0.2 ms ahead (profiles/r05/decoder_tail_r05ad.txt).
// DADMM_HYPER_TAIL=0 / =1: never / always (A/B timing, the bit-identity test).
bool tail_usable(const dadmm_hyper_net* net, int B) {
    const char* e = getenv("DADMM_HYPER_TAIL");
    if (e != nullptr && e[0] == '0') return false;
    if (!(e != nullptr && e[0] == '1') && B < 2048) return false;
    for (int j = 0; j < 3; ++j)
        if (net->dec_width[j] > 2048) return false;
    if (dadmm::hyper_linear_splits(B, net->dec_width[0], net->dec_width[1]) != 1 ||
        dadmm::hyper_linear_splits(B, net->dec_width[1], net->dec_width[2]) != 1)
        return false;
    dadmm::TailArgs t{};
    t.H = net->H;
    for (int j = 0; j < 3; ++j) t.D[j] = net->dec_width[j];
    return dadmm::tail_lds_bytes(t, true) <= 160 * 1024;
}

dadmm::TailArgs tail_args(const dadmm_hyper_net* net, int B, uint64_t seed) {
    dadmm::TailArgs t{};
    t.B = B;
    t.H = net->H;
    for (int j = 0; j < 3; ++j) t.D[j] = net->dec_width[j];
    t.W[0] = net->dec_w[1];
    t.W[1] = net->dec_w[2];
    t.W[2] = net->fc_w;
    t.bias[0] = net->dec_b[1];
    t.bias[1] = net->dec_b[2];
    t.bias[2] = net->fc_b;
    for (int q = 0; q < 2; ++q) {
        t.lnw[q] = net->ln_w[1 + q];
        t.lnb[q] = net->ln_b[1 + q];
        t.eps[q] = net->ln_eps[1 + q];
        t.slope[q] = net->dec_slope[1 + q];
        t.drop[q] = net->dec_drop[1 + q];
    }
    t.seed = seed;
    t.site0 = 5;   // the dropout sites of decoder blocks j are 4 + j
    for (int c = 0; c < 4; ++c) t.maxv[c] = net->maxv[c];
    return t;
}

#define TRY(call)                       \
    do {                                \
        const int rc_ = (call);         \
        if (rc_ != DADMM_OK) return rc_; \
    } while (0)

}  // namespace

extern "C" {

size_t dadmm_hyper_train_work_bytes(const dadmm_hyper_net* net, int32_t B) {
    if (check_net(net, B) != DADMM_OK) return 0;
    Work w;
    return layout(net, B, &w, nullptr);
}

int dadmm_hyper_train_atb_mix(const dadmm_hyper_net* net, int32_t B, const float* Atb, const float* ahat,
                              int32_t ahat_per_sample, float* out, void* stream) {
    if (check_net(net, B) != DADMM_OK || !Atb || !ahat || !out) return DADMM_EINVAL;
    if (net->n & 15) return DADMM_EUNSUPPORTED;
    const int n = net->n, N = net->width[0];
    // raw GCN epilogue: A_hat (Atb W1[:, n:2n]^T), no bias / activation / normalisation
    return dadmm_hyper_gcn_ex(B, net->P, n, N, Atb, net->ld, net->conv_w[0] + n, 2 * n, nullptr, 0, nullptr, ahat,
                              ahat_per_sample, nullptr, nullptr, nullptr, nullptr, 0.0f, 0.0f, 1, out, N, stream);
}

int dadmm_hyper_train_forward(const dadmm_hyper_net* net, int32_t B, const float* AtAy, const float* Atb,
                              const float* ahat, int32_t ahat_per_sample, uint64_t seed,
                              const dadmm_hyper_saved* sv, void* work, void* stream) {
    return dadmm_hyper_train_forward_ex(net, B, AtAy, Atb, nullptr, ahat, ahat_per_sample, seed, sv, work, stream);
}

int dadmm_hyper_train_forward_ex(const dadmm_hyper_net* net, int32_t B, const float* AtAy, const float* Atb,
                                 const float* atb_mix, const float* ahat, int32_t ahat_per_sample, uint64_t seed,
                                 const dadmm_hyper_saved* sv, void* work, void* stream) {
    if (check_net(net, B) != DADMM_OK || !sv || !work) return DADMM_EINVAL;
    if (B == 0) return DADMM_OK;
    Work w;
    layout(net, B, &w, (char*)work);
    const int P = net->P, n = net->n, rows = B * P;
    // layer 1 reads cat(AtAy, Atb) in place (two segments; the kernels need 16-column segments)
    const float* x1 = AtAy;
    const float* x2 = Atb;
    int ld1 = net->ld, ld2 = net->ld, K1 = n, K = 2 * n;
    if (n & 15) return DADMM_EUNSUPPORTED;   // the caller concatenates in that case (dadmm_hip)
    for (int i = 0; i < 5; ++i) {
        const int N = net->width[i];
        // layer 1 with the Atb half precomputed (atb_mix): its GEMM runs over AtAy alone, the first
        // n columns of W1, and the mix of the Atb half is added before the bias
        const bool half = i == 0 && atb_mix != nullptr;
        TRY(dadmm::gcn_train_impl(B, P, half ? n : K, N, x1, ld1, half ? n : K1, half ? nullptr : x2, half ? 0 : ld2,
                                  net->conv_w[i], K, half ? atb_mix : nullptr, half ? N : 0, net->conv_b[i], ahat,
                                  ahat_per_sample, net->bn_w[i], net->bn_b[i], net->bn_eps[i], LEAKY,
                                  i < 4 ? net->drop_enc : 0.0f, seed, i, sv->y[i], N, sv->m[i], sv->mean[i],
                                  sv->var[i], net->bn_eval ? net->bn_rm[i] : nullptr,
                                  net->bn_eval ? net->bn_rv[i] : nullptr, stream));
        x1 = sv->y[i];
        ld1 = N;
        K1 = N;
        K = N;
        x2 = nullptr;
        ld2 = 0;
    }
    // self.norm (:69) over 4h per node -> the flattened decoder input [B][P 4h]
    const int C = net->width[4];
    TRY(dadmm_hyper_rownorm(rows, C, sv->y[4], net->norm_w, net->norm_b, net->norm_eps, 0, 0.0f, sv->e, stream));
    const float* x = sv->e;
    int width = P * C;
    const bool tail = tail_usable(net, B);
    for (int j = 0; j < (tail ? 1 : 3); ++j) {
        const int N = net->dec_width[j];
        TRY(dadmm_hyper_linear_ln_train(B, width, N, x, width, net->dec_w[j], net->dec_b[j], net->ln_w[j],
                                        net->ln_b[j], net->ln_eps[j], 1, net->dec_slope[j], net->dec_drop[j],
                                        seed, 4 + j, sv->dec_y[j], sv->dec_xd[j], w.lscr, stream));
        x = sv->dec_y[j];
        width = N;
    }
    if (tail) {   // blocks 2, 3, fc and the head in one launch
        dadmm::TailArgs t = tail_args(net, B, seed);
        t.x0 = sv->dec_y[0];
        t.xd[0] = sv->dec_xd[1];
        t.xd[1] = sv->dec_xd[2];
        t.y[0] = sv->dec_y[1];
        t.y[1] = sv->dec_y[2];
        t.z = sv->z;
        t.hyp = sv->hyp;
        return dadmm::launch_tail(t, false, (hipStream_t)stream) == hipSuccess ? DADMM_OK : DADMM_EHIP;
    }
    // fc and the head in one launch (the logits saved for the backward)
    TRY(dadmm_hyper_head_train(B, width, net->H, x, width, net->fc_w, net->fc_b, net->maxv[0], net->maxv[1],
                               net->maxv[2], net->maxv[3], sv->z, sv->hyp, stream));
    return DADMM_OK;
}

static int train_backward(const dadmm_hyper_net* net, int32_t B, const float* AtAy, const float* Atb,
                          const float* ahat, int32_t ahat_per_sample, uint64_t seed, const dadmm_hyper_saved* sv,
                          const float* dhyp, const dadmm_hyper_grads* g, float* dAtAy, void* work, float* dsave,
                          bool acc_dA, void* stream, bool dz_ready = false) {
    if (check_net(net, B) != DADMM_OK || !sv || (!dhyp && !dz_ready) || !g || !dAtAy || !work) return DADMM_EINVAL;
    if (dz_ready && !dsave) return DADMM_EINVAL;
    if (B == 0) return DADMM_OK;
    Work w;
    layout(net, B, &w, (char*)work);
    // dsave: the gradient operands go to the iteration's block and the parameter-gradient GEMMs /
    // sums are left to dadmm_hyper_train_wgrad (one batched launch per parameter for all iterations)
    DSave d;
    const bool defer = dsave != nullptr;
    if (defer) dsave_layout(net, B, &d, dsave);
    const int P = net->P, n = net->n, rows = B * P, H4 = 4 * net->H;
    if (n & 15) return DADMM_EUNSUPPORTED;
    float* dzh = defer ? d.dz : w.dz;
    // head (sigmoid, clamps, maxima) -> d logits
    if (!dz_ready)
        TRY(dadmm_hyper_head_act(1, B, net->H, sv->z, dhyp, net->maxv[0], net->maxv[1], net->maxv[2],
                                 net->maxv[3], dzh, stream));
    // fc: dW, db; dx = dz fc
    const int hid = net->dec_width[2];
    if (!defer)
        TRY(dadmm_hyper_wgrad(B, H4, hid, dzh, H4, sv->dec_y[2], hid, hid, nullptr, 0, g->fc_w, g->fc_b, 1, w.wscr,
                              stream));
    float* dx = w.dx[0];
    // deferred: fc's input gradient and decoder blocks 3 and 2 in one launch (dadmm_hyper_tail.hip),
    // their dZ and LayerNorm partials into the iteration's dsave block
    const bool tail = defer && tail_usable(net, B);
    if (tail) {
        dadmm::TailArgs t = tail_args(net, B, seed);
        t.xd[0] = sv->dec_xd[1];
        t.xd[1] = sv->dec_xd[2];
        t.dz = dzh;
        t.Wt[0] = g->dec_wt[1];
        t.Wt[1] = g->dec_wt[2];
        t.Wt[2] = g->fc_wt;
        t.dv[0] = d.dv[1];
        t.dv[1] = d.dv[2];
        t.part[0] = d.pdec[1];
        t.part[1] = d.pdec[2];
        t.dx0 = dx;
        if (dadmm::launch_tail(t, true, (hipStream_t)stream) != hipSuccess) return DADMM_EHIP;
    } else {
        TRY(dadmm_hyper_linear(B, H4, hid, dzh, H4, H4, nullptr, 0, g->fc_wt, nullptr, dx, hid, stream));
    }
    // decoder blocks, last to first
    for (int j = tail ? 0 : 2; j >= 0; --j) {
        const int N = net->dec_width[j];
        const int Kin = j > 0 ? net->dec_width[j - 1] : P * net->width[4];
        const float* xin = j > 0 ? sv->dec_y[j - 1] : sv->e;
        float* dv = defer ? d.dv[j] : w.dv;
        float* part = defer ? d.pdec[j] : w.part;
        TRY(dadmm_hyper_rownorm_bwd(B, N, dx, sv->dec_xd[j], net->ln_w[j], net->ln_b[j], net->ln_eps[j], 1,
                                    net->dec_slope[j], net->dec_drop[j], seed, 4 + j, dv, part, stream));
        if (!defer) {
            const int nblk = (int)(dadmm_hyper_rownorm_bwd_part_bytes(B, N) / (4 * 2 * (size_t)N));
            TRY(dadmm_hyper_colsum(part, 1, nblk, 2 * N, g->ln_wb[j], 1, stream));
            TRY(dadmm_hyper_wgrad(B, N, Kin, dv, N, xin, Kin, Kin, nullptr, 0, g->dec_w[j], g->dec_b[j], 1, w.wscr,
                                  stream));
        }
        float* nx = dx == w.dx[0] ? w.dx[1] : w.dx[0];
        TRY(dadmm_hyper_linear(B, N, Kin, dv, N, N, nullptr, 0, g->dec_wt[j], nullptr, nx, Kin, stream));
        dx = nx;
    }
    // self.norm backward (no dropout, no activation): dx [B][P 4h] = [rows][4h]
    const int C = net->width[4];
    {
        float* nx = dx == w.dx[0] ? w.dx[1] : w.dx[0];
        float* part = defer ? d.pnorm : w.part;
        TRY(dadmm_hyper_rownorm_bwd(rows, C, dx, sv->y[4], net->norm_w, net->norm_b, net->norm_eps, 0, 0.0f, 0.0f,
                                    seed, 99, nx, part, stream));
        if (!defer) {
            const int nblk = (int)(dadmm_hyper_rownorm_bwd_part_bytes(rows, C) / (4 * 2 * (size_t)C));
            TRY(dadmm_hyper_colsum(part, 1, nblk, 2 * C, g->norm_wb, 1, stream));
        }
        dx = nx;
    }
    // GCN layers, last to first: dZ (gcn backward), [dgamma, dbeta, dbias], dW, dX. Layer 5's
    // gcn backward is its own launch (its dy comes from the LayerNorm backward); layers 4 .. 1 run
    // theirs in the epilogue of the input-gradient GEMM of the layer above
    // (hyper_linear_gcn_bwd: no dy round trip, one launch instead of two)
    float* dZ = nullptr;   // this layer's dZ once formed
    for (int i = 4; i >= 0; --i) {
        const int N = net->width[i];
        float* part = defer ? d.pgcn[i] : w.part;
        if (dZ == nullptr) {
            dZ = defer ? d.dZ[i] : (dx == w.dx[0] ? w.dx[1] : w.dx[0]);
            TRY(dadmm_hyper_gcn_train_bwd(B, P, N, dx, sv->m[i], sv->mean[i], sv->var[i], net->bn_w[i],
                                          net->bn_eps[i], ahat, ahat_per_sample, LEAKY,
                                          i < 4 ? net->drop_enc : 0.0f, seed, i, dZ, part, net->bn_eval, stream));
        }
        if (!defer) TRY(dadmm_hyper_colsum(part, 3, B, N, g->bn_wbc[i], 1, stream));
        if (i > 0) {
            const int Kin = net->width[i - 1];
            if (!defer)
                TRY(dadmm_hyper_wgrad(rows, N, Kin, dZ, N, sv->y[i - 1], Kin, Kin, nullptr, 0, g->conv_w[i],
                                      nullptr, 1, w.wscr, stream));
            if (gcn_bwd_fused(B, P, Kin)) {
                // layer i - 1's dZ straight from this layer's dZ (not the buffer holding it)
                float* nz = defer ? d.dZ[i - 1] : (dZ == w.dx[0] ? w.dx[1] : w.dx[0]);
                TRY(dadmm::hyper_linear_gcn_bwd(B, P, N, Kin, dZ, N, g->conv_wt[i], sv->m[i - 1], sv->mean[i - 1],
                                                sv->var[i - 1], net->bn_w[i - 1], net->bn_eps[i - 1], ahat,
                                                ahat_per_sample, LEAKY, net->drop_enc, seed, i - 1, nz,
                                                defer ? d.pgcn[i - 1] : w.part, net->bn_eval, stream));
                dZ = nz;
            } else {
                // dX into the buffer dx held (gcn backward consumed it)
                TRY(dadmm::hyper_linear_gcn_dx(P, rows, N, Kin, dZ, N, g->conv_wt[i], nullptr, 0, dx, Kin, stream));
                dZ = nullptr;
            }
        } else {
            // layer 1's input cat(AtAy, Atb); only d AtAy (its first n columns) flows back
            if (!defer)
                TRY(dadmm_hyper_wgrad(rows, N, 2 * n, dZ, N, AtAy, net->ld, n, Atb, net->ld, g->conv_w[0], nullptr,
                                      1, w.wscr, stream));
            // (acc_dA: dAtAy += ..., in the linear's epilogue instead of a separate add)
            TRY(dadmm::hyper_linear_gcn_dx(P, rows, N, n, dZ, N, g->conv_wt[0], acc_dA ? dAtAy : nullptr, net->ld,
                                           dAtAy, net->ld, stream));
        }
    }
    return DADMM_OK;
}

int dadmm_hyper_train_backward(const dadmm_hyper_net* net, int32_t B, const float* AtAy, const float* Atb,
                               const float* ahat, int32_t ahat_per_sample, uint64_t seed,
                               const dadmm_hyper_saved* sv, const float* dhyp, const dadmm_hyper_grads* g,
                               float* dAtAy, void* work, void* stream) {
    return train_backward(net, B, AtAy, Atb, ahat, ahat_per_sample, seed, sv, dhyp, g, dAtAy, work, nullptr,
                          false, stream);
}

size_t dadmm_hyper_train_dsave_floats(const dadmm_hyper_net* net, int32_t B) {
    if (check_net(net, B) != DADMM_OK) return 0;
    DSave d;
    return dsave_layout(net, B, &d, nullptr);
}

int dadmm_hyper_train_backward_deferred(const dadmm_hyper_net* net, int32_t B, const float* AtAy, const float* Atb,
                                        const float* ahat, int32_t ahat_per_sample, uint64_t seed,
                                        const dadmm_hyper_saved* sv, const float* dhyp, const dadmm_hyper_grads* g,
                                        float* dAtAy, void* work, float* dsave, int32_t accumulate,
                                        void* stream) {
    if (!dsave || ((uintptr_t)dsave & 15)) return DADMM_EINVAL;
    return train_backward(net, B, AtAy, Atb, ahat, ahat_per_sample, seed, sv, dhyp, g, dAtAy, work, dsave,
                          (accumulate & 1) != 0, stream, (accumulate & 2) != 0);
}

// the (R, N, K) of every batched weight gradient of one deferred pass, in launch order
extern "C++" template <class F>
static int for_each_wgrad(const dadmm_hyper_net* net, int32_t B, F&& f) {
    const int P = net->P, n = net->n, rows = B * P, H4 = 4 * net->H;
    TRY(f(B, H4, net->dec_width[2]));
    for (int j = 2; j >= 0; --j) TRY(f(B, net->dec_width[j], j > 0 ? net->dec_width[j - 1] : P * net->width[4]));
    for (int i = 4; i >= 0; --i) TRY(f(rows, net->width[i], i > 0 ? net->width[i - 1] : 2 * n));
    return DADMM_OK;
}

size_t dadmm_hyper_train_wgrad_scratch_bytes(const dadmm_hyper_net* net, int32_t B, int32_t iters) {
    if (!net || B < 1 || iters < 1) return 0;
    size_t best = 0;
    for_each_wgrad(net, B, [&](int R, int N, int K) -> int {
        const int s = dadmm::wgrad_splits(R * iters, N, K);
        const size_t b = s > 1 ? 4 * (size_t)s * N * (K + 1) : 0;
        best = b > best ? b : best;
        return DADMM_OK;
    });
    // the colsums' per-iteration block sums [G][iters][C] (G <= 3: BatchNorm dgamma / dbeta / dbias)
    int cmax = 1;
    for (int i = 0; i < 5; ++i) cmax = net->width[i] > cmax ? net->width[i] : cmax;
    for (int j = 0; j < 3; ++j) cmax = net->dec_width[j] > cmax ? net->dec_width[j] : cmax;
    const size_t cs = 4 * (size_t)3 * iters * cmax;
    best = cs > best ? cs : best;
    return best;
}

int dadmm_hyper_train_wgrad(const dadmm_hyper_net* net, int32_t B, int32_t iters, const float* AtAy,
                            int64_t atay_stride, const float* Atb, const dadmm_hyper_saved* sv0, int64_t sv_stride,
                            const float* dsave, int64_t dsave_stride, const dadmm_hyper_grads* g, void* scratch,
                            void* stream) {
    if (check_net(net, B) != DADMM_OK || iters < 0 || !AtAy || !Atb || !sv0 || !dsave || !g) return DADMM_EINVAL;
    // the iteration blocks are read at k * stride: a stride shorter than one block (or negative)
    // would make the batched kernels read past (or before) the caller's buffers
    if (atay_stride < 0 || sv_stride < 0 || dsave_stride < 0) return DADMM_EINVAL;
    if (iters > 1 && B > 0) {
        if (atay_stride < (int64_t)B * net->P * net->ld || sv_stride == 0 ||
            (size_t)dsave_stride < dadmm_hyper_train_dsave_floats(net, B))
            return DADMM_EINVAL;
    }
    if (B == 0 || iters == 0) return DADMM_OK;
    if (net->n & 15) return DADMM_EUNSUPPORTED;
    if (scratch && ((uintptr_t)scratch & 15)) return DADMM_EINVAL;
    DSave d;
    dsave_layout(net, B, &d, const_cast<float*>(dsave));
    const int P = net->P, n = net->n, rows = B * P, H4 = 4 * net->H;
    const hipStream_t st = (hipStream_t)stream;
    // one batched weight gradient: nb = iters blocks; the rows split over workgroups when a scratch
    // (dadmm_hyper_train_wgrad_scratch_bytes) is given, partials added in split order
    auto wg = [&](int R, int N, int K, const float* dz, int ldz, const float* x1, int ld1, int K1, size_t s1,
                  const float* x2, int ld2, size_t s2, float* gw, float* gb) -> int {
        const int S = scratch ? dadmm::wgrad_splits(R * iters, N, K) : 1;
        float* part = S > 1 ? (float*)scratch : nullptr;
        dadmm::WgradArgs a{dz, x1, K1 < K ? x2 : x1, gw, gb, part, S > 1 ? part + (size_t)S * N * K : nullptr,
                           R, N, K, K1, ldz, ld1, K1 < K ? ld2 : ld1, S, 1};
        a.nb = iters;
        a.zs = (size_t)dsave_stride;
        a.s1 = s1;
        a.s2 = K1 < K ? s2 : s1;
        return dadmm::launch_wgrad(a, st) == hipSuccess ? DADMM_OK : DADMM_EHIP;
    };
    auto cs = [&](const float* part, int G, int R, int C, float* out) -> int {
        return dadmm::launch_colsum(part, G, R, C, out, 1, st, iters, (size_t)dsave_stride, (float*)scratch) == hipSuccess
                   ? DADMM_OK : DADMM_EHIP;
    };
    const size_t ss = (size_t)sv_stride;
    const int hid = net->dec_width[2];
    TRY(wg(B, H4, hid, d.dz, H4, sv0->dec_y[2], hid, hid, ss, nullptr, 0, 0, g->fc_w, g->fc_b));
    for (int j = 2; j >= 0; --j) {
        const int N = net->dec_width[j];
        const int Kin = j > 0 ? net->dec_width[j - 1] : P * net->width[4];
        const float* xin = j > 0 ? sv0->dec_y[j - 1] : sv0->e;
        const int nblk = (int)(dadmm_hyper_rownorm_bwd_part_bytes(B, N) / (4 * 2 * (size_t)N));
        TRY(cs(d.pdec[j], 1, nblk, 2 * N, g->ln_wb[j]));
        TRY(wg(B, N, Kin, d.dv[j], N, xin, Kin, Kin, ss, nullptr, 0, 0, g->dec_w[j], g->dec_b[j]));
    }
    {
        const int C = net->width[4];
        const int nblk = (int)(dadmm_hyper_rownorm_bwd_part_bytes(rows, C) / (4 * 2 * (size_t)C));
        TRY(cs(d.pnorm, 1, nblk, 2 * C, g->norm_wb));
    }
    for (int i = 4; i >= 0; --i) {
        const int N = net->width[i];
        TRY(cs(d.pgcn[i], 3, B, N, g->bn_wbc[i]));
        if (i > 0) {
            const int Kin = net->width[i - 1];
            TRY(wg(rows, N, Kin, d.dZ[i], N, sv0->y[i - 1], Kin, Kin, ss, nullptr, 0, 0, g->conv_w[i], nullptr));
        } else {
            // layer 1's input cat(AtAy_k, Atb): AtAy of iteration k at AtAy + k atay_stride, Atb shared
            TRY(wg(rows, N, 2 * n, d.dZ[0], N, AtAy, net->ld, n, (size_t)atay_stride, Atb, net->ld, 0,
                   g->conv_w[0], nullptr));
        }
    }
    return DADMM_OK;
}

}  // extern "C"

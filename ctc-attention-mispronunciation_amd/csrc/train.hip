// The training step behind the C ABI: CTC_Model.forward in train mode and its backward (BASELINE config 5).
//
// Reference: run_epoch, AA/steps/train_ctc.py:28-105 -- `out = model(inputs, trans)` in train mode (AA/models/model_ctc.py:160-223:
// BatchNorm on batch statistics with running-statistics update, Dropout(p) behind each LayerCNN and BatchRNN), nn.CTCLoss(sum)/B
// (mdd_ctc_loss), loss.backward() (autograd), optimizer.step() (torch.optim.Adam lr 1e-3, weight_decay 5e-4; train_ctc.py:187).
//
// Parameters stay where the caller keeps them (the drop-in CTC_Model's torch Parameters): every call receives the device
// pointers of the 55 float tensors of the state_dict in the order mdd_train_tensor_info() reports, and mdd_train_backward
// writes one gradient tensor per parameter.  The handle owns the saved activations of the last forward.
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "train.h"

namespace mdd {

struct TInfo { std::string key; int64_t numel; int is_buffer; };

// Where each tensor of the state_dict sits in tensors[] / grads[]: filled beside `info` at create, the only place that spells the keys.
struct BnIdx { int weight, bias, running_mean, running_var; };
struct LstmIdx { int w_ih[2], w_hh[2]; };                  // [forward, reverse]
struct ParamTable {
    struct Conv { int weight, bias; BnIdx bn; } conv[2];
    std::vector<BnIdx> rnn_bn;                             // BatchNorm in front of acoustic layer n (n >= 1; entry 0 unused)
    std::vector<LstmIdx> lstm;                             // acoustic layers 0..layers-1, then the text encoder
    int embeds, text_b_ih[2], text_b_hh[2], score, fc_weight;
    BnIdx fc_bn;
};

// Every size of one step, from (cfg, B, T, L).  BiLSTM n: 0..nl-1 the acoustic layers, nl the text encoder.
struct StepDims {
    int B, T, L, ch, H, H2, G2, Tp, W1, W2, Kin0, nl, E, C;
    size_t R0, R1, R, Rt;                                  // rows of conv0's / conv1's output, of the acoustic and of the text sequence
    StepDims(const mdd_config &c, int B_, int T_, int L_)
        : B(B_), T(T_), L(L_), ch(c.channels), H(c.hidden), H2(2 * H), G2(8 * H), Tp(T / 2), W1(conv_out(c.feat)), W2(conv_out(W1)), Kin0(ch * W2),
          nl(c.layers), E(c.emb_dim), C(c.num_class), R0((size_t)B * T * W1), R1((size_t)B * Tp * W2), R((size_t)Tp * B), Rt((size_t)L * B) {}
    int K(int n) const { return n == nl ? E : n == 0 ? Kin0 : H2; }      // input width of BiLSTM n
    int steps(int n) const { return n == nl ? L : Tp; }
    size_t rows(int n) const { return n == nl ? Rt : R; }
    // slots of the BatchNorm sites in the saved mean / invstd planes (stats_plane floats each)
    int conv_slot(int i) const { return i * ch; }
    int rnn_slot(int n) const { return 2 * ch + (n - 1) * H2; }
    int fc_slot() const { return 2 * ch + nl * H2; }
    int stats_plane() const { return fc_slot() + 2 * H2; }
    // bytes of dropout mask `site` (conv0, conv1, rnn 0..nl-1)
    int64_t mask_bytes(int site) const { return site == 0 ? (int64_t)R0 * ch : site == 1 ? (int64_t)R1 * ch : (int64_t)R * H2; }
};

}  // namespace mdd

// state of the training path of one handle
struct mdd_train_ws {
    mdd_config cfg;
    int device = 0;
    std::vector<mdd::TInfo> info;
    mdd::ParamTable params;
    // The forward whose activations the buffers below hold.  valid: it was enqueued completely and no backward has used it yet (the backward
    // overwrites saved activations, so it runs once per forward).  precision / conv1_direct: the kernels that forward chose; its backward
    // follows them, whatever the handle's mode is by then.
    struct Saved {
        bool valid = false, conv1_direct = false;
        int B = 0, T = 0, L = 0, precision = 0;
        float p_drop = 0.f;
        const int64_t *ids = nullptr; const float *x = nullptr;   // canonical ids and features (caller memory, must stay valid until backward)
    } saved;
    // saved activations / scratch
    mdd::DeviceBuf z0, a0, col1, w1r, z1, a1, seq0, gx, dgx, hb, cb, emb, text, key, att, cat, ycat, logits, logp, tbias;
    mdd::DeviceBuf stats;              // per-site mean / invstd
    std::vector<mdd::DeviceBuf> xin, hraw, pd, gates, cst, wihp, whhp, whht;    // per BiLSTM (index layers = the text encoder)
    mdd::DeviceBuf d_a, d_b, d_c, part, dtext, dkey;      // backward temporaries
    mdd::DeviceBuf whhs, hx;           // flagged variant: W_hh' as hi/lo planes and the h exchange buffer of the persistent layer kernel
    mdd::DeviceArray<unsigned int> sync_words;
    bool persist_ok = false;           // the device can hold the persistent layer kernel's grid
    mdd::DeviceBuf xs_a, xs_b;         // operand planes of the GEMMs of modes 1 (hi plane, then lo plane) and 2 (hi | mid | lo); written afresh by every GEMM
    int precision = 0;                 // mode of the NEXT forward.  0: exact fp32 MFMA everywhere (the reference trains in fp32); 1: the large contractions
                                       // as split-bf16 x3; 2: the large contractions as f32x6 (reference width), everything else as 0
    bool conv1_im2col = false;         // MDD_TRAIN_CONV1_IM2COL at create
    mdd::X6Raster x6_raster = mdd::kX6DefaultRaster;   // MDD_GEMM_X6_RASTER at create: the tile walk of the one-launch f32x6 products
    mdd::DeviceArray<int> err_flag;    // set by the embedding gather on an id outside the table
    mdd::DeviceBuf masks, maskt;       // generated dropout masks (bytes); the conv sites' in channels-last order
    std::vector<const unsigned char *> mask_ptr;
    const unsigned char *mask_rows[2] = {nullptr, nullptr};   // the two conv sites' masks in channels-last order
    mdd::DeviceArray<double> dacc;     // fp64 column sums
};

#define TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

namespace mdd {

static void build_info(mdd_train_ws *w) {
    const mdd_config &c = w->cfg;
    const StepDims d(c, 1, 2, 1);
    const int H = d.H, ch = d.ch;
    ParamTable &p = w->params;
    auto add = [&](const std::string &k, int64_t n, int buf = 0) { w->info.push_back(TInfo{k, n, buf}); return (int)w->info.size() - 1; };
    auto bn = [&](const std::string &k, int n) { return BnIdx{add(k + ".weight", n), add(k + ".bias", n), add(k + ".running_mean", n, 1), add(k + ".running_var", n, 1)}; };
    p.conv[0] = {add("conv.0.conv.weight", (int64_t)ch * 9), add("conv.0.conv.bias", ch), bn("conv.0.batch_norm", ch)};
    p.conv[1] = {add("conv.1.conv.weight", (int64_t)ch * ch * 9), add("conv.1.conv.bias", ch), bn("conv.1.batch_norm", ch)};
    p.rnn_bn.assign(d.nl, BnIdx{-1, -1, -1, -1});
    p.lstm.resize(d.nl + 1);
    auto lstm = [&](const std::string &k, int n, bool bias) {          // one nn.LSTM: per direction weight_ih, weight_hh (, bias_ih, bias_hh)
        for (int dir = 0; dir < 2; dir++) {
            const char *sfx = dir ? "_l0_reverse" : "_l0";
            p.lstm[n].w_ih[dir] = add(k + "weight_ih" + sfx, (int64_t)4 * H * d.K(n)); p.lstm[n].w_hh[dir] = add(k + "weight_hh" + sfx, (int64_t)4 * H * H);
            if (bias) { p.text_b_ih[dir] = add(k + "bias_ih" + sfx, 4 * H); p.text_b_hh[dir] = add(k + "bias_hh" + sfx, 4 * H); }
        }
    };
    for (int n = 0; n < d.nl; n++) {
        if (n > 0) p.rnn_bn[n] = bn("rnns." + std::to_string(n) + ".batch_norm", 2 * H);
        lstm("rnns." + std::to_string(n) + ".rnn.", n, false);
    }
    p.embeds = add("embeds.weight", (int64_t)c.emb_rows * c.emb_dim);
    lstm("lstm_embeds.", d.nl, true);
    p.score = add("score.weight", (int64_t)4 * H * H);
    p.fc_bn = bn("fc.0", 4 * H);
    p.fc_weight = add("fc.1.weight", (int64_t)c.num_class * 4 * H);
}

// "Few output tiles, long contraction" (the weight gradients, the classifier): the contraction is cut into chunks that run as partial products and
// are summed afterwards (sum_parts), so the whole chip works on it.  One rule per arithmetic: fewer than max_tiles output tiles of tile_m x 128 and
// K >= min_k -> min(max_chunks, max(1, min(K' / k_unit, wg_budget / tiles))) chunks, K' = K rounded up to k_round.  The exact kernels cut K into
// chunks of ceil(K / chunks), or of k_unit itself (fixed_len).  The values decide the order of summation, i.e. the bits.
enum class Arith { Exact, X3, X6, Classifier };
struct SplitRule { int tile_m, max_tiles, min_k, k_round, k_unit, wg_budget, max_chunks; bool fixed_len; };
static const SplitRule kSplitRules[] = {
    /* Exact      */ {128, 256, 1025, 1, 512, 512, 64, false},
    /* X3         */ {128, 256, 2049, 1, 1024, 512, 16, false},
    /* X6         */ {192, 256, 512, 32, 256, 256, 16, false},       // K' / 256 = K-tiles of 32 / 8: chunks of at least 8 K-tiles
    /* Classifier */ {128, 128, 1024, 256, 256, 1 << 30, 1 << 30, true},   // [R, 4H] x [C, 4H]^T: one column tile, 63 row tiles at R = 8000; chunks of 256
};
static int split_chunks(Arith a, int M, int N, int K) {
    const SplitRule &r = kSplitRules[(int)a];
    const int tiles = ((M + r.tile_m - 1) / r.tile_m) * ((N + 127) / 128);
    if (tiles >= r.max_tiles || K < r.min_k) return 1;
    return std::min(r.max_chunks, std::max(1, std::min((K + r.k_round - 1) / r.k_round * r.k_round / r.k_unit, r.wg_budget / tiles)));
}

// C[M,N] (ldc == N, no bias) = opA . opB^T in exact fp32, split by `rule` (Exact or Classifier)
static int gemm_f32_split(mdd_train_ws *w, Arith rule, const GemmOperand &A, const GemmOperand &B, float *C, int M, int N, int K, hipStream_t st) {
    const int chunks = split_chunks(rule, M, N, K);
    if (chunks <= 1) return launch_gemm_f32(A, B, C, N, M, N, K, st);
    const int kc = kSplitRules[(int)rule].fixed_len ? kSplitRules[(int)rule].k_unit : (K + chunks - 1) / chunks;
    return sum_parts(w->part, (K + kc - 1) / kc, (size_t)M * N, C, st,
                     [&](float *part) { return launch_gemm_f32(A, B, part, N, M, N, K, st, {.sC = (long)M * N, .ksplit = kc}); });
}

// C[M,N] = opA . opB^T (+ bias) for the large contractions of the step, in the arithmetic of the saved forward's mode.  A dispatcher:
//   mode 2 (f32x6, reference width: gemm_f32x6_ops)  M, N >= 128 (most of one 192 x 128 tile), K >= 64, M * N * K >= 2^27, lda, ldb and ldc multiples
//          of 4 and A, B and C 16-byte aligned (the split kernels' 16-byte reads, the GEMM's 16-byte stores).  The threshold is a quarter of mode 1's
//          on purpose: below ~2^27 multiply-adds the exact kernel finishes in the time of the x6 path's three or four launches (tools/time_train_step.py).
//   mode 1 (split-bf16 x3: gemm_bf16x3_ops)  a problem large enough to fill 256 x 256 tiles: M, N, K >= 256, ldc a multiple of 4, M * N * K >= 2^30.
//   otherwise, and in mode 0: exact fp32, bit for bit the same in every mode.
// A product without bias and with ldc == N may be cut along K (split_chunks); in exact fp32 only the weight gradients' form (both stored [K, *]) is.
static int gemm_big(mdd_train_ws *w, const GemmOperand &A, const GemmOperand &B, const float *bias, float *C, int ldc, int M, int N, int K, hipStream_t st) {
    const int mode = w->saved.precision;
    const size_t macs = (size_t)M * N * K;
    const bool may_split = !bias && ldc == N;
    if (mode == 2 && M >= 128 && N >= 128 && K >= 64 && macs >= ((size_t)1 << 27) && x6_ops_ok(A, B, C, ldc))
        return gemm_f32x6_ops(A, B, bias, C, ldc, M, N, K, may_split ? split_chunks(Arith::X6, M, N, K) : 1, w->xs_a, w->xs_b, w->part, st, w->x6_raster);
    if (mode == 1 && M >= 256 && N >= 256 && K >= 256 && ldc % 4 == 0 && macs >= ((size_t)1 << 30))
        return gemm_bf16x3_ops(A, B, bias, C, ldc, M, N, K, may_split ? split_chunks(Arith::X3, M, N, K) : 1, w->xs_a, w->xs_b, w->part, st);
    if (may_split && A.k_major && B.k_major) return gemm_f32_split(w, Arith::Exact, A, B, C, M, N, K, st);
    return launch_gemm_f32(A, B, C, ldc, M, N, K, st, {.bias = bias});
}

// BiLSTM n of the forward (0..nl-1 the acoustic layers, nl the text encoder, which alone has a bias): gate-packed weights, input projection into gx,
// the recurrence into hraw[n] with gates and cell states saved for the backward pass.  Exact mode: one launch per step, fp32 MFMA.  Flagged
// split-bf16 variant on a device that holds the persistent grid: the decode path's layer kernel (one launch, W_hh' resident in registers as
// bf16 hi/lo fragments, h exchanged inside 8-workgroup teams) with the saves added.
static int bilstm_forward(mdd_train_ws *w, const StepDims &d, float *const *tensors, int n, const float *xin, const float *bias, hipStream_t st) {
    const LstmIdx &p = w->params.lstm[n];
    const int H = d.H, K = d.K(n);
    TRY(launch_pack_gates(tensors[p.w_ih[0]], tensors[p.w_ih[1]], w->wihp[n].p, H, K, st));
    TRY(launch_pack_gates(tensors[p.w_hh[0]], tensors[p.w_hh[1]], w->whhp[n].p, H, H, st));
    TRY(gemm_big(w, {.p = xin, .ld = K}, {.p = w->wihp[n].p, .ld = K}, bias, w->gx.p, d.G2, (int)d.rows(n), d.G2, K, st));
    LstmStepArgs a;
    a.gx = w->gx.p; a.whh = w->whhp[n].p; a.hbuf = w->hb.p; a.cbuf = w->cb.p; a.out = a.out_raw = w->hraw[n].p; a.T = d.steps(n); a.B = d.B; a.H = H;
    a.whh_split = SplitPtr{nullptr, nullptr}; a.hsplit = nullptr; a.packed = 0; a.gates_save = w->gates[n].p; a.c_save = w->cst[n].p;
    if (w->saved.precision != 1 || !w->persist_ok || (H != 384 && H != 256) || d.B > 512) return launch_lstm_layer_train(a, st);
    const size_t nW = (size_t)8 * H * H;
    TRY(w->whhs.need(nW));
    unsigned short *hi = reinterpret_cast<unsigned short *>(w->whhs.p), *lo = hi + nW;
    TRY(launch_split_rows(a.whh, H, (size_t)8 * H, H, H, hi, lo, st));
    a.whh_split = SplitPtr{hi, lo};
    a.out = nullptr;
    TRY(w->hx.need(team8_hx_alloc_floats(H, d.B) + kHxTailFloats));
    return launch_lstm_layer_granule(a, reinterpret_cast<unsigned short *>(w->hx.p), w->sync_words.p, w->err_flag.p + 1, st);
}

// Work that may contain persistent launches (mode 1 on a device that holds their grid): one at a time per device.  Mode 2 has none.
template <class F> static int with_device_gate(mdd_train_ws *w, int precision, void *stream, F body) {
    const bool gated = precision == 1 && w->persist_ok;
    bool held = false;
    if (gated) { MDD_HIP_CHECK(hipSetDevice(w->device)); if (int rc = device_gate_enter(w->device, (hipStream_t)stream, &held)) return rc; }
    const int rc = body();
    return gated ? device_gate_leave(w->device, (hipStream_t)stream, held, rc) : rc;
}

}  // namespace mdd

using namespace mdd;

extern "C" int mdd_train_set_precision(mdd_train_ws *w, int32_t mode) {
    if (!w || mode < 0 || mode > 2) {
        set_error("mdd_train_set_precision: mode must be 0 (exact fp32), 1 (split-bf16 x3 contractions) or 2 (f32x6 contractions)"); return MDD_ERR_ARG;
    }
    w->precision = mode;
    return MDD_OK;
}

extern "C" int mdd_train_create(const mdd_config *cfg, int device, mdd_train_ws **out) {
    if (!cfg || !out) { set_error("mdd_train_create: null argument"); return MDD_ERR_ARG; }
    if (const char *why = geometry_error(*cfg)) { set_error("mdd_train_create: unsupported geometry: %s", why); return MDD_ERR_ARG; }
    MDD_HIP_CHECK(hipSetDevice(device));
    std::unique_ptr<mdd_train_ws> w(new mdd_train_ws());
    w->cfg = *cfg; w->device = device;
    const Switches sw = read_switches();   // the environment at create (plan.h); the mode can change later, a backward follows its own forward (Saved)
    w->precision = sw.train_precision;
    w->conv1_im2col = sw.train_conv1_im2col;
    w->x6_raster = sw.x6_raster;
    build_info(w.get());
    const int nl = cfg->layers + 1;
    w->xin.resize(nl); w->hraw.resize(nl); w->pd.resize(nl); w->gates.resize(nl); w->cst.resize(nl); w->wihp.resize(nl); w->whhp.resize(nl); w->whht.resize(nl);
    if (w->dacc.need(2 * 8192) || w->err_flag.need(2) || hipMemset(w->err_flag.p, 0, 2 * sizeof(int)) != hipSuccess || w->sync_words.need(32)) {
        set_error("mdd_train_create: out of memory"); return MDD_ERR_NOMEM;
    }
    TRY(init_gemm_attributes()); TRY(init_gemm_x6_attributes()); TRY(init_granule_attributes()); TRY(init_lstm_bwd_attributes()); TRY(init_conv1_attributes());
    { int n_cu = 0; w->persist_ok = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && persistent_grid_fits(n_cu) && !sw.lstm_step; }
    static_assert(2 * 8192 >= 2 * 8 * kMaxHidden, "dacc holds the two column sums of 8H features up to the largest hidden size (plan.h)");
    *out = w.release();
    return MDD_OK;
}
extern "C" void mdd_train_destroy(mdd_train_ws *w) { if (w) { (void)hipSetDevice(w->device); (void)hipDeviceSynchronize(); delete w; } }
extern "C" int32_t mdd_train_num_tensors(mdd_train_ws *w) { return w ? (int32_t)w->info.size() : 0; }
extern "C" int mdd_train_tensor_info(mdd_train_ws *w, int32_t i, char *key, int32_t cap, int64_t *numel, int32_t *is_buffer) {
    if (!w || i < 0 || i >= (int)w->info.size() || !key || cap < 2) { set_error("mdd_train_tensor_info: bad argument"); return MDD_ERR_ARG; }
    snprintf(key, cap, "%s", w->info[i].key.c_str());
    if (numel) *numel = w->info[i].numel;
    if (is_buffer) *is_buffer = w->info[i].is_buffer;
    return MDD_OK;
}
// bytes of each dropout mask the caller may pass (sites: conv0, conv1, rnn 0..layers-1), in that order
extern "C" int32_t mdd_train_num_masks(mdd_train_ws *w) { return w ? 2 + w->cfg.layers : 0; }
extern "C" int64_t mdd_train_mask_bytes(mdd_train_ws *w, int32_t site, int32_t B, int32_t T) {
    if (!w || site < 0 || site >= 2 + w->cfg.layers) return -1;
    return StepDims(w->cfg, B, T, 1).mask_bytes(site);
}

static int train_forward_enqueue(mdd_train_ws *w, float *const *tensors, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                                 const uint8_t *const *masks, uint64_t seed, float p_drop, float *logp_dev, hipStream_t st) {
    if (!tensors || !x_dev || !x1_dev || !logp_dev || B <= 0 || T < 2 || (T & 1) || L <= 0 || p_drop < 0.f || p_drop >= 1.f) {
        set_error("mdd_train_forward: bad argument"); return MDD_ERR_ARG;
    }
    MDD_HIP_CHECK(hipSetDevice(w->device));
    const mdd_config &c = w->cfg;
    const ParamTable &p = w->params;
    const StepDims d(c, B, T, L);
    const int ch = d.ch, H = d.H, H2 = d.H2, G2 = d.G2, Tp = d.Tp, W1 = d.W1, W2 = d.W2, nl = d.nl, E = d.E, C = d.C;
    const size_t R0 = d.R0, R1 = d.R1, R = d.R, Rt = d.Rt;
    const float scale = 1.f / (1.f - p_drop);
    w->saved.B = B; w->saved.T = T; w->saved.L = L; w->saved.p_drop = p_drop; w->saved.ids = x1_dev; w->saved.x = x_dev; w->saved.precision = w->precision;
    const bool direct1 = w->saved.conv1_direct = ch == 32 && W1 <= 128 && !w->conv1_im2col;    // conv1: the direct kernels (train_conv1.hip), else im2col + GEMM
    // ---- buffers
    TRY(w->z0.need(R0 * ch)); TRY(w->a0.need(R0 * ch)); TRY(w->w1r.need((size_t)ch * 9 * ch));
    if (!direct1) TRY(w->col1.need(R1 * 9 * ch));
    TRY(w->z1.need(R1 * ch)); TRY(w->a1.need(R1 * ch)); TRY(w->seq0.need(R * d.Kin0));
    TRY(w->gx.need(std::max(R, Rt) * G2)); TRY(w->hb.need((size_t)4 * B * H)); TRY(w->cb.need((size_t)2 * B * H));
    TRY(w->emb.need(Rt * E)); TRY(w->key.need(Rt * H2)); TRY(w->att.need((size_t)B * Tp * L));
    TRY(w->cat.need(R * 2 * H2)); TRY(w->ycat.need(R * 2 * H2)); TRY(w->logits.need(R * C)); TRY(w->logp.need(R * C));
    TRY(w->stats.need((size_t)2 * d.stats_plane() + 64)); TRY(w->tbias.need(G2)); TRY(w->d_a.need(G2));
    for (int n = 0; n <= nl; n++) {
        const size_t rows = d.rows(n), K = d.K(n);
        if (n > 0 && n < nl) TRY(w->xin[n].need(rows * K));
        TRY(w->hraw[n].need(rows * H2)); if (n < nl) TRY(w->pd[n].need(rows * H2));
        TRY(w->gates[n].need(rows * 2 * H * 4)); TRY(w->cst[n].need(rows * 2 * H));
        TRY(w->wihp[n].need(G2 * K)); TRY(w->whhp[n].need((size_t)G2 * H)); TRY(w->whht[n].need((size_t)G2 * H));
    }
    // ---- dropout masks: the caller's, or drawn here; the conv sites' kernels walk channels-last rows: their masks once more in that order
    const int nm = 2 + nl;
    auto pad16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    w->mask_ptr.assign(nm, nullptr);
    w->mask_rows[0] = w->mask_rows[1] = nullptr;
    if (p_drop > 0.f) {
        if (masks) {
            for (int s = 0; s < nm; s++) { if (!masks[s]) { set_error("mdd_train_forward: mask %d missing", s); return MDD_ERR_ARG; } w->mask_ptr[s] = masks[s]; }
        } else {
            size_t tot = 0;
            for (int s = 0; s < nm; s++) tot += pad16((size_t)d.mask_bytes(s));
            TRY(w->masks.need((tot + 3) / 4));
            unsigned char *m = reinterpret_cast<unsigned char *>(w->masks.p);
            for (int s = 0; s < nm; m += pad16((size_t)d.mask_bytes(s)), s++) {
                TRY(launch_dropout_mask(m, (size_t)d.mask_bytes(s), seed, (unsigned)s, p_drop, st));
                w->mask_ptr[s] = m;
            }
        }
        const size_t n0 = pad16(R0 * ch), n1 = R1 * ch;
        TRY(w->maskt.need((n0 + n1 + 3) / 4));
        unsigned char *m0 = reinterpret_cast<unsigned char *>(w->maskt.p), *m1 = m0 + n0;
        TRY(launch_mask_rows(w->mask_ptr[0], m0, B, ch, T * W1, st));
        TRY(launch_mask_rows(w->mask_ptr[1], m1, B, ch, Tp * W2, st));
        w->mask_rows[0] = m0; w->mask_rows[1] = m1;
    }
    // BatchNorm on batch statistics at one site: its parameters by table entry, its saved mean / invstd by slot
    float *mean = w->stats.p, *invstd = w->stats.p + d.stats_plane();
    auto bn = [&](const BnIdx &i, int slot, const float *x, size_t rows, int F, const BnSite *drop, float *y) {
        return launch_bn_train_fwd(x, rows, F, tensors[i.weight], tensors[i.bias], c.bn_eps, 0.1f, tensors[i.running_mean], tensors[i.running_var], w->dacc.p,
                                   mean + slot, invstd + slot, drop, y, st);
    };
    const BnSite drop0{w->mask_rows[0], scale}, drop1{w->mask_rows[1], scale};
    // ---- conv0 -> BN -> ReLU -> Dropout
    TRY(launch_conv0_train_fwd(x_dev, tensors[p.conv[0].weight], tensors[p.conv[0].bias], w->z0.p, B, T, c.feat, ch, st));
    TRY(bn(p.conv[0].bn, d.conv_slot(0), w->z0.p, R0, ch, &drop0, w->a0.p));
    // ---- conv1 (direct, or im2col + GEMM) -> BN -> ReLU -> Dropout -> [T',B,ch*W2]
    TRY(launch_pack_w1(tensors[p.conv[1].weight], w->w1r.p, ch, true, st));
    if (direct1) {
        TRY(launch_conv1_fwd_direct(w->a0.p, w->w1r.p, tensors[p.conv[1].bias], w->z1.p, B, T, W1, W2, ch, st));
    } else {
        TRY(launch_im2col1(w->a0.p, w->col1.p, B, T, W1, W2, ch, st));
        TRY(launch_gemm_f32({.p = w->col1.p, .ld = 9 * ch}, {.p = w->w1r.p, .ld = 9 * ch}, w->z1.p, ch, (int)R1, ch, 9 * ch, st, {.bias = tensors[p.conv[1].bias]}));
    }
    TRY(bn(p.conv[1].bn, d.conv_slot(1), w->z1.p, R1, ch, &drop1, w->a1.p));
    TRY(launch_cnn_seq(w->a1.p, w->seq0.p, B, Tp, W2, ch, true, st));
    // ---- BatchRNN x layers: (BN ->) BiLSTM -> Dropout
    for (int n = 0; n < nl; n++) {
        if (n > 0) TRY(bn(p.rnn_bn[n], d.rnn_slot(n), w->pd[n - 1].p, R, H2, nullptr, w->xin[n].p));
        TRY(bilstm_forward(w, d, tensors, n, n > 0 ? w->xin[n].p : w->seq0.p, nullptr, st));
        TRY(launch_dropout_rows(w->hraw[n].p, w->mask_ptr[2 + n], scale, R * H2, w->pd[n].p, st));
    }
    const float *X = w->pd[nl - 1].p, *text = w->hraw[nl].p;
    // ---- text encoder: Embedding -> BiLSTM with bias b_ih + b_hh (packed into tbias; d_a holds b_hh on the way) ; key = score(text)
    TRY(launch_embed(tensors[p.embeds], c.emb_rows, E, x1_dev, B, L, w->emb.p, SplitPtr{nullptr, nullptr}, w->err_flag.p, st));
    TRY(launch_pack_gates(tensors[p.text_b_ih[0]], tensors[p.text_b_ih[1]], w->tbias.p, H, 1, st));
    TRY(launch_pack_gates(tensors[p.text_b_hh[0]], tensors[p.text_b_hh[1]], w->d_a.p, H, 1, st));
    TRY(launch_copy_cols(w->d_a.p, G2, 0, w->tbias.p, G2, 0, 1, G2, true, st));
    TRY(bilstm_forward(w, d, tensors, nl, w->emb.p, w->tbias.p, st));
    TRY(launch_gemm_f32({.p = text, .ld = H2}, {.p = tensors[p.score], .ld = H2}, w->key.p, H2, (int)Rt, H2, H2, st));
    // ---- attention per batch entry b: S = X.key^T, softmax over L (no scale, no mask), ctx = A.text, cat(X, ctx)
    const long sS = (long)Tp * L;      // att is [B][T'][L]; X, key, text and cat are time-major rows, entry b at column offset b * width
    TRY(launch_gemm_f32({.p = X, .ld = B * H2, .stride = H2}, {.p = w->key.p, .ld = B * H2, .stride = H2}, w->att.p, L, Tp, L, H2, st, {.batch = B, .sC = sS}));
    TRY(launch_softmax_rows(w->att.p, (size_t)B * Tp, L, w->att.p, false, st));
    TRY(launch_copy_cols(X, H2, 0, w->cat.p, 2 * H2, 0, R, H2, false, st));
    TRY(launch_gemm_f32({.p = w->att.p, .ld = L, .stride = sS}, {.p = text, .ld = B * H2, .k_major = true, .stride = H2}, w->cat.p + H2, B * 2 * H2, Tp, H2, L, st,
                        {.batch = B, .sC = 2 * H2}));
    // ---- fc: BatchNorm1d(4H) -> Linear(4H -> C, no bias) -> log-softmax
    TRY(bn(p.fc_bn, d.fc_slot(), w->cat.p, R, 2 * H2, nullptr, w->ycat.p));
    TRY(gemm_f32_split(w, Arith::Classifier, {.p = w->ycat.p, .ld = 2 * H2}, {.p = tensors[p.fc_weight], .ld = 2 * H2}, w->logits.p, (int)R, C, 2 * H2, st));
    TRY(launch_softmax_rows(w->logits.p, R, C, w->logp.p, true, st));
    MDD_HIP_CHECK(hipMemcpyAsync(logp_dev, w->logp.p, R * C * sizeof(float), hipMemcpyDeviceToDevice, st));
    return MDD_OK;
}
extern "C" int mdd_train_forward(mdd_train_ws *w, float *const *tensors, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                                 const uint8_t *const *masks, uint64_t seed, float p_drop, float *logp_dev, void *stream) {
    if (!w) { set_error("mdd_train_forward: null handle"); return MDD_ERR_ARG; }
    w->saved.valid = false;            // whatever this call does to the buffers, the previous forward is gone
    const int rc = with_device_gate(w, w->precision, stream, [&] { return train_forward_enqueue(w, tensors, x_dev, B, T, x1_dev, L, masks, seed, p_drop, logp_dev, (hipStream_t)stream); });
    w->saved.valid = rc == MDD_OK;     // enqueued completely
    return rc;
}

// one BiLSTM's backward: dout [rows,2H] -> DG (in w->dgx), weight gradients into the reference-layout tensors (packed in d_b on the way), dxin [rows,K]
static int lstm_backward(mdd_train_ws *w, const StepDims &d, int n, const float *dout, const float *xin, float *const *grads, float *dxin, hipStream_t st) {
    const LstmIdx &p = w->params.lstm[n];
    const int H = d.H, H2 = d.H2, G2 = d.G2, G = 4 * H, Tn = d.steps(n), B = d.B, K = d.K(n), rows = (int)d.rows(n), rows1 = rows - B;
    TRY(launch_transpose_whh(w->whhp[n].p, w->whht[n].p, H, st));
    LstmBwdArgs a;
    a.dout = dout; a.gates = w->gates[n].p; a.cst = w->cst[n].p; a.whhT = w->whht[n].p; a.dg = w->dgx.p; a.dc = w->cb.p; a.T = Tn; a.B = B; a.H = H;
    if (w->saved.precision == 1 && w->persist_ok && (H == 384 || H == 256) && B <= 256) {   // flagged variant: the whole recurrence in one persistent launch
        const size_t nW = (size_t)8 * H * H;
        TRY(w->whhs.need(nW));
        unsigned short *hi = reinterpret_cast<unsigned short *>(w->whhs.p), *lo = hi + nW;
        TRY(launch_split_rows(w->whht[n].p, G, (size_t)2 * H, G, G, hi, lo, st));
        TRY(w->hx.need(lstm_bwd_granule_hx_bytes(H) / 4));
        TRY(launch_lstm_bwd_granule(dout, a.gates, a.cst, SplitPtr{hi, lo}, a.dg, Tn, B, H, reinterpret_cast<unsigned short *>(w->hx.p), w->sync_words.p, w->err_flag.p + 1, st));
    } else {
        TRY(launch_lstm_bwd(a, st));
    }
    // dWih' [2*4H, K] = DG^T . xin ;  dWhh'[d] [4H, H] = DG_d^T . h_prev_d  (h_prev = the layer's raw output one step earlier in that direction:
    // forward t = 1.., h_{t-1}; reverse t = 0..T-2, h_{t+1})
    float *const dg = w->dgx.p, *const h = w->hraw[n].p, *const dwp = w->d_b.p;
    TRY(gemm_big(w, {.p = dg, .ld = G2, .k_major = true}, {.p = xin, .ld = K, .k_major = true}, nullptr, dwp, K, G2, K, rows, st));
    TRY(launch_unpack_gates(dwp, grads[p.w_ih[0]], grads[p.w_ih[1]], H, K, st));
    if (Tn > 1) {
        TRY(gemm_big(w, {.p = dg + (size_t)B * G2, .ld = G2, .k_major = true}, {.p = h, .ld = H2, .k_major = true}, nullptr, dwp, H, G, H, rows1, st));
        TRY(gemm_big(w, {.p = dg + G, .ld = G2, .k_major = true}, {.p = h + (size_t)B * H2 + H, .ld = H2, .k_major = true}, nullptr, dwp + (size_t)G * H, H, G, H, rows1, st));
    } else {
        MDD_HIP_CHECK(hipMemsetAsync(dwp, 0, sizeof(float) * G2 * H, st));
    }
    TRY(launch_unpack_gates(dwp, grads[p.w_hh[0]], grads[p.w_hh[1]], H, H, st));
    return gemm_big(w, {.p = dg, .ld = G2}, {.p = w->wihp[n].p, .ld = K, .k_major = true}, nullptr, dxin, K, rows, K, G2, st);
}

static int train_backward_enqueue(mdd_train_ws *w, float *const *tensors, const float *dlogp_dev, float *const *grads, hipStream_t st) {
    MDD_HIP_CHECK(hipSetDevice(w->device));
    const mdd_config &c = w->cfg;
    const ParamTable &p = w->params;
    const StepDims d(c, w->saved.B, w->saved.T, w->saved.L);
    const int B = d.B, T = d.T, L = d.L, ch = d.ch, H = d.H, H2 = d.H2, G2 = d.G2, Tp = d.Tp, W1 = d.W1, W2 = d.W2, nl = d.nl, E = d.E, C = d.C;
    const size_t R0 = d.R0, R1 = d.R1, R = d.R, Rt = d.Rt;
    const float scale = 1.f / (1.f - w->saved.p_drop);
    const bool direct1 = w->saved.conv1_direct;
    const size_t big = std::max(std::max(std::max(R * 2 * H2, R0 * ch), std::max(R * (size_t)d.Kin0, Rt * (size_t)E)), std::max((size_t)B * Tp * L, R1 * ch));
    TRY(w->dgx.need(std::max(R, Rt) * G2)); TRY(w->d_a.need(big)); TRY(w->d_c.need(big)); TRY(w->dtext.need(Rt * H2)); TRY(w->dkey.need(Rt * H2));
    TRY(w->d_b.need(std::max((size_t)G2 * std::max(std::max(d.Kin0, H2), std::max(E, H)), (size_t)ch * 9 * ch)));
    const float *X = w->pd[nl - 1].p, *text = w->hraw[nl].p, *att = w->att.p, *key = w->key.p, *ycat = w->ycat.p;     // saved by the forward
    // ---- scratch roles, in the order they come alive.  Three temporaries (d_a, d_c, d_b) and the forward buffers that are read for the last
    // time on the way are reused; each line names the buffer, what it held before and why that is dead.  Reusing ycat, a1, col1 and logits is
    // why a saved forward serves ONE backward.
    float *dlogits = w->logits.p;   // [R,C]       logits: the forward kept logp, which is all the log-softmax backward reads
    float *dycat = w->d_a.p;        // [R,4H]      d_a: first use (in the forward it passed b_hh to tbias)
    float *dcat = w->d_c.p;         // [R,4H]      d_c: first use
    float *dX = w->ycat.p;          // [R,2H]      ycat: read last by the fc.1.weight gradient
    float *dS = w->d_a.p;           // [B][T'][L]  dycat: consumed by the classifier BatchNorm's backward
    float *dtext = w->dtext.p, *dkey = w->dkey.p;   // [Rt,2H] each, buffers of their own
    float *demb = w->d_c.p;         // [Rt,E]      dcat: its halves went into dX and into dS / dtext
    float *dbias = w->tbias.p;      // [8H]        tbias: the text projection's bias, read by the forward only
    float *dh = w->d_a.p;           // [R,2H]      dS (then the dh of the layer above): dS read last by dkey, a dh by its layer's lstm_backward
    float *dxin = w->d_c.p;         // [R,K]       demb (then the dxin of the layer above): scattered by embed_bwd / consumed by that layer's BatchNorm backward
    float *dpd = w->ycat.p;         // [R,2H]      dX (then the dpd of the layer above): already turned into that layer's dh
    float *da1 = w->a1.p;           // [R1,ch]     a1: the forward relaid it into seq0
    float *dz1 = w->d_a.p;          // [R1,ch]     dh of layer 0
    float *dw1 = w->d_b.p;          // [ch,9ch]    lstm_backward's packed weight gradients, unpacked by then
    float *dcol = w->col1.p;        // [R1,9ch]    im2col path only.  col1: read last by the conv1 weight gradient
    float *da0 = w->d_c.p;          // [R0,ch]     dxin of layer 0, relaid into da1
    float *dz0 = w->d_a.p;          // [R0,ch]     dz1: read last by conv1's input gradient
    float *mean = w->stats.p, *invstd = w->stats.p + d.stats_plane();
    auto bn_bwd = [&](const BnIdx &i, int slot, const float *x, const float *g, size_t rows, int F, const BnSite *drop, float *dx) {
        return launch_bn_train_bwd(x, g, rows, F, tensors[i.weight], tensors[i.bias], mean + slot, invstd + slot, drop, w->dacc.p, dx, grads[i.weight], grads[i.bias], st);
    };
    const BnSite drop0{w->mask_rows[0], scale}, drop1{w->mask_rows[1], scale};
    // ---- log-softmax, Linear, BatchNorm1d of the classifier
    TRY(launch_softmax_bwd_rows(w->logp.p, dlogp_dev, R, C, dlogits, true, st));
    TRY(gemm_f32_split(w, Arith::Exact, {.p = dlogits, .ld = C, .k_major = true}, {.p = ycat, .ld = 2 * H2, .k_major = true}, grads[p.fc_weight], C, 2 * H2, (int)R, st));
    TRY(launch_gemm_f32({.p = dlogits, .ld = C}, {.p = tensors[p.fc_weight], .ld = 2 * H2, .k_major = true}, dycat, 2 * H2, (int)R, 2 * H2, C, st));
    TRY(bn_bwd(p.fc_bn, d.fc_slot(), w->cat.p, dycat, R, 2 * H2, nullptr, dcat));
    // ---- attention, per batch entry b (dctx = the right half of dcat)
    const long sS = (long)Tp * L;
    const GemmOperand dctx{.p = dcat + H2, .ld = B * 2 * H2, .stride = 2 * H2};
    const GemmOperand dctx_t{.p = dcat + H2, .ld = B * 2 * H2, .k_major = true, .stride = 2 * H2};
    TRY(launch_copy_cols(dcat, 2 * H2, 0, dX, H2, 0, R, H2, false, st));
    TRY(launch_gemm_f32(dctx, {.p = text, .ld = B * H2, .stride = H2}, dS, L, Tp, L, H2, st, {.batch = B, .sC = sS}));                                        // dA = dctx . text^T
    TRY(launch_gemm_f32({.p = att, .ld = L, .k_major = true, .stride = sS}, dctx_t, dtext, B * H2, L, H2, Tp, st, {.batch = B, .sC = H2}));                  // dtext = A^T . dctx
    TRY(launch_softmax_bwd_rows(att, dS, (size_t)B * Tp, L, dS, false, st));
    TRY(launch_gemm_f32({.p = dS, .ld = L, .stride = sS}, {.p = key, .ld = B * H2, .k_major = true, .stride = H2}, dX, B * H2, Tp, H2, L, st,
                        {.batch = B, .sC = H2, .accumulate = true}));                                                                                       // dX += dS . key
    TRY(launch_gemm_f32({.p = dS, .ld = L, .k_major = true, .stride = sS}, {.p = X, .ld = B * H2, .k_major = true, .stride = H2}, dkey, B * H2, L, H2, Tp, st,
                        {.batch = B, .sC = H2}));                                                                                                           // dkey = dS^T . X
    TRY(gemm_f32_split(w, Arith::Exact, {.p = dkey, .ld = H2, .k_major = true}, {.p = text, .ld = H2, .k_major = true}, grads[p.score], H2, H2, (int)Rt, st));
    TRY(launch_gemm_f32({.p = dkey, .ld = H2}, {.p = tensors[p.score], .ld = H2, .k_major = true}, dtext, H2, (int)Rt, H2, H2, st, {.accumulate = true}));    // dtext += dkey . Ws
    // ---- text encoder
    TRY(lstm_backward(w, d, nl, dtext, w->emb.p, grads, demb, st));
    TRY(launch_col_sum(w->dgx.p, Rt, G2, w->dacc.p, dbias, st));            // packed bias gradient (u*4+g order)
    TRY(launch_unpack_gates(dbias, grads[p.text_b_ih[0]], grads[p.text_b_ih[1]], H, 1, st));
    TRY(launch_unpack_gates(dbias, grads[p.text_b_hh[0]], grads[p.text_b_hh[1]], H, 1, st));
    TRY(launch_embed_bwd(demb, w->saved.ids, B, L, E, c.emb_rows, grads[p.embeds], st));
    // ---- BatchRNN layers, last to first: Dropout, BiLSTM, (BN)
    for (int n = nl - 1; n >= 0; n--) {
        TRY(launch_dropout_rows(n == nl - 1 ? dX : dpd, w->mask_ptr[2 + n], scale, R * H2, dh, st));    // from the gradient at the layer's (post-dropout) output
        TRY(lstm_backward(w, d, n, dh, n == 0 ? w->seq0.p : w->xin[n].p, grads, dxin, st));
        if (n > 0) TRY(bn_bwd(p.rnn_bn[n], d.rnn_slot(n), w->pd[n - 1].p, dxin, R, H2, nullptr, dpd));
    }
    // ---- conv1: relayout, BN/ReLU/Dropout, weight and input gradients
    TRY(launch_cnn_seq(da1, dxin, B, Tp, W2, ch, false, st));
    TRY(bn_bwd(p.conv[1].bn, d.conv_slot(1), w->z1.p, da1, R1, ch, &drop1, dz1));
    TRY(launch_col_sum(dz1, R1, ch, w->dacc.p, grads[p.conv[1].bias], st));
    if (direct1) {
        TRY(sum_parts(w->part, conv1_wgrad_parts(B, T, W2), (size_t)ch * 9 * ch, dw1, st,
                      [&](float *part) { return launch_conv1_wgrad_direct(dz1, w->a0.p, part, B, T, W1, W2, ch, st); }));
        TRY(launch_pack_w1(dw1, grads[p.conv[1].weight], ch, false, st));
        TRY(launch_conv1_dgrad_direct(dz1, w->w1r.p, da0, B, T, W1, W2, ch, st));
    } else {
        TRY(gemm_f32_split(w, Arith::Exact, {.p = dz1, .ld = ch, .k_major = true}, {.p = w->col1.p, .ld = 9 * ch, .k_major = true}, dw1, ch, 9 * ch, (int)R1, st));
        TRY(launch_pack_w1(dw1, grads[p.conv[1].weight], ch, false, st));
        TRY(launch_gemm_f32({.p = dz1, .ld = ch}, {.p = w->w1r.p, .ld = 9 * ch, .k_major = true}, dcol, 9 * ch, (int)R1, 9 * ch, ch, st));
        TRY(launch_col2im1(dcol, da0, B, T, W1, W2, ch, st));
    }
    // ---- conv0
    TRY(bn_bwd(p.conv[0].bn, d.conv_slot(0), w->z0.p, da0, R0, ch, &drop0, dz0));
    return launch_conv0_train_bwd(w->saved.x, dz0, w->dacc.p, grads[p.conv[0].weight], grads[p.conv[0].bias], B, T, c.feat, ch, st);
}
extern "C" int mdd_train_backward(mdd_train_ws *w, float *const *tensors, const float *dlogp_dev, float *const *grads, void *stream) {
    if (!w) { set_error("mdd_train_backward: null handle"); return MDD_ERR_ARG; }
    if (!tensors || !dlogp_dev || !grads || !w->saved.valid) { set_error("mdd_train_backward: bad argument (forward first)"); return MDD_ERR_ARG; }
    w->saved.valid = false;            // consumed: from here on saved activations are overwritten
    return with_device_gate(w, w->saved.precision, stream, [&] { return train_backward_enqueue(w, tensors, dlogp_dev, grads, (hipStream_t)stream); });
}

// wait for `stream`; reports an out-of-range canonical id seen by the last forward (the reference raises IndexError)
extern "C" int mdd_train_sync(mdd_train_ws *w, void *stream) {
    if (!w) { set_error("null handle"); return MDD_ERR_ARG; }
    MDD_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    int flag[2] = {0, 0};
    MDD_HIP_CHECK(hipMemcpy(flag, w->err_flag.p, 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (flag[0] || flag[1]) MDD_HIP_CHECK(hipMemset(w->err_flag.p, 0, 2 * sizeof(int)));
    if (flag[1]) { set_error("persistent BiLSTM layer kernel gave up waiting for its team (was another persistent launch resident on this device?)"); return MDD_ERR_HIP; }
    if (flag[0]) { set_error("index out of range in self"); return MDD_ERR_ARG; }
    return MDD_OK;
}

// torch.optim.Adam step over n tensors (AA/steps/train_ctc.py:187: lr, weight_decay as L2 added to the gradient); step counts from 1.  The betas are
// doubles: 1 - beta and the bias corrections are formed from the caller's Python doubles, not from their float roundings (train_rows.hip)
extern "C" int mdd_adam_step(float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq, const int64_t *numel, int32_t n,
                             int32_t step, float lr, double beta1, double beta2, float eps, float weight_decay, void *stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !numel || n < 0 || step < 1 || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1)) { set_error("mdd_adam_step: bad argument"); return MDD_ERR_ARG; }
    for (int i = 0; i < n; i++)
        if (params[i] && grads[i] && numel[i] > 0 && (!exp_avg[i] || !exp_avg_sq[i])) { set_error("mdd_adam_step: state of tensor %d missing", i); return MDD_ERR_ARG; }
    return launch_adam_multi(params, grads, exp_avg, exp_avg_sq, numel, n, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}

// C-ABI of libmdd_hip.so: handle, weights, workspace, forward orchestration (include/mdd_hip.h).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

#include "mdd_internal.h"

namespace mdd {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Per-device gate for forwards that contain persistent BiLSTM launches.  A persistent layer kernel needs all of its
// 256 workgroups resident (one per CU); two of them in flight on one device -- two handles, two host threads, two
// streams -- would each hold CUs the other is waiting for until the wall-clock abort.  So every such forward is
// ordered behind the previous one on the same device: the new stream waits for an event recorded at the end of the
// previous forward (a device-side dependency, the host never blocks).  Process-wide; one process per device is the
// deployment model (a second PROCESS on the same device is outside this gate: use MDD_LSTM=step there).
struct DeviceGate {
    std::mutex mu;
    hipEvent_t done = nullptr;        // recorded behind the last gated forward
    hipStream_t stream = nullptr;     // the stream it was recorded on
    bool armed = false;
};
static DeviceGate g_gate[64];

struct GraphKey {
    const void *x, *x1, *out, *tlen, *llen;
    int B, T, L, Traw;
    bool operator<(const GraphKey &o) const { return memcmp(this, &o, sizeof(GraphKey)) < 0; }
};

// The weights of one BiLSTM layer on the device; the text encoder's sit at index cfg.layers.
struct LstmWeights {
    float *wih = nullptr, *whh = nullptr;          // fp32, gate rows permuted (whh in the packed layout where packed_whh)
    SplitPtr wih_s{nullptr, nullptr}, whh_s{nullptr, nullptr};   // split-bf16 copies (whh row-major)
    unsigned short *wih_3 = nullptr;               // three-plane (f32x6) copy of W_ih, K-tile-major
    unsigned short *whh_3 = nullptr;               // Whh' [3][2][4H][H]: three row-major planes (f32x6 layer kernel)
    float *scale = nullptr, *shift = nullptr;      // the BatchNorm of the layer's input (layers 1 .. cfg.layers - 1)
};

// Every device weight of one mdd_finalize_weights: built whole, read-only while in use, freed whole with the set.
struct DecodeWeights {
    float *w_conv0 = nullptr, *sc0 = nullptr, *sh0 = nullptr;
    float *w_conv1t = nullptr, *sc1 = nullptr, *sh1 = nullptr;
    SplitPtr w_conv1_s{nullptr, nullptr};
    unsigned short *w_conv1_3 = nullptr;           // conv1 weights [co][kh][kw][ci] as three row-major planes
    std::vector<LstmWeights> rnn;                  // cfg.layers + 1
    float *emb = nullptr, *t_bias = nullptr;
    float *w_score = nullptr, *fscale = nullptr, *fshift = nullptr, *w_fc = nullptr, *w_fcp = nullptr;
    SplitPtr w_score_s{nullptr, nullptr};
    std::vector<DeviceArray<unsigned char>> mem;   // the allocations behind every pointer above
    template <class T> int alloc(T **p, size_t n) {
        DeviceArray<unsigned char> b;
        if (int rc = b.need(n * sizeof(T))) return rc;
        *p = reinterpret_cast<T *>(b.p);
        mem.push_back(std::move(b));
        return MDD_OK;
    }
};

}  // namespace mdd

struct mdd_model {
    mdd_config cfg;
    int device = 0;
    bool finalized = false, taps = false;
    int precision = 2;   // 2 (default): fp32-grade, the large contractions as f32x6 on the bf16 matrix cores (falls back to 0 when the geometry does not allow);
                         // 0: exact fp32 MFMA everywhere; 1: split-bf16 x3 for every contraction (narrower than fp32: flagged variant)
    mdd::Switches sw;    // the environment at create (plan.h)
    mdd::DeviceFit fit;
    std::map<std::string, std::vector<float>> host;  // state_dict entries as loaded
    std::unique_ptr<mdd::DecodeWeights> weights;   // the set of the last successful mdd_finalize_weights
    // workspace
    mdd::DeviceBuf y0, seq0, gx, act[2], xraw, hbuf, cbuf, embo, text, key, S;
    mdd::DeviceBuf seq0_s, act_s[2], x_s, embo_s, text_s, key_s, hsplit, hx;   // split-bf16 activations (hi plane, then lo plane)
    mdd::DeviceBuf p3;          // f32x6 mode: the three bf16 planes of the projection GEMM's A operand (rewritten per GEMM)
    std::vector<mdd::DeviceBuf> tap_rnn;
    mdd::DeviceArray<int> err_flag;
    hipStream_t cap_stream = nullptr;  // graphs are captured here (the legacy default stream cannot capture)
    int lastB = 0, lastT = 0, lastL = 0;
    mdd::ForwardPlan plan{};    // the kernels of the last prepared forward (shape lastB / lastT / lastL)
    int raw_T = 0;              // > 0 while mdd_forward_raw runs the fused front-end straight on unstacked frames
    const int *tlen = nullptr, *llen = nullptr;   // set while mdd_forward_fused runs: per-row posterior frames / canonical length of the row's own batch
    mdd::DeviceBuf xstack;      // mdd_forward_raw without the fused front-end: stacked copy
    std::map<mdd::GraphKey, hipGraphExec_t> graphs;
    void drop_graphs() { for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second); graphs.clear(); }
    ~mdd_model() { drop_graphs(); if (cap_stream) (void)hipStreamDestroy(cap_stream); }
    int W1() const { return mdd::conv_out(cfg.feat); }
    int W2() const { return mdd::conv_out(W1()); }
    int rnn_in() const { return mdd::rnn_in(cfg); }
    mdd::DeviceArray<unsigned int> sync_words;
};

namespace mdd {

static int upload(DecodeWeights &w, const std::vector<float> &h, float **dev) {
    if (int rc = w.alloc(dev, h.size())) return rc;
    MDD_HIP_CHECK(hipMemcpy(*dev, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return MDD_OK;
}

static unsigned short host_bf16(float x) {   // round-to-nearest-even (weights are finite)
    unsigned u; memcpy(&u, &x, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
static float host_bf16_f32(unsigned short b) { unsigned u = (unsigned)b << 16; float f; memcpy(&f, &u, 4); return f; }

static int upload_split(DecodeWeights &w, const std::vector<float> &h, SplitPtr *out) {
    const size_t n = h.size();
    std::vector<unsigned short> buf(2 * n);
    for (size_t i = 0; i < n; i++) {
        buf[i] = host_bf16(h[i]);
        buf[n + i] = host_bf16(h[i] - host_bf16_f32(buf[i]));
    }
    unsigned short *d = nullptr;
    if (int rc = w.alloc(&d, 2 * n)) return rc;
    MDD_HIP_CHECK(hipMemcpy(d, buf.data(), 2 * n * sizeof(unsigned short), hipMemcpyHostToDevice));
    out->hi = d; out->lo = d + n;
    return MDD_OK;
}

// a DeviceBuf of n floats holds a split tensor of n elements: hi plane then lo plane
static SplitPtr split_view(const DeviceBuf &b, size_t n) {
    SplitPtr s; s.hi = reinterpret_cast<unsigned short *>(b.p); s.lo = s.hi ? s.hi + n : nullptr; return s;
}
static const SplitPtr kNoSplit = {nullptr, nullptr};

// a workspace buffer was reallocated: captured graphs of THIS thread's handle hold stale pointers (set by ensure(), consumed
// by the forward_prepare() call that ran it; thread-local because handles on different host threads prepare concurrently)
static thread_local bool g_ws_moved = false;

// Workspace growth (hipFree / hipMalloc / clearing) and stream capture exclude each other process-wide: a capture in
// progress on one host thread makes another thread's allocation-time calls fail ("operation would make the legacy
// stream depend on a capturing stream").  Both are rare (first call of a shape); graph REPLAYS never take this lock.
static std::mutex g_prep_mu;

static int ensure(DeviceBuf &b, size_t n, hipStream_t zero_stream) {
    if (b.cap >= n) return MDD_OK;
    g_ws_moved = true;
    if (int rc = b.need(n)) return rc;
    b.cap = 0;   // grown only once cleared
    MDD_HIP_CHECK(hipMemsetAsync(b.p, 0, n * sizeof(float), zero_stream));  // padded batch rows of the packed h exchange must be finite
    MDD_HIP_CHECK(hipStreamSynchronize(zero_stream));
    b.cap = n;
    return MDD_OK;
}

static const std::vector<float> *get(mdd_model *m, const std::string &key, size_t numel) {
    auto it = m->host.find(key);
    if (it == m->host.end()) { set_error("weight '%s' was never loaded", key.c_str()); return nullptr; }
    if (it->second.size() != numel) {
        set_error("weight '%s' has %zu elements, expected %zu", key.c_str(), it->second.size(), numel);
        return nullptr;
    }
    return &it->second;
}

// eval-mode BatchNorm as y = x*scale + shift
static bool bn_fold(mdd_model *m, const std::string &prefix, int n, std::vector<float> &scale, std::vector<float> &shift) {
    const auto *w = get(m, prefix + ".weight", n), *b = get(m, prefix + ".bias", n);
    const auto *mu = get(m, prefix + ".running_mean", n), *var = get(m, prefix + ".running_var", n);
    if (!w || !b || !mu || !var) return false;
    scale.resize(n); shift.resize(n);
    for (int i = 0; i < n; i++) {
        scale[i] = (*w)[i] / sqrtf((*var)[i] + m->cfg.bn_eps);
        shift[i] = (*b)[i] - (*mu)[i] * scale[i];
    }
    return true;
}

// rows n = g*H + u  ->  n' = u*4 + g (see lstm.hip); concatenates the two directions
static bool pack_gate_rows(mdd_model *m, const std::string &base, const char *what, int H, int K, std::vector<float> &out) {
    out.assign((size_t)2 * 4 * H * K, 0.f);
    for (int d = 0; d < 2; d++) {
        const auto *w = get(m, base + what + (d ? "_reverse" : ""), (size_t)4 * H * K);
        if (!w) return false;
        for (int g = 0; g < 4; g++)
            for (int u = 0; u < H; u++)
                memcpy(&out[((size_t)d * 4 * H + u * 4 + g) * K], &(*w)[((size_t)g * H + u) * K], sizeof(float) * K);
    }
    return true;
}

// Whh' [2][4H][H] (gate-permuted rows) -> Wp[d][ut][j][lane][m] (see lstm.hip)
static void pack_whh(const std::vector<float> &w, int H, std::vector<float> &out) {
    const int NUT = H / 4, J = H / 16;
    out.resize(w.size());
    for (int d = 0; d < 2; d++)
        for (int ut = 0; ut < NUT; ut++)
            for (int j = 0; j < J; j++)
                for (int lane = 0; lane < 64; lane++)
                    for (int mm = 0; mm < 4; mm++)
                        out[((((size_t)d * NUT + ut) * J + j) * 64 + lane) * 4 + mm] =
                            w[((size_t)d * 4 * H + ut * 16 + (lane & 15)) * H + 16 * j + 4 * (lane >> 4) + mm];
}

// fp32 matrix -> three bf16 planes (hi | mid | lo, same element order), on the device
static int upload_split3(DecodeWeights &w, const std::vector<float> &h, unsigned short **out) {
    const size_t n = h.size();
    std::vector<unsigned short> buf(3 * n);
    for (size_t i = 0; i < n; i++) {
        buf[i] = host_bf16(h[i]);
        const float r1 = h[i] - host_bf16_f32(buf[i]);
        buf[n + i] = host_bf16(r1);
        buf[2 * n + i] = host_bf16(r1 - host_bf16_f32(buf[n + i]));
    }
    if (int rc = w.alloc(out, 3 * n)) return rc;
    MDD_HIP_CHECK(hipMemcpy(*out, buf.data(), 3 * n * sizeof(unsigned short), hipMemcpyHostToDevice));
    return MDD_OK;
}

// Build a complete weight set from the loaded state_dict into `w` (a fresh set: on failure it is discarded whole).
static int build_weights(mdd_model *m, DecodeWeights &w) {
    const mdd_config &c = m->cfg;
    const int ch = c.channels, H = c.hidden;
    int rc;
    std::vector<float> sc, sh, tmp;
    {   // conv0 / conv1: fold bias + BN into scale/shift; conv1 weights -> [ci][kh][kw][co]
        const auto *w0 = get(m, "conv.0.conv.weight", (size_t)ch * 9), *b0 = get(m, "conv.0.conv.bias", ch);
        const auto *w1 = get(m, "conv.1.conv.weight", (size_t)ch * ch * 9), *b1 = get(m, "conv.1.conv.bias", ch);
        if (!w0 || !b0 || !w1 || !b1) return MDD_ERR_STATE;
        if (!bn_fold(m, "conv.0.batch_norm", ch, sc, sh)) return MDD_ERR_STATE;
        for (int i = 0; i < ch; i++) sh[i] += (*b0)[i] * sc[i];
        if ((rc = upload(w, *w0, &w.w_conv0)) || (rc = upload(w, sc, &w.sc0)) || (rc = upload(w, sh, &w.sh0))) return rc;
        if (!bn_fold(m, "conv.1.batch_norm", ch, sc, sh)) return MDD_ERR_STATE;
        for (int i = 0; i < ch; i++) sh[i] += (*b1)[i] * sc[i];
        tmp.assign((size_t)ch * 9 * ch, 0.f);
        for (int co = 0; co < ch; co++)
            for (int ci = 0; ci < ch; ci++)
                for (int k = 0; k < 9; k++) tmp[((size_t)ci * 9 + k) * ch + co] = (*w1)[((size_t)co * ch + ci) * 9 + k];
        if ((rc = upload(w, tmp, &w.w_conv1t)) || (rc = upload(w, sc, &w.sc1)) || (rc = upload(w, sh, &w.sh1))) return rc;
        // conv1 weights for the fused MFMA front-end: [co][kh][kw][ci] (k = (kh*3+kw)*ch + ci), split-bf16, and the same matrix as
        // three planes (hi | mid | lo, each [co][288] row-major) for the fp32-grade fused front-end
        tmp.assign((size_t)ch * 9 * ch, 0.f);
        for (int co = 0; co < ch; co++)
            for (int ci = 0; ci < ch; ci++)
                for (int k = 0; k < 9; k++) tmp[((size_t)co * 9 + k) * ch + ci] = (*w1)[((size_t)co * ch + ci) * 9 + k];
        if ((rc = upload_split(w, tmp, &w.w_conv1_s)) || (rc = upload_split3(w, tmp, &w.w_conv1_3))) return rc;
    }
    w.rnn.resize(c.layers + 1);
    for (int n = 0; n <= c.layers; n++) {   // the BiLSTM layers, then the text encoder
        LstmWeights &lw = w.rnn[n];
        char base[64];
        if (n < c.layers) snprintf(base, sizeof(base), "rnns.%d.rnn.", n);
        else snprintf(base, sizeof(base), "lstm_embeds.");
        const int K = n == c.layers ? c.emb_dim : (n == 0 ? m->rnn_in() : 2 * H);
        if (!pack_gate_rows(m, base, "weight_ih_l0", H, K, tmp)) return MDD_ERR_STATE;
        if ((rc = upload(w, tmp, &lw.wih)) || (rc = upload_split(w, tmp, &lw.wih_s))) return rc;
        // f32x6: hi | mid | lo planes in the kernel's K-tile-major order, made on the device from the fp32 copy
        if (K % 32 == 0 && ((rc = w.alloc(&lw.wih_3, (size_t)3 * 8 * H * K)) || (rc = launch_split3(lw.wih, 8 * H, K, K, lw.wih_3, nullptr)))) return rc;
        if (!pack_gate_rows(m, base, "weight_hh_l0", H, H, tmp)) return MDD_ERR_STATE;
        if ((rc = upload_split(w, tmp, &lw.whh_s))) return rc;
        if (packed_whh(c) && (rc = upload_split3(w, tmp, &lw.whh_3))) return rc;
        if (packed_whh(c)) { std::vector<float> pk; pack_whh(tmp, H, pk); tmp.swap(pk); }
        if ((rc = upload(w, tmp, &lw.whh))) return rc;
        if (n > 0 && n < c.layers) {
            snprintf(base, sizeof(base), "rnns.%d.batch_norm", n);
            if (!bn_fold(m, base, 2 * H, sc, sh)) return MDD_ERR_STATE;
            if ((rc = upload(w, sc, &lw.scale)) || (rc = upload(w, sh, &lw.shift))) return rc;
        }
    }
    {   // text encoder: the embedding table; bias_ih + bias_hh folded into the input projection's epilogue
        const auto *e = get(m, "embeds.weight", (size_t)c.emb_rows * c.emb_dim);
        if (!e) return MDD_ERR_STATE;
        if ((rc = upload(w, *e, &w.emb))) return rc;
        std::vector<float> bi, bh;
        if (!pack_gate_rows(m, "lstm_embeds.", "bias_ih_l0", H, 1, bi) || !pack_gate_rows(m, "lstm_embeds.", "bias_hh_l0", H, 1, bh)) return MDD_ERR_STATE;
        for (size_t i = 0; i < bi.size(); i++) bi[i] += bh[i];
        if ((rc = upload(w, bi, &w.t_bias))) return rc;
    }
    {
        const auto *ws = get(m, "score.weight", (size_t)4 * H * H), *wf = get(m, "fc.1.weight", (size_t)c.num_class * 4 * H);
        if (!ws || !wf) return MDD_ERR_STATE;
        if (!bn_fold(m, "fc.0", 4 * H, sc, sh)) return MDD_ERR_STATE;
        if ((rc = upload_split(w, *ws, &w.w_score_s))) return rc;
        if ((rc = upload(w, *ws, &w.w_score)) || (rc = upload(w, *wf, &w.w_fc)) || (rc = upload(w, sc, &w.fscale)) ||
            (rc = upload(w, sh, &w.fshift))) return rc;
        const int D2 = 4 * H;
        if (D2 % 64 == 0 && c.num_class <= 48) {   // consumer-order repack for attn_tail_mfma_kernel
            const int J = D2 / 64;
            std::vector<float> pk((size_t)4 * 3 * J * 64 * 4, 0.f);
            for (int wv = 0; wv < 4; wv++)
                for (int nt = 0; nt < 3; nt++)
                    for (int j = 0; j < J; j++)
                        for (int lane = 0; lane < 64; lane++)
                            for (int mm = 0; mm < 4; mm++) {
                                const int n = nt * 16 + (lane & 15), k = wv * (D2 / 4) + 16 * j + 4 * (lane >> 4) + mm;
                                if (n < c.num_class) pk[((((size_t)wv * 3 + nt) * J + j) * 64 + lane) * 4 + mm] = (*wf)[(size_t)n * D2 + k];
                            }
            if ((rc = upload(w, pk, &w.w_fcp))) return rc;
        }
    }
    return MDD_OK;
}

// The forward as an ordered list of stages (one or more kernel launches each).  mdd_forward captures all
// of them into one graph; mdd_forward_profile replays them one by one between HIP events.
struct Stage { const char *name; int launches; double flops; };

static int n_stages(const mdd_model *m) { return 2 + 2 * m->cfg.layers + 6; }

// The kernels a forward of B rows runs on this handle as it stands now (plan.h)
static ForwardPlan plan_of(const mdd_model *m, int B) { return plan_forward(m->cfg, m->precision, m->sw, m->fit, B); }

// One BiLSTM layer: the caller sets a.T, a.B, a.seqlen and the outputs, the rest is filled here.  The persistent layer kernel where
// the plan has one (f32x6, split-bf16 or exact-fp32 teams), else one launch per step (launch_lstm_layer: hsplit selects the x3 step).
static int run_lstm(mdd_model *m, const LstmWeights &lw, LstmStepArgs &a, hipStream_t st, Stage *info) {
    const ForwardPlan &p = m->plan;
    a.gx = m->gx.p; a.whh = lw.whh; a.hbuf = m->hbuf.p; a.cbuf = m->cbuf.p;
    a.H = m->cfg.hidden; a.packed = packed_whh(m->cfg);
    a.whh_split = lw.whh_s; a.hsplit = p.lstm == Lstm::StepX3 ? reinterpret_cast<unsigned short *>(m->hsplit.p) : nullptr;
    if (!p.gated) return launch_lstm_layer(a, st);
    info->launches = 1;
    unsigned short *hx = reinterpret_cast<unsigned short *>(m->hx.p);
    long long *stamps = m->sw.lstm_dbg && a.T > 100 ? reinterpret_cast<long long *>(m->hx.p + p.stamps_at) : nullptr;
    if (p.lstm == Lstm::X6) return launch_lstm_layer_x6(a, lw.whh_3, hx, m->sync_words.p, m->err_flag.p, st, stamps, m->sw.x6_redo_mask);
    if (p.lstm == Lstm::Granule) return launch_lstm_layer_granule(a, hx, m->sync_words.p, m->err_flag.p, st, stamps, m->sw.lstm_early);
    return launch_lstm_layer_f32(a, hx, m->sync_words.p, m->err_flag.p, st, stamps);
}

static int run_stage(mdd_model *m, int si, const float *x, int B, int T, const int64_t *x1, int L, float *logp,
                     hipStream_t st, Stage *info) {
    const mdd_config &c = m->cfg;
    const DecodeWeights &w = *m->weights;
    const int H = c.hidden, H2 = 2 * H, G2 = 8 * H, Tp = T / 2, Lp = L, nl = c.layers;
    const ForwardPlan &p = m->plan;
    const bool x3 = p.precision == 1, fused = p.conv != Conv::Separate;   // x3: the activations travel as split-bf16 planes
    const size_t rows = (size_t)Tp * B, trows = (size_t)L * B;
    static thread_local char namebuf[32];
    Stage dummy; if (!info) info = &dummy;
    info->launches = 1; info->flops = 0.0;
    if (si == 0 && fused) {   // conv0 recomputed per output row (x1.5) + conv1 as implicit GEMM, one kernel
        info->name = "conv_fused";
        info->flops = 2.0 * 9 * c.channels * (double)B * Tp * m->W2() * (c.channels + 6.0);
        if (p.conv == Conv::FusedX3)
            return launch_conv_fused(x, w.w_conv0, w.sc0, w.sh0, w.w_conv1_s, w.sc1, w.sh1, split_view(m->seq0_s, rows * m->rnn_in()),
                                     nullptr, B, T, m->raw_T, st);
        // fp32-grade form: three K-tile-major planes straight into the projection GEMM's operand buffer
        return launch_conv_fused3(x, w.w_conv0, w.sc0, w.sh0, w.w_conv1_3, w.sc1, w.sh1, reinterpret_cast<unsigned short *>(m->p3.p),
                                  m->taps ? m->seq0.p : nullptr, B, T, m->raw_T, st, p.conv == Conv::FusedX6Rowwise);
    }
    if (si == 1 && fused) { info->name = "conv1_in_fused"; info->launches = 0; return MDD_OK; }
    if (si == 0) { info->name = "conv0"; info->flops = 2.0 * 9 * c.channels * (double)B * T * m->W1();
        return launch_conv0(x, w.w_conv0, w.sc0, w.sh0, m->y0.p, B, T, c.feat, c.channels, st); }
    if (si == 1) { info->name = "conv1"; info->flops = 2.0 * 9 * c.channels * c.channels * (double)B * Tp * m->W2();
        return launch_conv1(m->y0.p, w.w_conv1t, w.sc1, w.sh1, x3 ? nullptr : m->seq0.p,
                            x3 ? split_view(m->seq0_s, rows * m->rnn_in()) : kNoSplit, B, T, m->W1(), c.channels, st); }
    si -= 2;
    if (si < 2 * nl) {
        const int n = si / 2;
        const int K = n == 0 ? m->rnn_in() : H2;
        if (si % 2 == 0) {
            snprintf(namebuf, sizeof(namebuf), "gemm_ih%d", n); info->name = namebuf;
            info->flops = 2.0 * (double)Tp * B * G2 * K;
            if (p.proj == Gemm::Bf16x3) {
                const SplitPtr in = n == 0 ? split_view(m->seq0_s, rows * K) : split_view(m->act_s[(n - 1) & 1], rows * K);
                return launch_gemm_bf16x3(in, w.rnn[n].wih_s, nullptr, m->gx.p, nullptr, Tp * B, G2, K, K, K, G2, 1, 0, 0, 0, st);
            }
            const float *in = n == 0 ? m->seq0.p : m->act[(n - 1) & 1].p;
            if (p.proj == Gemm::F32x6) {   // fp32-grade arithmetic at 6/16 of the fp32 MFMA's cost (gemm_bf16x6.hip)
                unsigned short *p3 = reinterpret_cast<unsigned short *>(m->p3.p);
                if (!(n == 0 && fused) && !(n >= 1 && p.planes_out))   // (the fused front-end / the layer kernel before has written the planes already)
                    if (int rc = launch_split3(in, Tp * B, K, K, p3, st)) return rc;
                return launch_gemm_f32x6(p3, (size_t)Tp * B * K, w.rnn[n].wih_3, (size_t)G2 * K, nullptr, m->gx.p, Tp * B, G2, K, G2, st);
            }
            return launch_gemm_nt(in, w.rnn[n].wih, nullptr, m->gx.p, Tp * B, G2, K, K, K, G2, 1, 0, 0, 0, st);
        }
        snprintf(namebuf, sizeof(namebuf), "lstm%d", n); info->name = namebuf;
        info->launches = Tp; info->flops = 2.0 * 2 * (double)B * H * 4 * H * Tp;
        LstmStepArgs a;
        a.T = Tp; a.B = B; a.seqlen = m->tlen;
        if (n == nl - 1) {   // raw h: the attention queries X (fp32 for the tail, split for the score GEMM)
            a.out = m->xraw.p; a.out_raw = m->xraw.p; a.oscale = nullptr; a.oshift = nullptr;
            a.out_split = x3 ? split_view(m->x_s, rows * H2) : kNoSplit;
        } else {             // next layer's BatchNorm folded into the store
            a.out = x3 || p.planes_out ? nullptr : m->act[n & 1].p; a.out_raw = m->taps ? m->tap_rnn[n].p : nullptr;
            if (p.planes_out) {   // straight into the next projection's operand buffer (gemm_ih<n> has read it: same stream, stages in order)
                a.out_planes = reinterpret_cast<unsigned short *>(m->p3.p); a.out_planes_stride = rows * H2;
            }
            a.out_split = x3 ? split_view(m->act_s[n & 1], rows * H2) : kNoSplit;
            a.oscale = w.rnn[n + 1].scale; a.oshift = w.rnn[n + 1].shift;
        }
        return run_lstm(m, w.rnn[n], a, st, info);
    }
    si -= 2 * nl;
    const LstmWeights &tw = w.rnn[nl];   // the text encoder
    switch (si) {
    case 0:  // text encoder (model_ctc.py:193,198) and keys (:201)
        info->name = "embed";
        return launch_embed(w.emb, c.emb_rows, c.emb_dim, x1, B, L, x3 ? nullptr : m->embo.p,
                            x3 ? split_view(m->embo_s, trows * c.emb_dim) : kNoSplit, m->err_flag.p, st);
    case 1:
        info->name = "gemm_text"; info->flops = 2.0 * (double)L * B * G2 * c.emb_dim;
        if (p.proj == Gemm::Bf16x3) return launch_gemm_bf16x3(split_view(m->embo_s, trows * c.emb_dim), tw.wih_s, w.t_bias, m->gx.p, nullptr, L * B, G2,
                                                              c.emb_dim, c.emb_dim, c.emb_dim, G2, 1, 0, 0, 0, st);
        if (p.proj == Gemm::F32x6) {
            unsigned short *p3 = reinterpret_cast<unsigned short *>(m->p3.p);
            if (int rc = launch_split3(m->embo.p, L * B, c.emb_dim, c.emb_dim, p3, st)) return rc;
            return launch_gemm_f32x6(p3, (size_t)L * B * c.emb_dim, tw.wih_3, (size_t)G2 * c.emb_dim, w.t_bias, m->gx.p, L * B, G2, c.emb_dim, G2, st);
        }
        return launch_gemm_nt(m->embo.p, tw.wih, w.t_bias, m->gx.p, L * B, G2, c.emb_dim, c.emb_dim, c.emb_dim, G2, 1, 0, 0, 0, st);
    case 2: {
        info->name = "lstm_text"; info->launches = L; info->flops = 2.0 * 2 * (double)B * H * 4 * H * L;
        LstmStepArgs a;
        a.T = L; a.B = B; a.seqlen = m->llen;
        a.out = m->text.p; a.out_raw = m->text.p; a.oscale = nullptr; a.oshift = nullptr;
        a.out_split = x3 ? split_view(m->text_s, trows * H2) : kNoSplit;
        return run_lstm(m, tw, a, st, info);
    }
    case 3:
        info->name = "gemm_key"; info->flops = 2.0 * (double)L * B * H2 * H2;
        if (x3) {
            const SplitPtr ks = split_view(m->key_s, trows * H2);
            return launch_gemm_bf16x3(split_view(m->text_s, trows * H2), w.w_score_s, nullptr, nullptr, &ks, L * B, H2, H2, H2, H2, H2,
                                      1, 0, 0, 0, st);
        }
        return launch_gemm_nt(m->text.p, w.w_score, nullptr, m->key.p, L * B, H2, H2, H2, H2, H2, 1, 0, 0, 0, st);
    case 4:  // scores S[b][t][l] = X[t,b,:] . key[l,b,:]   (:204)
        info->name = "gemm_score"; info->flops = 2.0 * (double)B * Tp * L * H2;
        if (x3) return launch_gemm_bf16x3(split_view(m->x_s, rows * H2), split_view(m->key_s, trows * H2), nullptr, m->S.p, nullptr, Tp, L,
                                          H2, B * H2, B * H2, Lp, B, H2, H2, (long)Tp * Lp, st);
        return launch_gemm_nt(m->xraw.p, m->key.p, nullptr, m->S.p, Tp, L, H2, B * H2, B * H2, Lp, B, H2, H2, (long)Tp * Lp, st);
    default:
        info->name = "attn_tail"; info->flops = 2.0 * (double)B * Tp * ((double)L * H2 + 2.0 * H2 * c.num_class);
        return launch_attn_tail(m->S.p, Lp, m->xraw.p, m->text.p, w.fscale, w.fshift, w.w_fc, w.w_fcp, logp, Tp, B, L, H2, c.num_class, st, m->llen);
    }
}

// Enter / leave the device gate around the enqueue of one forward on `st` (no-op while `st` is being captured by the
// caller: the captured graph then carries the caller's own ordering).
int device_gate_enter(int device, hipStream_t st, bool *held) {
    *held = false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return MDD_OK;
    DeviceGate &g = g_gate[device & 63];
    g.mu.lock();
    *held = true;
    if (g.armed && g.stream != st) {
        hipError_t e = hipStreamWaitEvent(st, g.done, 0);
        if (e != hipSuccess) { g.mu.unlock(); *held = false; set_error("device gate: %s", hipGetErrorString(e)); return MDD_ERR_HIP; }
    }
    return MDD_OK;
}
int device_gate_leave(int device, hipStream_t st, bool held, int rc) {
    if (!held) return rc;
    DeviceGate &g = g_gate[device & 63];
    hipError_t e = hipSuccess;
    if (!g.done) e = hipEventCreateWithFlags(&g.done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(g.done, st);
    if (e == hipSuccess) { g.armed = true; g.stream = st; }
    g.mu.unlock();
    if (e != hipSuccess && rc == MDD_OK) { set_error("device gate: %s", hipGetErrorString(e)); return MDD_ERR_HIP; }
    return rc;
}
static int gate_enter(mdd_model *m, hipStream_t st, bool *held) { return device_gate_enter(m->device, st, held); }
static int gate_leave(mdd_model *m, hipStream_t st, bool held, int rc) { return device_gate_leave(m->device, st, held, rc); }

static int forward_enqueue(mdd_model *m, const float *x, int B, int T, const int64_t *x1, int L, float *logp, hipStream_t st) {
    for (int si = 0; si < n_stages(m); si++)
        if (int rc = run_stage(m, si, x, B, T, x1, L, logp, st, nullptr)) return rc;
    return MDD_OK;
}

}  // namespace mdd

using namespace mdd;

extern "C" const char *mdd_last_error(void) { return g_err; }
extern "C" int mdd_version(void) { return 100; }

extern "C" int mdd_create(const mdd_config *cfg, int device, mdd_model **out) {
    if (!cfg || !out) { set_error("mdd_create: null argument"); return MDD_ERR_ARG; }
    if (cfg->hidden <= 0 || cfg->hidden % 4 || cfg->layers < 1 || cfg->num_class < 2 || cfg->feat < 3 ||
        (cfg->channels != 32 && cfg->channels != 4) || cfg->emb_rows < 1 || cfg->emb_dim < 1) {
        set_error("mdd_create: unsupported geometry (hidden %% 4 == 0, channels in {32,4})");
        return MDD_ERR_ARG;
    }
    int ndev = 0;
    MDD_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_error("mdd_create: device %d of %d", device, ndev); return MDD_ERR_ARG; }
    MDD_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    MDD_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("libmdd_hip is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
        return MDD_ERR_ARG;
    }
    std::unique_ptr<mdd_model> m(new mdd_model());
    m->cfg = *cfg;
    m->device = device;
    m->sw = read_switches();
    m->precision = m->sw.precision;
    if (int rc = init_kernel_attributes()) return rc;
    if (int rc = init_lstm_attributes()) return rc;
    if (int rc = init_granule_attributes()) return rc;
    if (int rc = init_lstm_f32_attributes()) return rc;
    if (int rc = init_lstm_x6_attributes()) return rc;
    if (int rc = init_conv_attributes()) return rc;
    if (int rc = init_gemm_attributes()) return rc;
    if (int rc = init_gemm_x6_attributes()) return rc;
    const int n_cu = prop.multiProcessorCount;   // (where a grid does not fit: per-step kernels, e.g. smaller partitions, other gfx950 SKUs)
    m->fit = {persistent_grid_fits(n_cu) != 0, persistent_f32_grid_fits(n_cu) != 0, persistent_x6_grid_fits(n_cu) != 0};
    if (int rc = m->err_flag.need(1)) return rc;
    if (int rc = m->sync_words.need(32)) return rc;
    hipError_t e = hipMemset(m->err_flag.p, 0, sizeof(int));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { set_error("mdd_create: %s", hipGetErrorString(e)); return MDD_ERR_HIP; }
    *out = m.release();
    return MDD_OK;
}

extern "C" void mdd_destroy(mdd_model *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    delete m;
}

extern "C" int mdd_load_weight(mdd_model *m, const char *key, const float *data, const int64_t *shape, int32_t ndim) {
    if (!m || !key || (!data && ndim > 0) || ndim < 0 || ndim > 4) { set_error("mdd_load_weight: bad argument"); return MDD_ERR_ARG; }
    std::string k(key);
    if (k.size() > 19 && k.compare(k.size() - 19, 19, "num_batches_tracked") == 0) return MDD_OK;  // unused in eval
    size_t n = 1;
    for (int i = 0; i < ndim; i++) { if (shape[i] < 0) { set_error("negative dim"); return MDD_ERR_ARG; } n *= (size_t)shape[i]; }
    m->host[k].assign(data, data + n);
    m->finalized = false;
    return MDD_OK;
}

// Builds a whole new weight set, then swaps it in.  On failure the handle is left not finalized, still holding no pointer to freed memory.
extern "C" int mdd_finalize_weights(mdd_model *m) {
    if (!m) { set_error("null model"); return MDD_ERR_ARG; }
    m->finalized = false;
    MDD_HIP_CHECK(hipSetDevice(m->device));
    std::unique_ptr<DecodeWeights> w(new DecodeWeights());
    if (int rc = build_weights(m, *w)) return rc;
    m->drop_graphs();                         // captured graphs bake the old set's pointers
    MDD_HIP_CHECK(hipDeviceSynchronize());    // (also: no forward still reads the old set)
    m->weights.swap(w);
    m->finalized = true;
    return MDD_OK;
}

extern "C" int mdd_enable_taps(mdd_model *m, int32_t on) {
    if (!m) return MDD_ERR_ARG;
    m->taps = on != 0;
    m->drop_graphs();
    return MDD_OK;
}

extern "C" int mdd_set_precision(mdd_model *m, int32_t mode) {
    if (!m || mode < 0 || mode > 2) { set_error("mdd_set_precision: mode must be 0 (fp32 MFMA), 1 (split-bf16 x3) or 2 (f32x6 projections)"); return MDD_ERR_ARG; }
    if (m->precision != mode) {
        m->precision = mode;
        m->drop_graphs();
    }
    return MDD_OK;
}
extern "C" int32_t mdd_get_precision(mdd_model *m) { return m ? plan_of(m, 1).precision : -1; }   // (the same for every batch size)

extern "C" int mdd_stack_skip(const float *raw_dev, int32_t B, int32_t T_raw, int32_t D, int32_t right, int32_t skip,
                              int32_t n_down, float *out_dev, void *stream) {
    if (!raw_dev || !out_dev) { set_error("mdd_stack_skip: null pointer"); return MDD_ERR_ARG; }
    return launch_stack_skip(raw_dev, B, T_raw, D, right, skip, n_down, out_dev, (hipStream_t)stream);
}

static int forward_prepare(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L, float *logp_dev) {
    if (!m || !x_dev || !x1_dev || !logp_dev) { set_error("mdd_forward: null pointer"); return MDD_ERR_ARG; }
    if (!m->finalized) { set_error("mdd_forward: call mdd_finalize_weights first"); return MDD_ERR_STATE; }
    if (B <= 0 || T < 2 || L <= 0) { set_error("mdd_forward: bad shape B=%d T=%d L=%d", B, T, L); return MDD_ERR_ARG; }
    if (T % 2) { set_error("mdd_forward: T must be even (data_loader.py:140-142 pads to n_downsample)"); return MDD_ERR_ARG; }
    MDD_HIP_CHECK(hipSetDevice(m->device));
    std::lock_guard<std::mutex> prep_lock(g_prep_mu);
    hipStream_t zs = m->cap_stream;
    const mdd_config &c = m->cfg;
    const int H = c.hidden, Tp = T / 2;
    const ForwardPlan p = plan_of(m, B);
    int rc;
    const size_t rows = (size_t)Tp * B, trows = (size_t)L * B, mrows = rows > trows ? rows : trows;
    if ((p.conv == Conv::Separate && (rc = ensure(m->y0, (size_t)B * c.channels * T * m->W1(), zs))) || (rc = ensure(m->seq0, rows * m->rnn_in(), zs)) ||
        (rc = ensure(m->gx, mrows * 8 * H, zs)) || (rc = ensure(m->act[0], rows * 2 * H, zs)) || (rc = ensure(m->act[1], rows * 2 * H, zs)) ||
        (rc = ensure(m->xraw, rows * 2 * H, zs)) || (rc = ensure(m->hbuf, (size_t)4 * ((B + 15) / 16 * 16) * H, zs)) || (rc = ensure(m->cbuf, (size_t)2 * ((B + 15) / 16 * 16) * H, zs)) ||
        (rc = ensure(m->embo, trows * c.emb_dim, zs)) || (rc = ensure(m->text, trows * 2 * H, zs)) || (rc = ensure(m->key, trows * 2 * H, zs)) ||
        (rc = ensure(m->S, (size_t)B * Tp * L, zs)))
        return rc;
    if (p.precision == 1 && ((rc = ensure(m->seq0_s, rows * m->rnn_in(), zs)) || (rc = ensure(m->act_s[0], rows * 2 * H, zs)) ||
                             (rc = ensure(m->act_s[1], rows * 2 * H, zs)) || (rc = ensure(m->x_s, rows * 2 * H, zs)) ||
                             (rc = ensure(m->embo_s, trows * c.emb_dim, zs)) || (rc = ensure(m->text_s, trows * 2 * H, zs)) ||
                             (rc = ensure(m->key_s, trows * 2 * H, zs)) || (rc = ensure(m->hsplit, (size_t)4 * B * H, zs))))
        return rc;
    {   // f32x6: three bf16 planes of the largest projection operand = 1.5 x its fp32 size (in floats: 3/2)
        const size_t kmax = (size_t)(m->rnn_in() > 2 * H ? m->rnn_in() : 2 * H), k2 = (size_t)c.emb_dim;
        const size_t need = (rows * kmax > trows * k2 ? rows * kmax : trows * k2) * 3 / 2 + 64;
        if (p.proj == Gemm::F32x6 && (rc = ensure(m->p3, need, zs))) return rc;
    }
    if (p.hx_floats && (rc = ensure(m->hx, p.hx_floats, zs))) return rc;   // the exchange buffer of the persistent layers + stamps
    if (m->taps) {
        m->tap_rnn.resize(c.layers);
        for (int n = 0; n + 1 < c.layers; n++) if ((rc = ensure(m->tap_rnn[n], rows * 2 * H, zs))) return rc;
    }
    m->lastB = B; m->lastT = T; m->lastL = L;
    m->plan = p;
    if (g_ws_moved) {   // hipFree above synchronised the device, so no replay of an old graph is still running
        m->drop_graphs();
        g_ws_moved = false;
    }
    return MDD_OK;
}

extern "C" int mdd_forward(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                           float *logp_dev, void *stream) {
    int rc = forward_prepare(m, x_dev, B, T, x1_dev, L, logp_dev);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool gated = m->plan.gated;
    bool held = false;
    if (!m->sw.graph) {
        if (gated && (rc = gate_enter(m, st, &held))) return rc;
        rc = forward_enqueue(m, x_dev, B, T, x1_dev, L, logp_dev, st);
        return gate_leave(m, st, held, rc);
    }
    GraphKey key;
    memset(&key, 0, sizeof(key));
    key.x = x_dev; key.x1 = x1_dev; key.out = logp_dev; key.B = B; key.T = T; key.L = L; key.Traw = m->raw_T; key.tlen = m->tlen; key.llen = m->llen;
    auto it = m->graphs.find(key);
    if (it == m->graphs.end()) {
        if (m->graphs.size() >= 8) m->drop_graphs();
        hipGraph_t graph = nullptr;
        std::lock_guard<std::mutex> prep_lock(g_prep_mu);
        MDD_HIP_CHECK(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeRelaxed));
        rc = forward_enqueue(m, x_dev, B, T, x1_dev, L, logp_dev, m->cap_stream);
        hipError_t e = hipStreamEndCapture(m->cap_stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) { set_error("graph capture failed: %s", hipGetErrorString(e)); return MDD_ERR_HIP; }
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { set_error("graph instantiate failed: %s", hipGetErrorString(e)); return MDD_ERR_HIP; }
        it = m->graphs.emplace(key, exec).first;
    }
    if (gated && (rc = gate_enter(m, st, &held))) return rc;
    hipError_t le = hipGraphLaunch(it->second, st);
    if (le != hipSuccess) { set_error("hipGraphLaunch failed: %s", hipGetErrorString(le)); return gate_leave(m, st, held, MDD_ERR_HIP); }
    return gate_leave(m, st, held, MDD_OK);
}

// Several reference batches of DIFFERENT padded lengths in one launch sequence.  The reference pads every batch to its own
// maximum and masks nothing (AA/models/model_ctc.py:186,198,204-205), so an utterance's posteriors depend on its batch's
// padded length T_g and canonical length L_g: rows of batch g carry frames_dev[b] = T_g / 2 and canon_dev[b] = L_g.  What
// depends on the batch's length -- where the reverse BiLSTM direction starts (frame T_g/2 - 1 / token L_g - 1, zero state) and
// which keys the attention softmax runs over (l < L_g) -- follows those per-row values; everything else is row-local.  x_dev
// [B, T, F] is zero beyond each batch's T_g (as the collate's zero padding leaves it), x1_dev [B, L] is zero-padded.  Rows
// t >= frames_dev[b] of logp_dev are not meaningful.  Results for every utterance are bit-identical to running its batch alone.
extern "C" int mdd_forward_fused(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                                 const int32_t *frames_dev, const int32_t *canon_dev, float *logp_dev, void *stream) {
    if (!m || !frames_dev || !canon_dev) { set_error("mdd_forward_fused: null pointer"); return MDD_ERR_ARG; }
    m->tlen = frames_dev; m->llen = canon_dev;
    const int rc = mdd_forward(m, x_dev, B, T, x1_dev, L, logp_dev, stream);
    m->tlen = nullptr; m->llen = nullptr;
    return rc;
}

// A1 + forward in one call: raw_dev = unstacked frames [B, T_raw, feat/3].  With the fused conv front-end the stack/skip
// is only an index map inside its x-tile load (no [B,T,243] copy at all); otherwise a stacked copy is made first.
extern "C" int mdd_forward_raw(mdd_model *m, const float *raw_dev, int32_t B, int32_t T_raw, const int64_t *x1_dev, int32_t L,
                               float *logp_dev, void *stream) {
    if (!m || !raw_dev || B <= 0 || T_raw < 1) { set_error("mdd_forward_raw: bad argument"); return MDD_ERR_ARG; }
    const int D = m->cfg.feat / 3, T = mdd_stack_len(T_raw, 2, 2);
    if (m->cfg.feat != 3 * D) { set_error("mdd_forward_raw: feat=%d is not 3 stacked frames", m->cfg.feat); return MDD_ERR_ARG; }
    if (m->finalized && plan_of(m, B).conv != Conv::Separate) {
        m->raw_T = T_raw;
        const int rc = mdd_forward(m, raw_dev, B, T, x1_dev, L, logp_dev, stream);
        m->raw_T = 0;
        return rc;
    }
    MDD_HIP_CHECK(hipSetDevice(m->device));
    {
        std::lock_guard<std::mutex> prep_lock(g_prep_mu);
        if (int rc = ensure(m->xstack, (size_t)B * T * m->cfg.feat, m->cap_stream)) return rc;
    }
    if (g_ws_moved) { m->drop_graphs(); g_ws_moved = false; }
    if (int rc = mdd_stack_skip(raw_dev, B, T_raw, D, 2, 2, 2, m->xstack.p, stream)) return rc;
    return mdd_forward(m, m->xstack.p, B, T, x1_dev, L, logp_dev, stream);
}

extern "C" int32_t mdd_forward_num_stages(mdd_model *m) { return m ? n_stages(m) : 0; }

extern "C" int mdd_forward_profile(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                                   float *logp_dev, void *stream, char *names, int32_t names_cap, float *ms,
                                   int32_t *launches, double *flops, int32_t cap) {
    int rc = forward_prepare(m, x_dev, B, T, x1_dev, L, logp_dev);
    if (rc) return rc;
    const int ns = n_stages(m);
    if (cap < ns || !ms || !launches || !flops || !names) { set_error("mdd_forward_profile: need room for %d stages", ns); return MDD_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    if (m->plan.gated) {   // keep other handles' forwards off the device while the stages replay: wait for the last gated forward
        bool held = false;
        if ((rc = gate_enter(m, st, &held))) return rc;
        if ((rc = gate_leave(m, st, held, MDD_OK))) return rc;
    }
    hipEvent_t e0, e1;
    MDD_HIP_CHECK(hipEventCreate(&e0));
    MDD_HIP_CHECK(hipEventCreate(&e1));
    std::string all;
    for (int si = 0; si < ns; si++) {
        Stage info;
        hipGraph_t graph = nullptr;
        std::unique_lock<std::mutex> prep_lock(g_prep_mu);
        MDD_HIP_CHECK(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeRelaxed));
        rc = run_stage(m, si, x_dev, B, T, x1_dev, L, logp_dev, m->cap_stream, &info);
        hipError_t e = hipStreamEndCapture(m->cap_stream, &graph);
        prep_lock.unlock();
        if (rc || e != hipSuccess) { if (graph) (void)hipGraphDestroy(graph); if (!rc) set_error("stage capture failed"); return rc ? rc : MDD_ERR_HIP; }
        if (info.launches == 0) {   // stage folded into a neighbour in this configuration
            (void)hipGraphDestroy(graph);
            ms[si] = 0.f; launches[si] = 0; flops[si] = 0.0;
            if (si) all += ",";
            all += info.name;
            continue;
        }
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { set_error("stage instantiate failed: %s", hipGetErrorString(e)); return MDD_ERR_HIP; }
        MDD_HIP_CHECK(hipGraphLaunch(exec, st));          // warm (first replay pays upload)
        MDD_HIP_CHECK(hipStreamSynchronize(st));
        MDD_HIP_CHECK(hipEventRecord(e0, st));
        MDD_HIP_CHECK(hipGraphLaunch(exec, st));
        MDD_HIP_CHECK(hipEventRecord(e1, st));
        MDD_HIP_CHECK(hipEventSynchronize(e1));
        float t = 0.f;
        MDD_HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        (void)hipGraphExecDestroy(exec);
        ms[si] = t; launches[si] = info.launches; flops[si] = info.flops;
        if (si) all += ",";
        all += info.name;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    snprintf(names, names_cap, "%s", all.c_str());
    return MDD_OK;
}

extern "C" const float *mdd_tap(mdd_model *m, const char *name, int64_t *numel) {
    if (!m || !name || !m->lastB) return nullptr;
    const int Tp = m->lastT / 2, B = m->lastB, L = m->lastL, H2 = 2 * m->cfg.hidden;
    std::string n(name);
    const float *p = nullptr;
    int64_t ne = 0;
    if (m->plan.precision == 1 && (n == "conv1" || n == "key")) {   // these stages exist only as split-bf16 planes: rebuild fp32 = hi + lo
        const bool cv = n == "conv1";
        ne = cv ? (int64_t)Tp * B * m->rnn_in() : (int64_t)L * B * H2;
        DeviceBuf &dst = cv ? m->seq0 : m->key;
        if (launch_unsplit(split_view(cv ? m->seq0_s : m->key_s, (size_t)ne), (size_t)ne, dst.p, nullptr) != MDD_OK) return nullptr;
        if (hipStreamSynchronize(nullptr) != hipSuccess) return nullptr;
        p = dst.p;
    }
    else if (n == "lstm_dbg" && m->plan.gated) {   // diagnostic stamps of the last persistent layer launch (MDD_LSTM_DBG=1)
        p = m->hx.p + m->plan.stamps_at;
        ne = 256 * 6 * 2;
    }
    else if (n == "conv1") { p = m->seq0.p; ne = (int64_t)Tp * B * m->rnn_in(); }
    else if (n == "text") { p = m->text.p; ne = (int64_t)L * B * H2; }
    else if (n == "key") { p = m->key.p; ne = (int64_t)L * B * H2; }
    else if (n.compare(0, 3, "rnn") == 0) {
        int i = atoi(n.c_str() + 3);
        if (i == m->cfg.layers - 1) { p = m->xraw.p; ne = (int64_t)Tp * B * H2; }
        else if (m->taps && i >= 0 && i < (int)m->tap_rnn.size()) { p = m->tap_rnn[i].p; ne = (int64_t)Tp * B * H2; }
    }
    if (numel) *numel = ne;
    return p;
}

extern "C" int mdd_tap_copy(mdd_model *m, const char *name, float *dst_dev, int64_t capacity, void *stream) {
    int64_t n = 0;
    const float *p = mdd_tap(m, name, &n);
    if (!p || !dst_dev) { set_error("mdd_tap_copy: no tap named '%s' (taps enabled?)", name ? name : "(null)"); return MDD_ERR_ARG; }
    if (capacity < n) { set_error("mdd_tap_copy: capacity %lld < %lld", (long long)capacity, (long long)n); return MDD_ERR_ARG; }
    MDD_HIP_CHECK(hipMemcpyAsync(dst_dev, p, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MDD_OK;
}

extern "C" int mdd_sync(mdd_model *m, void *stream) {
    if (!m) { set_error("null model"); return MDD_ERR_ARG; }
    MDD_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    int flag = 0;
    MDD_HIP_CHECK(hipMemcpy(&flag, m->err_flag.p, sizeof(int), hipMemcpyDeviceToHost));
    if (flag == 2) {
        MDD_HIP_CHECK(hipMemset(m->err_flag.p, 0, sizeof(int)));
        set_error("persistent BiLSTM kernel timed out waiting for its team (grid not fully resident?); set MDD_LSTM=step");
        return MDD_ERR_HIP;
    }
    if (flag) {
        MDD_HIP_CHECK(hipMemset(m->err_flag.p, 0, sizeof(int)));
        set_error("index out of range in self");  // the message of the IndexError nn.Embedding raises
        return MDD_ERR_ARG;
    }
    return MDD_OK;
}

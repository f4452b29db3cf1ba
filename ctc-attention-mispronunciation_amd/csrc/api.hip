// C-ABI of libmdd_hip.so: handle lifetime, the device gate, workspace, forward orchestration, profile, taps (include/mdd_hip.h).
// The handle itself is model.h; its weights are built in weights.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <mutex>

#include "model.h"

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

// a DeviceBuf of n floats holds a split tensor of n elements: hi plane then lo plane
static SplitPtr split_view(const DeviceBuf &b, size_t n) {
    SplitPtr s; s.hi = reinterpret_cast<unsigned short *>(b.p); s.lo = s.hi ? s.hi + n : nullptr; return s;
}
static const SplitPtr kNoSplit = {nullptr, nullptr};
static unsigned short *as_u16(const DeviceBuf &b) { return reinterpret_cast<unsigned short *>(b.p); }

// Workspace growth (hipFree / hipMalloc / clearing) and stream capture exclude each other process-wide: a capture in
// progress on one host thread makes another thread's allocation-time calls fail ("operation would make the legacy
// stream depend on a capturing stream").  Both are rare (first call of a shape); graph REPLAYS never take this lock.
static std::mutex g_prep_mu;

// Grow a workspace buffer to n floats, cleared.  *moved is set when it was reallocated: captured graphs hold its old address.
static int ensure(DeviceBuf &b, size_t n, hipStream_t zero_stream, bool *moved) {
    if (b.cap >= n) return MDD_OK;
    *moved = true;
    if (int rc = b.need(n)) return rc;
    b.cap = 0;   // grown only once cleared
    MDD_HIP_CHECK(hipMemsetAsync(b.p, 0, n * sizeof(float), zero_stream));  // padded batch rows of the packed h exchange must be finite
    MDD_HIP_CHECK(hipStreamSynchronize(zero_stream));
    b.cap = n;
    return MDD_OK;
}

// The kernels a forward of B rows runs on this handle as it stands now (plan.h)
static ForwardPlan plan_of(const mdd_model *m, int B) { return plan_forward(m->cfg, m->precision, m->sw, m->fit, B, m->ctc_only); }

// One BiLSTM layer: the caller sets a.T, a.B, a.seqlen and the outputs, the rest is filled here.  The persistent layer kernel where
// the plan has one (f32x6, split-bf16 or exact-fp32 teams), else one launch per step (launch_lstm_layer: hsplit selects the x3 step).
static int run_lstm(mdd_model *m, const LstmWeights &lw, LstmStepArgs a, hipStream_t st) {
    const ForwardPlan &p = m->plan;
    a.gx = m->gx.p; a.whh = lw.whh; a.hbuf = m->hbuf.p; a.cbuf = m->cbuf.p;
    a.H = m->cfg.hidden; a.packed = packed_whh(m->cfg);
    a.whh_split = lw.whh_s; a.hsplit = p.lstm == Lstm::StepX3 ? as_u16(m->hsplit) : nullptr;
    if (!p.gated) return launch_lstm_layer(a, st);
    unsigned short *hx = as_u16(m->hx);
    long long *stamps = m->sw.lstm_dbg && a.T > 100 ? reinterpret_cast<long long *>(m->hx.p + p.stamps_at) : nullptr;
    if (p.lstm == Lstm::X6) return launch_lstm_layer_x6(a, lw.whh_3, hx, m->sync_words.p, m->err_flag.p, st, stamps, m->sw.x6_redo_mask);
    if (p.lstm == Lstm::Granule) return launch_lstm_layer_granule(a, hx, m->sync_words.p, m->err_flag.p, st, stamps, m->sw.lstm_early);
    return launch_lstm_layer_f32(a, hx, m->sync_words.p, m->err_flag.p, st, stamps);
}

// A layer that hands on its raw h (the last BiLSTM layer: the queries; the text encoder): fp32 for the tail, split planes for the mode-1 GEMMs.
static LstmStepArgs lstm_raw_out(int T, int B, const int *seqlen, float *out, SplitPtr split) {
    LstmStepArgs a;
    a.T = T; a.B = B; a.seqlen = seqlen; a.out = out; a.out_raw = out; a.out_split = split;
    return a;
}
// BiLSTM layer n < layers - 1: the next layer's BatchNorm folded into the store, in the form the next projection reads.
static LstmStepArgs lstm_folded_out(mdd_model *m, int n, int T, int B, const int *seqlen) {
    const ForwardPlan &p = m->plan;
    const bool x3 = p.precision == 1;
    const size_t n_out = (size_t)T * B * 2 * m->cfg.hidden;
    LstmStepArgs a;
    a.T = T; a.B = B; a.seqlen = seqlen;
    a.out = x3 || p.planes_out ? nullptr : m->act[n & 1].p; a.out_raw = m->taps ? m->tap_rnn[n].p : nullptr;
    if (p.planes_out) {   // straight into the next projection's operand buffer (gemm_ih<n> has read it: same stream, stages in order)
        a.out_planes = as_u16(m->p3); a.out_planes_stride = n_out;
    }
    a.out_split = x3 ? split_view(m->act_s[n & 1], n_out) : kNoSplit;
    a.oscale = m->weights->rnn[n + 1].scale; a.oshift = m->weights->rnn[n + 1].shift;
    return a;
}

// The input projection of one BiLSTM (gemm_ih<n>, gemm_text): gx[rows, 8H] = in[rows, K] . W_ih'^T (+ bias) in the plan's arithmetic.
// The operand is fp32, or in mode 1 its split-bf16 planes; planes_written (f32x6): its producer has left the three bf16 planes in p3 already.
struct ProjIn { const float *f32; SplitPtr split; bool planes_written; };
static int project(mdd_model *m, const ProjIn &in, int rows, int K, const LstmWeights &lw, const float *bias, hipStream_t st) {
    const int G2 = 8 * m->cfg.hidden;
    if (m->plan.proj == Gemm::Bf16x3) return launch_gemm_bf16x3({.p = in.split, .ld = K}, {.p = lw.wih_s, .ld = K}, m->gx.p, nullptr, G2, rows, G2, K, st, {.bias = bias});
    if (m->plan.proj == Gemm::F32x6) {   // fp32-grade arithmetic at 6/16 of the fp32 MFMA's cost (gemm_bf16x6.hip)
        if (!in.planes_written)
            if (int rc = launch_split3(in.f32, rows, K, K, as_u16(m->p3), st)) return rc;
        return launch_gemm_f32x6(as_u16(m->p3), (size_t)rows * K, lw.wih_3, (size_t)G2 * K, bias, m->gx.p, rows, G2, K, G2, st, m->sw.x6_raster, nullptr, m->sw.x6_rt);
    }
    return launch_gemm_nt({.p = in.f32, .ld = K}, {.p = lw.wih, .ld = K}, m->gx.p, G2, rows, G2, K, st, {.bias = bias});
}

// One stage of the forward: one or more kernel launches (none where a neighbour has absorbed it in this configuration); run enqueues it.
struct Stage { std::string name; int launches; double flops; std::function<int(hipStream_t)> run; };

// The forward of `call` under the handle's prepared plan, top to bottom as the model reads.  Built only where it is consumed: a capture,
// the stage-by-stage enqueue under MDD_GRAPH=0 and mdd_forward_profile's replay between HIP events; never for the replay of a captured graph.
static std::vector<Stage> forward_stages(mdd_model *m, const ForwardCall &call) {
    const mdd_config &c = m->cfg;
    const DecodeWeights *w = m->weights.get();
    const ForwardPlan p = m->plan;
    const float *x = call.x;
    const int B = call.B, T = call.T, L = call.L, Traw = call.Traw, Tp = T / 2, Lp = L;
    const int Bt = call.K * B;   // rows of the text side: candidate set k's canonical of utterance b is text row k * B + b (K = 1: the utterances themselves)
    const int H = c.hidden, H2 = 2 * H, ch = c.channels, E = c.emb_dim, K0 = m->rnn_in(), nl = c.layers;
    const bool x3 = p.precision == 1, fused = p.conv != Conv::Separate;   // x3: the activations travel as split-bf16 planes
    const size_t rows = (size_t)Tp * B, trows = (size_t)L * Bt;
    const auto split = [x3](const DeviceBuf &b, size_t n) { return x3 ? split_view(b, n) : kNoSplit; };
    const double step_flops = 2.0 * 2 * (double)B * H * 4 * H, tstep_flops = step_flops * call.K;   // one step of a BiLSTM layer, of the text encoder
    std::vector<Stage> s;

    if (fused) {   // conv0 recomputed per output row (x1.5) + conv1 as implicit GEMM, one kernel
        s.push_back({"conv_fused", 1, 2.0 * 9 * ch * (double)B * Tp * m->W2() * (ch + 6.0), [=](hipStream_t st) {
            if (p.conv == Conv::FusedX3)
                return launch_conv_fused(x, w->w_conv0, w->sc0, w->sh0, w->w_conv1_s, w->sc1, w->sh1, split_view(m->seq0_s, rows * K0), nullptr, B, T, Traw, st);
            // fp32-grade form: three K-tile-major planes straight into the projection GEMM's operand buffer
            return launch_conv_fused3(x, w->w_conv0, w->sc0, w->sh0, w->w_conv1_3, w->sc1, w->sh1, as_u16(m->p3), m->taps ? m->seq0.p : nullptr, B, T, Traw, st,
                                      p.conv == Conv::FusedX6Rowwise);
        }});
        s.push_back({"conv1_in_fused", 0, 0.0, [](hipStream_t) { return (int)MDD_OK; }});
    } else {
        s.push_back({"conv0", 1, 2.0 * 9 * ch * (double)B * T * m->W1(), [=](hipStream_t st) {
            return launch_conv0(x, w->w_conv0, w->sc0, w->sh0, m->y0.p, B, T, c.feat, ch, st);
        }});
        s.push_back({"conv1", 1, 2.0 * 9 * ch * ch * (double)B * Tp * m->W2(), [=](hipStream_t st) {
            return launch_conv1(m->y0.p, w->w_conv1t, w->sc1, w->sh1, x3 ? nullptr : m->seq0.p, split(m->seq0_s, rows * K0), B, T, m->W1(), ch, st);
        }});
    }

    for (int n = 0; n < nl; n++) {   // the BiLSTM layers
        const LstmWeights *lw = &w->rnn[n];
        const int K = n == 0 ? K0 : H2;
        // (layer 0: the fused front-end has written the planes; layers >= 1: the layer kernel before, where the plan says so)
        const ProjIn in = n == 0 ? ProjIn{m->seq0.p, split(m->seq0_s, rows * K), fused}
                                 : ProjIn{m->act[(n - 1) & 1].p, split(m->act_s[(n - 1) & 1], rows * K), p.planes_out};
        s.push_back({"gemm_ih" + std::to_string(n), 1, 2.0 * (double)Tp * B * 8 * H * K, [=](hipStream_t st) {
            return project(m, in, Tp * B, K, *lw, nullptr, st);
        }});
        const LstmStepArgs a = n == nl - 1 ? lstm_raw_out(Tp, B, call.tlen, m->xraw.p, split(m->x_s, rows * H2)) : lstm_folded_out(m, n, Tp, B, call.tlen);
        s.push_back({"lstm" + std::to_string(n), p.gated ? 1 : Tp, step_flops * Tp, [=](hipStream_t st) { return run_lstm(m, *lw, a, st); }});
    }

    if (m->ctc_only) {   // the CTC-only model ends here: the classifier on the last layer's raw output (CRC/models/cnn_rnn.py:168-172)
        s.push_back({"ctc_tail", 1, 2.0 * (double)rows * H2 * c.num_class, [=](hipStream_t st) {
            return launch_ctc_tail(m->xraw.p, w->fscale, w->fshift, w->w_fc, w->w_fcp, call.logp, Tp * B, H2, c.num_class, st);
        }});
        return s;
    }

    const LstmWeights *tw = &w->rnn[nl];   // the text encoder (model_ctc.py:193,198) and keys (:201)
    // Its input projection multiplies two weights: emb[id] . W_ih'^T + bias is one of emb_rows constant rows.  Where the plan says so the two
    // stages are the id check with the row indices, and a gather from the weight set's table of those rows; gemm_text keeps the flops of the
    // product it stands for (bench.py's roofline counts them).
    const float *table = p.text_table ? w->text_table[p.proj == Gemm::F32x6] : nullptr;
    int *tidx = reinterpret_cast<int *>(m->tidx.p);
    s.push_back({"embed", 1, 0.0, [=](hipStream_t st) {
        if (table) return launch_embed_index(c.emb_rows, call.x1, Bt, L, tidx, m->err_flag.p, st);
        return launch_embed(w->emb, c.emb_rows, E, call.x1, Bt, L, x3 ? nullptr : m->embo.p, split(m->embo_s, trows * E), m->err_flag.p, st);
    }});
    s.push_back({"gemm_text", 1, 2.0 * (double)L * Bt * 8 * H * E, [=](hipStream_t st) {
        if (table) return launch_gather_rows(table, tidx, m->gx.p, L * Bt, 8 * H, st);
        return project(m, ProjIn{m->embo.p, split(m->embo_s, trows * E), false}, L * Bt, E, *tw, w->t_bias, st);
    }});
    const LstmStepArgs ta = lstm_raw_out(L, Bt, call.llen, m->text.p, split(m->text_s, trows * H2));
    s.push_back({"lstm_text", p.gated ? 1 : L, tstep_flops * L, [=](hipStream_t st) { return run_lstm(m, *tw, ta, st); }});
    s.push_back({"gemm_key", 1, 2.0 * (double)L * Bt * H2 * H2, [=](hipStream_t st) {
        if (x3) {
            const SplitPtr ks = split_view(m->key_s, trows * H2);
            return launch_gemm_bf16x3({.p = split_view(m->text_s, trows * H2), .ld = H2}, {.p = w->w_score_s, .ld = H2}, nullptr, &ks, H2, L * Bt, H2, H2, st);
        }
        return launch_gemm_nt({.p = m->text.p, .ld = H2}, {.p = w->w_score, .ld = H2}, m->key.p, H2, L * Bt, H2, H2, st);
    }});
    // scores S[j][t][l] = X[t, j % B, :] . key[l, j, :]   (:204): one product per text row; with candidates the X operand repeats with period B
    const int xperiod = call.K > 1 ? B : 0;
    s.push_back({"gemm_score", 1, 2.0 * (double)Bt * Tp * L * H2, [=](hipStream_t st) {
        const GemmOpts per_row{.batch = Bt, .sC = (long)Tp * Lp};
        if (x3) return launch_gemm_bf16x3({.p = split_view(m->x_s, rows * H2), .ld = B * H2, .stride = H2, .period = xperiod},
                                          {.p = split_view(m->key_s, trows * H2), .ld = Bt * H2, .stride = H2}, m->S.p, nullptr, Lp, Tp, L, H2, st, per_row);
        return launch_gemm_nt({.p = m->xraw.p, .ld = B * H2, .stride = H2, .period = xperiod}, {.p = m->key.p, .ld = Bt * H2, .stride = H2}, m->S.p, Lp, Tp, L, H2, st,
                              per_row, m->sw.score_wide);
    }});
    s.push_back({"attn_tail", 1, 2.0 * (double)Bt * Tp * ((double)L * H2 + 2.0 * H2 * c.num_class), [=](hipStream_t st) {
        return launch_attn_tail(m->S.p, Lp, m->xraw.p, m->text.p, w->fscale, w->fshift, w->w_fc, w->w_fcp, call.logp, Tp, Bt, L, H2, c.num_class, st, call.llen, B);
    }});
    return s;
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

}  // namespace mdd

using namespace mdd;

extern "C" const char *mdd_last_error(void) { return g_err; }
extern "C" int mdd_version(void) { return 100; }

// mdd_create and mdd_create_ctc: `what` names the entry point in messages, the geometry contract is the one thing that differs
static int create_handle(const char *what, bool ctc_only, const mdd_config *cfg, int device, mdd_model **out) {
    if (!cfg || !out) { set_error("%s: null argument", what); return MDD_ERR_ARG; }
    if (const char *why = ctc_only ? ctc_geometry_error(*cfg) : geometry_error(*cfg)) { set_error("%s: unsupported geometry: %s", what, why); return MDD_ERR_ARG; }
    int ndev = 0;
    MDD_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_error("%s: device %d of %d", what, device, ndev); return MDD_ERR_ARG; }
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
    m->ctc_only = ctc_only;
    m->sw = read_switches();
    m->precision = m->sw.precision;
    for (auto init : {init_kernel_attributes, init_lstm_attributes, init_granule_attributes, init_lstm_bwd_attributes, init_lstm_f32_attributes, init_lstm_x6_attributes,
                      init_conv_attributes, init_gemm_attributes, init_gemm_x6_attributes})
        if (int rc = init()) return rc;
    const int n_cu = prop.multiProcessorCount;   // (where a grid does not fit: per-step kernels, e.g. smaller partitions, other gfx950 SKUs)
    m->fit = {persistent_grid_fits(n_cu) != 0, persistent_f32_grid_fits(n_cu) != 0, persistent_x6_grid_fits(n_cu) != 0};
    if (int rc = m->err_flag.need(1)) return rc;
    if (int rc = m->sync_words.need(32)) return rc;
    hipError_t e = hipMemset(m->err_flag.p, 0, sizeof(int));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return MDD_ERR_HIP; }
    *out = m.release();
    return MDD_OK;
}

extern "C" int mdd_create(const mdd_config *cfg, int device, mdd_model **out) { return create_handle("mdd_create", false, cfg, device, out); }
extern "C" int mdd_create_ctc(const mdd_config *cfg, int device, mdd_model **out) { return create_handle("mdd_create_ctc", true, cfg, device, out); }
extern "C" int32_t mdd_is_ctc_only(mdd_model *m) { return m && m->ctc_only ? 1 : 0; }

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
    if (m->ctc_only)
        if (int rc = check_ctc_entry(m, k, shape, ndim)) return rc;
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
    m->graphs.clear();                         // captured graphs bake the old set's pointers
    MDD_HIP_CHECK(hipDeviceSynchronize());    // (also: no forward still reads the old set)
    m->weights.swap(w);
    m->finalized = true;
    return MDD_OK;
}

extern "C" int mdd_enable_taps(mdd_model *m, int32_t on) {
    if (!m) return MDD_ERR_ARG;
    m->taps = on != 0;
    m->graphs.clear();
    return MDD_OK;
}

extern "C" int mdd_set_precision(mdd_model *m, int32_t mode) {
    if (!m || mode < 0 || mode > 2) { set_error("mdd_set_precision: mode must be 0 (fp32 MFMA), 1 (split-bf16 x3) or 2 (f32x6 projections)"); return MDD_ERR_ARG; }
    if (m->precision != mode) {
        m->precision = mode;
        m->graphs.clear();
    }
    return MDD_OK;
}
extern "C" int32_t mdd_get_precision(mdd_model *m) { return m ? plan_of(m, 1).precision : -1; }   // (the same for every batch size)

extern "C" int mdd_stack_skip(const float *raw_dev, int32_t B, int32_t T_raw, int32_t D, int32_t right, int32_t skip,
                              int32_t n_down, float *out_dev, void *stream) {
    if (!raw_dev || !out_dev) { set_error("mdd_stack_skip: null pointer"); return MDD_ERR_ARG; }
    return launch_stack_skip(raw_dev, B, T_raw, D, right, skip, n_down, out_dev, (hipStream_t)stream);
}

static int forward_enqueue(mdd_model *m, const ForwardCall &call, hipStream_t st) {
    for (const Stage &s : forward_stages(m, call))
        if (int rc = s.run(st)) return rc;
    return MDD_OK;
}

// Capture what `enqueue` puts on the handle's capture stream into an executable graph (`what` names it in the error message).
static int capture(mdd_model *m, const char *what, const std::function<int(hipStream_t)> &enqueue, GraphExec *exec) {
    std::lock_guard<std::mutex> prep_lock(g_prep_mu);
    Graph graph;
    MDD_HIP_CHECK(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeRelaxed));
    const int rc = enqueue(m->cap_stream);
    hipError_t e = hipStreamEndCapture(m->cap_stream, &graph.h);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("%s capture failed: %s", what, hipGetErrorString(e)); return MDD_ERR_HIP; }
    e = hipGraphInstantiate(&exec->h, graph.h, nullptr, nullptr, 0);
    if (e != hipSuccess) { set_error("%s instantiate failed: %s", what, hipGetErrorString(e)); return MDD_ERR_HIP; }
    return MDD_OK;
}

// Check the arguments every forward shares, pick the kernels for its batch size (m->plan) and grow the workspace to its shape.  The one
// place that drops the captured graphs because a workspace buffer moved.
static int prepare(mdd_model *m, const ForwardCall &call) {
    const int B = call.B, T = call.T, L = call.L;
    if (!m || !call.x || !call.logp) { set_error("mdd_forward: null pointer"); return MDD_ERR_ARG; }
    const bool ctc = m->ctc_only;   // (its calls come with x1 = null and L = 0: plain_call)
    if (!ctc && !call.x1) { set_error("mdd_forward: null pointer"); return MDD_ERR_ARG; }
    if (!m->finalized) { set_error("mdd_forward: call mdd_finalize_weights first"); return MDD_ERR_STATE; }
    if (B <= 0 || T < 2 || (!ctc && L <= 0)) { set_error("mdd_forward: bad shape B=%d T=%d L=%d", B, T, L); return MDD_ERR_ARG; }
    if (call.K < 1 || (long long)call.K * B > (1 << 24)) { set_error("mdd_forward: bad candidate count K=%d (B=%d)", call.K, B); return MDD_ERR_ARG; }
    if (T % 2) { set_error("mdd_forward: T must be even (data_loader.py:140-142 pads to n_downsample)"); return MDD_ERR_ARG; }
    MDD_HIP_CHECK(hipSetDevice(m->device));
    std::lock_guard<std::mutex> prep_lock(g_prep_mu);
    const mdd_config &c = m->cfg;
    // Candidates: the whole call runs under the plan of its K * B text rows, acoustic stages included.  Every condition plan_forward puts on the
    // row count is an upper bound, so the B acoustic rows are valid under it, and they get the kernels they would get in the repeated batch.
    const int Bt = call.K * B;
    const int H = c.hidden, Tp = T / 2, K0 = m->rnn_in(), Bpad = (Bt + 15) / 16 * 16;
    const ForwardPlan p = plan_of(m, Bt);
    const size_t rows = (size_t)Tp * B, trows = (size_t)L * Bt, mrows = rows > trows ? rows : trows;
    const bool x3 = p.precision == 1, separate = p.conv == Conv::Separate;
    // f32x6: three bf16 planes of the largest projection operand = 1.5 x its fp32 size (in floats: 3/2)
    const size_t kmax = (size_t)(K0 > 2 * H ? K0 : 2 * H), emb = (size_t)c.emb_dim;
    const size_t p3_floats = (rows * kmax > trows * emb ? rows * kmax : trows * emb) * 3 / 2 + 64;
    bool moved = false;
    int rc = MDD_OK;
    // b holds n floats (on a replay a comparison and no more); false once a growth has failed with rc
    const auto grow = [&](DeviceBuf &b, size_t n) { return b.cap >= n || (rc = ensure(b, n, m->cap_stream, &moved)) == MDD_OK; };
    bool ok = (!(call.Traw > 0 && separate) || grow(m->xstack, (size_t)B * T * c.feat)) && (!separate || grow(m->y0, (size_t)B * c.channels * T * m->W1())) &&
              grow(m->seq0, rows * K0) && grow(m->gx, mrows * 8 * H) && grow(m->act[0], rows * 2 * H) && grow(m->act[1], rows * 2 * H) &&
              grow(m->xraw, rows * 2 * H) && grow(m->hbuf, (size_t)4 * Bpad * H) && grow(m->cbuf, (size_t)2 * Bpad * H) &&
              (ctc || ((p.text_table ? grow(m->tidx, trows) : grow(m->embo, trows * emb)) && grow(m->text, trows * 2 * H) && grow(m->key, trows * 2 * H) &&
                       grow(m->S, (size_t)Bt * Tp * L))) &&   // (a CTC-only handle has no text side)
              (p.proj != Gemm::F32x6 || grow(m->p3, p3_floats)) &&
              (!p.hx_floats || grow(m->hx, p.hx_floats));   // the exchange buffer of the persistent layers + stamps
    if (ok && x3)
        ok = grow(m->seq0_s, rows * K0) && grow(m->act_s[0], rows * 2 * H) && grow(m->act_s[1], rows * 2 * H) && grow(m->x_s, rows * 2 * H) &&
             (ctc || (grow(m->embo_s, trows * emb) && grow(m->text_s, trows * 2 * H) && grow(m->key_s, trows * 2 * H))) && grow(m->hsplit, (size_t)4 * Bt * H);
    if (ok && m->taps) {
        m->tap_rnn.resize(c.layers);
        for (int n = 0; ok && n + 1 < c.layers; n++) ok = grow(m->tap_rnn[n], rows * 2 * H);
    }
    if (moved) m->graphs.clear();   // (the hipFree behind it synchronised the device, so no replay of an old graph is still running)
    if (rc) return rc;
    m->lastB = B; m->lastT = T; m->lastL = L; m->lastK = call.K;
    m->plan = p;
    return MDD_OK;
}

// Every decode entry point ends here.
static int forward(mdd_model *m, ForwardCall call, hipStream_t st) {
    int rc = prepare(m, call);
    if (rc) return rc;
    if (call.Traw && m->plan.conv == Conv::Separate) {   // no fused front-end to take the stack / skip as an index map: a stacked copy, then an ordinary call
        if ((rc = launch_stack_skip(call.x, call.B, call.Traw, m->cfg.feat / 3, 2, 2, 2, m->xstack.p, st))) return rc;
        call.x = m->xstack.p; call.Traw = 0;
    }
    const GraphExec *graph = nullptr;
    if (m->sw.graph) {
        auto it = m->graphs.find(call);
        if (it == m->graphs.end()) {
            if (m->graphs.size() >= 8) m->graphs.clear();
            GraphExec exec;
            if ((rc = capture(m, "graph", [&](hipStream_t cs) { return forward_enqueue(m, call, cs); }, &exec))) return rc;
            it = m->graphs.emplace(call, std::move(exec)).first;
        }
        graph = &it->second;
    }
    bool held = false;
    if (m->plan.gated && (rc = device_gate_enter(m->device, st, &held))) return rc;
    if (!graph) rc = forward_enqueue(m, call, st);
    else if (hipError_t e = hipGraphLaunch(graph->h, st)) { set_error("hipGraphLaunch failed: %s", hipGetErrorString(e)); rc = MDD_ERR_HIP; }
    return device_gate_leave(m->device, st, held, rc);
}

// A CTC-only handle ignores the canonical side of every entry point: the pointers are dropped here, before anything could read them or
// key a captured graph on them.
static ForwardCall plain_call(const mdd_model *m, const float *x, int B, int T, const int64_t *x1, int L, float *logp) {
    ForwardCall call;
    call.x = x; call.logp = logp; call.B = B; call.T = T;
    if (!(m && m->ctc_only)) { call.x1 = x1; call.L = L; }
    return call;
}

extern "C" int mdd_forward(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                           float *logp_dev, void *stream) {
    return forward(m, plain_call(m, x_dev, B, T, x1_dev, L, logp_dev), (hipStream_t)stream);
}

// Several reference batches of different padded lengths in one launch sequence (contract: include/mdd_hip.h).  What depends on a batch's
// own lengths -- where the reverse BiLSTM direction starts, which keys the attention softmax runs over -- follows the per-row values
// (LstmStepArgs::seqlen, launch_attn_tail's llen); everything else is row-local.
extern "C" int mdd_forward_fused(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                                 const int32_t *frames_dev, const int32_t *canon_dev, float *logp_dev, void *stream) {
    if (!m || !frames_dev || (!canon_dev && !m->ctc_only)) { set_error("mdd_forward_fused: null pointer"); return MDD_ERR_ARG; }
    ForwardCall call = plain_call(m, x_dev, B, T, x1_dev, L, logp_dev);
    call.tlen = frames_dev; call.llen = m->ctc_only ? nullptr : canon_dev;
    return forward(m, call, (hipStream_t)stream);
}

// K canonical candidates per utterance on one acoustic pass (contract: include/mdd_hip.h).  The text stages run on K * B rows, the score GEMM and
// the attention tail pair text row j with acoustic row j % B (forward_stages); everything that can be refused is refused here, by name.
extern "C" int mdd_forward_candidates(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t K, int32_t L,
                                      const int32_t *frames_dev, const int32_t *canon_dev, float *logp_dev, void *stream) {
    const char *null_arg = !m ? "m" : !x_dev ? "x_dev" : !x1_dev ? "x1_dev" : !logp_dev ? "logp_dev" : nullptr;
    if (null_arg) { set_error("mdd_forward_candidates: %s is NULL", null_arg); return MDD_ERR_ARG; }
    if (m->ctc_only) { set_error("mdd_forward_candidates: a CTC-only handle has no canonical side (mdd_create_ctc); use mdd_forward"); return MDD_ERR_ARG; }
    if (K < 1) { set_error("mdd_forward_candidates: K=%d, at least one candidate set is needed", K); return MDD_ERR_ARG; }
    if (B < 1) { set_error("mdd_forward_candidates: B=%d must be at least 1", B); return MDD_ERR_ARG; }
    if (T < 2 || T % 2) { set_error("mdd_forward_candidates: T=%d must be even and at least 2", T); return MDD_ERR_ARG; }
    if (L < 1 || L > max_canonical_len(m->cfg)) {
        set_error("mdd_forward_candidates: L=%d outside 1 .. %ld, the canonical length the attention tail holds", L, max_canonical_len(m->cfg)); return MDD_ERR_ARG;
    }
    ForwardCall call = plain_call(m, x_dev, B, T, x1_dev, L, logp_dev);
    call.K = K; call.tlen = frames_dev; call.llen = canon_dev;
    return forward(m, call, (hipStream_t)stream);
}

// A1 + forward in one call: raw_dev = unstacked frames [B, T_raw, feat/3].  With the fused conv front-end the stack/skip
// is only an index map inside its x-tile load (no [B,T,243] copy at all); otherwise a stacked copy is made first.
extern "C" int mdd_forward_raw(mdd_model *m, const float *raw_dev, int32_t B, int32_t T_raw, const int64_t *x1_dev, int32_t L,
                               float *logp_dev, void *stream) {
    if (!m || !raw_dev || B <= 0 || T_raw < 1) { set_error("mdd_forward_raw: bad argument"); return MDD_ERR_ARG; }
    if (m->cfg.feat % 3) { set_error("mdd_forward_raw: feat=%d is not 3 stacked frames", m->cfg.feat); return MDD_ERR_ARG; }
    ForwardCall call = plain_call(m, raw_dev, B, mdd_stack_len(T_raw, 2, 2), x1_dev, L, logp_dev);
    call.Traw = T_raw;
    return forward(m, call, (hipStream_t)stream);
}

extern "C" int32_t mdd_forward_num_stages(mdd_model *m) { return m ? 2 + 2 * m->cfg.layers + (m->ctc_only ? 1 : 6) : 0; }

extern "C" int mdd_forward_profile(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                                   float *logp_dev, void *stream, char *names, int32_t names_cap, float *ms,
                                   int32_t *launches, double *flops, int32_t cap) {
    const ForwardCall call = plain_call(m, x_dev, B, T, x1_dev, L, logp_dev);
    int rc = prepare(m, call);
    if (rc) return rc;
    const std::vector<Stage> stages = forward_stages(m, call);
    const int ns = (int)stages.size();
    if (cap < ns || !ms || !launches || !flops || !names) { set_error("mdd_forward_profile: need room for %d stages", ns); return MDD_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    if (m->plan.gated) {   // keep other handles' forwards off the device while the stages replay: wait for the last gated forward
        bool held = false;
        if ((rc = device_gate_enter(m->device, st, &held))) return rc;
        if ((rc = device_gate_leave(m->device, st, held, MDD_OK))) return rc;
    }
    Event e0, e1;
    MDD_HIP_CHECK(hipEventCreate(&e0.h));
    MDD_HIP_CHECK(hipEventCreate(&e1.h));
    std::string all;
    for (int si = 0; si < ns; si++) {
        const Stage &s = stages[si];
        if (si) all += ",";
        all += s.name;
        ms[si] = 0.f; launches[si] = s.launches; flops[si] = s.flops;
        if (s.launches == 0) continue;   // stage folded into a neighbour in this configuration
        GraphExec exec;
        if ((rc = capture(m, "stage", s.run, &exec))) return rc;
        MDD_HIP_CHECK(hipGraphLaunch(exec.h, st));          // warm (first replay pays upload)
        MDD_HIP_CHECK(hipStreamSynchronize(st));
        MDD_HIP_CHECK(hipEventRecord(e0.h, st));
        MDD_HIP_CHECK(hipGraphLaunch(exec.h, st));
        MDD_HIP_CHECK(hipEventRecord(e1.h, st));
        MDD_HIP_CHECK(hipEventSynchronize(e1.h));
        MDD_HIP_CHECK(hipEventElapsedTime(&ms[si], e0.h, e1.h));
    }
    snprintf(names, names_cap, "%s", all.c_str());
    return MDD_OK;
}

extern "C" const float *mdd_tap(mdd_model *m, const char *name, int64_t *numel) {
    if (!m || !name || !m->lastB) return nullptr;
    const int64_t B = m->lastB, Bt = B * m->lastK, rows = (int64_t)(m->lastT / 2) * B, trows = (int64_t)m->lastL * Bt, H2 = 2 * m->cfg.hidden;
    const std::string n(name);
    const bool x3 = m->plan.precision == 1;
    float *p = nullptr;
    int64_t ne = 0;
    if (n == "conv1") { p = m->seq0.p; ne = rows * m->rnn_in(); }
    else if (m->ctc_only && (n == "text" || n == "key" || n == "score")) return nullptr;   // stages a CTC-only forward does not have
    else if (n == "text") { p = m->text.p; ne = trows * H2; }
    else if (n == "key") { p = m->key.p; ne = trows * H2; }
    else if (n == "score") { p = m->S.p; ne = Bt * (m->lastT / 2) * m->lastL; }   // S[b][t][l] (b over the text rows)
    else if (n == "lstm_dbg" && m->plan.gated) {   // diagnostic stamps of the last persistent layer launch (MDD_LSTM_DBG=1)
        p = m->hx.p + m->plan.stamps_at;
        ne = 256 * 6 * 2;
    }
    else if (n.compare(0, 3, "rnn") == 0) {
        const int i = atoi(n.c_str() + 3);
        if (i == m->cfg.layers - 1) p = m->xraw.p;
        else if (m->taps && i >= 0 && i < (int)m->tap_rnn.size()) p = m->tap_rnn[i].p;
        ne = p ? rows * H2 : 0;
    }
    if (x3 && (n == "conv1" || n == "key")) {   // these stages exist only as split-bf16 planes: rebuild fp32 = hi + lo
        if (launch_unsplit(split_view(n == "key" ? m->key_s : m->seq0_s, (size_t)ne), (size_t)ne, p, nullptr) != MDD_OK) return nullptr;
        if (hipStreamSynchronize(nullptr) != hipSuccess) return nullptr;
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
    if (!flag) return MDD_OK;
    MDD_HIP_CHECK(hipMemset(m->err_flag.p, 0, sizeof(int)));
    if (flag == 2) {
        set_error("persistent BiLSTM kernel timed out waiting for its team (grid not fully resident?); set MDD_LSTM=step");
        return MDD_ERR_HIP;
    }
    set_error("index out of range in self");  // the message of the IndexError nn.Embedding raises
    return MDD_ERR_ARG;
}

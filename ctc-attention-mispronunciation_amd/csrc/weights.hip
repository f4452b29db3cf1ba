// State_dict -> device weights of the decode handle: BatchNorm folding, gate-row permutation, the packed / split-bf16 / three-plane copies
// the kernels read.  mdd_finalize_weights (api.hip) builds a whole set with build_weights() and swaps it in.
#include <string.h>

#include <cmath>

#include "model.h"

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

// fp32 matrix -> P bf16 planes on the device (same element order, plane p at out + p * n), each the rounded remainder of the ones before:
// hi | lo (split-bf16, hi + lo ~ x to 16 bits) or hi | mid | lo (f32x6, exact)
static int upload_planes(DecodeWeights &w, const std::vector<float> &h, int P, unsigned short **out) {
    const size_t n = h.size();
    std::vector<unsigned short> buf(P * n);
    for (size_t i = 0; i < n; i++) {
        float r = h[i];
        for (int p = 0; p < P; p++) {
            buf[p * n + i] = host_bf16(r);
            r -= host_bf16_f32(buf[p * n + i]);
        }
    }
    if (int rc = w.alloc(out, P * n)) return rc;
    MDD_HIP_CHECK(hipMemcpy(*out, buf.data(), P * n * sizeof(unsigned short), hipMemcpyHostToDevice));
    return MDD_OK;
}
static int upload_split(DecodeWeights &w, const std::vector<float> &h, SplitPtr *out) {
    if (int rc = upload_planes(w, h, 2, &out->hi)) return rc;
    out->lo = out->hi + h.size();
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

// rows n = g*H + u  ->  n' = u*4 + g (see lstm_step.hip); concatenates the two directions
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

// Whh' [2][4H][H] (gate-permuted rows) -> Wp[d][ut][j][lane][m] (see lstm_step.hip)
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

// The float entries of the CTC-only state_dict (CRC/models/cnn_rnn.py:82-145) with their shapes: 12 + 4 layers + 4 (layers - 1) + 5.
static std::map<std::string, std::vector<int64_t>> ctc_entries(const mdd_model *m) {
    const mdd_config &c = m->cfg;
    const int64_t ch = c.channels, H = c.hidden;
    std::map<std::string, std::vector<int64_t>> e;
    const auto bn = [&e](const std::string &prefix, int64_t n) {
        for (const char *s : {".weight", ".bias", ".running_mean", ".running_var"}) e[prefix + s] = {n};
    };
    e["conv.0.conv.weight"] = {ch, 1, 3, 3}; e["conv.0.conv.bias"] = {ch}; bn("conv.0.batch_norm", ch);
    e["conv.1.conv.weight"] = {ch, ch, 3, 3}; e["conv.1.conv.bias"] = {ch}; bn("conv.1.batch_norm", ch);
    for (int n = 0; n < c.layers; n++) {
        const std::string base = "rnns." + std::to_string(n);
        if (n > 0) bn(base + ".batch_norm", 2 * H);
        for (const char *d : {"", "_reverse"}) {
            e[base + ".rnn.weight_ih_l0" + d] = {4 * H, n == 0 ? (int64_t)m->rnn_in() : 2 * H};
            e[base + ".rnn.weight_hh_l0" + d] = {4 * H, H};
        }
    }
    bn("fc.0", 2 * H);
    e["fc.1.weight"] = {c.num_class, 2 * H};
    return e;
}

int check_ctc_entry(const mdd_model *m, const std::string &key, const int64_t *shape, int ndim) {
    if (key == "embeds.weight" || key == "score.weight" || key.compare(0, 12, "lstm_embeds.") == 0) {
        set_error("mdd_load_weight: '%s' belongs to the attention branch, which a CTC-only model does not have (mdd_create makes a handle for it)", key.c_str());
        return MDD_ERR_ARG;
    }
    const auto entries = ctc_entries(m);
    const auto it = entries.find(key);
    if (it == entries.end()) { set_error("mdd_load_weight: '%s' is no entry of the CTC-only state_dict", key.c_str()); return MDD_ERR_ARG; }
    const std::vector<int64_t> &want = it->second;
    bool same = ndim == (int)want.size();
    for (int i = 0; same && i < ndim; i++) same = shape[i] == want[i];
    if (!same) {
        std::string got, exp;
        for (int i = 0; i < ndim; i++) got += (i ? ", " : "") + std::to_string(shape[i]);
        for (size_t i = 0; i < want.size(); i++) exp += (i ? ", " : "") + std::to_string(want[i]);
        set_error("mdd_load_weight: '%s' has shape [%s], the CTC-only geometry expects [%s]", key.c_str(), got.c_str(), exp.c_str());
        return MDD_ERR_ARG;
    }
    return MDD_OK;
}

int build_weights(mdd_model *m, DecodeWeights &w) {
    const mdd_config &c = m->cfg;
    const int ch = c.channels, H = c.hidden;
    const bool ctc = m->ctc_only;
    if (ctc)   // name the first missing entry of the 45 (at 4 layers) before anything is built
        for (const auto &e : ctc_entries(m))
            if (!m->host.count(e.first)) { set_error("weight '%s' was never loaded", e.first.c_str()); return MDD_ERR_STATE; }
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
        // conv1 weights [ci][kh][kw][co], and for the fused MFMA front-end [co][kh][kw][ci] (k = (kh*3+kw)*ch + ci): split-bf16, and the same
        // matrix as three planes (hi | mid | lo, each [co][288] row-major) for the fp32-grade fused front-end
        std::vector<float> tmp2((size_t)ch * 9 * ch);
        tmp.assign((size_t)ch * 9 * ch, 0.f);
        for (int co = 0; co < ch; co++)
            for (int ci = 0; ci < ch; ci++)
                for (int k = 0; k < 9; k++) tmp[((size_t)ci * 9 + k) * ch + co] = tmp2[((size_t)co * 9 + k) * ch + ci] = (*w1)[((size_t)co * ch + ci) * 9 + k];
        if ((rc = upload(w, tmp, &w.w_conv1t)) || (rc = upload(w, sc, &w.sc1)) || (rc = upload(w, sh, &w.sh1))) return rc;
        if ((rc = upload_split(w, tmp2, &w.w_conv1_s)) || (rc = upload_planes(w, tmp2, 3, &w.w_conv1_3))) return rc;
    }
    const int n_rnn = ctc ? c.layers : c.layers + 1;
    w.rnn.resize(n_rnn);
    for (int n = 0; n < n_rnn; n++) {   // the BiLSTM layers, then the text encoder (none in a CTC-only model)
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
        if (packed_whh(c) && (rc = upload_planes(w, tmp, 3, &lw.whh_3))) return rc;
        if (packed_whh(c)) { std::vector<float> pk; pack_whh(tmp, H, pk); tmp.swap(pk); }
        if ((rc = upload(w, tmp, &lw.whh))) return rc;
        if (n > 0 && n < c.layers) {
            snprintf(base, sizeof(base), "rnns.%d.batch_norm", n);
            if (!bn_fold(m, base, 2 * H, sc, sh)) return MDD_ERR_STATE;
            if ((rc = upload(w, sc, &lw.scale)) || (rc = upload(w, sh, &lw.shift))) return rc;
        }
    }
    if (!ctc) {   // text encoder: the embedding table; bias_ih + bias_hh folded into the input projection's epilogue
        const auto *e = get(m, "embeds.weight", (size_t)c.emb_rows * c.emb_dim);
        if (!e) return MDD_ERR_STATE;
        if ((rc = upload(w, *e, &w.emb))) return rc;
        std::vector<float> bi, bh;
        if (!pack_gate_rows(m, "lstm_embeds.", "bias_ih_l0", H, 1, bi) || !pack_gate_rows(m, "lstm_embeds.", "bias_hh_l0", H, 1, bh)) return MDD_ERR_STATE;
        for (size_t i = 0; i < bi.size(); i++) bi[i] += bh[i];
        if ((rc = upload(w, bi, &w.t_bias))) return rc;
        // the projected rows, through the launchers project() (api.hip) takes per call, with the embedding matrix as the operand
        const LstmWeights &tw = w.rnn[c.layers];
        const int G2 = 8 * H, E = c.emb_dim, V = c.emb_rows;
        if ((rc = w.alloc(&w.text_table[0], (size_t)V * G2))) return rc;
        if ((rc = launch_gemm_nt({.p = w.emb, .ld = E}, {.p = tw.wih, .ld = E}, w.text_table[0], G2, V, G2, E, nullptr, {.bias = w.t_bias}))) return rc;
        if (tw.wih_3) {
            unsigned short *planes = nullptr;   // (kept with the set: the GEMM below reads it after this function has returned)
            if ((rc = w.alloc(&planes, (size_t)3 * V * E)) || (rc = w.alloc(&w.text_table[1], (size_t)V * G2))) return rc;
            if ((rc = launch_split3(w.emb, V, E, E, planes, nullptr))) return rc;
            if ((rc = launch_gemm_f32x6(planes, (size_t)V * E, tw.wih_3, (size_t)G2 * E, w.t_bias, w.text_table[1], V, G2, E, G2, nullptr, m->sw.x6_raster, nullptr, m->sw.x6_rt))) return rc;
        }
    }
    if (ctc) {   // the classifier on the last layer's 2H outputs (CRC/models/cnn_rnn.py:140-142): no score, no 4H operands
        const int K = 2 * H;
        const auto *wf = get(m, "fc.1.weight", (size_t)c.num_class * K);
        if (!wf || !bn_fold(m, "fc.0", K, sc, sh)) return MDD_ERR_STATE;
        if ((rc = upload(w, *wf, &w.w_fc)) || (rc = upload(w, sc, &w.fscale)) || (rc = upload(w, sh, &w.fshift))) return rc;
        if (mfma_ctc_tail(c)) {   // consumer-order repack for ctc_tail_mfma_kernel, where launch_ctc_tail takes it (plan.h)
            const int J = K / 16;
            std::vector<float> pk((size_t)3 * J * 64 * 4, 0.f);
            for (int nt = 0; nt < 3; nt++)
                for (int j = 0; j < J; j++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int mm = 0; mm < 4; mm++) {
                            const int n = nt * 16 + (lane & 15), k = 16 * j + 4 * (lane >> 4) + mm;
                            if (n < c.num_class) pk[(((size_t)nt * J + j) * 64 + lane) * 4 + mm] = (*wf)[(size_t)n * K + k];
                        }
            if ((rc = upload(w, pk, &w.w_fcp))) return rc;
        }
    } else {
        const auto *ws = get(m, "score.weight", (size_t)4 * H * H), *wf = get(m, "fc.1.weight", (size_t)c.num_class * 4 * H);
        if (!ws || !wf) return MDD_ERR_STATE;
        if (!bn_fold(m, "fc.0", 4 * H, sc, sh)) return MDD_ERR_STATE;
        if ((rc = upload_split(w, *ws, &w.w_score_s))) return rc;
        if ((rc = upload(w, *ws, &w.w_score)) || (rc = upload(w, *wf, &w.w_fc)) || (rc = upload(w, sc, &w.fscale)) ||
            (rc = upload(w, sh, &w.fshift))) return rc;
        const int D2 = 4 * H;
        if (mfma_tail(c)) {   // consumer-order repack for attn_tail_mfma_kernel, where launch_attn_tail takes it (plan.h)
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

}  // namespace mdd

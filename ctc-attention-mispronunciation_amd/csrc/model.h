// The decode handle (mdd_model), its device weights and the arguments of one forward: private to api.hip (handle lifetime, forward
// orchestration) and weights.hip (state_dict -> device weights).
#pragma once
#include <memory>

#include "mdd_internal.h"

struct mdd_model;
namespace mdd {

// Everything that distinguishes one decode forward from another: every entry point builds one, and it is the key of the handle's captured
// graphs (every member initialised and no padding, so it compares bytewise).
struct ForwardCall {
    const float *x = nullptr;          // [B, T, feat] stacked frames; [B, Traw, feat / 3] unstacked ones where Traw > 0
    const int64_t *x1 = nullptr;       // [K, B, L] canonical ids
    float *logp = nullptr;             // [K, T / 2, B, num_class]
    const int *tlen = nullptr, *llen = nullptr;   // mdd_forward_fused: per-row posterior frames [B] / canonical length [K * B] of the row's own batch (null: T / 2, L)
    int B = 0, T = 0, L = 0;
    int Traw = 0;                      // mdd_forward_raw: the stack / skip is still to be applied to x
    int K = 1;                         // mdd_forward_candidates: candidate sets -- K * B text rows (j = k * B + b) attend over the B acoustic rows (j % B)
    int reserved = 0;                  // (keeps the struct free of padding)
    bool operator<(const ForwardCall &o) const { return memcmp(this, &o, sizeof(ForwardCall)) < 0; }
};
static_assert(sizeof(ForwardCall) == 5 * sizeof(void *) + 6 * sizeof(int), "ForwardCall is compared bytewise: no padding");

// Move-only owner of a HIP event / graph / executable graph, in the style of DeviceArray.
template <class T, hipError_t (*Destroy)(T)> struct HipOwned {
    T h = nullptr;
    HipOwned() = default;
    HipOwned(const HipOwned &) = delete;
    HipOwned &operator=(const HipOwned &) = delete;
    HipOwned(HipOwned &&o) noexcept : h(o.h) { o.h = nullptr; }
    HipOwned &operator=(HipOwned &&o) noexcept { std::swap(h, o.h); return *this; }
    ~HipOwned() { if (h) (void)Destroy(h); }
};
using Event = HipOwned<hipEvent_t, hipEventDestroy>;
using Graph = HipOwned<hipGraph_t, hipGraphDestroy>;
using GraphExec = HipOwned<hipGraphExec_t, hipGraphExecDestroy>;

// The weights of one BiLSTM layer on the device; the text encoder's sit at index cfg.layers (a CTC-only handle has none).
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
    std::vector<LstmWeights> rnn;                  // cfg.layers + 1; cfg.layers in a CTC-only handle
    float *emb = nullptr, *t_bias = nullptr;
    // The text encoder's input projection of every embedding row, [emb_rows][8H]: text_table[v] = emb[v] . W_ih_text'^T + t_bias, made at finalize
    // by the forward's own GEMM of each arithmetic on emb itself, so a row carries the bits gemm_text would produce for it.  [0]: the exact
    // fp32 MFMA GEMM (mode 0), [1]: f32x6 (mode 2; null where the geometry has no f32x6 planes).  Mode 1 has none (plan.h, text_table).
    float *text_table[2] = {nullptr, nullptr};
    // the classifier: BatchNorm folded to fscale / fshift, Linear as it is and in the matrix-core tail's lane order.  4H wide; 2H wide in a
    // CTC-only handle, which has no emb, t_bias, text_table or w_score
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
// Build a complete weight set from the loaded state_dict into `w` (a fresh set: on failure it is discarded whole).  weights.hip
int build_weights(mdd_model *m, DecodeWeights &w);
// A CTC-only handle checks every entry as it is loaded: MDD_OK, or MDD_ERR_ARG with the key named (a key of the attention branch, a key the
// CTC-only state_dict does not have, a shape other than the geometry's).  weights.hip
int check_ctc_entry(const mdd_model *m, const std::string &key, const int64_t *shape, int ndim);

}  // namespace mdd

struct mdd_model {
    mdd_config cfg;
    int device = 0;
    bool ctc_only = false;   // mdd_create_ctc: the acoustic model with the classifier on it, no text side (ctc_tail instead of the attention tail)
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
    mdd::DeviceBuf xstack;      // mdd_forward_raw without the fused front-end: stacked copy
    mdd::DeviceBuf tidx;        // the text projection as a table: int32 row index of every (l, b), time-major (embo is then not allocated)
    std::vector<mdd::DeviceBuf> tap_rnn;
    mdd::DeviceArray<int> err_flag;
    mdd::DeviceArray<unsigned int> sync_words;
    hipStream_t cap_stream = nullptr;  // graphs are captured here (the legacy default stream cannot capture)
    int lastB = 0, lastT = 0, lastL = 0, lastK = 1;
    mdd::ForwardPlan plan{};    // the kernels of the last prepared forward (shape lastB / lastT / lastL, lastK candidate sets)
    std::map<mdd::ForwardCall, mdd::GraphExec> graphs;
    ~mdd_model() { graphs.clear(); if (cap_stream) (void)hipStreamDestroy(cap_stream); }
    int W1() const { return mdd::conv_out(cfg.feat); }
    int W2() const { return mdd::conv_out(W1()); }
    int rnn_in() const { return mdd::rnn_in(cfg); }
};

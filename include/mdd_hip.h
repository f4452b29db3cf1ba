/*
 * mdd_hip.h -- C ABI of libmdd_hip.so: the MI355X (gfx950) implementation of the
 * CTC-attention mispronunciation-detection hot path.
 *
 * The reference (dyustc/CTC-Attention-Mispronunciation, egs/attention_aug = "AA") has no FFI
 * layer: its seam is Python objects.  Each entry point below names the reference interface it
 * replaces; INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * The reference's CTC-only baseline recipe (egs/cnn-rnn-ctc = "CRC": the same acoustic model without the text encoder and the attention)
 * runs through the same entry points on a handle of mdd_create_ctc; its eval-mode forward only.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross the boundary
 *   - pointers named *_dev are device (HBM) addresses, everything else is host memory
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all GPU work is
 *     enqueued on it and nothing synchronises unless a function says so
 *   - every function returns 0 on success or a negative mdd_status; mdd_last_error() gives text
 *   - a handle is not thread-safe: one handle per host thread / stream / device
 *   - the caller owns every buffer it passes; the library owns device weights and a workspace
 *     that grows on demand (never inside a stream capture)
 */
#ifndef MDD_HIP_H
#define MDD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdd_model mdd_model;

enum mdd_status {
    MDD_OK = 0,
    MDD_ERR_ARG = -1,       /* bad argument / shape */
    MDD_ERR_HIP = -2,       /* a HIP runtime call failed */
    MDD_ERR_STATE = -3,     /* weights missing / not finalised */
    MDD_ERR_NOMEM = -4,
    MDD_ERR_EMPTY = -5      /* mdd_align with an empty side: the reference raises TypeError */
};

/* per-utterance status written by mdd_beam: the exception the reference's BeamDecoder.decode
 * would raise for that utterance (AA/utils/BeamSearch.py:64,66,103,106,135; AA/utils/NgramLM.py:75-76) */
enum mdd_beam_status { MDD_BEAM_OK = 0, MDD_BEAM_INDEX_ERROR = 1, MDD_BEAM_VALUE_ERROR = 2, MDD_BEAM_KEY_ERROR = 3 };

/* Geometry of CTC_Model.__init__ (AA/models/model_ctc.py:84-158) for the one architecture the
 * reference recipe builds: 2x LayerCNN(k3x3, strides (1,2),(2,2), pad 1) -> `layers` x BiLSTM(hidden)
 * -> Embedding(emb_rows, emb_dim) + BiLSTM text encoder -> dot attention -> BN + Linear(num_class).
 * mdd_create and mdd_train_create accept the same geometries (geometry_error, csrc/plan.h) and return MDD_ERR_ARG, with
 * mdd_last_error() naming the field, for any other:
 *   feat >= 3;  hidden a multiple of 4, 4 <= hidden <= 1024;  layers >= 1;  num_class >= 2;  channels 32 or 4;  emb_rows >= 1;
 *   emb_dim a multiple of 4;  and room for at least one canonical phoneme in the attention tail (the L limit at mdd_forward >= 1:
 *   always so with the matrix-core tail, 4 hidden + num_class <= 2559 with the scalar one).
 * Every accepted geometry runs in every mode; which kernels it gets is decided in csrc/plan.h.  The fast forms need: feat = 243 and
 * channels = 32 (the fused conv front end), hidden 256 or 384 (the persistent layer kernels and mode 1), contraction lengths
 * channels x W2, 2 x hidden and emb_dim that are multiples of 32 (modes 1 and 2), hidden a multiple of 64 and num_class <= 48 (the
 * matrix-core attention tail).  tests/geometry_cases.py lists the geometries the suite runs and the kernels each is expected to get. */
typedef struct mdd_config {
    int32_t feat;       /* stacked input width F (243 = 3 x 81), rnn_param["rnn_input_size"]; >= 3 (mdd_forward_raw: a multiple of 3) */
    int32_t hidden;     /* rnn_hidden_size H (384; 256 for BASELINE.json's variant); a multiple of 4, at most 1024 */
    int32_t layers;     /* rnn_layers (4); >= 1 */
    int32_t num_class;  /* C (45 for the 41-phone set); >= 2 */
    int32_t channels;   /* CNN channels (32); 32 or 4 */
    int32_t emb_rows;   /* 44  (model_ctc.py:149); >= 1 */
    int32_t emb_dim;    /* 512 (model_ctc.py:149-150); a multiple of 4 */
    float bn_eps;       /* 1e-5 */
} mdd_config;

const char *mdd_last_error(void);
int mdd_version(void);

/* ---- model lifetime + weights: replaces CTC_Model(...) + load_state_dict (AA/infer.py:251-254) */
int mdd_create(const mdd_config *cfg, int device, mdd_model **out);
void mdd_destroy(mdd_model *m);
/* ---- the CTC-only model: replaces CTC_Model(...) of CRC/models/cnn_rnn.py:70-145 + load_state_dict.  The handle runs the eval forward
 * conv x 2 -> `layers` x BiLSTM -> BatchNorm1d(2H) + Linear(2H -> num_class, no bias) -> log-softmax (cnn_rnn.py:147-179) and is used
 * through the same functions as an mdd_create handle.  Geometry (ctc_geometry_error, csrc/plan.h); any other returns MDD_ERR_ARG with
 * mdd_last_error() naming the field:
 *   feat, hidden, layers, num_class, channels as for mdd_config above (the same messages);  emb_rows = 0 and emb_dim = 0: the model has no
 *   embedding.  The attention tail's room condition does not apply.
 * Weights: the 12 + 4 layers + 4 (layers - 1) + 5 float entries of its state_dict (45 at 4 layers), fc.0.* [2H] and fc.1.weight [C, 2H].
 *   mdd_load_weight checks each entry as it arrives and returns MDD_ERR_ARG naming the key for a key of the attention branch
 *   (embeds.weight, lstm_embeds.*, score.weight), any other key the state_dict does not have, or a shape other than the geometry's;
 *   mdd_finalize_weights returns MDD_ERR_STATE naming the first entry that never arrived.  No embedding, text table, score or 4H-wide
 *   classifier operand is built.
 * Forward: mdd_forward, mdd_forward_raw, mdd_forward_fused, mdd_forward_profile ignore x1_dev, L and canon_dev: the pointers may be NULL
 *   and are never read, there is no id check and no limit on L, and no text-side buffer is allocated.  frames_dev of mdd_forward_fused
 *   keeps its meaning (the reverse direction of every BiLSTM starts at the utterance's own batch length; rows t < frames_dev[b] are
 *   bit-identical to mdd_forward on that batch alone).  The stage list is the acoustic stages of an mdd_create handle followed by
 *   `ctc_tail` (csrc/ctc_tail.hip: fp32 in every mode; on the matrix cores where hidden is a multiple of 32 and num_class <= 48).
 *   Modes 0, 1, 2, MDD_PRECISION and the fallbacks are those of mdd_set_precision below with emb_dim taking no part.
 * Taps: "conv1" and "rnn<i>" as below; "text", "key" and "score" return NULL.
 * The decoders, alignment, one-edit posteriors and the CTC loss take log-probs and do not care which handle made them.  There is no training
 * step for this model (mdd_train_create builds the attention model only). */
int mdd_create_ctc(const mdd_config *cfg, int device, mdd_model **out);
int32_t mdd_is_ctc_only(mdd_model *m);   /* 1 for a handle of mdd_create_ctc, else 0 */
/* Copy one state_dict entry (host fp32, contiguous, reference key name and shape) to the device.
 * `num_batches_tracked` entries are accepted and ignored. */
int mdd_load_weight(mdd_model *m, const char *key, const float *data, const int64_t *shape, int32_t ndim);
/* Check that all 55 float entries arrived (mdd_create_ctc: 45), fold eval-mode BatchNorm into scale/shift vectors and
 * repack LSTM gate rows for the step kernel.  Synchronises the device. */
int mdd_finalize_weights(mdd_model *m);

/* Arithmetic of the model's contractions.  Modes 2 and 0 are reference width (the arithmetic of the reference's ATen fp32 ops,
 * AA/models/model_ctc.py:27-29,59-66,149-158: every operand with its full 24-bit significand, fp32 accumulation); measured against a
 * float64 evaluation both are CLOSER to it than ATen's own fp32 (tests/test_gpu_parity.py::test_error_against_fp64_beside_aten_fp32).
 * 2 (default) = "f32x6": the large time-batched contractions -- conv0 / conv1 and the BiLSTM / text input projections -- on the bf16
 *     matrix cores with every fp32 operand carried as THREE bf16 planes (hi + mid + lo = its 24 significand bits exactly) and the six
 *     cross products down to 2^-24 of a product, fp32 accumulate, hi.hi in an accumulator of its own (gemm_bf16x6.hip: 6/16 of the cost
 *     of the fp32 MFMA, which on gfx950 runs at the fp32 vector rate); so do the recurrent W_hh.h products where that is the faster of
 *     the two reference-width layer kernels (lstm_x6.hip: W_hh and the state h as three planes each; H = 384 up to 1024 rows, H = 256
 *     up to 128 rows; env MDD_LSTM_X6=0 / force); everything else as mode 0.  Needs contraction lengths that are multiples of 32 (falls
 *     back to 0 otherwise).
 * 0 = every product an exact fp32 MFMA (v_mfma_f32_32x32x2_f32 in the time-batched GEMMs, v_mfma_f32_16x16x4_f32 in the recurrent
 *     W_hh.h products, the attention tail and the convolutions).
 * 1 = split-bf16 "x3" on v_mfma_f32_16x16x32_bf16: each fp32 operand = bf16 hi + bf16 lo (~16 significand bits), products hi.lo +
 *     lo.hi + hi.hi, for EVERY contraction of the forward including the recurrent W_hh.h products (h is re-split every step); cell state,
 *     gates, softmax and the classifier tail stay fp32.  NARROWER than the reference's arithmetic: a flagged variant.  Its effect on the
 *     log-probs grows with the magnitude of the attention scores, because a score carries an error of ~2^-17 of its size into exp():
 *     measured against float64 (tests/test_canonical_length.py, profiles/canonical_length_margins.json) <= 1.1e-5 with the synthetic
 *     weights as they are (|score| ~ 1, near-uniform attention, L up to 1852), <= 5.2e-5 with score.weight x 16 (|score| ~ 13),
 *     <= 2.0e-4 at x 64 (|score| ~ 50) and <= 6.1e-4 at x 256 (|score| ~ 200, rows dominated by one key) -- i.e. past the 1e-4
 *     tolerance once scores reach a few tens, where modes 0 and 2 stay <= 2.2e-5.  Use mode 2 or 0 for a model with peaked attention.
 *     Falls back to 0 when a contraction length is not a multiple of 32 or H is not 256 / 384.
 * The contraction lengths are channels x W2 (W2 = the width after both convolutions: always a multiple of 32 with 32 channels), 2H and
 * emb_dim.  In mode 2 a hidden size other than 256 / 384 keeps the f32x6 projections and runs the recurrences per step in exact fp32.
 * Env MDD_PRECISION=f32x6 / f32 / bf16x3 selects the mode at mdd_create.  mdd_get_precision returns the mode actually in use. */
int mdd_set_precision(mdd_model *m, int32_t mode);
int32_t mdd_get_precision(mdd_model *m);

/* ---- A1: make_context(feat,0,right) + skip_feat(.,skip) + pad to a multiple of n_down
 * (AA/utils/tools.py:207-227, AA/utils/data_loader.py:138-142) for B equal-length utterances.
 * raw_dev [B,T_raw,D] -> out_dev [B,T_out,(right+1)*D] with T_out = mdd_stack_len(T_raw,skip,n_down). */
int32_t mdd_stack_len(int32_t T_raw, int32_t skip, int32_t n_down);
int mdd_stack_skip(const float *raw_dev, int32_t B, int32_t T_raw, int32_t D, int32_t right, int32_t skip,
                   int32_t n_down, float *out_dev, void *stream);
/* float32 length bookkeeping of create_input / infer (data_loader.py:177, infer.py:296-297) -- host */
int32_t mdd_len_frames(int32_t len, int32_t maxlen, int32_t t_out);

/* ---- A2-A7: CTC_Model.forward(x, x1) in eval mode (AA/models/model_ctc.py:160-223)
 * x_dev [B,T,F] fp32 (T even), x1_dev [B,L] int64 canonical ids (0-padded) ->
 * logp_dev [T/2,B,C] fp32 log-probabilities.  ids outside [0,emb_rows) are an error
 * (the reference raises IndexError) and are reported by the next mdd_sync().
 * Canonical length: the attention tail keeps 16 rows of attention weights in LDS next to its classifier operands (160 KB in all),
 * which bounds L (max_canonical_len, csrc/plan.h).  With the matrix-core tail (hidden a multiple of 64 and C <= 48) L <= 2364 - 2H:
 * 1596 at H = 384, 1852 at H = 256, 2108 at H = 128; with the scalar tail (every other geometry) L <= 2560 - 4H - C: 1999 at
 * H = 128, C = 49.  A longer L returns MDD_ERR_ARG
 * (mdd_last_error() names L) from mdd_forward, mdd_forward_fused (whose bound applies to the common L) and mdd_forward_raw.  It is a
 * host check: logp_dev is untouched and the handle stays usable; in the default graph mode it fires while the library's own capture
 * is open, so nothing of that forward has been enqueued (with MDD_GRAPH=0 the stages before the tail have run into the workspace). */
int mdd_forward(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                float *logp_dev, void *stream);
/* ---- A2-A7 for several reference batches of different padded lengths in ONE launch sequence.  The reference pads each
 * batch to its own maximum and masks nothing (model_ctc.py:186,198,204-205; collate AA/utils/data_loader.py:151-181), so an
 * utterance's posteriors depend on its batch's padded length.  frames_dev[b] = T_g / 2 (posterior frames) and canon_dev[b] = L_g
 * (canonical length) of the batch utterance b belongs to; x_dev [B,T,F] holds every batch zero-padded to the common T (zero from
 * its own T_g on), x1_dev [B,L] zero-padded to the common L.  Every utterance's rows t < frames_dev[b] of logp_dev [T/2,B,C] are
 * bit-identical to mdd_forward on its batch alone; rows beyond are undefined. */
int mdd_forward_fused(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                      const int32_t *frames_dev, const int32_t *canon_dev, float *logp_dev, void *stream);
/* ---- A2-A7 for K canonical candidates per utterance on ONE acoustic pass (no reference counterpart: the reference would run K forwards).
 * The posteriors are conditioned on the canonical sequence, so scoring an utterance against several pronunciations of its word, several
 * target words or a teacher's variant needs one posterior tensor per candidate; the conv front end and the BiLSTM layers (28 of the 30 ms
 * of a pass) do not depend on the canonical and run once.  x_dev [B,T,F]; x1_dev [K,B,L] int64: candidate set k is one reference batch,
 * the B utterances of x_dev with the canonicals x1_dev[k], 0-padded to the common L; logp_dev [K,T/2,B,C].
 *   frames_dev [B] or NULL     frames_dev[b] = T_g / 2 of utterance b's batch, exactly as in mdd_forward_fused; NULL: T / 2 for all
 *   canon_dev [K*B] or NULL    canon_dev[k*B + b] = the padded canonical length L_k of candidate set k, at least 1 and at most L (the
 *                              reference pads each batch to its own longest canonical and masks nothing); NULL: L for all.  A device
 *                              array: a value outside 1 .. L is clamped into it, as mdd_forward_fused does
 * Rows t < frames_dev[b] of logp_dev[k] are what mdd_forward_fused gives row k*B + b of the batch made by repeating x_dev K times, with
 * the same frames (repeated) and canon: bit for bit, in every arithmetic mode.  Rows beyond are undefined.
 * Kernel choice: the whole call, acoustic stages included, runs under ONE plan, plan_forward(..., K*B) (csrc/plan.h).  Every condition
 * that plan puts on the row count is an upper bound, so the B acoustic rows are valid under it, and it is what makes the equality above
 * hold for every geometry.  The consequence: logp_dev[k] equals mdd_forward(x_dev, x1_dev[k]) bit for bit wherever plan_forward gives B and
 * K*B rows the same kernels -- hidden = 384 up to K*B = 1024 rows, and any geometry while K*B <= 128 or the mode in effect is not 2;
 * elsewhere (mode 2 at hidden = 256 with B <= 128 < K*B: the f32x6 recurrence against the exact-fp32 one; B <= 1024 < K*B: a persistent
 * layer kernel against the per-step one) the two agree within the parity tolerance, 1e-4 on the log-probs.
 * The text stages (embedding / text projection, text encoder, keys) run on K*B rows j = k*B + b; the scores and the attention tail pair
 * text row j with acoustic row j % B.  The limit on L is mdd_forward's (max_canonical_len).  K*B > 1024 is legal and takes the per-step
 * recurrences, as any such B does.
 * MDD_ERR_ARG, with the argument named in mdd_last_error() and before anything is enqueued (logp_dev untouched, the handle usable): K < 1;
 * m, x_dev, x1_dev or logp_dev NULL; a handle of mdd_create_ctc (no canonical side); B < 1; T odd or < 2; L < 1 or over the limit.  An id
 * outside [0,emb_rows) is reported by the next mdd_sync(), as for mdd_forward. */
int mdd_forward_candidates(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev /* [K,B,L] */, int32_t K, int32_t L,
                           const int32_t *frames_dev /* [B] or NULL */, const int32_t *canon_dev /* [K*B] or NULL */,
                           float *logp_dev /* [K,T/2,B,C] */, void *stream);

/* ---- A1 + A2..A7 in one call: raw_dev holds the unstacked frames [B, T_raw, feat/3] (make_context(.,0,2) + skip_feat(.,2)
 * + even padding are applied on the fly: AA/utils/tools.py:207-227, AA/utils/data_loader.py:138-142); logp_dev is
 * [mdd_stack_len(T_raw,2,2)/2, B, C].  Same results, bit for bit, as mdd_stack_skip followed by mdd_forward. */
int mdd_forward_raw(mdd_model *m, const float *raw_dev, int32_t B, int32_t T_raw, const int64_t *x1_dev, int32_t L,
                    float *logp_dev, void *stream);

/* The same forward replayed stage by stage between HIP events on `stream` (measurement aid for bench.py:
 * per-stage wall time, kernel launches and algorithmic flops).  names: comma-separated stage names. */
int32_t mdd_forward_num_stages(mdd_model *m);
int mdd_forward_profile(mdd_model *m, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                        float *logp_dev, void *stream, char *names, int32_t names_cap, float *ms, int32_t *launches,
                        double *flops, int32_t cap);
/* Optional taps for parity tests: copies of stage outputs of the last mdd_forward (device buffers,
 * valid until the next forward).  name: "conv1" [T/2,B,ch*W2], "rnn<i>" [T/2,B,2H] (raw, before the
 * next layer's BatchNorm), "text" [L,B,2H], "key" [L,B,2H], "score" [B,T/2,L] (the attention
 * scores before the softmax).  Returns the device pointer or NULL. */
const float *mdd_tap(mdd_model *m, const char *name, int64_t *numel);
/* Same, copied device-to-device into a caller buffer of `capacity` floats on `stream`. */
int mdd_tap_copy(mdd_model *m, const char *name, float *dst_dev, int64_t capacity, void *stream);
/* Keep the raw output of every BiLSTM layer (off by default: only the last layer's is needed). */
int mdd_enable_taps(mdd_model *m, int32_t on);
/* Wait for `stream` and report asynchronous errors of earlier calls on this handle. */
int mdd_sync(mdd_model *m, void *stream);

/* ---- A8: GreedyDecoder.decode (AA/utils/ctcDecoder.py:188-200, 80-92)
 * logp_dev [T,B,C], len_dev [B] (clamped to [0,T]) -> ids_dev [B,T] (collapsed, blanks removed; only the first nids[b] entries of a
 * row are written), nids_dev [B].  Any C >= 1, 0 <= blank < C; ties go to the lowest class, an all -inf row to class 0.
 * Limit: T <= 38400 (one int of LDS per frame, 150 KB); a longer T returns MDD_ERR_ARG. */
int mdd_greedy(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t blank,
               int32_t *ids_dev, int32_t *nids_dev, void *stream);

/* ---- A9: BeamDecoder.decode -> ctcBeamSearch.decode (AA/utils/ctcDecoder.py:215-226,
 * AA/utils/BeamSearch.py:73-153): CTC prefix beam search, float64 scores.
 * lm_dev: dense (C+1)x(C+1) table of natural-log bigram scores T[prev][next] as
 * LanguageModel.get_bi_prob returns them (prev == C: sentence start, next == C: sentence end),
 * NaN where the reference would raise KeyError.  1 <= beam <= 64, 2 <= C <= 256, 0 <= blank < C; len_dev is clamped to [0,T].
 * Outputs: ids_dev [B,T] (only the first nids[b] entries of a row are written), nids_dev [B], status_dev [B] (mdd_beam_status),
 * score_dev [B] or NULL (length-normalised score of the winner; NaN for an utterance whose status is an error).
 * Kernels and limits.  With Tcap = (T + 4) & ~3 (a prefix row: one byte per id, whole words):
 *   - beam <= 16, C <= 64 and beam*C <= 1024: the single-wave kernel (beam_fast_kernel), up to four utterances per workgroup once
 *     B > 64.  Needs  lm + wave <= 160 KB  of LDS, each term rounded up to 16 bytes, with lm = 8 (C+1)^2 and
 *     wave = 24 S + 33 Tcap + 2688, S = 512 slots if beam*C <= 512, else 1024:  33 Tcap <= 161152 - 24 S - 8 (C+1)^2.
 *   - every other shape: the generic kernel (beam_kernel), one utterance per workgroup.  Needs
 *     base = 20 beam C + (2 beam + 1) Tcap <= 140 KB;  the LM table is held in LDS while base + 8 (C+1)^2 <= 96 KB and read from
 *     global memory beyond that.
 *   The generic bound is checked for every shape, so the single-wave kernel obeys both.  For C = 45: T <= 3995 at beam 10,
 *   T <= 663 at beam 64.  A shape over a limit returns MDD_ERR_ARG (mdd_last_error names the LDS need) and writes nothing.
 *   These sums, the route and the waves per workgroup are one host function, beam_plan in csrc/plan.h (tests/test_beam_plan_host.py).
 * Environment, read at every call (diagnostics and tests): MDD_BEAM_GENERIC (any value) sends every shape to the generic kernel;
 * MDD_BEAM_W = w sets the utterances per workgroup of the single-wave kernel when B > 64 and 1 <= w <= W, W = min(4, what the LDS
 * holds); any other value is ignored, and so is the variable when B <= 64 (one utterance per workgroup).  The entry reads nothing else
 * and writes only its outputs; the phase stamps of the single-wave kernel are mdd_diag_beam_stamps's (Diagnostics, below). */
int mdd_beam(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t beam,
             int32_t blank, const double *lm_dev, double lm_alpha, int32_t *ids_dev, int32_t *nids_dev,
             int32_t *status_dev, double *score_dev, void *stream);

/* ---- A9, N best: the same search, ending with the `nbest` best final hypotheses instead of the winner alone.  The reference builds this
 * list and keeps its head (AA/utils/BeamSearch.py:130-148: the final state, EOS-scored and length-normalised, sorted, `[0]` taken).
 * Inputs, argument ranges, kernels, LDS limits (the ending needs no LDS of its own: for C = 45 still T <= 3995 at beam 10, T <= 663 at
 * beam 64) and the environment switches MDD_BEAM_GENERIC / MDD_BEAM_W are those of the winner-only entry above; plus 1 <= nbest <= beam,
 * and score_dev is required.
 * Outputs, hypothesis-major: ids_dev [nbest,B,T] (only the first nids[n,b] entries of a row are written), nids_dev [nbest,B],
 * score_dev [nbest,B] (length-normalised beam score), status_dev [B].  Slice n of ids / nids / score has the winner-only entry's layout,
 * so it chains into the CTC alignment, loss and variant entries with no conversion and no copy.
 *   - Slice 0 and status are the winner-only entry's outputs bit for bit: ids, nids, status, score.
 *   - Slices are in the order of the reference's final sort() (BeamSearch.py:29-33,148): descending score; equal scores keep the order of
 *     the final beam (`BHat = last.sort()[0:beamWidth]`), as Python's stable sort leaves them.
 *   - An utterance whose status is an error has nids = 0 and score NaN in every slice, and none of its ids are written.
 *   - There is no count output: an utterance of status 0 always has exactly `beam` final hypotheses (every kept prefix re-enters the next
 *     state as itself, so once the empty prefix has left the top `beam` the state never shrinks below `beam`; while it holds fewer, the
 *     empty prefix is still among them and the ending raises IndexError), so every rank < nbest exists.
 * The score is the beam's own and no CTC likelihood (the search skips near-certain blank frames and applies its repeat rule to raw
 * frames); the loss entry on a slice gives the exact one.  A bad argument (those of the winner-only entry, nbest outside [1,beam], a NULL
 * score_dev) or a shape over an LDS limit returns MDD_ERR_ARG with nothing enqueued and nothing written; the message starts with the
 * entry's name. */
int mdd_beam_nbest(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t beam, int32_t blank,
                   const double *lm_dev, double lm_alpha, int32_t nbest,
                   int32_t *ids_dev    /* [nbest,B,T] */, int32_t *nids_dev /* [nbest,B] */,
                   int32_t *status_dev /* [B] */,         double *score_dev /* [nbest,B], required */, void *stream);

/* ---- A9, wide: the same search past the LDS limits of the two entries above, as the reference's own has none (a dict and a sort).
 * mdd_beam_fits: host only, no other effect.  1 where mdd_beam / mdd_beam_nbest would accept (T, B, C, beam) at this moment -- their
 *   argument ranges and their LDS limits, under MDD_BEAM_GENERIC / MDD_BEAM_W as they read them -- else 0.  A caller routes on it: 1, the
 *   entries above; 0, mdd_beam_wide.
 * mdd_beam_wide: 1 <= beam <= 256, 2 <= C <= 256, 1 <= T <= 38400 (mdd_greedy's bound), B >= 1, 0 <= blank < C, 1 <= nbest <= beam; every
 *   shape mdd_beam accepts is among them.  Inputs, outputs (hypothesis-major, score_dev required), status codes and the ordering of the
 *   slices are mdd_beam_nbest's; nbest = 1 is the winner.  On a shape both accept, ids, nids, status and score are mdd_beam_nbest's bits:
 *   the kernel (beam_wide_kernel, csrc/beam_wide.hip) computes every total in the generic kernel's order and selects under the same
 *   total order.  One workgroup of eight waves per utterance; the state of 2 x 256 beams in LDS, the candidate totals and the compacted
 *   candidate list in LDS up to 112 KB (8 beam C for the totals, 12 bytes per list entry in what is left) and in the workspace beyond,
 *   prefix rows (2 beam rows of Tcap bytes) in the workspace.  No environment switches.
 *   Cost to know: on inputs whose candidates tie exactly the compacted list is the whole candidate set and the rank count is quadratic
 *   in it (beam C)^2 / 512 comparisons per thread and frame.
 * workspace_dev: caller scratch of at least mdd_beam_wide_workspace_bytes(T, B, C, beam) bytes, 16-byte aligned, which holds all the call
 *   needs beyond its outputs (the pre-pass's fp64 log-probs and flags, and per utterance the live-frame list, the prefix rows and what
 *   of the candidate arrays is not in LDS); NULL = the library allocates stream-ordered for the call.  The count is one host function,
 *   beam_wide_plan in csrc/plan.h; mdd_beam_wide_workspace_bytes returns 0 for a shape outside the ranges above.
 * Bad arguments (a range above, a required pointer NULL, nbest outside [1, beam], a caller workspace that is too small) return
 *   MDD_ERR_ARG before any device work, with nothing written; the message starts with mdd_beam_wide. */
int32_t mdd_beam_fits(int32_t T, int32_t B, int32_t C, int32_t beam);
int64_t mdd_beam_wide_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t beam);
int mdd_beam_wide(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t beam, int32_t blank,
                  const double *lm_dev, double lm_alpha, int32_t nbest,
                  int32_t *ids_dev    /* [nbest,B,T] */, int32_t *nids_dev /* [nbest,B] */,
                  int32_t *status_dev /* [B] */,         double *score_dev /* [nbest,B], required */,
                  void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- Minimum-Bayes-risk decode of an N-best list (no reference counterpart: the reference sorts its final list and keeps `[0]`,
 * AA/utils/BeamSearch.py:148): every pairwise edit distance inside an utterance's list, the expected distance of each hypothesis under
 * the list's own weights, and the hypothesis that minimises it (csrc/mbr.hip, DESIGN.md "Minimum Bayes risk").
 * Inputs: ids_dev [N,B,pitch] / nids_dev [N,B], hypothesis-major: mdd_beam_nbest's and mdd_beam_wide's outputs as they are; h_n of
 *   utterance b is the first nids[n,b] ids of row (n,b).  status_dev [B] (nullable): non-zero = skip the utterance.  weight_dev [N,B]
 *   fp64, finite and >= 0, e.g. each hypothesis' share of the list's CTC likelihood; they need not sum to 1.  Optionally a reference
 *   sequence per utterance (the canonical ids): ref_dev [B,ref_pitch] / ref_len_dev [B]; both NULL or both set, ref_pitch >= 1 where set.
 * d(x, y) is the unit-cost Levenshtein distance: the `dist` of mdd_align, and the other side's length where a side is empty.  Outputs:
 *   dist_dev [B,N,N]   (nullable) dist[b,n,m] = d(h_n, h_m)
 *   risk_dev [N,B]     fp64, risk[n,b] = sum_m weight[m,b] d(h_n, h_m); written for every n, also where weight[n,b] = 0
 *   best_dev [B]       the lowest n with weight[n,b] > 0 that minimises risk[n,b]: ties go to the lower rank, so a list that agrees with
 *                      itself keeps mdd_beam's answer
 *   ref_dist_dev [N,B] (nullable) d(h_n, ref_b);   ref_risk_dev [B] (nullable) fp64, sum_n weight[n,b] d(h_n, ref_b).  Either without the
 *                      reference is an argument error
 *   flag_dev [B]       0 fine.  1 skipped: status[b] != 0, or no weight of the utterance is above 0.  2: a length outside [0, max_len]
 *                      (the reference's: outside [0, min(max_len, ref_pitch)]) or, within a row's length, an id outside [0, C) -- the
 *                      reference row included.  Looked at in this order: a skipped utterance by status is not read at all, and a bad
 *                      length or id is flag 2 whatever the weights are.  A flagged utterance has best -1, risk and ref_risk NaN, dist
 *                      and ref_dist -1, and changes nothing in its neighbours.
 * Ids past a row's length are never read.  No id is used as an index before it is range-checked: the call first packs the checked ids,
 *   one byte each, into the workspace, and the distance kernel reads only that.
 * Ranges: 1 <= N <= 256 (mdd_beam_wide's bound), B >= 1, 2 <= C <= 256, 1 <= max_len <= min(pitch, 1024).  max_len bounds nids and picks
 *   the kernel's form: 64-bit words of vertical deltas per pattern, 1, 2, 4, 8 or 16 of them for max_len up to 64, 128, 256, 512, 1024
 *   (the bit-vector recurrence of Myers / Hyyro, csrc/mbr.h).  The one-word form is the fast one: a workgroup keeps the utterance's packed
 *   list and four match tables in LDS (8 C x 4 + 64 (N + 1 rounded up to 16) bytes); the others read the list from the workspace and keep four
 *   tables of 8 C words bytes (128 KB at C = 256, 16 words).  The counts are one host function, mbr_plan in csrc/plan.h.
 * Arithmetic: the distances are integers and exact; risk in fp64, each lane of a wave adding weight[m] d for its texts m = lane, lane + 64,
 *   .. in that order, then a butterfly over the 64 lanes: no floating-point atomics, the same bits on every call.
 * workspace_dev: caller scratch of at least mdd_nbest_mbr_workspace_bytes(N, B, C, max_len) bytes (16-byte aligned; the packed lists:
 *   B x 64 words x (N + 1 rounded up to 16) bytes), NULL = the library allocates stream-ordered for the call.
 *   mdd_nbest_mbr_workspace_bytes returns 0 for a shape outside the ranges above.  Nothing synchronises.
 * Bad arguments (a range above, a required pointer NULL, the reference given in part, a ref_* output without the reference, a caller
 *   workspace that is too small) return MDD_ERR_ARG before any device work, with nothing written; the message starts with mdd_nbest_mbr
 *   and names the argument. */
int64_t mdd_nbest_mbr_workspace_bytes(int32_t N, int32_t B, int32_t C, int32_t max_len);
int mdd_nbest_mbr(const int32_t *ids_dev /* [N,B,pitch] */, int32_t pitch, const int32_t *nids_dev /* [N,B] */,
                  const int32_t *status_dev /* [B], nullable */, const double *weight_dev /* [N,B] */,
                  int32_t N, int32_t B, int32_t C, int32_t max_len,
                  const int32_t *ref_dev /* [B,ref_pitch], nullable */, const int32_t *ref_len_dev /* [B] */, int32_t ref_pitch,
                  int32_t *best_dev /* [B] */, double *risk_dev /* [N,B] */, int32_t *dist_dev /* [B,N,N], nullable */,
                  int32_t *ref_dist_dev /* [N,B], nullable */, double *ref_risk_dev /* [B], nullable */, int32_t *flag_dev /* [B] */,
                  void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- Rescoring an N-best list (no reference counterpart): the exact CTC log-likelihood of every hypothesis of every utterance in one
 * launch (csrc/ctc_nbest.hip, DESIGN.md "N-best rescoring"), where one mdd_ctc_loss call per rank staged the same log-probs N times.
 * Inputs: logp_dev [T,B,C] fp32, len_dev [B] (clamped to [0,T]); ids_dev [N,B,pitch] / nids_dev [N,B], hypothesis-major int32:
 *   mdd_beam_nbest's and mdd_beam_wide's outputs as they are.  nids is clamped to [0, max_len]; ids past a row's length are never read.
 * Output: loglik_dev [N,B] fp64, every element written.  (float)(-loglik[n,b]) has the bits of mdd_ctc_loss's nll for row (n, b) -- the
 *   kernel restates ctc_wave_kernel's alpha scan step for step: finite, -inf where the hypothesis is no CTC path of the frames (also an
 *   utterance without frames and a hypothesis with ids), 0 for an empty hypothesis of an utterance without frames, the sum of the blank
 *   column for an empty hypothesis, and NaN for that (n, b) alone where a label within the row's length is outside [0, C).
 * Ranges: 1 <= N <= 256 (mdd_beam_wide's bound), 1 <= B <= 65535 (the grid), 2 <= C <= 256, 0 <= blank < C, 0 <= max_len <= min(pitch,
 *   255), T >= 1 with the utterance's log-prob block in LDS: 4 T C <= 116 KiB (T <= 659 at C = 45, 116 at C = 256).  The bound is where
 *   mdd_ctc_loss still runs the kernel whose bits the entry reproduces; a caller routes on mdd_ctc_nbest_fits (host only, 1 / 0) and
 *   takes mdd_ctc_loss per rank otherwise.  One workgroup of eight waves per utterance and group of ranks (four while the list has no
 *   more scans than the device has SIMDs, ten beyond), a scan per wave at a time; the counts are one host function, ctc_nbest_plan in
 *   csrc/plan.h.  MDD_CTC_NBEST_WAVES = w (1..16) and MDD_CTC_NBEST_HPB = h (1..256), read at every call, set the waves and the ranks of
 *   a workgroup for timing sweeps (tools/time_ctc_nbest.py); the results do not depend on them.
 * One launch on the caller's stream, no workspace, nothing synchronises; the same call gives the same bits every time.
 * Bad arguments (a range above, a pointer NULL, a shape mdd_ctc_nbest_fits refuses) return MDD_ERR_ARG before any device work, with
 *   nothing written; the message starts with mdd_ctc_nbest and names the argument. */
int mdd_ctc_nbest_fits(int32_t T, int32_t C, int32_t max_len);         /* 1 / 0, host only */
int mdd_ctc_nbest(const float *logp_dev /* [T,B,C] */, int32_t T, int32_t B, int32_t C, const int32_t *len_dev /* [B] */,
                  const int32_t *ids_dev /* [N,B,pitch] */, int32_t pitch, const int32_t *nids_dev /* [N,B] */,
                  int32_t N, int32_t max_len, int32_t blank, double *loglik_dev /* [N,B] */, void *stream);

/* ---- MWER training (no reference counterpart; Prabhavalkar et al. 2018): the expected number of phoneme errors over the N-best list as a
 * training objective (csrc/ctc_nbest_grad.hip, DESIGN.md "MWER training").  With nll_n the CTC negative log-likelihood of hypothesis n,
 * g_n the tensor mdd_ctc_loss deposits on the log-probs for it as target, and cost[n,b] its edit distance to the annotated phones
 * (mdd_nbest_mbr's ref_dist):  P = softmax_n(-nll_n),  R_b = sum_n P_n cost_n,  dR_b/dnll_n = P_n (R_b - cost_n) =: coef[n,b], and the
 * tensor R_b deposits on the log-probs is sum_n coef[n,b] g_n.
 *
 * mdd_nbest_risk: loglik_dev [N,B] fp64 (mdd_ctc_nbest's output), cost_dev [N,B] int32, status_dev [B] or NULL -> post_dev [N,B] (the
 *   fp64 softmax over the ranks whose loglik is finite; -inf, +inf and NaN ranks get 0), risk_dev [B] = sum post cost, coef_dev [N,B] =
 *   post (risk - cost), flag_dev [B].  One wave per utterance, lanes take ranks lane, lane + 64, .. and a butterfly adds them: the same
 *   bits on every call.  flag 1: status[b] != 0, or no rank is finite; flag 2: a negative cost (the -1 of a row mdd_nbest_mbr flagged);
 *   status is looked at first, then the costs.  A flagged utterance has post and coef 0 and risk NaN.  N = 1 gives coef exactly 0.
 *   Ranges: 1 <= N <= 256, B >= 1.
 *
 * mdd_ctc_nbest_grad: grad_dev [T,B,C] = sum_n coef[n,b] g_n[t,b,c], every element written, frames >= len zeros.  Inputs as mdd_ctc_nbest
 *   takes them (len clamped to [0,T], nids to [0,max_len], ids past a row's length never read, no id an index before its range check).
 *   A rank with coef == 0 is not scanned and contributes nothing whatever its ids are: a list with one live hypothesis costs one lattice.
 *   The exp(lp) term is added once, as exp(lp) * sum_n coef (the sum in fp64, ascending n).  Lattice values are fp64 with fp32
 *   increments, as mdd_ctc_loss keeps them; with N = 1 and coef = 1 the output has the bits of mdd_ctc_loss's gradient.
 *   loglik_dev [N,B] (nullable): written for every rank; a scanned rank has the bits of mdd_ctc_nbest's value for that (n, b) (NaN where
 *   a label is outside [0, C), 0 / -inf for an utterance without frames), a skipped rank (coef == 0) NaN.
 *   flag_dev [B]: 0 fine; 1 a rank with coef != 0 is no CTC path of the frames (nll = +inf: also an utterance without frames and a live
 *   hypothesis with ids); 2 a rank with coef != 0 has a label outside [0, C), or a coef is not finite (2 wins over 1).  A flagged
 *   utterance gets all-zero gradient rows and changes nothing in its neighbours.
 *   Ranges: mdd_ctc_nbest's (1 <= N <= 256, 1 <= B <= 65535, 2 <= C <= 256, 0 <= blank < C, 0 <= max_len <= min(pitch, 255), T >= 1), and
 *   the workgroup's LDS -- the log-prob block, an accumulator of its size and ctc_wave_kernel's arrays, 8 T C + 2560 NL + 4 (C + 1) bytes
 *   within 160 KiB less 256: T <= 425 at C = 45 and max_len 255 -- which mdd_ctc_nbest_grad_fits answers (host only, 1 / 0); every shape
 *   it accepts mdd_ctc_nbest_fits accepts.  A caller takes mdd_ctc_loss per rank otherwise.
 *   Grid (groups of ranks, B), eight waves; a workgroup runs its ranks in ascending order, alpha and beta side by side on two waves,
 *   then all waves add coef * occupancy into an LDS accumulator whose every element has one owning lane.  With several groups each
 *   stores a partial slab and a second kernel adds the slabs in ascending group order.  No floating-point atomics, no switch: the same
 *   call gives the same bits.  The counts are one host function, ctc_nbest_grad_plan in csrc/plan.h.
 *   workspace_dev: mdd_ctc_nbest_grad_workspace_bytes (0 outside the ranges) or more, or NULL (allocated on the stream for the call).
 * Both entries launch on the caller's stream and synchronise nothing.  Bad arguments (a range above, a required pointer NULL, a refused
 *   shape, a caller workspace that is too small) return MDD_ERR_ARG before any device work, with nothing written; the message starts
 *   with the entry's name and names the argument. */
int mdd_nbest_risk(const double *loglik_dev /* [N,B] */, const int32_t *cost_dev /* [N,B] */, const int32_t *status_dev /* [B], nullable */,
                   int32_t N, int32_t B, double *post_dev /* [N,B] */, double *risk_dev /* [B] */, double *coef_dev /* [N,B] */,
                   int32_t *flag_dev /* [B] */, void *stream);
int mdd_ctc_nbest_grad_fits(int32_t T, int32_t C, int32_t max_len);    /* 1 / 0, host only */
int64_t mdd_ctc_nbest_grad_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t N, int32_t max_len);
int mdd_ctc_nbest_grad(const float *logp_dev /* [T,B,C] */, int32_t T, int32_t B, int32_t C, const int32_t *len_dev /* [B] */,
                       const int32_t *ids_dev /* [N,B,pitch] */, int32_t pitch, const int32_t *nids_dev /* [N,B] */,
                       int32_t N, int32_t max_len, int32_t blank, const double *coef_dev /* [N,B] */,
                       double *loglik_dev /* [N,B], nullable */, float *grad_dev /* [T,B,C] */, int32_t *flag_dev /* [B] */,
                       void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- A12: nn.CTCLoss(reduction='sum') pieces (AA/steps/train_ctc.py:72,186): alpha/beta lattice.
 * logp_dev [T,B,C], targets_dev [B,Lmax] int64 (padded), in_len_dev/tgt_len_dev [B] int64 ->
 * nll_dev [B] (per-utterance negative log-likelihood; the reference's loss is their sum; +inf for an utterance with no
 * valid alignment, as the reference gives without zero_infinity) and, if grad_dev != NULL, the tensor autograd deposits
 * on the log-probs: [T,B,C] (zero on frames >= in_len).  A target label outside [0,C) makes that utterance's nll NaN
 * and its gradient rows zero (ATen would index past the row).
 * workspace_dev: caller-owned scratch of at least mdd_ctc_workspace_bytes(T,B,C,Lmax, grad_dev != NULL) bytes (16-byte
 * aligned; the alpha/beta rows of the backward sweep); NULL = the library allocates stream-ordered for the call.
 * Bad host arguments (a required pointer NULL, T/B/C <= 0, blank outside [0,C), Lmax < 0, an Lmax past 255 whose 2 Lmax + 1
 *   lattice states do not fit the general kernel's LDS rows (Lmax > 2742), a caller workspace that is too small) return
 *   MDD_ERR_ARG before any device work. */
int64_t mdd_ctc_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Lmax, int32_t want_grad);
int mdd_ctc_loss(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int64_t *targets_dev, int32_t Lmax,
                 const int64_t *in_len_dev, const int64_t *tgt_len_dev, int32_t blank, float *nll_dev,
                 float *grad_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- CTC forced alignment (no reference counterpart): the best (max-product) path of ids through the posteriors, for phoneme
 * timestamps (align the decoded ids) and goodness-of-pronunciation scores (align the canonical ids).
 * logp_dev [T,B,C], len_dev [B] (clamped to [0,T]), ids_dev [B,ids_stride] / nids_dev [B] int32: exactly what mdd_greedy / mdd_beam
 * write, so a decode chains into an alignment with no conversion; Lmax (0 <= Lmax <= ids_stride) is the host's bound on nids that
 * sizes the launch.  Outputs:
 *   score_dev [B]   fp32 log-probability of the best path;  status_dev [B]  mdd_align_status
 *   path_dev [B,T]  (nullable) written whole: the label position i in [0,nids[b]) a frame emits, -1 for a blank frame and for t >= len
 *   seg_dev [B,ids_stride,2] + seg_logp_dev [B,ids_stride]  (nullable, only together) every position i < Lmax written: first frame and
 *                   one past the last frame of label i (its frames are contiguous) and the fp32 sum of logp[t,b,ids[i]] over them in
 *                   ascending frame order; -1, -1, 0 for nids[b] <= i < Lmax
 * MDD_ALIGN_INFEASIBLE: no path (len < nids + number of adjacent equal labels, or every path scores -inf; len = 0 with nids > 0):
 *   score -inf, path -1, seg -1,-1, seg_logp 0.  MDD_ALIGN_BAD_TARGET: a label outside [0,C) or equal to blank, or nids[b] outside
 *   [0,Lmax]: score NaN, the rest as for infeasible; other utterances are unaffected.  nids = 0 is the all-blank path (score 0 at len 0).
 * Arithmetic: fp32, one addition per state and step; on equal values staying wins over the move from s-1, which wins over the skip
 *   from s-2; the path ends in the closing blank only if that is strictly better than the last label (csrc/ctc_align.hip):
 *   a float32 loop with those rules gives the same bits.  NaN inputs are unspecified.
 * workspace_dev: caller-owned scratch of at least mdd_ctc_align_workspace_bytes(T,B,C,Lmax) bytes (16-byte aligned; 0 when the shapes
 *   fit the wave form: Lmax <= 255, C <= 256, LDS budget), NULL = the library allocates stream-ordered for the call.  Nothing
 *   synchronises.  Env MDD_CTC_ALIGN=generic (read per call) forces the general kernel; both forms give the same bits.
 * Bad host arguments (a required pointer NULL, T/B/C <= 0, blank outside [0,C), Lmax < 0 or > ids_stride, one of seg_dev /
 *   seg_logp_dev without the other, a caller workspace that is too small) return MDD_ERR_ARG before any device work. */
enum mdd_align_status { MDD_ALIGN_OK = 0, MDD_ALIGN_INFEASIBLE = 1, MDD_ALIGN_BAD_TARGET = 2 };
int64_t mdd_ctc_align_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Lmax);
int mdd_ctc_align(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev,
                  const int32_t *ids_dev, int32_t ids_stride, const int32_t *nids_dev, int32_t Lmax, int32_t blank,
                  float *score_dev, int32_t *status_dev, int32_t *path_dev, int32_t *seg_dev, float *seg_logp_dev,
                  void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- Per-phoneme CTC posteriors (no reference counterpart): the CTC log-likelihood of every sequence one edit away from ids -- every
 * substitution, deletion and insertion -- from the alpha / beta lattices of ids alone (csrc/ctc_variants.hip, DESIGN.md "One-edit
 * variants").  Inputs as mdd_ctc_align (logp_dev [T,B,C], len_dev [B] clamped to [0,T], frames >= len never read; ids_dev [B,ids_stride] /
 * nids_dev [B] int32; 0 <= Lmax <= ids_stride bounds nids).  Outputs, all absolute log-likelihoods in fp64:
 *   base_dev [B]                  log P(ids)
 *   sub_dev [B,ids_stride,C]      [i,k]: ids[i] replaced by k;  k == blank: ids[i] deleted;  k == ids[i]: base, the same bits;
 *                                 rows nids[b] <= i < Lmax are -inf, rows >= Lmax are not written
 *   ins_dev [B,ids_stride+1,C]    (nullable) [g,k]: k inserted before position g, 0 <= g <= nids[b];  k == blank: base, the same bits;
 *                                 rows nids[b] < g <= Lmax are -inf, rows > Lmax are not written
 *   status_dev [B]                mdd_align_status
 * A variant without an alignment (a repeat that len cannot hold) is -inf; that is no error.  ids itself without an alignment:
 * MDD_ALIGN_INFEASIBLE, base -inf, the variants still scored on their own.  len = 0: the empty variant scores 0, every other -inf.
 * MDD_ALIGN_BAD_TARGET (a label outside [0,C) or equal to blank, nids[b] outside [0,Lmax]): every output row of that utterance is NaN;
 * other utterances are unaffected.  Arithmetic: mdd_ctc_loss's (fp64 values, fp32 exp / log increments); no atomics, the same bits on
 * every call.  base equals -nll of mdd_ctc_loss to fp32 rounding.
 * workspace_dev: caller-owned scratch of at least mdd_ctc_variants_workspace_bytes(T,B,C,Lmax) bytes (16-byte aligned; the two lattices),
 *   NULL = the library allocates stream-ordered for the call.  Nothing synchronises.  Env MDD_CTC_VARIANTS_WAVES = 1, 2, 4 or 8 (read per call, default 4) sets the
 *   slots per workgroup of the variant kernel, for timing; the results do not depend on it.  Env MDD_CTC=generic selects the general lattice
 *   kernel as for mdd_ctc_loss (it is also what Lmax > 255 runs).
 * Bad host arguments (a required pointer NULL, T/B/C <= 0, C > 256, blank outside [0,C), Lmax < 0 or > ids_stride, an Lmax past 255 whose
 *   2 Lmax + 1 lattice states do not fit the general kernel's LDS rows (Lmax > 2742), a caller workspace that is too small) return
 *   MDD_ERR_ARG before any device work. */
int64_t mdd_ctc_variants_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Lmax);
int mdd_ctc_variants(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev,
                     const int32_t *ids_dev, int32_t ids_stride, const int32_t *nids_dev, int32_t Lmax, int32_t blank,
                     double *base_dev, double *sub_dev, double *ins_dev, int32_t *status_dev,
                     void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- Joint per-phoneme posteriors (no reference counterpart): CTC over an error network, a confusion network whose every slot may
 * emit one label or nothing (csrc/ctc_confnet.hip, DESIGN.md "Error network").  logp_dev / len_dev as mdd_ctc_variants.  Utterance b has
 * nslots_dev[b] slots, 0 <= nslots <= Jmax <= slot_stride; slot j has the C fp32 log-weights w_dev[b, j, :]: entry k != blank "slot j emits
 * label k", entry k == blank "slot j emits nothing", -inf "no such arc"; rows need not be normalised.  A reading picks one entry r_j per
 * slot; its labels are the non-blank r_j in slot order, its score sum_j w[j, r_j] + log P_CTC(labels | logp, len).  Readings are counted
 * as readings: two with the same labels both count.  The readings are weighted by the given priors -- with all-zero rows every entry
 * counts alike, so a gap slot offers C - 1 insertions at the weight of "none".  Outputs, absolute log values in fp64:
 *   total_dev [B]                 log-sum of the scores of all readings
 *   post_dev [B,slot_stride,C]    (nullable) [j,k]: log-sum over the readings with r_j = k; exp(post - total) is the posterior and
 *                                 logsumexp_k post[j,:] = total for every slot; rows nslots[b] <= j < Jmax are -inf, rows >= Jmax are not
 *                                 written.  NULL: only the forward sweep runs, total has the same bits.
 *   status_dev [B]                mdd_align_status
 * The network of ids[0..L) is 2L+1 slots, slot 2g = gap g, slot 2i+1 = position i.  With gap rows "blank only, 0" and position rows "own
 * label only, 0", total is mdd_ctc_variants' base; with one position (gap) row opened to all C entries at weight 0, its post row is that
 * call's sub (ins) row, to rounding.  len = 0: only the all-empty reading has a path.
 * MDD_ALIGN_INFEASIBLE: no reading has a path; total -inf, the written post rows -inf.  MDD_ALIGN_BAD_TARGET (nslots[b] outside [0,Jmax],
 * a NaN or +inf weight in a slot in use): total and the rows below Jmax NaN; other utterances are unaffected.  Arithmetic: mdd_ctc_loss's
 * (fp64 values, fp32 exp / log increments), no log-domain subtraction -- a reading that does not exist is exactly -inf; no atomics, the
 * same bits on every call.
 * mdd_ctc_confnet_max_slots(C): the largest Jmax accepted for C classes -- three [Jmax, C] fp64 rows of the lattice and a [16, C] one
 *   live in 159 KB of LDS: (20344 - 16 (C + 1)) / (3 C + 6), 139 at C = 45, 20 at C = 256 -- or -1 for C outside 2..256.
 * workspace_dev: caller-owned scratch of at least mdd_ctc_confnet_workspace_bytes(T,B,C,Jmax,want_post) bytes (16-byte aligned; with
 *   want_post the forward's entry flow of every frame, 8 T B C Jmax bytes, else nothing), NULL = the library allocates stream-ordered
 *   for the call.  Nothing synchronises.
 * Bad host arguments (a required pointer NULL, T/B/C <= 0, C > 256, blank outside [0,C), Jmax < 0, > slot_stride or >
 *   mdd_ctc_confnet_max_slots(C), a caller workspace that is too small) return MDD_ERR_ARG before any device work. */
int32_t mdd_ctc_confnet_max_slots(int32_t C);
int64_t mdd_ctc_confnet_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Jmax, int32_t want_post);
int mdd_ctc_confnet(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev,
                    const float *w_dev, int32_t slot_stride, const int32_t *nslots_dev, int32_t Jmax, int32_t blank,
                    double *total_dev, double *post_dev, int32_t *status_dev,
                    void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- Best reading of an error network (no reference counterpart): decoding constrained to the network of mdd_ctc_confnet, the
 * max-product sweep with a backtrace (csrc/ctc_confnet_best.hip, DESIGN.md "Best reading").  Inputs, accepted shapes (C in 2..256, Jmax <=
 * mdd_ctc_confnet_max_slots(C)) and the meaning of w_dev / nslots_dev are exactly mdd_ctc_confnet's.  The call finds
 *     max over readings r and over CTC paths pi of r's labels of   sum_j w[j, r_j] + sum_{t < len} logp[t, pi_t]
 * -- the best PAIR of reading and alignment, NOT the reading with the largest likelihood summed over its alignments.  Outputs:
 *   score_dev [B]                 fp64, that maximum
 *   reading_dev [B,slot_stride]   the entry slot j takes (the blank entry: it emits nothing); rows nslots[b] <= j < Jmax are -1, rows
 *                                 >= Jmax are not written
 *   status_dev [B]                mdd_align_status
 *   path_dev [B,T]                (nullable) written whole: the slot whose label frame t emits, -1 for a blank frame and for t >= len
 *   seg_dev [B,slot_stride,2]     (nullable) first frame and one past the last frame of the label slot j emits (its frames are
 *                                 contiguous); -1, -1 for a slot that emits nothing and for rows up to Jmax; rows >= Jmax are not written
 * path_dev / seg_dev as NULL leave the other outputs' bits unchanged.  len = 0: only the all-empty reading has a path, its score the sum
 * of the skips.  Frames >= len are never read.
 * MDD_ALIGN_INFEASIBLE: no reading has a path; score -inf, reading and path -1, seg -1, -1.  MDD_ALIGN_BAD_TARGET (nslots[b] outside
 * [0,Jmax], a NaN or +inf weight in a slot in use): score NaN, the rest as for infeasible.  Other utterances are unaffected by either.
 * Arithmetic: fp64 additions and comparisons of the fp32 inputs, no exp or log.  Exactly equal values are resolved by a fixed priority:
 *   staying in a label wins over entering it; coming from the nearer slot wins over skipping that slot (also at the end: ending in slot
 *   j wins over skipping it); among classes the lower one wins.  Values that differ only by the rounding of a differently ordered sum are
 *   not ties.  No atomics: the same bits on every call.
 * workspace_dev: caller-owned scratch of at least mdd_ctc_confnet_best_workspace_bytes(T,B,C,Jmax) bytes (16-byte aligned; the
 *   backpointers, 2 ceil(C / 64) + 1 64-bit words per frame and slot: 8 T B Jmax (2 ceil(C / 64) + 1) bytes), NULL = the library allocates
 *   stream-ordered for the call.  Nothing synchronises.
 * Bad host arguments (a required pointer NULL, T/B/C <= 0, C > 256, blank outside [0,C), Jmax < 0, > slot_stride or >
 *   mdd_ctc_confnet_max_slots(C), a caller workspace that is too small) return MDD_ERR_ARG before any device work. */
int64_t mdd_ctc_confnet_best_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Jmax);
int mdd_ctc_confnet_best(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev,
                         const float *w_dev, int32_t slot_stride, const int32_t *nslots_dev, int32_t Jmax, int32_t blank,
                         double *score_dev, int32_t *reading_dev, int32_t *status_dev, int32_t *path_dev, int32_t *seg_dev,
                         void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ---- A10: Decoder.wer core = _edit_distance + printChanges (AA/utils/ctcDecoder.py:118-184), host.
 * a = hypothesis tokens, b = canonical tokens; ops (capacity >= na+nb): 0 '-', 1 'S', 2 'I', 3 'D'.
 * Either side empty -> MDD_ERR_EMPTY (reference: TypeError). */
int mdd_align(const int32_t *a, int32_t na, const int32_t *b, int32_t nb, int32_t *dist, uint8_t *ops,
              int32_t *nops);
/* The same for the n utterances of a batch in one call (the reference loops over the batch calling decoder.wer per
 * utterance, AA/steps/test_ctc_nosil.py:218-221, AA/infer.py:318-331): row x of a / b (row pitch a_stride / b_stride
 * ids) with a_len[x] / b_len[x] ids; dist[x], nops[x] and row x of ops (pitch ops_stride >= a_len[x] + b_len[x]).
 * A row with an empty side gets dist[x] = -1, nops[x] = 0 (the reference's wer raises TypeError for it) and does not
 * fail the call. */
int mdd_align_batch(const int32_t *a, const int32_t *a_len, int32_t a_stride, const int32_t *b, const int32_t *b_len,
                    int32_t b_stride, int32_t n, int32_t *dist, uint8_t *ops, int32_t ops_stride, int32_t *nops);

/* ---- Kaldi-compatible log-mel filterbank + global CMVN (replaces the reference's subprocess pipe
 * `compute-fbank-feats --config=conf/fbank.conf | apply-cmvn --norm-vars=true data/global_fbank_cmvn.txt`,
 * AA/infer.py:567-574; options of AA/conf/fbank.conf:1-4 over Kaldi's defaults, dither 0).
 * wav_dev: n_samples mono samples at 16 kHz on the int16 scale, as float.  out_dev: [mdd_fbank_num_frames(n), 81],
 * column 0 = raw log energy, 1..80 = log mel energies; if both cmvn pointers are non-NULL (81 floats each, device)
 * every column c is written as value * scale[c] + offset[c].  Parity with Kaldi is unpinned. */
int32_t mdd_fbank_num_frames(int64_t n_samples);
int mdd_fbank(const float *wav_dev, int64_t n_samples, const float *cmvn_scale_dev, const float *cmvn_offset_dev,
              float *out_dev, void *stream);
/* The same front end for B utterances at once, up to the padded model input the reference's infer.py builds from them:
 * fbank + CMVN (AA/infer.py:567-574), then per utterance make_context(., 0, right) + skip_feat(., skip) + zero rows up to a
 * multiple of n_down (SpeechDataset.__getitem__, AA/utils/data_loader.py:123-146), then create_input's zero padding to the
 * batch's longest utterance (:151-181), all in one launch.
 * mdd_fbank_batch_len (host): T_out of that batch = max_b mdd_stack_len(mdd_fbank_num_frames(n_samples[b]), skip, n_down);
 *   -1 (and mdd_last_error names the index) if any utterance is shorter than one 400-sample window.
 * mdd_fbank_batch: wav_dev holds the B utterances back to back, utterance b at [offsets_dev[b], offsets_dev[b+1]) (int64,
 *   device, B+1 entries); T_out must be mdd_fbank_batch_len's.  out_dev [B, T_out, (right+1)*81] is written whole (padding
 *   rows included, no memset needed); every stored frame has the bits mdd_fbank gives it.  CMVN pointers as mdd_fbank. */
int32_t mdd_fbank_batch_len(const int64_t *n_samples, int32_t B, int32_t skip, int32_t n_down);
int mdd_fbank_batch(const float *wav_dev, const int64_t *offsets_dev, int32_t B, int32_t T_out,
                    const float *cmvn_scale_dev, const float *cmvn_offset_dev,
                    int32_t right, int32_t skip, int32_t n_down, float *out_dev, void *stream);
/* The train-time form of the batched front end: SpecAugment's masks (AA/utils/tools.py:229-255) applied to each utterance's own
 * [T_raw, 81] matrix after CMVN and before the stacking, where SpeechDataset.__getitem__ applies them (AA/utils/data_loader.py:132-137).
 * fmask_dev [B, NF, 2] and tmask_dev [B, NT, 2] (int32, device) hold (start, width) spans: an fmask span zeroes columns
 *   start <= c < start + width of every frame, a tmask span all 81 columns of raw frames start <= s < start + width.  A zeroed value
 *   is stored as +0.0f in every stacked slot that reads it (a zeroed last frame in each of its edge repeats).  width <= 0 is empty;
 *   any other value is intersected with the valid range (sums in 64 bits) and none leads to an access: the spans only predicate.
 *   NF = NT = 0 gives mdd_fbank_batch's bits; every value that is not masked has mdd_fbank's bits.
 *   Refused (MDD_ERR_ARG before any device call): what mdd_fbank_batch refuses, NF or NT outside 0..8, a count > 0 with a NULL
 *   pointer. */
int mdd_fbank_batch_aug(const float *wav_dev, const int64_t *offsets_dev, int32_t B, int32_t T_out,
                        const float *cmvn_scale_dev, const float *cmvn_offset_dev,
                        int32_t right, int32_t skip, int32_t n_down, float *out_dev,
                        const int32_t *fmask_dev /* [B,NF,2] */, int32_t NF,
                        const int32_t *tmask_dev /* [B,NT,2] */, int32_t NT, void *stream);
/* Global CMVN statistics on the GPU (Kaldi's compute-cmvn-stats, AA/steps/make_feat.sh:24-39): adds the sums of the un-normalised
 * fbank rows (mdd_fbank's bits) of the B utterances, laid out as for mdd_fbank_batch, to stats_dev [2, 82] (double, device):
 *   stats[0][c] += sum x_c, stats[0][81] += frames, stats[1][c] += sum x_c^2, stats[1][81] stays as it is (0).
 *   Squares and sums in fp64, no atomics, a fixed order: the same inputs give the same bits on every call.  max_samples is the
 *   host's bound on the longest utterance and sizes the grid (frames past it are not counted).  An utterance shorter than one
 *   window adds nothing.  The partial sums live in memory allocated on `stream` for the call.
 *   Refused (MDD_ERR_ARG before any device call): B outside 1..65535, max_samples < 0 or beyond 2^31 frames, a NULL pointer. */
int mdd_cmvn_accumulate(const float *wav_dev, const int64_t *offsets_dev, int32_t B, int64_t max_samples,
                        double *stats_dev /* [2,82] */, void *stream);

/* ---- Any-rate input -> 16 kHz PCM16 in front of the fbank: the reference resamples every WAV that is not 16 kHz and writes it
 * back as a 16-bit WAV (`librosa.resample(data, orig_sr=fs, target_sr=16000)` = resampy kaiser_best, then `sf.write`,
 * AA/infer.py:498-501), restated in float64 without contraction (csrc/resample.hip).  Rates 1000..384000 Hz.
 * mdd_resample_len (host, AA/infer.py:498-501): librosa's output length int(ceil(n * (16000.0 / rate))) (n itself at 16 kHz),
 *   -1 for a rate outside the range or n < 0. */
int64_t mdd_resample_len(int64_t n, int32_t rate);
/* mdd_resample_filter (host, AA/infer.py:498-501): the library's own kaiser_best table for `rate`, 32769 entries each of win (the
 *   half window, times 16000/rate when that is below 1) and delta (win[j+1] - win[j], delta[32768] = 0); cap >= 32769. */
int mdd_resample_filter(int32_t rate, double *win, double *delta, int64_t cap);
/* mdd_resample_batch (AA/infer.py:498-501): B utterances back to back in wav_dev (int16 scale, as float), utterance b at
 *   [in_off_dev[b], in_off_dev[b+1]) sampled at rates_dev[b]; writes mdd_resample_len(n_b, rate_b) samples at
 *   [out_off_dev[b], out_off_dev[b+1]) of out_dev, in one launch (one per 16 distinct rates beyond that): the quantised 16 kHz
 *   PCM16 values clamp(rint(32767 * y), -32768, 32767) as float, y the filtered x / 32768; 16 kHz rows are copied bit for bit.
 *   All arrays are device memory; the call reads the offsets and rates back (a sync of `stream`) for the launch geometry, the
 *   per-rate tables (built once per device and rate) and its checks: every row's output span must be mdd_resample_len's. */
int mdd_resample_batch(const float *wav_dev, const int64_t *in_off_dev, const int32_t *rates_dev, int32_t B,
                       const int64_t *out_off_dev, float *out_dev, void *stream);

/* ---- evaluation counts of a batch (AA/steps/test_ctc_nosil.py:33-60,218-298), host.
 * Row x of dec / lab / can (row pitch `stride` ids) holds the decoded, annotated and canonical phoneme ids of utterance x
 * with 'sil' already removed (:196-209).  counts[8] = { phonemes in canonical, TA, FR, FA, TR correctly diagnosed,
 * TR wrongly diagnosed, sum of edit distances decoded vs annotated, annotated phonemes }.  Any empty sequence ->
 * MDD_ERR_EMPTY (the reference's loop dies with TypeError there). */
int mdd_eval_batch(const int32_t *dec, const int32_t *dec_len, const int32_t *lab, const int32_t *lab_len,
                   const int32_t *can, const int32_t *can_len, int32_t n, int32_t stride, int64_t *counts);

/* ---- SURVEY 8(f) #3 / BASELINE config 5: one training step of run_epoch (AA/steps/train_ctc.py:28-105).
 * The drop-in CTC_Model keeps its parameters as torch tensors; every call receives their device pointers.
 *   mdd_train_create            geometry as mdd_create; the handle owns the activations saved between forward and backward
 *   mdd_train_tensor_info       key / element count / "is a BatchNorm running-statistics buffer" of tensor i: the 55 float entries
 *                               of CTC_Model.state_dict() (AA/models/model_ctc.py:84-158), in state_dict order
 *   mdd_train_forward           CTC_Model.forward in TRAIN mode (model_ctc.py:160-223): BatchNorm on batch statistics (biased
 *                               variance; running statistics updated in place with momentum 0.1 and the unbiased variance),
 *                               Dropout(p_drop) behind each LayerCNN and BatchRNN.  masks: NULL (masks drawn from `seed` by a
 *                               counter-based generator) or mdd_train_num_masks() device byte arrays (1 = keep) laid out like the
 *                               reference's tensor at that site -- [B,ch,T,W1], [B,ch,T/2,W2], then [T/2,B,2H] per BatchRNN --
 *                               of mdd_train_mask_bytes() bytes each.  x_dev / x1_dev must stay valid until the backward call.
 *   mdd_train_backward          autograd's backward of that forward: dlogp_dev [T/2,B,C] (e.g. mdd_ctc_loss's gradient scaled
 *                               by 1/B as train_ctc.py:73-74 divides the loss) -> one gradient per parameter into grads[i]
 *                               (entries of running-statistics buffers are ignored and may be NULL).  ONE backward per forward:
 *                               the backward overwrites activations the forward saved, so the handle holds a saved forward only
 *                               from a forward that was enqueued completely (a refused or failed forward leaves none) until the next
 *                               backward or forward; without one, mdd_train_backward returns MDD_ERR_ARG ("forward first") and
 *                               writes nothing -- also for a second backward on the same forward (autograd's retain_graph).
 *   mdd_adam_step               torch.optim.Adam over n tensors (train_ctc.py:187: lr 1e-3, weight_decay 5e-4 added to the gradient)
 *                               beta1, beta2 in [0, 1) are DOUBLES: 1 - beta, 1 - beta1^step and sqrt(1 - beta2^step) are formed in double on the
 *                               host and rounded to float once, as torch rounds them (1.f - 0.999f would be 1.3e-5 off, and exp_avg_sq with it).
 *                               Entries with a NULL parameter or gradient or numel <= 0 are passed over; step counts from 1.
 * Arithmetic: three modes, chosen per handle by mdd_train_set_precision (or MDD_TRAIN_PRECISION at create) and read by the next FORWARD:
 * the saved forward remembers its mode (and its conv1 path), and its backward follows that, whatever the handle's mode is by then.  They differ only in how the
 * LARGE CONTRACTIONS of the step run -- the BiLSTM and text-encoder input projections, dW_ih, the dW_hh products and dX:
 *   0 "f32"     exact fp32 MFMA (v_mfma_f32_*) everywhere, as the reference trains.  The default.
 *   1 "bf16x3"  flagged variant: those contractions through the split-bf16 x3 matrix-core GEMM of the decode path (operands to 16
 *               significand bits, fp32 accumulate) and the recurrences in the persistent split-bf16 layer kernels.  Narrower than the
 *               reference: log-probs within 5e-4.
 *   2 "f32x6"   reference width on the bf16 matrix cores: those contractions as f32x6 (every fp32 operand as three bf16 planes, six
 *               products, fp32 accumulate: csrc/gemm_bf16x6.hip), the weight gradients with the contraction cut into chunks that run as
 *               one launch and are summed afterwards (no atomics: run-to-run deterministic).  The recurrences -- forward and backward,
 *               about half of the exact step -- and everything else are mode 0's kernels and bits; mode 2 meets mode 0's bounds.
 * Fallback: in modes 1 and 2 a contraction outside the mode's size / alignment rule (the header comment of gemm_big, csrc/train.hip;
 * mode 2: M, N >= 128, K >= 64, M.N.K >= 2^27, leading dimensions multiples of 4, 16-byte aligned operands) runs as in mode 0.
 * Mode 1's persistent recurrences are built for hidden 256 / 384 (forward up to 512 rows, backward up to 256); any other hidden size or
 * batch runs the exact per-step recurrences of mode 0, decided before anything is enqueued.  A geometry whose contractions are all under
 * the mode's thresholds therefore computes mode 0's step in modes 1 and 2. */
typedef struct mdd_train_ws mdd_train_ws;
int mdd_train_create(const mdd_config *cfg, int device, mdd_train_ws **out);
int mdd_train_set_precision(mdd_train_ws *w, int32_t mode);   /* 0 exact fp32 (default), 1 split-bf16 x3, 2 f32x6 contractions */
void mdd_train_destroy(mdd_train_ws *w);
int32_t mdd_train_num_tensors(mdd_train_ws *w);
int mdd_train_tensor_info(mdd_train_ws *w, int32_t i, char *key, int32_t cap, int64_t *numel, int32_t *is_buffer);
int32_t mdd_train_num_masks(mdd_train_ws *w);
int64_t mdd_train_mask_bytes(mdd_train_ws *w, int32_t site, int32_t B, int32_t T);
int mdd_train_forward(mdd_train_ws *w, float *const *tensors, const float *x_dev, int32_t B, int32_t T, const int64_t *x1_dev, int32_t L,
                      const uint8_t *const *masks, uint64_t seed, float p_drop, float *logp_dev, void *stream);
int mdd_train_backward(mdd_train_ws *w, float *const *tensors, const float *dlogp_dev, float *const *grads, void *stream);
int mdd_train_sync(mdd_train_ws *w, void *stream);
int mdd_adam_step(float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq, const int64_t *numel, int32_t n,
                  int32_t step, float lr, double beta1, double beta2, float eps, float weight_decay, void *stream);

/* ---- Diagnostics (test and measurement aid; no reference counterpart).
 * mdd_diag_gemm_ph8: race screen of the 8-phase projection GEMM -- the same pseudo-random operands through the single-barrier
 * kernel and the 8-phase kernel, `reps` times each; *mismatches_out = C words of the 8-phase kernel that ever differed
 * (must be 0; tests/test_gpu_parity.py::test_gemm_8phase_race_screen).  ms_out (nullable, 16 floats; other slots are left alone):
 * [0] single-barrier, [1] 8-phase mean kernel ms; with MDD_GEMM_STAMP set [3..6] the 8-phase kernel's load-phase / load-barrier /
 * MFMA-phase / MFMA-barrier cycles per K-tile and wave; with MDD_GEMM_T128 set [14] the 128x128 kernel's mean ms on the same problem. */
int mdd_diag_gemm_ph8(int M, int N, int K, int reps, unsigned seed, unsigned *mismatches_out, float *ms_out);
/* mdd_diag_gates: the gate nonlinearities of the reference-width recurrences (csrc/lstm_persist.h) evaluated on n device floats:
 * sig_dev[i] = sigmoid(x_dev[i]), tanh_dev[i] = tanh(x_dev[i]) (tests/test_gpu_parity.py::test_gate_functions_accuracy). */
/* mdd_diag_gemm: C_dev[M,N] = A_dev[M,K] . W_dev[N,K]^T through one arithmetic (0 exact fp32 MFMA, 1 split-bf16 x3,
 * 3 the f32x6 kernel; any other mode is MDD_ERR_ARG), fp32 operands and result on the device; synchronises (tests/test_gpu_parity.py::test_gemm_f32x6_accuracy). */
int mdd_diag_gemm(int mode, const float *A_dev, const float *W_dev, float *C_dev, int M, int N, int K, void *stream);
/* mdd_diag_gemm_ops: C_dev[M,N] (row stride ldc) = opA . opB^T in the operand forms of the training step's large contractions:
 * opA[m,k] = ta ? A_dev[k*lda + m] : A_dev[m*lda + k], opB[n,k] likewise with tb / ldb.  mode 0: the exact-fp32 kernels; mode 3: the f32x6
 * path (operands split -- transposed on the way for ta / tb -- into K-tile-major planes with the contraction zero-padded to whole K-tiles);
 * splits = 1 the one-launch form, splits > 1 the split-K form with that many chunks.  Any size: the training step's
 * dispatch thresholds do not apply.  Synchronises (tests/test_train_f32x6.py). */
int mdd_diag_gemm_ops(int mode, int ta, int tb, const float *A_dev, int lda, const float *B_dev, int ldb, float *C_dev, int ldc, int M, int N, int K,
                      int splits, void *stream);
/* mdd_diag_gemm_time: mean milliseconds of `reps` launches of one GEMM kernel on resident, pre-split pseudo-random operands. */
int mdd_diag_gemm_time(int mode, int M, int N, int K, int reps, float *ms_out);
/* mdd_diag_gemm_clock: mdd_diag_gemm_time of the f32x6 kernel (mode 3), and the clock the chip held inside it straight behind those
   launches, in MHz: the median over workgroups of shader-clock ticks per tick of the 100 MHz constant clock, stamped once around the
   tile loop of the diagnostic instantiation.  The f32x6 launches of the mdd_diag_gemm* entries take their tile walk from
   MDD_GEMM_X6_RASTER as it stands at the call (rows, or <rb>x<cb> blocks; csrc/gemm_raster.h) and their tile from MDD_GEMM_X6_RT
   (3: 192 x 128, 4: 256 x 128; unset: the launcher's rule, in mdd_diag_gemm_ops the training step's 3), and return MDD_ERR_ARG for
   any other value of either. */
int mdd_diag_gemm_clock(int M, int N, int K, int reps, float *ms_out, float *mhz_out);
/* mdd_diag_conv_time: mean milliseconds of `reps` launches of the f32x6 conv front end on pseudo-random features [B, T, 243] and weights.
   which: 0 the default kernel, 1 the row-at-a-time kernel.  phases (nullable; 8 waves x 10 phases): mean cycles per workgroup of each
   wave in each phase, from one launch of the stamped instantiation of the default kernel.  mismatch (nullable): the number of output
   words in which the two kernels differ. */
int mdd_diag_conv_time(int B, int T, int reps, int which, float *ms_out, double *phases, long long *mismatch);
/* mdd_diag_beam_stamps: mdd_beam (same arguments, outputs and refusals; the outputs are mdd_beam's bits) through the stamped instantiation of
   the single-wave kernel.  stamps_dev [B,12], the caller's own buffer: per utterance the cycles its wave spent in each of the eleven phases
   of the frame loop, summed over the live frames (tools/beam_stamps.py names them), and in word 11 the sum of the candidate-list lengths.
   Returns MDD_ERR_ARG with nothing enqueued and nothing written when stamps_dev is NULL or the shape is not routed to the single-wave
   kernel (beam > 16, C > 64, beam*C > 1024, or MDD_BEAM_GENERIC set): the generic kernel has no stamps. */
int mdd_diag_beam_stamps(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t beam,
                         int32_t blank, const double *lm_dev, double lm_alpha, int32_t *ids_dev, int32_t *nids_dev,
                         int32_t *status_dev, double *score_dev, long long *stamps_dev /* [B,12] */, void *stream);
int mdd_diag_gates(const float *x_dev, float *sig_dev, float *tanh_dev, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MDD_HIP_H */

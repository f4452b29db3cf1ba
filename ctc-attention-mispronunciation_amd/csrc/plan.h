// Kernel selection of the decode forward in one place: which kernel each stage of api.hip's forward_stages() runs, as a pure function of the
// geometry, the arithmetic mode, the environment switches, what the device can hold and the batch size; and the sizes of the persistent layers'
// exchange buffers.  Host only: no HIP, no device code (tests/test_host.py builds it with the host compiler and checks the selection table).
//
// Environment switches.  read_switches() parses them once, in mdd_create, mdd_create_ctc and mdd_train_create; a handle keeps what it read for its
// whole life, so a switch is set before the handle is created.  Any other value of a switch is its default.
//
//   switch               selects                                                      read at   relied on by
//   MDD_PRECISION=m      the arithmetic mode a handle starts in: f32x6|2 (default),   create    infer.py --precision
//                        f32|0 or bf16x3|1 (mdd_set_precision changes it later)
//   MDD_GRAPH=0          every forward enqueued stage by stage, no captured graph     create    (diagnostic)
//   MDD_LSTM=step        the per-step recurrence in every mode: no persistent layer   create    test_persistent_f32_lstm_batch_sizes_match_step_kernels,
//                        launch, no device gate (a second process on the device)                test_persistent_f32_lstm_full_length_and_poisoned_input,
//                                                                                               test_bench_two_ranks_rehearsal, test_bench_exchange_runs_beside_the_next_forward,
//                                                                                               test_forward_tiles_against_float64[*-f32-step],
//                                                                                               test_variant_forward_is_the_persistent_layer_kernel, tools/lstm_bcheck.py
//   MDD_LSTM=x3          mode 1: lstm_step_x3_kernel, the LDS-tiled split-bf16 step;  create    test_persistent_lstm_equals_step_kernels_bitwise,
//                        modes 0 and 2: the packed step kernel                                  test_persistent_lstm_batch_sizes_match_step_kernels,
//                                                                                               test_fused_batches_of_different_lengths_equal_their_own_runs[*-bf16x3-x3],
//                                                                                               test_fused_batches_straddling_64_equal_their_own_runs[*-bf16x3-x3],
//                                                                                               test_forward_tiles_against_float64[*-bf16x3-x3]
//   MDD_LSTM_X6=0        mode 2: the exact-fp32 layer kernel instead of the f32x6 one create    test_persistent_x6_lstm_tracks_exact_fp32_recurrence,
//                                                                                               test_persistent_x6_lstm_full_length_and_poisoned_input, tools/lstm_kernel_choice.py
//   MDD_LSTM_X6=force    mode 2: the f32x6 layer kernel wherever it can run           create    test_persistent_x6_lstm_tracks_exact_fp32_recurrence,
//                                                                                               test_forward_tiles_against_float64[H256-*-f32x6-x6force]
//   MDD_CONV=rowwise     mode 2: the row-at-a-time conv_fused_kernel<3>               create    tests/test_conv_multirow.py, tests/test_conv_pipeline.py
//   MDD_LSTM_DBG         persistent layer launches with T' > 100 write phase stamps   create    test_persistent_lstm_stale_panel_redo_path, tools/lstm_stamps.py,
//                        behind their exchange buffer (mdd_tap "lstm_dbg")                      tools/lstm_f32_stamps.py
//   MDD_LSTM_EARLY       split-bf16 layer kernel: the next panel requested a whole    create    test_persistent_lstm_stale_panel_redo_path
//                        MFMA section early, so that the redo path runs
//   MDD_X6_FORCE_REDO=n  f32x6 layer kernel: every n-th phase declared stale (n a     create    test_persistent_x6_lstm_redo_branch
//                        power of two), so that the refetch branch runs
//   MDD_X6_OUT=fp32      f32x6 layer kernel: fp32 layer outputs and a launch_split3   create    tests/test_x6_plane_output.py
//                        pass in front of the next projection, instead of the layer
//                        kernel writing that projection's bf16 planes itself
//   MDD_TEXT_PROJ=gemm   modes 0 and 2: the text encoder's input projection as a GEMM  create    tests/test_text_table.py
//                        per call (embed_kernel, gemm_text), instead of a gather from
//                        the weight set's table of projected embedding rows
//   MDD_SCORE_TILE=128   modes 0 and 2: the attention scores on the 128-column tile   create    tests/test_score_tile.py
//                        of gemm_nt_f32_kernel where L <= 64, instead of the
//                        64-column one
//   MDD_GEMM_X6_RASTER   gemm_f32x6_kernel's tile walk (gemm_raster.h): rows is the    create    tests/test_gemm_raster.py, tools/gemm_time.py
//                        row walk in every launch, <rb>x<cb> blocks of that shape     (the mdd_diag_gemm* entries read it per call
//                        instead of the default's                                      and refuse any other value)
//   MDD_GEMM_X6_RT=3|4   gemm_f32x6_kernel's tile in every projection and the text     create    tests/test_gemm_x6_rt4.py, tools/gemm_time.py
//                        table's product: 192 x 128 (3) or 256 x 128 with the hi.hi   (the mdd_diag_gemm* entries read it per call
//                        total in LDS (4), instead of x6_choose_tile's rule per        and refuse any other value)
//                        launch (gemm_raster.h); the same bits either way
//   MDD_TRAIN_PRECISION  training handle: bf16x3|1 starts it in the split-bf16        create    train.py
//                        variant (mdd_train_set_precision changes it later)
//   MDD_TRAIN_PRECISION  training handle: f32x6|2 starts it with the large            create    train.py, tests/test_train_f32x6.py
//                        contractions as f32x6 on the bf16 matrix cores
//   MDD_TRAIN_CONV1_IM2COL  training handle: conv1 as im2col + GEMM in the forward    create    tests/test_forward_call.py
//                        and the backward, instead of the direct kernels
//
// The training handle takes MDD_LSTM=step (per-step recurrence in its split-bf16 variant too), MDD_GEMM_X6_RASTER (its one-launch f32x6
// products; the split-K ones are always in the row walk), its own two switches and nothing else of this table: its persistent layer
// launches carry no diagnostics, and its f32x6 products stay on the 192-row tile.
//
// The beam entries take no handle: their two switches (MDD_BEAM_GENERIC, MDD_BEAM_W) are read at every call by read_beam_switches(), and
// beam_plan() below is their selection, the same kind of pure function.  mdd_ctc_nbest's two (MDD_CTC_NBEST_WAVES, MDD_CTC_NBEST_HPB: the
// handles of its timing sweep) are read at every call by read_ctc_nbest_switches() for ctc_nbest_plan().
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mdd_hip.h"
#include "gemm_raster.h"

namespace mdd {

struct Switches {
    int precision = 2;          // MDD_PRECISION
    bool graph = true;          // MDD_GRAPH
    bool lstm_step = false;     // MDD_LSTM=step
    bool lstm_x3 = false;       // MDD_LSTM=x3
    bool x6_off = false;        // MDD_LSTM_X6=0
    bool x6_force = false;      // MDD_LSTM_X6=force
    bool conv_rowwise = false;  // MDD_CONV=rowwise
    bool lstm_dbg = false;      // MDD_LSTM_DBG
    bool lstm_early = false;    // MDD_LSTM_EARLY
    int x6_redo_mask = -1;      // MDD_X6_FORCE_REDO=n: n - 1, or -1 (off)
    bool x6_out_fp32 = false;   // MDD_X6_OUT=fp32
    bool text_gemm = false;     // MDD_TEXT_PROJ=gemm
    bool score_wide = false;    // MDD_SCORE_TILE=128
    X6Raster x6_raster = kX6DefaultRaster;   // MDD_GEMM_X6_RASTER
    int x6_rt = kX6RtRule;      // MDD_GEMM_X6_RT=3|4
    int train_precision = 0;    // MDD_TRAIN_PRECISION
    bool train_conv1_im2col = false;   // MDD_TRAIN_CONV1_IM2COL
};

inline Switches read_switches() {
    Switches s;
    auto is = [](const char *e, const char *v) { return e && !strcmp(e, v); };
    const char *e = getenv("MDD_PRECISION");
    if (is(e, "f32") || is(e, "0")) s.precision = 0;
    if (is(e, "bf16x3") || is(e, "1")) s.precision = 1;
    e = getenv("MDD_GRAPH");
    s.graph = !(e && e[0] == '0');
    e = getenv("MDD_LSTM");
    s.lstm_step = is(e, "step");
    s.lstm_x3 = is(e, "x3");
    e = getenv("MDD_LSTM_X6");
    s.x6_off = e && e[0] == '0';
    s.x6_force = e && e[0] == 'f';
    s.conv_rowwise = is(getenv("MDD_CONV"), "rowwise");
    s.lstm_dbg = getenv("MDD_LSTM_DBG") != nullptr;
    s.lstm_early = getenv("MDD_LSTM_EARLY") != nullptr;
    e = getenv("MDD_X6_FORCE_REDO");
    const int n = e ? atoi(e) : 0;
    if (n > 0 && (n & (n - 1)) == 0) s.x6_redo_mask = n - 1;
    s.x6_out_fp32 = is(getenv("MDD_X6_OUT"), "fp32");
    s.text_gemm = is(getenv("MDD_TEXT_PROJ"), "gemm");
    s.score_wide = is(getenv("MDD_SCORE_TILE"), "128");
    s.x6_raster = x6_raster_from_env(getenv("MDD_GEMM_X6_RASTER"));
    s.x6_rt = x6_rt_from_env(getenv("MDD_GEMM_X6_RT"));
    e = getenv("MDD_TRAIN_PRECISION");
    if (is(e, "bf16x3") || is(e, "1")) s.train_precision = 1;
    if (is(e, "f32x6") || is(e, "2")) s.train_precision = 2;
    s.train_conv1_im2col = getenv("MDD_TRAIN_CONV1_IM2COL") != nullptr;
    return s;
}

// Whether a device holds the whole grid of each persistent layer kernel (persistent_grid_fits, persistent_f32_grid_fits,
// persistent_x6_grid_fits), asked once at create.
struct DeviceFit { bool granule, f32, x6; };

// Width after a 3x3 convolution with stride 2 and padding 1, and the first BiLSTM layer's input width.
inline int conv_out(int w) { return (w + 2 - 3) / 2 + 1; }
inline int rnn_in(const mdd_config &c) { return c.channels * conv_out(conv_out(c.feat)); }

// W_hh' in the packed consumer layout (lstm_step_packed_kernel, lstm_layer_f32_kernel); every persistent layer kernel and the
// split-bf16 step kernel are built for these hidden sizes only.
inline bool packed_whh(const mdd_config &c) { return c.hidden == 384 || c.hidden == 256; }

// The attention tail (attn.hip) keeps 16 rows of attention weights in LDS next to its classifier operands, 160 KB in all, which bounds
// the canonical length L of a forward.  mfma_tail: the matrix-core tail's condition (J = 4H / 64 float4 groups per wave quarter, four at a
// time; three 16-column classifier tiles); every other geometry runs the scalar tail.  launch_attn_tail checks the same sums per call.
inline bool mfma_tail(const mdd_config &c) { return (4 * c.hidden) % 256 == 0 && c.num_class <= 48; }
inline long max_canonical_len(const mdd_config &c) {
    //   matrix-core tail  4 * (16 * ((L + 3) & ~3) + 16 * (2H + 4) + 4 * 16 * 48) <= 163840   ->   L <= 2364 - 2H
    //   scalar tail       4 * (16 * L + 16 * 4H + 16 * C) <= 163840                           ->   L <= 2560 - 4H - C
    return mfma_tail(c) ? 2364L - 2L * c.hidden : 2560L - 4L * c.hidden - c.num_class;
}

// The geometries mdd_create and mdd_train_create accept (include/mdd_hip.h at mdd_config): nullptr, or what is wrong with c.
//   hidden    a multiple of 4 (the gate-packed rows u * 4 + g and the float4 gate loads of every recurrence), at most 1024 (the training
//             step's column statistics hold 8H sums), and small enough that the attention tail holds at least one canonical phoneme
//   channels  32 or 4: the instantiations of the convolution kernels
//   emb_dim   a multiple of 4: an embedding row, and a row of the text projection's operand, is then whole 16-byte vectors (the only form
//             the training handle has ever accepted; the decode GEMM would take its scalar-load form otherwise, which no test runs)
static constexpr int kMaxHidden = 1024;
// the fields both model families share, in the order the messages have always come
inline const char *acoustic_geometry_error(const mdd_config &c) {
    if (c.feat < 3) return "feat must be at least 3";
    if (c.hidden < 4 || c.hidden % 4) return "hidden must be a positive multiple of 4";
    if (c.hidden > kMaxHidden) return "hidden must be at most 1024";
    if (c.layers < 1) return "layers must be at least 1";
    if (c.num_class < 2) return "num_class must be at least 2";
    if (c.channels != 32 && c.channels != 4) return "channels must be 32 or 4";
    return nullptr;
}
inline const char *geometry_error(const mdd_config &c) {
    if (const char *why = acoustic_geometry_error(c)) return why;
    if (c.emb_rows < 1) return "emb_rows must be at least 1";
    if (c.emb_dim < 4 || c.emb_dim % 4) return "emb_dim must be a positive multiple of 4";
    if (max_canonical_len(c) < 1) return "hidden and num_class leave the attention tail no room for a canonical phoneme (L <= 2560 - 4 hidden - num_class)";
    return nullptr;
}

// The geometries mdd_create_ctc accepts (include/mdd_hip.h at mdd_create_ctc): the CTC-only model (the reference's egs/cnn-rnn-ctc) is the
// acoustic model alone -- no embedding, no text encoder, no attention -- with the classifier BatchNorm1d(2H) + Linear(2H -> C) on the last
// BiLSTM layer's output.
//   feat, hidden, layers, num_class, channels   as geometry_error above, the same messages
//   emb_rows, emb_dim                           both 0: the model has no embedding (a handle for a model that has one comes from mdd_create)
// The attention tail's room condition does not apply: ctc_tail (ctc_tail.hip) holds no more than one row of 2H values per wave in LDS.
inline const char *ctc_geometry_error(const mdd_config &c) {
    if (const char *why = acoustic_geometry_error(c)) return why;
    if (c.emb_rows != 0) return "emb_rows must be 0 for a CTC-only model";
    if (c.emb_dim != 0) return "emb_dim must be 0 for a CTC-only model";
    return nullptr;
}
// ctc_tail's matrix-core form (J = 2H / 16 float4 groups per lane, four at a time; three 16-column classifier tiles); every other
// geometry runs its scalar form.  launch_ctc_tail checks the same sums per call.
inline bool mfma_ctc_tail(const mdd_config &c) { return (2 * c.hidden) % 64 == 0 && c.num_class <= 48; }

// 16-row tiles per team of the persistent layer kernels, which is the template instantiation a launcher picks: the 8-workgroup teams
// (lstm_granule.hip, lstm_f32.hip, lstm_bwd.hip) split the batch over 16 groups, the 16-workgroup teams (lstm_x6.hip) over 8.  What each family
// is built for: the split-bf16 and exact-fp32 layers, the training forward, the f32x6 layer, the backward layer.
inline int team8_tiles(int B) { return ((B + 15) / 16 + 15) / 16; }
inline int x6_tiles(int B) { return ((B + 7) / 8 + 15) / 16; }
static constexpr int kTeam8MaxTiles = 4, kTrainMaxTiles = 2, kX6MaxTiles = 8, kBwdMaxTiles = 1;
// Exchange buffers of the persistent layer kernels: batch rows per group of the 8-workgroup teams (padded to whole 16-row tiles), and the
// bytes of the 16-workgroup teams' buffer.  Both cover at most 1024 rows.
inline int granule_bg(int B) { return team8_tiles(B) * 16; }
inline size_t lstm_x6_hx_bytes(int H, int B) { return (size_t)2 * 16 * x6_tiles(B) * 3 * (H / 8) * 256; }
// The 8-workgroup teams' buffer, two sizes on purpose.  What the owners ALLOCATE, in floats: 2 parities x 32 teams x granule_bg(B) rows x H
// u64 granules.  What the launchers zero before every launch and the kernels use, in bytes: 2 x 32 x BG rows x H tagged 4-byte words, half of
// the allocation (the 2x slack is kept: the allocation's value is pinned by tests/test_host.py and the stamps sit behind it).
inline size_t team8_hx_alloc_floats(int H, int B) { return (size_t)2 * 32 * granule_bg(B) * H * 2; }
inline size_t team8_hx_live_bytes(int H, int BG) { return (size_t)2 * 32 * BG * H * 4; }
static constexpr size_t kHxTailFloats = 64 + 256 * 6 * 2;   // behind either buffer: a gap and the 256 x 6 diagnostic stamps (MDD_LSTM_DBG)
static constexpr int kPersistMaxB = 1024;

enum class Conv { Separate, FusedX3, FusedX6, FusedX6Rowwise };   // conv0 + conv1 | conv_fused_kernel<2> | <3, 2> | <3>
enum class Gemm { Nt, Bf16x3, F32x6 };                             // gemm_nt_f32_kernel | the bf16x3 kernels | gemm_f32x6_kernel
enum class Lstm { X6, F32, Granule, StepX3, StepPacked, Step };    // persistent layer kernels | per-step kernels (lstm_step_kernel<0>)

struct ForwardPlan {
    int precision;      // the mode in effect; in mode 1 the activations travel as split-bf16 planes and the key and score GEMMs are bf16x3
    Conv conv;
    Gemm proj;          // the input projections: gemm_ih<n>, gemm_text
    Lstm lstm;
    bool gated;         // a persistent layer kernel runs: the forward is ordered behind the device's previous one
    size_t hx_floats;   // the persistent kernels' exchange buffer with the stamp area (0 when none runs)
    size_t stamps_at;   // where the stamps start in it
    bool planes_out;    // BiLSTM layers 0 .. layers - 2 write the next projection's three bf16 planes themselves: no fp32 copy, no launch_split3 pass
    bool text_table;    // gemm_text gathers rows of the weight set's projected embedding table (DecodeWeights::text_table) instead of multiplying
};

// ctc_only: a handle of mdd_create_ctc.  Its forward has no text side: emb_dim (0 there) is no contraction length, and there is no text table.
inline ForwardPlan plan_forward(const mdd_config &c, int precision, const Switches &sw, const DeviceFit &fit, int B, bool ctc_only = false) {
    const int H = c.hidden, K0 = rnn_in(c);
    const bool packed = packed_whh(c);
    // bf16x3 and f32x6 need every contraction length a multiple of 32 (bf16x3 also the packed LSTM layouts); mode 0 otherwise
    const bool emb_ok = ctc_only || c.emb_dim % 32 == 0;
    const bool x3 = precision == 1 && packed && K0 % 32 == 0 && emb_ok;
    const bool x6 = precision == 2 && K0 % 32 == 0 && (2 * H) % 32 == 0 && emb_ok;
    ForwardPlan p{};
    p.precision = x3 ? 1 : x6 ? 2 : 0;
    if ((x3 || x6) && c.feat == 243 && c.channels == 32) p.conv = x3 ? Conv::FusedX3 : sw.conv_rowwise ? Conv::FusedX6Rowwise : Conv::FusedX6;
    else p.conv = Conv::Separate;
    p.proj = x3 ? Gemm::Bf16x3 : x6 ? Gemm::F32x6 : Gemm::Nt;
    // one persistent launch per BiLSTM layer: the split-bf16 teams in mode 1, the exact-fp32 teams in modes 0 and 2 ...
    const bool persist = fit.granule && !sw.lstm_step && !sw.lstm_x3 && packed && B <= kPersistMaxB && (x3 || fit.f32);
    // ... and in mode 2 the f32x6 teams where they are the faster of the two reference-width layer kernels (tools/lstm_kernel_choice.py,
    // profiles/round3_lstm_x6_notes.txt): at H = 384 for every batch size (0.60 - 0.93 of the exact-fp32 kernel's time), at H = 256 up to
    // 128 rows (0.83; beyond, the fp32 kernel's shorter products win: 1.07 - 1.5)
    const bool lx6 = x6 && persist && fit.x6 && !sw.x6_off && (sw.x6_force || H == 384 || B <= 128);
    if (lx6) p.lstm = Lstm::X6;
    else if (persist) p.lstm = x3 ? Lstm::Granule : Lstm::F32;
    else if (x3 && sw.lstm_x3) p.lstm = Lstm::StepX3;
    else p.lstm = packed ? Lstm::StepPacked : Lstm::Step;
    p.gated = persist;
    p.planes_out = p.proj == Gemm::F32x6 && lx6 && !sw.x6_out_fp32;
    // The table's rows carry the bits of the per-call projection where a C element depends on its own A row and W row alone, in one K order:
    // gemm_nt_f32_kernel and gemm_f32x6_kernel.  The bf16x3 launcher picks its kernel by problem size, so mode 1 keeps the per-call GEMM.
    p.text_table = !ctc_only && p.proj != Gemm::Bf16x3 && !sw.text_gemm;
    if (persist) {   // u64 granules of the 8-workgroup teams or the three bf16 planes of the 16-workgroup ones, in floats; 256 x 6 stamps behind
        const size_t granules = team8_hx_alloc_floats(H, B), planes = lstm_x6_hx_bytes(H, B) / 4;
        p.stamps_at = lx6 ? planes : granules;
        p.hx_floats = (lx6 && planes > granules ? planes : granules) + kHxTailFloats;
    }
    return p;
}

// ---- The beam entries (beam.hip): everything mdd_beam / mdd_beam_nbest decide from numbers -- the LDS needs of the two search kernels, the
// route, the waves per workgroup, and which limit a shape is over.  tests/test_beam_plan_host.py walks it against the expressions written out.
#if defined(__HIPCC__)
#define MDD_PLAN_HD __host__ __device__
#else
#define MDD_PLAN_HD
#endif

constexpr int kBeamMax = 64;       // beams of the generic kernel (beam.h: MAXBEAM)
constexpr int kBeamFastMax = 16;   // beams of the single-wave kernel (beam.h: FB)

// LDS bytes of one wave's private state in beam_fast_kernel (NS*64 slots, beam prefixes of up to Tcap ids), and of the LM table its waves share.
// The kernel lays its LDS out by these two, the plan budgets it by them.
MDD_PLAN_HD inline size_t beam_fast_wave_bytes(int NS, int beam, int Tcap) {
    constexpr int FB = kBeamFastMax;
    return sizeof(double) * ((size_t)2 * NS * 64 + 64 + 6 * FB + 4 * FB) + sizeof(unsigned long long) * 4 * FB +
           sizeof(int) * ((size_t)2 * NS * 64 + 4 * FB + 2 * FB) + (size_t)(2 * FB + 1) * Tcap;   // FB prefix rows whatever the beam: no row guards
}
MDD_PLAN_HD inline size_t beam_fast_lm_bytes(int C) { return (sizeof(double) * (size_t)(C + 1) * (C + 1) + 15) & ~(size_t)15; }

// The switches of the beam entries, read at every call (include/mdd_hip.h promises it; tests/test_decoders.py sets them per test).
struct BeamSwitches {
    bool generic = false;   // MDD_BEAM_GENERIC (any value): every shape to the generic kernel
    int w = 0;              // MDD_BEAM_W = w: utterances per workgroup of the single-wave kernel (0: unset; honoured where 1 <= w <= W and B > 64)
};
static inline BeamSwitches read_beam_switches() {   // (static, and beam_plan: no symbol of the library, the exports stay as they were)
    BeamSwitches s;
    s.generic = getenv("MDD_BEAM_GENERIC") != nullptr;
    if (const char *e = getenv("MDD_BEAM_W")) s.w = atoi(e);
    return s;
}

constexpr size_t kBeamGenericLdsMax = 140 * 1024, kBeamLmInLdsMax = 96 * 1024, kBeamFastLdsMax = 160 * 1024;
enum class BeamLimit { Ok, GenericLds, FastLds };   // "beam*C / T too large for LDS" | "T too long for LDS"
struct BeamPlan {
    BeamLimit over;      // Ok, or the first limit the shape is over, in the order the entries refuse; the fields behind it are then not filled in
    size_t over_bytes;   // the LDS need its message prints
    bool nbest;          // the ending: mdd_beam_nbest's ranked list, or the winner alone
    int Tcap;            // a prefix row: T ids + 1, in whole words
    size_t smem;         // generic kernel: dynamic LDS,
    int lm_in_lds;       //   with the LM table in it
    bool fast;           // the route: beam_fast_kernel, or beam_kernel
    int NS;              // fast kernel: slots per lane (the instantiation),
    size_t lmb, pw;      //   LDS of the shared LM table and of one wave, each rounded up to 16 bytes,
    int W;               //   waves (utterances) per workgroup; 0 on the generic route
};
static inline BeamPlan beam_plan(int T, int B, int C, int beam, bool nbest_entry, const BeamSwitches &sw) {
    BeamPlan p{};
    p.nbest = nbest_entry;
    p.Tcap = (T + 1 + 3) & ~3;
    const size_t lm_bytes = sizeof(double) * (size_t)(C + 1) * (C + 1);
    const size_t base = (sizeof(double) * 2 + sizeof(int)) * (size_t)beam * C + (size_t)(2 * beam + 1) * p.Tcap;
    p.lm_in_lds = (base + lm_bytes <= kBeamLmInLdsMax) ? 1 : 0;
    p.smem = base + (p.lm_in_lds ? lm_bytes : 0);
    if (p.smem > kBeamGenericLdsMax) { p.over = BeamLimit::GenericLds; p.over_bytes = p.smem; return p; }
    const int nslots = beam * C;
    p.fast = beam <= kBeamFastMax && C <= 64 && nslots <= 1024 && !sw.generic;
    p.NS = nslots <= 512 ? 8 : 16;
    p.lmb = beam_fast_lm_bytes(C);
    p.pw = (beam_fast_wave_bytes(p.NS, beam, p.Tcap) + 15) & ~(size_t)15;
    if (p.fast && p.lmb + p.pw > kBeamFastLdsMax) { p.over = BeamLimit::FastLds; p.over_bytes = p.lmb + p.pw; return p; }
    if (p.fast) {
        // waves per workgroup: as many as the LDS holds (<= 4); a small batch spreads out instead (one wave per CU is the
        // lowest latency when nothing else wants the CUs)
        int W = (int)((kBeamFastLdsMax - p.lmb) / p.pw);
        W = W > 4 ? 4 : W;                                              // one wave per SIMD: the kernel is built for the 512-VGPR budget
        if (B <= 64) W = 1;
        if (sw.w >= 1 && sw.w <= W) W = sw.w;
        p.W = W;
    }
    return p;
}

// ---- The wide beam entry (beam_wide.hip: mdd_beam_wide): beam <= 256 at any T mdd_greedy takes.  One workgroup of kBeamWideThreads per
// utterance; the per-beam state of 2 x 256 entries is static LDS (about 45 KB), the candidate totals and the compacted list are dynamic LDS
// while they fit kBeamWideLdsBudget and lie in the utterance's slice of the workspace beyond it; everything whose size grows with T is in the workspace.
// beam_wide_plan is the one place the byte counts and offsets come from: the host path, the kernel's arguments and
// mdd_beam_wide_workspace_bytes all read it.  The entry has no environment switches.
constexpr int kBeamWideMax = 256;          // beams of the wide kernel
constexpr int kBeamWideThreads = 512;      // its workgroup: at least kBeamWideMax threads hold maxima in the selection
constexpr int kBeamWideMaxT = 38400;       // mdd_greedy's bound on T
// Dynamic LDS of the wide kernel.  With its static 45 KB this stays under the 160 KB of a CU; one workgroup per CU either way.
constexpr size_t kBeamWideLdsBudget = 112 * 1024;
struct BeamWidePlan {
    int Tcap;              // a prefix row: T ids + 1, in whole words
    size_t n;              // candidate slots of a frame: beam * C
    int tot_in_lds;        // the candidate totals (8 n bytes) are dynamic LDS
    size_t list_cap;       // entries of the compacted list (12 bytes each) the rest of the budget holds, at most n; a frame whose list is
                           //   longer (exact ties) writes it to the workspace instead
    size_t smem;           // dynamic LDS of the launch: tot [n] f64 (if in LDS) | cl_v [list_cap] f64 | cl_o [list_cap] i32
    // the workspace: lp [T,B,C] fp64 | flags [T,B] u8 | B utterance slices of `utt` bytes; every part starts on a multiple of 16 bytes
    size_t off_flags, off_utt, utt;
    // inside a slice: live [T] i32 (the live frames, t * 2 + repeat bit) | pref [2][beam][Tcap] u8 | tot [n] f64 where not in LDS |
    // cl_v [n] f64, cl_o [n] i32 where list_cap < n (the offsets of absent parts are 0 and unused)
    size_t u_pref, u_tot, u_clv, u_clo;
    size_t bytes;          // the whole workspace
};
MDD_PLAN_HD inline size_t beam_wide_round16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline BeamWidePlan beam_wide_plan(int T, int B, int C, int beam) {
    BeamWidePlan p{};
    p.Tcap = (T + 1 + 3) & ~3;
    p.n = (size_t)beam * C;
    p.tot_in_lds = sizeof(double) * p.n <= kBeamWideLdsBudget;
    const size_t tot_lds = p.tot_in_lds ? sizeof(double) * p.n : 0;
    p.list_cap = (kBeamWideLdsBudget - tot_lds) / (sizeof(double) + sizeof(int));
    p.list_cap &= ~(size_t)1;                                       // cl_o starts on 8 bytes either way
    if (p.list_cap > p.n) p.list_cap = p.n;
    p.smem = tot_lds + (sizeof(double) + sizeof(int)) * p.list_cap;
    p.off_flags = beam_wide_round16(sizeof(double) * (size_t)T * B * C);
    p.off_utt = p.off_flags + beam_wide_round16((size_t)T * B);
    size_t u = beam_wide_round16(sizeof(int) * (size_t)T);
    p.u_pref = u;
    u += beam_wide_round16((size_t)2 * beam * p.Tcap);
    if (!p.tot_in_lds) { p.u_tot = u; u += beam_wide_round16(sizeof(double) * p.n); }
    if (p.list_cap < p.n) {
        p.u_clv = u; u += beam_wide_round16(sizeof(double) * p.n);
        p.u_clo = u; u += beam_wide_round16(sizeof(int) * p.n);
    }
    p.utt = u;
    p.bytes = p.off_utt + (size_t)B * p.utt;
    return p;
}
// The argument ranges of mdd_beam_wide, and of mdd_beam / mdd_beam_nbest (mdd_beam_fits)
inline bool beam_wide_shape_ok(int T, int B, int C, int beam) { return T >= 1 && T <= kBeamWideMaxT && B >= 1 && C >= 2 && C <= 256 && beam >= 1 && beam <= kBeamWideMax; }
inline bool beam_shape_ok(int T, int B, int C, int beam) { return T >= 1 && B >= 1 && C >= 2 && C <= 256 && beam >= 1 && beam <= kBeamMax; }

// ---- Minimum Bayes risk over an N-best list (mbr.hip: mdd_nbest_mbr): every pairwise edit distance of an utterance's N hypotheses by the
// bit-vector recurrence (mbr.h).  A pattern's vertical deltas are `words` 64-bit words; the kernel is instantiated for 1, 2, 4, 8 and 16 of
// them, so max_len is rounded up to the next of 64, 128, 256, 512, 1024.  The call first packs the ids it has range-checked, one byte each,
// into the workspace: per utterance [Lp / 4][NP] 32-bit words, word (jq, r) holding ids 4 jq .. 4 jq + 3 of row r -- the N hypotheses and,
// in column N, the reference -- so that the 64 lanes of a wave, each walking another row, read consecutive words.  A workgroup of
// kMbrWaves waves takes kMbrRowsPerBlock patterns of one utterance, a wave one pattern at a time with its match table peq [C][words] in LDS;
// in the one-word form the workgroup also holds the utterance's packed list in LDS, in the others the lanes read it from the workspace.
// mbr_plan is the one place these counts come from: the host path, the kernels' arguments and mdd_nbest_mbr_workspace_bytes read it.
constexpr int kMbrMaxN = kBeamWideMax;     // hypotheses of a list: the wide beam entry's bound
constexpr int kMbrMaxLen = 1024;           // ids of a hypothesis: 16 words
constexpr int kMbrWaves = 4;               // waves of a workgroup of the distance kernel, one pattern each at a time
constexpr int kMbrRowsPerBlock = 16;       // patterns of a workgroup: four per wave, so that the list is staged 16 times less often than read
constexpr size_t kMbrLdsMax = 160 * 1024;
struct MbrPlan {
    int words;          // 64-bit words of a pattern: 1, 2, 4, 8 or 16
    int Lp;             // ids of a packed row: 64 * words
    int NP;             // columns of the packed list: N + 1 (the reference) rounded up to 16 words = 64 bytes
    int text_in_lds;    // the one-word form: the workgroup's copy of the packed list
    size_t peq_bytes;   // the match tables of a workgroup: kMbrWaves * C * words u64
    size_t text_bytes;  // the LDS copy of the list: [16][NP] u32, or 0
    size_t smem;        // dynamic LDS of the distance kernel: peq | text
    size_t utt;         // workspace bytes of one utterance: [Lp / 4][NP] u32
    size_t bytes;       // the whole workspace
};
inline bool mbr_shape_ok(int N, int B, int C, int max_len) {
    return N >= 1 && N <= kMbrMaxN && B >= 1 && C >= 2 && C <= 256 && max_len >= 1 && max_len <= kMbrMaxLen;
}
static inline MbrPlan mbr_plan(int N, int B, int C, int max_len) {
    MbrPlan p{};
    p.words = 1;
    while (64 * p.words < max_len) p.words *= 2;
    p.Lp = 64 * p.words;
    p.NP = (N + 1 + 15) & ~15;
    p.text_in_lds = p.words == 1;
    p.peq_bytes = sizeof(unsigned long long) * (size_t)kMbrWaves * C * p.words;
    p.text_bytes = p.text_in_lds ? sizeof(unsigned) * (size_t)(p.Lp / 4) * p.NP : 0;
    p.smem = p.peq_bytes + p.text_bytes;
    p.utt = sizeof(unsigned) * (size_t)(p.Lp / 4) * p.NP;
    p.bytes = (size_t)B * p.utt;
    return p;
}

// ---- Rescoring an N-best list (ctc_nbest.hip: mdd_ctc_nbest): the exact CTC log-likelihood of every hypothesis of every utterance in one
// launch.  A workgroup of `waves` waves takes one utterance and hyps_per_block consecutive ranks: it stages the utterance's log-prob
// block [T][C] fp32 into LDS once, then every wave runs the alpha scans of its ranks on its own (labels and lattice in registers: no LDS
// per wave, no barrier behind the staging).  ctc_nbest_plan is the one place the counts come from: the entry, the launch and
// mdd_ctc_nbest_fits read it.
// consecutive labels a lane owns in the wave forms of the lattice (ctc_wave_kernel, ctc_align_wave_kernel, ctc_nbest_kernel): 64 NL >= Lmax + 1
// up to Lmax = 255
inline int ctc_labels_per_lane(int Lmax) { return Lmax <= 63 ? 1 : (Lmax <= 127 ? 2 : 4); }
constexpr int kCtcNbestMaxN = kBeamWideMax;    // hypotheses of a list: the wide beam entry's bound
constexpr int kCtcNbestMaxLen = 255;           // labels of a hypothesis: 64 lanes x 4 labels hold 2 max_len + 1 states
constexpr int kCtcNbestMaxWaves = 16;          // waves of a workgroup the kernel is built for (its launch bounds)
// Waves of a workgroup, a scan each at a time, and the ranks a workgroup takes.  A scan is bound by its SIMD's issue rate, not by waiting:
// at B = 64, N = 10 a fifth scanning wave on a CU's four SIMDs lengthens the call from 0.086 to 0.119 ms (profiles/ctc_nbest_notes.txt),
// and staging the block again costs far less than that.  So while
// the list has no more scans than the device has SIMDs, a workgroup takes four ranks, one per SIMD of its CU (its other four waves only
// help staging); beyond, ten, which stages less often and was the best or within 10 % of it at every full-device shape of the sweep,
// also where a block over 80 KiB leaves a CU one workgroup.  The ranks are then dealt evenly over the groups (10 ranks as 5 + 5, not
// 8 + 2).  The results do not depend on any of this.  MDD_CTC_NBEST_WAVES = w (1..16) and MDD_CTC_NBEST_HPB = h (1..256), read at every
// call and taken as they are, are the sweep's handles.
constexpr int kCtcNbestWaves = 8;
constexpr int kCtcNbestSimds = 256 * 4;        // of an MI355X
constexpr int kCtcNbestRanksSpread = 4, kCtcNbestRanksFull = 10;
// The log-prob block of a launch.  At most 160 KiB is a CU's; this bound is lower for the bits' sake: mdd_ctc_loss runs ctc_wave_kernel,
// whose nll the entry reproduces, while its block and 11.1 KiB of its own arrays (at C = 256, NL = 4) fit 128 KiB, and its general kernel
// with other roundings beyond.  Every shape accepted here is one mdd_ctc_loss gives to ctc_wave_kernel.
constexpr size_t kCtcNbestLdsMax = 116 * 1024;
struct CtcNbestPlan {
    int waves;            // waves of a workgroup
    int hyps_per_block;   // consecutive ranks of a workgroup: wave w scans first + w, first + w + waves, ..
    int NL;               // labels per lane: the instantiation
    size_t smem;          // dynamic LDS: lpt [T][C] f32 (the waves keep nothing else there)
    int groups;           // the grid is (groups, B): ceil(N / hyps_per_block)
};
inline bool ctc_nbest_fits(int T, int C, int max_len) {
    return T >= 1 && C >= 2 && C <= 256 && max_len >= 0 && max_len <= kCtcNbestMaxLen && sizeof(float) * (size_t)T * C <= kCtcNbestLdsMax;
}
struct CtcNbestSwitches {
    int waves = 0;   // MDD_CTC_NBEST_WAVES (0: unset)
    int hpb = 0;     // MDD_CTC_NBEST_HPB (0: unset)
};
static inline CtcNbestSwitches read_ctc_nbest_switches() {
    CtcNbestSwitches s;
    const char *e = getenv("MDD_CTC_NBEST_WAVES");
    int v = e ? atoi(e) : 0;
    if (v >= 1 && v <= kCtcNbestMaxWaves) s.waves = v;
    e = getenv("MDD_CTC_NBEST_HPB");
    v = e ? atoi(e) : 0;
    if (v >= 1 && v <= kCtcNbestMaxN) s.hpb = v;
    return s;
}
static inline CtcNbestPlan ctc_nbest_plan(int T, int B, int C, int N, int max_len, const CtcNbestSwitches &sw = CtcNbestSwitches()) {
    CtcNbestPlan p{};
    p.waves = sw.waves ? sw.waves : kCtcNbestWaves;
    p.NL = ctc_labels_per_lane(max_len);
    p.smem = sizeof(float) * (size_t)T * C;
    if (sw.hpb) {
        p.hyps_per_block = sw.hpb;
    } else {
        const bool spread = 2 * p.smem <= 160 * 1024 && (long long)N * B <= kCtcNbestSimds;
        const int target = spread ? kCtcNbestRanksSpread : kCtcNbestRanksFull, groups = (N + target - 1) / target;
        p.hyps_per_block = (N + groups - 1) / groups;
    }
    p.groups = (N + p.hyps_per_block - 1) / p.hyps_per_block;
    return p;
}

// ---- MWER training (ctc_nbest_grad.hip: mdd_ctc_nbest_grad): sum_n coef[n,b] * (the gradient mdd_ctc_loss deposits for hypothesis n) in one
// call.  A workgroup of eight waves takes one utterance and `ranks` consecutive ranks, one after the other: alpha on wave 0, beta on wave 1,
// then all waves turn frames into occupancy rows and add them into an LDS accumulator.  Its LDS is ctc_wave_kernel's with the accumulator
// beside the block:  lpt [T][C] f32 | acc [T][C] f32 | lab [LC] i32 | cls_off [C + 1] i32 | cls_idx [LC] i32 | gam [8][LC] f32  (LC = 64 NL),
// rounded up to 16 bytes, at most kCtcNbestGradLdsMax (a CU's 160 KiB less the kernel's few static bytes); the block is then at most
// 80 KiB, so every shape accepted here is one mdd_ctc_nbest_fits accepts and one mdd_ctc_loss gives to ctc_wave_kernel.
// With 90 KiB and more a CU holds one workgroup, and a rank is a chain of T dependent steps: the ranks are spread over as many groups as
// leave the launch within one workgroup per CU (kCtcNbestGradCus / B, at least one), dealt evenly (10 ranks over 8 groups as 5 x 2).
// The workspace:  rows [groups * B][2][T][SP] f64 (SP = 2 (max_len + 1): a workgroup's alpha and beta rows, reused from rank to rank) and,
// with more than one group, slabs [groups][T][B][C] f32 (each group's partial sum) and gflag [groups][B] i32.  No switch is read: the
// counts, and with them the bits, follow from the shape alone.
constexpr int kCtcNbestGradWaves = 8;
constexpr int kCtcNbestGradCus = 256;          // of an MI355X
constexpr size_t kCtcNbestGradLdsMax = 160 * 1024 - 256;
struct CtcNbestGradPlan {
    int NL;               // labels per lane: the instantiation
    int ranks;            // consecutive ranks of a workgroup
    int groups;           // the grid is (groups, B): ceil(N / ranks)
    int SP;               // pitch of a lattice row in doubles
    size_t smem;          // dynamic LDS
    size_t rows_bytes, slab_bytes, flag_bytes, bytes;      // the workspace's three parts and their sum
};
inline size_t ctc_nbest_grad_smem(int T, int C, int NL) {
    const size_t LC = 64 * (size_t)NL;
    return (2 * sizeof(float) * (size_t)T * C + 4 * LC + 4 * ((size_t)C + 1) + 4 * LC + 4 * kCtcNbestGradWaves * LC + 15) & ~(size_t)15;
}
inline bool ctc_nbest_grad_fits(int T, int C, int max_len) {
    return T >= 1 && T <= (1 << 20) && C >= 2 && C <= 256 && max_len >= 0 && max_len <= kCtcNbestMaxLen &&
           ctc_nbest_grad_smem(T, C, ctc_labels_per_lane(max_len)) <= kCtcNbestGradLdsMax;
}
static inline CtcNbestGradPlan ctc_nbest_grad_plan(int T, int B, int C, int N, int max_len) {
    CtcNbestGradPlan p{};
    p.NL = ctc_labels_per_lane(max_len);
    p.smem = ctc_nbest_grad_smem(T, C, p.NL);
    int groups = kCtcNbestGradCus / B;
    groups = groups < 1 ? 1 : (groups > N ? N : groups);
    p.ranks = (N + groups - 1) / groups;
    p.groups = (N + p.ranks - 1) / p.ranks;
    p.SP = 2 * (max_len + 1);
    p.rows_bytes = sizeof(double) * (size_t)p.groups * B * 2 * T * p.SP;
    p.slab_bytes = p.groups > 1 ? sizeof(float) * (size_t)p.groups * T * B * C : 0;
    p.flag_bytes = p.groups > 1 ? sizeof(int32_t) * (size_t)p.groups * B : 0;
    p.bytes = p.rows_bytes + p.slab_bytes + p.flag_bytes;
    return p;
}

}  // namespace mdd

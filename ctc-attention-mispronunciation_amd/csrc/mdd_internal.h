// Internal declarations shared by the translation units of libmdd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mdd_hip.h"
#include "plan.h"

namespace mdd {

void set_error(const char *fmt, ...);

#define MDD_HIP_CHECK(expr)                                                                     \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            mdd::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MDD_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

#define MDD_LAUNCH_CHECK() MDD_HIP_CHECK(hipGetLastError())

// init() runs once per device of the process (kernel attributes belong to the device that is current when they are set), under a lock;
// an init that fails runs again on the next call.  One state per family of kernels, a static of the entry that launches them.
struct OncePerDevice {
    std::mutex mu;
    bool done[64] = {false};
};
template <class Init> int once_per_device(OncePerDevice &s, Init init) {
    int dev = 0;
    MDD_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(s.mu);
    if (!s.done[dev & 63]) {
        if (int rc = init()) return rc;
        s.done[dev & 63] = true;
    }
    return MDD_OK;
}

// A device array with exactly one owner: move-only, freed by its destructor.  need(n) grows it to at least n elements by freeing
// and allocating afresh (the contents are not kept).
template <class T> struct DeviceArray {
    T *p = nullptr;
    size_t cap = 0;   // in elements
    DeviceArray() = default;
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    DeviceArray(DeviceArray &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DeviceArray &operator=(DeviceArray &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DeviceArray() { if (p) (void)hipFree(p); }
    int need(size_t n) {
        if (cap >= n) return MDD_OK;
        T *old = p;
        p = nullptr; cap = 0;
        if (old) MDD_HIP_CHECK(hipFree(old));
        MDD_HIP_CHECK(hipMalloc((void **)&p, n * sizeof(T)));
        cap = n;
        return MDD_OK;
    }
};
using DeviceBuf = DeviceArray<float>;

// A split-bf16 tensor: hi = bf16(x), lo = bf16(x - hi), two planes of the same [rows][ld] shape.
struct SplitPtr { unsigned short *hi, *lo; };

// ---- kernel launchers (each enqueues on `st`, returns an mdd_status) -------------------------
// Every GEMM launcher takes its operands and options in one shape, written at the call site with the field names:
//   launch_gemm_f32({.p = dS, .ld = L, .stride = (long)Tp * L}, {.p = key, .ld = B * H2, .k_major = true, .stride = H2}, dX, B * H2, Tp, H2, L, st,
//                   {.batch = B, .sC = H2, .accumulate = true});
struct GemmOperand {
    const float *p; int ld;    // op[r,k] = k_major ? p[k * ld + r] : p[r * ld + k]
    bool k_major = false;      // the operand is stored [K, rows]
    long stride = 0;           // elements from one matrix of a batch to the next
    int period = 0;            // > 0: matrix z of the batch is the operand's matrix z % period (several products share one), 0: matrix z.  Only
                               // launch_gemm_nt and launch_gemm_bf16x3 run it; every other launcher refuses a non-zero value
};
struct GemmOpts {
    const float *bias = nullptr;   // [N], added to every row
    int batch = 1; long sC = 0;    // `batch` products, C + z * sC each
    bool accumulate = false;       // C += the product
    int ksplit = 0;                // > 0: split-K instead of a batch -- partial product z contracts k in [z * ksplit, (z + 1) * ksplit) into C + z * sC
};
// General fp32 GEMM (training step): C[m,n] (+)= sum_k opA[m,k] opB[n,k] (see gemm.hip).
int launch_gemm_f32(const GemmOperand &A, const GemmOperand &B, float *C, int ldc, int M, int N, int K, hipStream_t st, const GemmOpts &o = GemmOpts());
// The decode path's C[M,N] = A[M,K] . W[N,K]^T (+ bias[N]); fp32 MFMA (v_mfma_f32_32x32x2_f32), batched over o.batch.  Row-major operands
// only: k_major, accumulate and ksplit are refused.  N <= 64: a 128x64 tile unless `wide`.  An operand's period is honoured on both tiles.
int launch_gemm_nt(const GemmOperand &A, const GemmOperand &W, float *C, int ldc, int M, int N, int K, hipStream_t st, const GemmOpts &o = GemmOpts(),
                   bool wide = false);

// C = A . W^T on the bf16 matrix cores with split-bf16 operands (see gemm_bf16x3.hip).  Output fp32 C, or a split-bf16 tensor when
// Csplit != nullptr.  K % 32 == 0, ld and stride % 8 == 0; accumulate and ksplit are refused.  tile128: the 128x128 kernel also on a large
// projection (timing aid).  An operand's period is honoured (the 128x128 kernel, which is what every batched product runs).
struct SplitOperand { SplitPtr p; int ld; long stride = 0; int period = 0; };   // period: as GemmOperand's
int launch_gemm_bf16x3(const SplitOperand &A, const SplitOperand &W, float *C, const SplitPtr *Csplit, int ldc, int M, int N, int K, hipStream_t st,
                       const GemmOpts &o = GemmOpts(), bool tile128 = false);
// One product through one of the 256x256-tile kernels: the 8-phase kernel (what launch_gemm_bf16x3 takes for a large projection), the
// single-barrier kernel it is screened against, or its stamped instantiation (stamps nullable: [(workgroup * 8 + wave) * 4 + phase] cycle sums
// of the first 256 workgroups).
enum class X3Form { SingleBarrier, Phase8, Phase8Stamped };
int launch_gemm_bf16x3_256(X3Form form, const SplitOperand &A, const SplitOperand &W, float *C, int ldc, int M, int N, int K, hipStream_t st,
                           const float *bias = nullptr, long long *stamps = nullptr);
int init_gemm_attributes();

// ---- fp32 -> bf16 planes (split.hip).  Two row-major planes hi | lo for the x3 GEMM:
int launch_split(const float *x, size_t n, const SplitPtr &out, hipStream_t st);
int launch_unsplit(const SplitPtr &in, size_t n, float *x, hipStream_t st);
// a matrix as it stands (the contraction along its columns, zero-padded to cols_pad) or transposed (out[c][r] = src[r][c], zero-padded to rows_pad)
int launch_split_rows(const float *src, int ld, size_t rows, int cols, int cols_pad, unsigned short *hi, unsigned short *lo, hipStream_t st);
int launch_transpose_split(const float *src, int ld, int rows, int cols, int rows_pad, unsigned short *hi, unsigned short *lo, hipStream_t st);
// x [rows][ld] (K columns used) -> three bf16 planes hi | mid | lo (rows x K elements each, consecutive), hi + mid + lo == x exactly,
// each in the K-tile-major order [K / 32][rows][32] the f32x6 kernel streams (split3_pad_kernel with Kp == K)
int launch_split3(const float *x, int rows, int K, int ld, unsigned short *planes, hipStream_t st);
// three row-major planes hi | mid | lo of n elements each
int launch_split3_rowmajor(const float *w, int n, unsigned short *planes, hipStream_t st);
// C = A . W^T with fp32-grade arithmetic on the bf16 matrix cores: operands as three K-tile-major bf16 planes each (gemm_bf16x6.hip)
// raster: the tile walk asked for (gemm_raster.h; a handle's Switches::x6_raster); the launcher falls back to the row walk per shape.
// stamps (diagnostic): the stamped instantiation's X6_STAMP_WORDS words
// rt: 16-row MFMA tiles per wave, 3 or 4 (a 192- or 256-row tile; the same bits), or kX6RtRule: x6_choose_tile decides (a handle's Switches::x6_rt)
int launch_gemm_f32x6(const unsigned short *A3, size_t a_plane, const unsigned short *W3, size_t w_plane, const float *bias, float *C, int M, int N, int K,
                      int ldc, hipStream_t st, X6Raster raster = kX6DefaultRaster, long long *stamps = nullptr, int rt = kX6RtRule);
int init_gemm_x6_attributes();
constexpr int X6_STAMP_WGS = 1024, X6_STAMP_PHASE_WORDS = X6_STAMP_WGS * 4 * 4, X6_STAMP_WORDS = X6_STAMP_PHASE_WORDS + X6_STAMP_WGS * 2;
// The same planes for the training step's operands: the contraction zero-padded from K to Kp (a multiple of 32), planes plane_elems apart.
// launch_split3_pad: x [rows][ld], K leading columns; launch_transpose_split3: x stored [K][ld], operand row r = column r of x.
int launch_split3_pad(const float *x, int rows, int K, int ld, int Kp, unsigned short *planes, size_t plane_elems, hipStream_t st);
int launch_transpose_split3(const float *x, int K, int rows, int ld, int Kp, unsigned short *planes, size_t plane_elems, hipStream_t st);
// split-K form of the f32x6 GEMM: S partial products [S][M][N] of Kc contraction elements each, in one launch (gemm_bf16x6.hip)
int launch_gemm_f32x6_splitk(const unsigned short *A3, size_t a_plane, const unsigned short *W3, size_t w_plane, float *part, int M, int N, int Kc, int S,
                             hipStream_t st);

// ---- conv_f32.hip: input stacking and the exact-fp32 convs (mode 0, the tiny geometries)
int launch_stack_skip(const float *raw, int B, int T_raw, int D, int right, int skip, int n_down, float *out,
                      hipStream_t st);
// conv0: x [B,T,F] -> y0 [B,ch,T,W1]; conv1: y0 -> seq [T/2,B,ch*W2] (BN+ReLU folded; scale/shift per channel)
int launch_conv0(const float *x, const float *w, const float *scale, const float *shift, float *y0, int B, int T, int F,
                 int ch, hipStream_t st);
int launch_conv1(const float *y0, const float *w_t, const float *scale, const float *shift, float *seq, SplitPtr seq_split, int B,
                 int T, int W1, int ch, hipStream_t st);  // seq (fp32) and/or seq_split may be null
// The channel counts the exact-fp32 conv kernels (decode and training) are built for: f(integral_constant<int, ch>), false for any other count
template <class F> bool with_conv_channels(int ch, F f) {
    if (ch == 32) f(std::integral_constant<int, 32>{});
    else if (ch == 4) f(std::integral_constant<int, 4>{});
    return ch == 32 || ch == 4;
}

// ---- conv_fused.hip (row at a time), conv_multirow.hip (launch_conv_fused3's default); what they share: conv_fused.h
// conv0 -> conv1 fused on the bf16 matrix cores (feat 243, 32 channels): x [B,T,243] -> split-bf16 rows [T/2*B, 1952]
// (w1: conv1 weights as [co][kh][kw][ci] hi/lo planes).  out_f32 optional (taps).
int launch_conv_fused(const float *x, const float *w0, const float *sc0, const float *sh0, SplitPtr w1, const float *sc1,
                      const float *sh1, SplitPtr out, float *out_f32, int B, int T, int Traw, hipStream_t st);
int launch_conv_fused3(const float *x, const float *w0, const float *sc0, const float *sh0, const unsigned short *w1_3, const float *sc1,
                       const float *sh1, unsigned short *out3, float *out_f32, int B, int T, int Traw, hipStream_t st,
                       bool rowwise = false,    // f32x6 form: three K-tile-major planes out (rowwise: the row-at-a-time kernel, MDD_CONV=rowwise)
                       long long *stamps = nullptr);   // stamps (diagnostic, default kernel only): the stamped instantiation's phase cycle sums
int init_conv_attributes();
constexpr int CM_NPH = 10;  // stamped phases per wave of the default fused3 kernel (conv_multirow.hip)

// C = opA . opB^T (+ bias) as f32x6 in the training step's operand forms (ta / tb: stored [K, rows]); S > 1: split-K into `part` and a sum.
// x6_ops_ok: the alignment half of the rule (leading dimensions multiples of 4, 16-byte aligned pointers).
bool x6_ops_ok(const GemmOperand &A, const GemmOperand &B, const float *C, int ldc);
int gemm_f32x6_ops(const GemmOperand &A, const GemmOperand &B, const float *bias, float *C, int ldc, int M, int N, int K, int S, DeviceBuf &xs_a,
                   DeviceBuf &xs_b, DeviceBuf &part, hipStream_t st, X6Raster raster = kX6DefaultRaster, int rt = 3);   // rt: the one-launch form's tile
// The same for the split-bf16 x3 GEMM (gemm_bf16x3.hip): operands as hi/lo planes with the contraction along their rows, zero-padded to S chunks
// of whole K-tiles; S > 1 (no bias, ldc == N): the chunks as a batch of partial products into `part` and a sum.
int gemm_bf16x3_ops(const GemmOperand &A, const GemmOperand &B, const float *bias, float *C, int ldc, int M, int N, int K, int S, DeviceBuf &xs_a,
                    DeviceBuf &xs_b, DeviceBuf &part, hipStream_t st);

struct LstmStepArgs {
    const float *gx;     // [T][B][2][4H], gate columns permuted to u*4+g
    const float *whh;    // [2][4H][H], rows permuted the same way
    float *hbuf;         // [2 parity][2 dir][B][H]
    float *cbuf;         // [2 dir][B][H]
    float *out = nullptr;          // [T][B][2H] layer output with oscale/oshift applied (may equal out_raw; nullable)
    SplitPtr out_split = {nullptr, nullptr};   // same values as split-bf16 planes (nullable): the next GEMM's A operand
    float *out_raw = nullptr;      // [T][B][2H] raw h (nullable)
    const float *oscale = nullptr; // [2H] (nullable -> identity)
    const float *oshift = nullptr;
    int T, B, H;
    SplitPtr whh_split;  // row-major Whh' [2][4H][H] as hi/lo planes (split-bf16 step only)
    unsigned short *hsplit;  // h exchange of the split-bf16 step: [2 parity][hi|lo][2 dir][B][H]; null selects the fp32 steps
    int packed;          // 1: whh / hbuf / cbuf use the packed consumer layouts of lstm_step_packed_kernel
    float *gates_save = nullptr;   // train mode (generic step kernel only): [T][B][2][H][4] post-activation i,f,g,o
    float *c_save = nullptr;       //                                          [T][B][2][H]    cell state
    const int *seqlen = nullptr;   // fused batches of different lengths: steps valid per batch row; the REVERSE direction holds h = c = 0 while t >= seqlen[b]
                                   // (it starts at seqlen[b]-1 with a zero state, as it would in the row's own batch); null = all T steps
    unsigned short *out_planes = nullptr;   // f32x6 layer kernel only (the others ignore it): the values of `out` as the next projection's A operand, three
    size_t out_planes_stride = 0;           // K-tile-major bf16 planes (launch_split3's layout, rows = T * B, K = 2H) out_planes_stride elements apart
};
// Enqueue all T steps of one bidirectional layer.
int launch_lstm_layer(const LstmStepArgs &a, hipStream_t st);

int launch_embed(const float *table, int rows, int E, const int64_t *ids, int B, int L, float *out, SplitPtr out_split,
                 int *err_flag, hipStream_t st);
// The same gather through a table of projected rows (the text encoder's input projection, DecodeWeights::text_table): launch_embed_index
// checks the ids by launch_embed's rule and writes the time-major row indices idx[l * B + b]; launch_gather_rows copies
// out[m, :] = table[idx[m], :] (N a multiple of 4, 16-byte aligned pointers).
int launch_embed_index(int rows, const int64_t *ids, int B, int L, int *idx, int *err_flag, hipStream_t st);
int launch_gather_rows(const float *table, const int *idx, float *out, int M, int N, hipStream_t st);
// softmax over L of S[b][t][:], ctx = A.V, y = BN(cat(X, ctx)), logits = y.Wfc^T, log-softmax
int launch_attn_tail(const float *S, int Lp, const float *X, const float *V, const float *fscale, const float *fshift,
                     const float *wfc, const float *wfcp, float *logp, int Tp, int B, int L, int H2, int C, hipStream_t st,
                     const int *llen = nullptr,    // llen[b]: canonical length of b's own batch (softmax / context over l < llen[b]); null = L
                     int Bx = 0);                  // > 0: X holds Bx acoustic rows per frame, text row b reads X row b % Bx and writes
                                                   // logp [B / Bx][Tp][Bx][C] (the K = B / Bx candidate sets of mdd_forward_candidates); 0: Bx = B

// The CTC-only model's tail (ctc_tail.hip): logp[r, :] = log_softmax((X[r, :] * fscale + fshift) . Wfc^T) over R rows of K = 2H values; wfcp: Wfc in
// the matrix-core form's lane order (DecodeWeights::w_fcp), null where the geometry runs the scalar form
int launch_ctc_tail(const float *X, const float *fscale, const float *fshift, const float *wfc, const float *wfcp, float *logp, int R, int K, int C,
                    hipStream_t st);

int init_kernel_attributes();
int init_ctc_attributes();
// The alpha / beta lattice of ctc.hip on int32 ids (mdd_ctc_variants): row t of utterance b starts at alpha + b * utt_stride + t * pitch
// (beta likewise) and holds states 0 .. 2 nids[b] (fp64, the emission at t included); frames >= len[b] and the utterances the scan rejects
// (len 0, a label outside [0, C)) are not written.  ws: ctc_lattice_bytes(T, B, C, Lmax) bytes.
struct CtcLattice { const double *alpha, *beta; long long utt_stride; int pitch; };
int64_t ctc_lattice_bytes(int T, int B, int C, int Lmax);
bool ctc_lattice_fits(int T, int C, int Lmax);   // false: Lmax is past what either form of the scan holds in LDS
int ctc_lattice(const float *logp, int T, int B, int C, const int32_t *len, const int32_t *ids, int ids_stride, const int32_t *nids, int Lmax,
                int blank, double *ws, hipStream_t st, CtcLattice *out);
// ---- lstm_step.hip: one launch per time step (launch_lstm_layer above; launch_lstm_layer_train: train.h)
int init_lstm_attributes();
// ---- lstm_persist.hip: zero fill by a kernel (n a multiple of 16, p 16-byte aligned; see its definition for why not hipMemsetAsync)
int launch_zero_fill(void *p, size_t n, hipStream_t st);
// ---- lstm_granule.hip: one launch for the whole layer (256 co-resident workgroups in 8-workgroup teams, data-tagged hand-off, no counter),
// split-bf16 arithmetic.  hx = team8_hx_alloc_floats(H, B) floats (+ stamps; plan.h), sync: 32 uints.
// Diagnostics: stamps (nullable) receive per-workgroup phase cycle sums; early requests the next panel too early (redo path).
int launch_lstm_layer_granule(const LstmStepArgs &s, unsigned short *hx, unsigned int *sync, int *err_flag, hipStream_t st,
                              long long *stamps = nullptr, bool early = false);
int init_granule_attributes();        // the forward and training-forward instantiations
int persistent_grid_fits(int n_cu);   // 1 when all 256 workgroups of a persistent layer launch can be resident at once
// ---- lstm_bwd.hip: the backward recurrence of a layer in one launch (split-bf16 training variant, B <= 256, H in {256, 384}); hx: lstm_bwd_granule_hx_bytes(H)
size_t lstm_bwd_granule_hx_bytes(int H);
int launch_lstm_bwd_granule(const float *dout, const float *gates, const float *cst, SplitPtr whhT, float *dg, int T, int B, int H, unsigned short *hx,
                            unsigned int *sync, int *err_flag, hipStream_t st);
__attribute__((visibility("hidden"))) int init_lstm_bwd_attributes();   // (hidden: the exported symbols stay as they were)
// ---- lstm_f32.hip: exact-fp32 persistent layer, same teams / exchange buffer; W_hh in the packed layout (LstmStepArgs::packed), fp32 outputs
int launch_lstm_layer_f32(const LstmStepArgs &s, unsigned short *hx, unsigned int *sync, int *err_flag, hipStream_t st, long long *stamps);
int init_lstm_f32_attributes();
int persistent_f32_grid_fits(int n_cu);
// ---- lstm_x6.hip: f32x6 persistent layer, teams of 16, W_hh' as three row-major bf16 planes [3][2][4H][H], h exchanged as three bf16 planes
// (lstm_x6_hx_bytes); fp32 outputs.  force_mask >= 0: every (force_mask + 1)-th phase is declared stale (refetch branch).
int launch_lstm_layer_x6(const LstmStepArgs &s, const unsigned short *whh3, unsigned short *hx, unsigned int *sync, int *err_flag, hipStream_t st,
                         long long *stamps, int force_mask);
int init_lstm_x6_attributes();
int persistent_x6_grid_fits(int n_cu);
// Per-device ticket around work that contains persistent launches (api.hip): launches of different handles / streams of one device run
// one after another on the GPU (event dependency; the host does not block).  enter locks, leave records the event and unlocks.
int device_gate_enter(int device, hipStream_t st, bool *held);
int device_gate_leave(int device, hipStream_t st, bool held, int rc);

}  // namespace mdd

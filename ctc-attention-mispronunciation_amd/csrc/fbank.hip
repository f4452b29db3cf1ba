// SURVEY 8(f) #1 -- Kaldi-compatible log-mel filterbank + global CMVN on the GPU: the step the reference runs as
//   compute-fbank-feats --config=conf/fbank.conf | apply-cmvn --norm-vars=true data/global_fbank_cmvn.txt
// (AA/infer.py:567-574, AA/conf/fbank.conf:1-4).  Kaldi itself is third-party and absent from the reference tree; the
// algorithm is its published one (feat/feature-window.cc, feat/mel-computations.cc, feat/feature-fbank.cc,
// transform/cmvn.cc) for: 16 kHz, 25 ms / 10 ms frames, snip-edges, no dither, remove-dc-offset, raw log-energy in
// column 0, preemphasis 0.97, hamming window, 512-point FFT, power spectrum, 80 triangular mel bins from 20 Hz to
// Nyquist, log.  PARITY UNPINNED (no Kaldi output to compare with here): tests check it against restatements of the same
// text.  tests/test_fbank.py holds every output element of both kernels, with and without CMVN, to the float64 restatement
// of tests/fbank_reference.py under its per-element conditioning model (noise, impulses, tones, Nyquist, DC, the floor,
// frame-count edges, recorded words; the batched kernel's stacking against float64 rows, not against fbank_kernel);
// tests/test_fbank_reference.py pins that restatement to oracle/oracle.py's and shows what the bound catches.
// tests/test_train_wav.py holds the train-time forms to these kernels' own rows: the masked batch (mdd_fbank_batch_aug) bit for bit,
// the global CMVN statistics (mdd_cmvn_accumulate) to their float64 sums.
//
// One wave per frame, four frames per workgroup.  A frame is 400 samples = 1.6 KB: the work is a 512-point FFT in LDS
// (9 radix-2 stages, 4 butterflies per lane and stage, wave-synchronous), 80 short dot products and a row store --
// HBM-bound at 640 B read (with 2.5x overlap from L2) and 324 B written per frame.
#include <math.h>
#include <mutex>
#include <vector>

#include "ctc_host.h"
#include "mdd_internal.h"

namespace mdd {

constexpr int FB_N = 400, FB_S = 160, FB_P = 512, FB_BINS = 80, FB_D = FB_BINS + 1, FB_HALF = FB_P / 2;

struct FbankTables {           // device pointers
    float *window;             // [400]
    float2 *twiddle;           // [256] exp(-2 pi i k / 512)
    int *first, *count, *woff; // [80] first FFT bin, number of bins, offset into weights
    float *weights;
};

#define FB_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// One frame of 400 samples at `src` -> its 81 output columns, computed by one wave in the LDS scratch z / xr of that wave.
// Lane l returns mel[0] = column 1 + l and, for l < 16, mel[1] = column 65 + l; every lane returns column 0 in `energy`.
// Shared by fbank_kernel and fbank_batch_kernel, so both give the same bits for the same frame.
__device__ __forceinline__ void fbank_frame(const float *__restrict__ src, const FbankTables &tb,
                                            const float *__restrict__ cscale, const float *__restrict__ coffset,
                                            float2 *z, float *xr, int lane, float mel[2], float &energy) {
    // 1. samples, DC offset, raw energy
    float v[7], sum = 0.f;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const int idx = lane + 64 * i;
        v[i] = idx < FB_N ? src[idx] : 0.f;
        sum += v[i];
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)FB_N;
    float e = 0.f;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const int idx = lane + 64 * i;
        if (idx < FB_N) { v[i] -= mean; e += v[i] * v[i]; xr[idx] = v[i]; }
    }
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    const float log_energy = logf(fmaxf(e, 1.1920929e-07f));
    FB_WAVE_SYNC();
    // 2. preemphasis, window, zero padding; stored bit-reversed for the in-place decimation-in-time FFT
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int idx = lane + 64 * i;
        float y = 0.f;
        if (idx < FB_N) y = (v[i < 7 ? i : 0] - 0.97f * xr[idx > 0 ? idx - 1 : 0]) * tb.window[idx];
        z[__brev((unsigned)idx) >> 23] = make_float2(y, 0.f);
    }
    FB_WAVE_SYNC();
    // 3. 9 radix-2 stages
#pragma unroll
    for (int s = 0; s < 9; s++) {
        const int half = 1 << s;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int bfly = lane + 64 * i;                    // 0..255
            const int j = bfly & (half - 1), base = ((bfly >> s) << (s + 1)) + j;
            const float2 w = tb.twiddle[j << (8 - s)];
            const float2 a = z[base], b = z[base + half];
            const float tr = b.x * w.x - b.y * w.y, ti = b.x * w.y + b.y * w.x;
            z[base] = make_float2(a.x + tr, a.y + ti);
            z[base + half] = make_float2(a.x - tr, a.y - ti);
        }
        FB_WAVE_SYNC();
    }
    // 4. power spectrum (bins 0..255 feed the mel banks), kept in the raw buffer
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int k = lane + 64 * i;
        const float2 c = z[k];
        xr[k] = c.x * c.x + c.y * c.y;
    }
    FB_WAVE_SYNC();
    // 5. mel energies, log, CMVN
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int b = lane + 64 * h;
        float val = 0.f;
        if (b < FB_BINS) {
            const int first = tb.first[b], n = tb.count[b];
            const float *w = tb.weights + tb.woff[b];
            float acc = 0.f;
            for (int k = 0; k < n; k++) acc += w[k] * xr[first + k];
            val = logf(fmaxf(acc, 1.1920929e-07f));
            if (cscale) val = val * cscale[1 + b] + coffset[1 + b];
        }
        mel[h] = val;
    }
    energy = cscale ? log_energy * cscale[0] + coffset[0] : log_energy;
}

// The 81 columns of one frame, as fbank_frame left them in the wave's registers, to one output row.
__device__ __forceinline__ void fbank_store_row(float *__restrict__ orow, int lane, const float mel[2], float energy) {
    orow[1 + lane] = mel[0];
    if (lane < FB_BINS - 64) orow[65 + lane] = mel[1];
    if (lane == 0) orow[0] = energy;
}

__global__ __launch_bounds__(256) void fbank_kernel(const float *__restrict__ wav, int nframes, FbankTables tb,
                                                    const float *__restrict__ cscale, const float *__restrict__ coffset,
                                                    float *__restrict__ out) {
    __shared__ float2 buf[4][FB_P];
    __shared__ float raw[4][FB_N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x * 4 + wave;
    if (f >= nframes) return;                      // wave-uniform: waves never meet at a workgroup barrier
    float mel[2], energy;
    fbank_frame(wav + (size_t)f * FB_S, tb, cscale, coffset, buf[wave], raw[wave], lane, mel, energy);
    fbank_store_row(out + (size_t)f * FB_D, lane, mel, energy);
}

// B utterances -> the padded, stacked batch of create_input (AA/utils/data_loader.py:123-181) in one launch.
// Wave (x, b) owns raw frame s = 4 * blockIdx.x + wave of utterance b: it computes the frame once (fbank_frame) and stores
// its 81 columns into every stacked slot (i, r) that reads it, min(i * skip + r, T_raw_b - 1) == s (make_context(., 0, right)
// repeats the last frame: AA/utils/tools.py:207-216; skip_feat keeps rows i * skip: :218-227).  The same wave also zeroes
// stacked row s when s lies in [kept_b, T_out) -- the even-pad row of data_loader.py:138-142 and the batch padding -- so every
// element of out [B, T_out, (right + 1) * 81] is written exactly once by this launch.  The grid's x extent covers
// max(T_raw_b) <= T_out * skip and T_out.
//
// AUG (mdd_fbank_batch_aug): SpecAugment's masks (AA/utils/tools.py:229-255) on the utterance's own [T_raw, 81] matrix, after CMVN and
// before the stacking, where SpeechDataset.__getitem__ applies them (AA/utils/data_loader.py:132-137).  The wave holds the frame's 81
// columns in registers, so a mask is a few compares in front of the stores: a masked value becomes +0.0f in every slot that reads it,
// the edge repeats of the last frame included.  The spans only ever predicate; no device value reaches an address.  The instantiation
// without AUG never reads `mk` and is mdd_fbank_batch's kernel as it was.
struct FbankMasks {
    const int32_t *f, *t;      // [B, nf, 2] column spans and [B, nt, 2] raw-frame spans, (start, width) each
    int nf, nt;
};

// Is x inside span (start, width) cut to [0, limit)?  width <= 0 is empty; the end is summed in 64 bits.
__device__ __forceinline__ bool fbank_in_span(int x, int start, int width, int limit) {
    if (width <= 0) return false;
    const int64_t lo = start > 0 ? start : 0;
    int64_t hi = (int64_t)start + (int64_t)width;
    if (hi > limit) hi = limit;
    return (int64_t)x >= lo && (int64_t)x < hi;
}

template <bool AUG>
__global__ __launch_bounds__(256) void fbank_batch_kernel(const float *__restrict__ wav, const int64_t *__restrict__ offsets,
                                                          int T_out, FbankTables tb, const float *__restrict__ cscale,
                                                          const float *__restrict__ coffset, int right, int skip,
                                                          float *__restrict__ out, FbankMasks mk) {
    __shared__ float2 buf[4][FB_P];
    __shared__ float raw[4][FB_N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * 4 + wave, b = blockIdx.y;
    const int64_t n = offsets[b + 1] - offsets[b];
    const int T_raw = n < FB_N ? 0 : (int)(1 + (n - FB_N) / FB_S);
    const int kept = (T_raw + skip - 1) / skip;
    const int W = (right + 1) * FB_D;
    float *ub = out + (size_t)b * T_out * W;
    if (s >= kept && s < T_out) {                  // a padding row: wave-uniform, no barrier follows
        float *orow = ub + (size_t)s * W;
        for (int j = lane; j < W; j += 64) orow[j] = 0.f;
    }
    if (s >= T_raw) return;                        // wave-uniform: waves never meet at a workgroup barrier
    float mel[2], energy;
    fbank_frame(wav + offsets[b] + (size_t)s * FB_S, tb, cscale, coffset, buf[wave], raw[wave], lane, mel, energy);
    if (AUG) {
        bool m0 = false, m1 = false, me = false;   // columns 1 + lane, 65 + lane and 0
        for (int j = 0; j < mk.nt; j++) {
            const int32_t *sp = mk.t + ((size_t)b * mk.nt + j) * 2;
            if (fbank_in_span(s, sp[0], sp[1], T_raw)) m0 = m1 = me = true;
        }
        for (int j = 0; j < mk.nf; j++) {
            const int32_t *sp = mk.f + ((size_t)b * mk.nf + j) * 2;
            const int st = sp[0], wd = sp[1];
            m0 |= fbank_in_span(1 + lane, st, wd, FB_D);
            m1 |= fbank_in_span(65 + lane, st, wd, FB_D);
            me |= fbank_in_span(0, st, wd, FB_D);
        }
        if (m0) mel[0] = 0.f;
        if (m1) mel[1] = 0.f;
        if (me) energy = 0.f;
    }
    for (int r = 0; r <= right; r++) {
        // rows i with i * skip + r == s, or, for the last frame, every i * skip + r >= s (the edge repeat)
        int i0, i1;
        if (s < T_raw - 1) {
            if (s < r || (s - r) % skip) continue;
            i0 = i1 = (s - r) / skip;
        } else {
            i0 = s > r ? (s - r + skip - 1) / skip : 0;
            i1 = kept - 1;
        }
        if (i1 >= T_out) i1 = T_out - 1;           // a T_out below the batch's stack length loses rows, never writes past them
        for (int i = i0; i <= i1; i++) fbank_store_row(ub + (size_t)i * W + r * FB_D, lane, mel, energy);
    }
}

// Global CMVN statistics (Kaldi's compute-cmvn-stats, which AA/steps/make_feat.sh:24-39 runs over the training set): the sums and
// sums of squares of the un-normalised rows.  Workgroup (x, b) walks the strip of CMVN_STRIP raw frames starting at x * CMVN_STRIP of
// utterance b; wave w takes frames w, w + 4, ... of the strip in rising order and keeps per-lane fp64 running sums (lane l: column
// 1 + l; lanes < 16 also column 65 + l; lane 0 also column 0).  The four waves meet at ONE workgroup barrier, so no wave returns early:
// the frame work is predicated (wave-uniform) and every wave reaches the barrier.  Their sums are added through LDS in wave order
// into one partial [2, 82] per workgroup; cmvn_reduce_kernel adds the partials to the statistics in index order.  No atomics: the
// same inputs give the same bits on every call.
constexpr int CMVN_STRIP = 64, CMVN_N = 2 * (FB_D + 1);

__global__ __launch_bounds__(256) void cmvn_partial_kernel(const float *__restrict__ wav, const int64_t *__restrict__ offsets,
                                                           FbankTables tb, double *__restrict__ part) {
    __shared__ float2 buf[4][FB_P];
    __shared__ float raw[4][FB_N];
    __shared__ double red[4][CMVN_N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, strip0 = blockIdx.x * CMVN_STRIP;
    const int64_t n = offsets[b + 1] - offsets[b];
    const int64_t frames = n < FB_N ? 0 : 1 + (n - FB_N) / FB_S;
    const int T_raw = frames > INT32_MAX ? INT32_MAX : (int)frames;
    double s0 = 0.0, q0 = 0.0, s1 = 0.0, q1 = 0.0, se = 0.0, qe = 0.0;
    for (int k = wave; k < CMVN_STRIP; k += 4) {
        const int f = strip0 + k;
        if (f < T_raw) {                           // wave-uniform; the wave goes on to the barrier either way
            float mel[2], energy;
            fbank_frame(wav + offsets[b] + (size_t)f * FB_S, tb, nullptr, nullptr, buf[wave], raw[wave], lane, mel, energy);
            const double a = (double)mel[0], c = (double)mel[1], e = (double)energy;
            s0 += a; q0 += a * a;
            s1 += c; q1 += c * c;
            se += e; qe += e * e;
            FB_WAVE_SYNC();                        // the next frame overwrites the scratch this one's mel sums read
        }
    }
    red[wave][1 + lane] = s0;
    red[wave][FB_D + 1 + 1 + lane] = q0;
    if (lane < FB_BINS - 64) { red[wave][65 + lane] = s1; red[wave][FB_D + 1 + 65 + lane] = q1; }
    if (lane == 0) {
        red[wave][0] = se;
        red[wave][FB_D + 1] = qe;
        red[wave][FB_D] = 0.0;                     // the count is set below, once per workgroup
        red[wave][CMVN_N - 1] = 0.0;
    }
    __syncthreads();
    const int idx = threadIdx.x;
    if (idx < CMVN_N) {
        double acc = ((red[0][idx] + red[1][idx]) + red[2][idx]) + red[3][idx];
        if (idx == FB_D) {
            const int left = T_raw - strip0;
            acc = (double)(left <= 0 ? 0 : (left < CMVN_STRIP ? left : CMVN_STRIP));
        }
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * CMVN_N + idx] = acc;
    }
}

__global__ __launch_bounds__(256) void cmvn_reduce_kernel(const double *__restrict__ part, int64_t parts, double *__restrict__ stats) {
    const int idx = threadIdx.x;
    if (idx >= CMVN_N) return;
    double acc = stats[idx];
    for (int64_t p = 0; p < parts; p++) acc += part[p * CMVN_N + idx];
    stats[idx] = acc;
}

static std::mutex g_fb_mutex;
static FbankTables g_fb_tables[16];
static bool g_fb_ready[16];

static int fbank_tables(int dev, FbankTables *out) {
    std::lock_guard<std::mutex> lk(g_fb_mutex);
    if (dev < 0 || dev >= 16) { set_error("mdd_fbank: device %d", dev); return MDD_ERR_ARG; }
    if (!g_fb_ready[dev]) {
        std::vector<float> window(FB_N);
        for (int i = 0; i < FB_N; i++) window[i] = (float)(0.54 - 0.46 * cos(2.0 * M_PI * i / (FB_N - 1)));
        std::vector<float2> tw(FB_HALF);
        for (int k = 0; k < FB_HALF; k++) tw[k] = make_float2((float)cos(-2.0 * M_PI * k / FB_P), (float)sin(-2.0 * M_PI * k / FB_P));
        // MelBanks (no VTLN): triangles in the mel domain, evaluated at the centre frequencies of FFT bins 0..255.
        // A weight is a difference of mel values near 2000 over a spacing of 35, so one ulp of the mel scale is up to 1e-4 of a
        // weight: with the C library's logf the table followed the build host (glibc's and numpy's float32 log differ in 31 of
        // these 256 values, which moved log-mel outputs by up to 12 units of tests/fbank_reference.py's model).  The scale is
        // therefore the correctly rounded one -- the double log of the float argument, rounded to float -- on every host.
        auto mel = [](float fr) { return 1127.0f * (float)log((double)(1.0f + fr / 700.0f)); };
        const float bin_width = 16000.0f / FB_P, mel_low = mel(20.0f), mel_high = mel(8000.0f);
        const float delta = (mel_high - mel_low) / (FB_BINS + 1);
        std::vector<int> first(FB_BINS), count(FB_BINS), woff(FB_BINS);
        std::vector<float> weights;
        for (int b = 0; b < FB_BINS; b++) {
            const float left = mel_low + b * delta, center = mel_low + (b + 1) * delta, right = mel_low + (b + 2) * delta;
            first[b] = -1; count[b] = 0; woff[b] = (int)weights.size();
            for (int i = 0; i < FB_HALF; i++) {
                const float m = mel(bin_width * i);
                if (m > left && m < right) {
                    if (first[b] < 0) first[b] = i;
                    count[b] = i - first[b] + 1;
                    weights.push_back(m <= center ? (m - left) / (center - left) : (right - m) / (right - center));
                }
            }
            if (first[b] < 0) first[b] = 0;
        }
        FbankTables t;
        MDD_HIP_CHECK(hipMalloc((void **)&t.window, FB_N * sizeof(float)));
        MDD_HIP_CHECK(hipMalloc((void **)&t.twiddle, FB_HALF * sizeof(float2)));
        MDD_HIP_CHECK(hipMalloc((void **)&t.first, FB_BINS * sizeof(int)));
        MDD_HIP_CHECK(hipMalloc((void **)&t.count, FB_BINS * sizeof(int)));
        MDD_HIP_CHECK(hipMalloc((void **)&t.woff, FB_BINS * sizeof(int)));
        MDD_HIP_CHECK(hipMalloc((void **)&t.weights, weights.size() * sizeof(float)));
        MDD_HIP_CHECK(hipMemcpy(t.window, window.data(), FB_N * sizeof(float), hipMemcpyHostToDevice));
        MDD_HIP_CHECK(hipMemcpy(t.twiddle, tw.data(), FB_HALF * sizeof(float2), hipMemcpyHostToDevice));
        MDD_HIP_CHECK(hipMemcpy(t.first, first.data(), FB_BINS * sizeof(int), hipMemcpyHostToDevice));
        MDD_HIP_CHECK(hipMemcpy(t.count, count.data(), FB_BINS * sizeof(int), hipMemcpyHostToDevice));
        MDD_HIP_CHECK(hipMemcpy(t.woff, woff.data(), FB_BINS * sizeof(int), hipMemcpyHostToDevice));
        MDD_HIP_CHECK(hipMemcpy(t.weights, weights.data(), weights.size() * sizeof(float), hipMemcpyHostToDevice));
        g_fb_tables[dev] = t;
        g_fb_ready[dev] = true;
    }
    *out = g_fb_tables[dev];
    return MDD_OK;
}

}  // namespace mdd

using namespace mdd;

extern "C" int32_t mdd_fbank_num_frames(int64_t n_samples) {
    return n_samples < FB_N ? 0 : (int32_t)(1 + (n_samples - FB_N) / FB_S);
}

extern "C" int mdd_fbank(const float *wav_dev, int64_t n_samples, const float *cmvn_scale_dev, const float *cmvn_offset_dev,
                         float *out_dev, void *stream) {
    if (n_samples < 0 || ((cmvn_scale_dev == nullptr) != (cmvn_offset_dev == nullptr))) {
        set_error("mdd_fbank: bad argument"); return MDD_ERR_ARG;
    }
    const int nframes = mdd_fbank_num_frames(n_samples);
    if (nframes == 0) return MDD_OK;                                   // shorter than one window: no rows (snip-edges)
    if (!wav_dev || !out_dev) { set_error("mdd_fbank: null buffer"); return MDD_ERR_ARG; }
    int dev = 0;
    MDD_HIP_CHECK(hipGetDevice(&dev));
    FbankTables tb;
    if (int rc = fbank_tables(dev, &tb)) return rc;
    hipLaunchKernelGGL(fbank_kernel, dim3((nframes + 3) / 4), dim3(256), 0, (hipStream_t)stream, wav_dev, nframes, tb,
                       cmvn_scale_dev, cmvn_offset_dev, out_dev);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

extern "C" int32_t mdd_fbank_batch_len(const int64_t *n_samples, int32_t B, int32_t skip, int32_t n_down) {
    if (!n_samples || B <= 0 || skip < 1) { set_error("mdd_fbank_batch_len: bad argument"); return -1; }
    int32_t t_out = 0;
    for (int32_t b = 0; b < B; b++) {
        const int32_t T_raw = mdd_fbank_num_frames(n_samples[b]);
        if (T_raw == 0) {
            set_error("mdd_fbank_batch_len: utterance %d has %lld samples, fewer than one %d-sample window", b,
                      (long long)n_samples[b], FB_N);
            return -1;
        }
        const int32_t t = mdd_stack_len(T_raw, skip, n_down);
        if (t > t_out) t_out = t;
    }
    return t_out;
}

// mdd_fbank_batch and mdd_fbank_batch_aug: one set of refusals, one launch; `mk` null launches the kernel without the masks
static int fbank_batch_entry(const char *entry, const float *wav_dev, const int64_t *offsets_dev, int32_t B, int32_t T_out,
                             const float *cmvn_scale_dev, const float *cmvn_offset_dev, int32_t right, int32_t skip, int32_t n_down,
                             float *out_dev, const FbankMasks *mk, void *stream) {
    if (B <= 0 || T_out < 0 || right < 0 || skip < 1 || n_down < 1 ||
        ((cmvn_scale_dev == nullptr) != (cmvn_offset_dev == nullptr))) {
        set_error("%s: bad argument (B=%d T_out=%d right=%d skip=%d n_down=%d, cmvn pointers must come as a pair)", entry,
                  B, T_out, right, skip, n_down);
        return MDD_ERR_ARG;
    }
    if (mk) {
        if (mk->nf < 0 || mk->nf > 8 || mk->nt < 0 || mk->nt > 8) {
            set_error("%s: bad argument (NF=%d NT=%d, each must lie in 0..8)", entry, mk->nf, mk->nt);
            return MDD_ERR_ARG;
        }
        if ((mk->nf > 0 && !mk->f) || (mk->nt > 0 && !mk->t)) {
            set_error("%s: null %s with %s > 0", entry, mk->nf > 0 && !mk->f ? "fmask_dev" : "tmask_dev",
                      mk->nf > 0 && !mk->f ? "NF" : "NT");
            return MDD_ERR_ARG;
        }
    }
    if (T_out == 0) return MDD_OK;
    if (!wav_dev || !offsets_dev || !out_dev) { set_error("%s: null buffer", entry); return MDD_ERR_ARG; }
    if ((int64_t)T_out * skip > INT32_MAX - 4 || B > 65535) { set_error("%s: batch too large", entry); return MDD_ERR_ARG; }
    int dev = 0;
    MDD_HIP_CHECK(hipGetDevice(&dev));
    FbankTables tb;
    if (int rc = fbank_tables(dev, &tb)) return rc;
    const int rows = T_out * skip > T_out ? T_out * skip : T_out;   // covers every raw frame (T_raw_b <= T_out * skip) and row
    if (mk)
        hipLaunchKernelGGL(fbank_batch_kernel<true>, dim3((rows + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, wav_dev, offsets_dev,
                           T_out, tb, cmvn_scale_dev, cmvn_offset_dev, right, skip, out_dev, *mk);
    else
        hipLaunchKernelGGL(fbank_batch_kernel<false>, dim3((rows + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, wav_dev, offsets_dev,
                           T_out, tb, cmvn_scale_dev, cmvn_offset_dev, right, skip, out_dev, FbankMasks{nullptr, nullptr, 0, 0});
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

extern "C" int mdd_fbank_batch(const float *wav_dev, const int64_t *offsets_dev, int32_t B, int32_t T_out,
                               const float *cmvn_scale_dev, const float *cmvn_offset_dev, int32_t right, int32_t skip,
                               int32_t n_down, float *out_dev, void *stream) {
    return fbank_batch_entry("mdd_fbank_batch", wav_dev, offsets_dev, B, T_out, cmvn_scale_dev, cmvn_offset_dev, right, skip, n_down,
                             out_dev, nullptr, stream);
}

extern "C" int mdd_fbank_batch_aug(const float *wav_dev, const int64_t *offsets_dev, int32_t B, int32_t T_out,
                                   const float *cmvn_scale_dev, const float *cmvn_offset_dev, int32_t right, int32_t skip,
                                   int32_t n_down, float *out_dev, const int32_t *fmask_dev, int32_t NF, const int32_t *tmask_dev,
                                   int32_t NT, void *stream) {
    const FbankMasks mk{fmask_dev, tmask_dev, NF, NT};
    return fbank_batch_entry("mdd_fbank_batch_aug", wav_dev, offsets_dev, B, T_out, cmvn_scale_dev, cmvn_offset_dev, right, skip,
                             n_down, out_dev, &mk, stream);
}

extern "C" int mdd_cmvn_accumulate(const float *wav_dev, const int64_t *offsets_dev, int32_t B, int64_t max_samples, double *stats_dev,
                                   void *stream) {
    if (B <= 0 || B > 65535 || max_samples < 0) {
        set_error("mdd_cmvn_accumulate: bad argument (B=%d, 1..65535; max_samples=%lld)", B, (long long)max_samples);
        return MDD_ERR_ARG;
    }
    if (!wav_dev || !offsets_dev || !stats_dev) { set_error("mdd_cmvn_accumulate: null buffer"); return MDD_ERR_ARG; }
    const int64_t frames = max_samples < FB_N ? 0 : 1 + (max_samples - FB_N) / FB_S;
    if (frames > INT32_MAX - CMVN_STRIP) { set_error("mdd_cmvn_accumulate: max_samples too large"); return MDD_ERR_ARG; }
    if (frames == 0) return MDD_OK;                                    // nothing reaches one window: nothing to add
    int dev = 0;
    MDD_HIP_CHECK(hipGetDevice(&dev));
    FbankTables tb;
    if (int rc = fbank_tables(dev, &tb)) return rc;
    const int strips = (int)((frames + CMVN_STRIP - 1) / CMVN_STRIP);
    const int64_t parts = (int64_t)strips * B;
    StreamWorkspace ws;
    if (int rc = ws.acquire(nullptr, parts * CMVN_N * (int64_t)sizeof(double), (hipStream_t)stream)) return rc;
    hipLaunchKernelGGL(cmvn_partial_kernel, dim3(strips, B), dim3(256), 0, (hipStream_t)stream, wav_dev, offsets_dev, tb, ws.as<double>());
    MDD_LAUNCH_CHECK();
    hipLaunchKernelGGL(cmvn_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws.as<double>(), parts, stats_dev);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

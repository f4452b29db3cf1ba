// Any-rate WAV -> 16 kHz PCM16 on the GPU: the step the reference runs on every input that is not 16 kHz (AA/infer.py:498-501)
//   data = librosa.resample(data, orig_sr=fs, target_sr=16000)    (librosa <= 0.9: resampy 'kaiser_best', fix=True, scale=False)
//   sf.write(wav_path, data, 16000)                               (PCM_16: lrint(x * 32767), clipped here)
// restated in float64 with no contraction.  resampy's windowed-sinc filter: 64 zero crossings, 512 table
// entries per crossing, rolloff 0.9475937167399596, Kaiser beta 14.769656459379492.  For output t (t < n_f = int(n * ratio)) the
// position t * fs / 16000 is taken from integers, p = t * fs, n0 = p / 16000, frac = scale * ((p % 16000) / 16000.0); the left
// wing sums i < min(n0 + 1, (N + 1 - off) / step) taps over x[n0 - i], the right wing (frac := scale - frac) k < min(n - n0 - 1,
// (N + 1 - off) / step) taps over x[n0 + 1 + k], each tap acc = acc + (win[j] + eta * delta[j]) * x in that order.  Outputs
// [n_f, ceil(n * ratio)) are librosa's fix_length zeros.  16 kHz rows are copied bit for bit.
//
// One thread per output sample, 256 consecutive outputs of one row per workgroup (grid.y = row).  The work is about
// 2 * 64 / scale taps per output, a serial float64 chain; each tap reads one 16-byte (win, delta) table entry (the 512 KB table
// of the row's rate stays in L2) and one input sample (neighbouring lanes read neighbouring samples, L1-resident).
#include <math.h>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "mdd_internal.h"

#pragma clang fp contract(off)   // one fused multiply-add breaks bit equality with the float64 restatement

namespace mdd {

constexpr int RS_TARGET = 16000, RS_MIN_RATE = 1000, RS_MAX_RATE = 384000;
constexpr int RS_ZEROS = 64, RS_PREC = 512, RS_N = RS_ZEROS * RS_PREC, RS_TAB = RS_N + 1;
constexpr double RS_ROLLOFF = 0.9475937167399596, RS_BETA = 14.769656459379492;
constexpr int RS_BLOCK = 256;
constexpr int RS_MAX_RATES = 16;   // distinct rates one launch serves; more take one launch per group

static bool rate_ok(int32_t rate) { return rate >= RS_MIN_RATE && rate <= RS_MAX_RATE; }

// The rates of one launch and their (win, delta) tables; a 16 kHz entry has no table.  Indexed only by unrolled constants.
struct RsRates {
    const double2 *tab[RS_MAX_RATES];
    int32_t rate[RS_MAX_RATES];
    int32_t n;
};

// One table tap: win[j] + eta * delta[j], then the product with the sample, then the sum (no contraction, see the pragma).
__device__ __forceinline__ double rs_tap(double acc, const double2 c, double eta, float x) {
    const double weight = c.x + eta * c.y;
    return acc + weight * (double)x;
}

// Samples are on the int16 scale; the restatement filters x / 32768.  Scaling every sample by 2^-15 scales every product and
// every partial sum by 2^-15 exactly (no value here comes near the float64 subnormal range), so the chain runs on the raw
// samples and the sum is scaled once at the end, with the same bits.
__global__ __launch_bounds__(RS_BLOCK) void resample_batch_kernel(const float *__restrict__ wav, const int64_t *__restrict__ in_off,
                                                                  const int32_t *__restrict__ rates, const int64_t *__restrict__ out_off,
                                                                  RsRates rs, float *__restrict__ out) {
    const int b = blockIdx.y;
    const int64_t n_out = out_off[b + 1] - out_off[b];
    const int64_t t = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    const int32_t fs = rates[b];
    const double2 *tab = nullptr;
    bool mine = false;
#pragma unroll
    for (int k = 0; k < RS_MAX_RATES; k++)
        if (k < rs.n && rs.rate[k] == fs) { tab = rs.tab[k]; mine = true; }
    if (!mine || t >= n_out) return;   // another launch's rate, or past this row's end
    const float *x = wav + in_off[b];
    float *y = out + out_off[b];
    if (fs == RS_TARGET) { y[t] = x[t]; return; }   // n_out == n for a 16 kHz row (checked on the host)
    const int64_t n = in_off[b + 1] - in_off[b];
    const double ratio = (double)RS_TARGET / (double)fs;
    const int64_t n_f = (int64_t)((double)n * ratio);
    float v = 0.f;
    if (t < n_f) {
        const double scale = ratio < 1.0 ? ratio : 1.0;
        const int step = (int)(scale * RS_PREC);
        const int64_t p = t * fs, n0 = p / RS_TARGET;
        double frac = scale * ((double)(p % RS_TARGET) / 16000.0);
        double acc = 0.0;
        {   // left wing: x[n0], x[n0 - 1], ...
            const double idx = frac * RS_PREC;
            const int off = (int)idx;
            const double eta = idx - off;
            const int64_t reach = (RS_TAB - off) / step, imax = reach < n0 + 1 ? reach : n0 + 1;
            const double2 *w = tab + off;
            const float *xs = x + n0;
#pragma unroll 4
            for (int i = 0; i < (int)imax; i++) acc = rs_tap(acc, w[i * step], eta, xs[-i]);
        }
        frac = scale - frac;
        {   // right wing: x[n0 + 1], x[n0 + 2], ...
            const double idx = frac * RS_PREC;
            const int off = (int)idx;
            const double eta = idx - off;
            const int64_t reach = (RS_TAB - off) / step, kmax = reach < n - n0 - 1 ? reach : n - n0 - 1;
            const double2 *w = tab + off;
            const float *xs = x + n0 + 1;
#pragma unroll 4
            for (int k = 0; k < (int)kmax; k++) acc = rs_tap(acc, w[k * step], eta, xs[k]);
        }
        const double q = rint(acc * 0x1p-15 * 32767.0);   // (x / 32768 filtered) * 32767, round half to even
        v = (float)fmin(fmax(q, -32768.0), 32767.0);       // clipped: libsndfile without SFC_SET_CLIPPING would wrap
    }
    y[t] = v;
}

// I0 by its power series sum_k ((x/2)^k / k!)^2 in long double: every term is positive, so the sum is good to the last bit of a
// double at the arguments here (x <= beta).
static double bessel_i0(double x) {
    const long double q = 0.25L * x * x;
    long double term = 1.0L, sum = 1.0L;
    for (int k = 1; k < 200; k++) {
        term *= q / ((long double)k * k);
        sum += term;
        if (term < sum * 1e-21L) break;
    }
    return (double)sum;
}

// resampy's kaiser_best half window, scaled by the ratio when downsampling, and its forward differences (delta[N] = 0):
// win[j] = rolloff * sinc(rolloff * j / 512) * kaiser(2N + 1, beta)[N + j], with numpy's sinc and scipy's kaiser.
static void build_filter(int32_t rate, double *win, double *delta) {
    const double ratio = (double)RS_TARGET / (double)rate, i0_beta = bessel_i0(RS_BETA);
    for (int j = 0; j <= RS_N; j++) {
        const double u = RS_ROLLOFF * ((double)j / RS_PREC);
        const double y = M_PI * (u == 0.0 ? 1.0e-20 : u);
        const double r = (double)j / RS_N;                       // (n - alpha) / alpha at n = N + j
        const double taper = bessel_i0(RS_BETA * sqrt(1.0 - r * r)) / i0_beta;
        double w = taper * (RS_ROLLOFF * (sin(y) / y));
        if (ratio < 1.0) w *= ratio;
        win[j] = w;
    }
    for (int j = 0; j < RS_N; j++) delta[j] = win[j + 1] - win[j];
    delta[RS_N] = 0.0;
}

// One device table per (device, rate), built on first use.  The cache lives as long as the process (the map is never destroyed,
// so no hipFree runs after the runtime's own teardown at exit); each table has its one owner in the map.
static std::mutex g_rs_mutex;
static std::map<std::pair<int, int32_t>, DeviceArray<double2>> *g_rs_tables = new std::map<std::pair<int, int32_t>, DeviceArray<double2>>;

static int resample_table(int dev, int32_t rate, const double2 **out) {
    std::lock_guard<std::mutex> lk(g_rs_mutex);
    auto key = std::make_pair(dev, rate);
    auto it = g_rs_tables->find(key);
    if (it == g_rs_tables->end()) {
        std::vector<double> win(RS_TAB), delta(RS_TAB);
        build_filter(rate, win.data(), delta.data());
        std::vector<double2> host(RS_TAB);
        for (int j = 0; j < RS_TAB; j++) host[j] = make_double2(win[j], delta[j]);
        DeviceArray<double2> t;
        if (int rc = t.need(RS_TAB)) return rc;
        MDD_HIP_CHECK(hipMemcpy(t.p, host.data(), RS_TAB * sizeof(double2), hipMemcpyHostToDevice));
        it = g_rs_tables->emplace(key, std::move(t)).first;
    }
    *out = it->second.p;
    return MDD_OK;
}

}  // namespace mdd

using namespace mdd;

extern "C" int64_t mdd_resample_len(int64_t n, int32_t rate) {
    if (n < 0 || !rate_ok(rate)) return -1;
    if (rate == RS_TARGET) return n;
    return (int64_t)ceil((double)n * ((double)RS_TARGET / (double)rate));
}

extern "C" int mdd_resample_filter(int32_t rate, double *win, double *delta, int64_t cap) {
    if (!rate_ok(rate) || !win || !delta || cap < RS_TAB) {
        set_error("mdd_resample_filter: bad argument (rate %d must be in [%d, %d], cap %lld must be >= %d)", rate, RS_MIN_RATE,
                  RS_MAX_RATE, (long long)cap, RS_TAB);
        return MDD_ERR_ARG;
    }
    build_filter(rate, win, delta);
    return MDD_OK;
}

extern "C" int mdd_resample_batch(const float *wav_dev, const int64_t *in_off_dev, const int32_t *rates_dev, int32_t B,
                                  const int64_t *out_off_dev, float *out_dev, void *stream) {
    if (B <= 0 || B > 65535 || !in_off_dev || !rates_dev || !out_off_dev) {
        set_error("mdd_resample_batch: bad argument (B=%d, offsets and rates must be device arrays)", B);
        return MDD_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    // The launch geometry and the per-rate tables need the rates and lengths on the host: B + 1 offsets twice and B rates.
    std::vector<int64_t> in_off(B + 1), out_off(B + 1);
    std::vector<int32_t> rates(B);
    MDD_HIP_CHECK(hipMemcpyAsync(in_off.data(), in_off_dev, (B + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MDD_HIP_CHECK(hipMemcpyAsync(out_off.data(), out_off_dev, (B + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MDD_HIP_CHECK(hipMemcpyAsync(rates.data(), rates_dev, B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MDD_HIP_CHECK(hipStreamSynchronize(st));
    int64_t max_out = 0;
    std::vector<int32_t> distinct;
    for (int32_t b = 0; b < B; b++) {
        const int64_t n = in_off[b + 1] - in_off[b], n_out = out_off[b + 1] - out_off[b];
        if (in_off[b] < 0 || out_off[b] < 0 || n < 0 || n_out < 0 || mdd_resample_len(n, rates[b]) != n_out) {
            set_error("mdd_resample_batch: row %d: %lld samples at %d Hz need %lld outputs, the output offsets give %lld "
                      "(rates must be in [%d, %d])", b, (long long)n, rates[b], (long long)mdd_resample_len(n, rates[b]),
                      (long long)n_out, RS_MIN_RATE, RS_MAX_RATE);
            return MDD_ERR_ARG;
        }
        if (n_out > max_out) max_out = n_out;
        bool seen = false;
        for (int32_t r : distinct) seen |= r == rates[b];
        if (!seen) distinct.push_back(rates[b]);
    }
    if (max_out == 0) return MDD_OK;
    if (!wav_dev || !out_dev) { set_error("mdd_resample_batch: null buffer"); return MDD_ERR_ARG; }
    if ((max_out + RS_BLOCK - 1) / RS_BLOCK > INT32_MAX) { set_error("mdd_resample_batch: utterance too long"); return MDD_ERR_ARG; }
    int dev = 0;
    MDD_HIP_CHECK(hipGetDevice(&dev));
    for (size_t g = 0; g < distinct.size(); g += RS_MAX_RATES) {   // one launch unless a batch holds more than 16 rates
        RsRates rs = {};
        for (size_t k = g; k < distinct.size() && k < g + RS_MAX_RATES; k++) {
            const int i = rs.n++;
            rs.rate[i] = distinct[k];
            rs.tab[i] = nullptr;
            if (distinct[k] != RS_TARGET)
                if (int rc = resample_table(dev, distinct[k], &rs.tab[i])) return rc;
        }
        hipLaunchKernelGGL(resample_batch_kernel, dim3((unsigned)((max_out + RS_BLOCK - 1) / RS_BLOCK), B), dim3(RS_BLOCK), 0, st,
                           wav_dev, in_off_dev, rates_dev, out_off_dev, rs, out_dev);
        MDD_LAUNCH_CHECK();
    }
    return MDD_OK;
}

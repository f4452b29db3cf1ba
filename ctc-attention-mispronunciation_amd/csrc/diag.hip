// The diagnostic entries of the C ABI (include/mdd_hip.h, "Diagnostics"): test and measurement aids that drive the production launchers on
// operands made here.  Device memory is a DeviceArray and an event an Event, so every early return frees what it holds.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "lstm_persist.h"
#include "model.h"

namespace mdd {

// The tile walk of an entry's f32x6 launches: MDD_GEMM_X6_RASTER as it stands at the call.  Unset: the default; a value that is neither rows
// nor <rb>x<cb> is an error here (at create it would be the default, plan.h), so that no arm of a comparison runs under another's name.
static int diag_raster(const char *entry, X6Raster *out) {
    const char *e = getenv("MDD_GEMM_X6_RASTER");
    *out = kX6DefaultRaster;
    if (e && !x6_raster_parse(e, out)) { set_error("%s: MDD_GEMM_X6_RASTER=%s (rows, or <rb>x<cb> with rb * cb <= 32)", entry, e); return MDD_ERR_ARG; }
    return MDD_OK;
}
// Likewise the tile, MDD_GEMM_X6_RT: unset, the launcher's rule (kX6RtRule; `unset` where an entry's default is another); 3 or 4; anything else is an error.
static int diag_rt(const char *entry, int *out, int unset = kX6RtRule) {
    const char *e = getenv("MDD_GEMM_X6_RT");
    *out = unset;
    if (e && !x6_rt_parse(e, out)) { set_error("%s: MDD_GEMM_X6_RT=%s (3 or 4)", entry, e); return MDD_ERR_ARG; }
    return MDD_OK;
}

// Pseudo-random fill: element i is value(hash(i, seed)).  The three formulas are the ones the figures under profiles/ were taken with.
template <class T, class F> __global__ void diag_fill_kernel(T *p, size_t n, unsigned seed, F value) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u + seed; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        p[i] = value(h);
    }
}
struct SmallBf16 {   // a bf16 of magnitude 0.0078..0.031, random sign (the race screen's planes)
    __device__ unsigned short operator()(unsigned h) const { return (unsigned short)(0x3c00u + (h & 0x3ffu) + ((h >> 10) & 1u) * 0x8000u); }
};
struct TwoScales {   // uniform in [-1, 1), every other value at a twentieth of that (the GEMM timing aid's operands)
    __device__ float operator()(unsigned h) const { return ((float)(h & 0xffffff) / 8388608.f - 1.f) * ((h >> 24) & 1 ? 1.f : 0.05f); }
};
struct Affine {      // uniform in [offset - scale, offset + scale) (the conv timing aid's features and weights)
    float scale, offset;
    __device__ float operator()(unsigned h) const { return ((float)(h & 0xffffff) / 8388608.f - 1.f) * scale + offset; }
};
template <class T, class F> static int fill(T *p, size_t n, unsigned seed, F value) {
    hipLaunchKernelGGL((diag_fill_kernel<T, F>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, nullptr, p, n, seed, value);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

__global__ void diag_diff_kernel(const unsigned *a, const unsigned *b, size_t n, unsigned *count) {
    unsigned c = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) c += a[i] != b[i];
    if (c) atomicAdd(count, c);
}

__global__ void diag_gates_kernel(const float *x, float *sg, float *th, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { sg[i] = gate_sigmoid(x[i]); th[i] = gate_tanh(x[i]); }
}

// `warm` untimed, then `reps` timed calls of launch() on the null stream between two events -> *ms = mean milliseconds of a timed one
template <class F> static int time_launches(int warm, int reps, float *ms, F launch) {
    Event e0, e1;
    MDD_HIP_CHECK(hipEventCreate(&e0.h));
    MDD_HIP_CHECK(hipEventCreate(&e1.h));
    for (int r = 0; r < warm; r++) if (int rc = launch()) return rc;
    MDD_HIP_CHECK(hipEventRecord(e0.h, nullptr));
    for (int r = 0; r < reps; r++) if (int rc = launch()) return rc;
    MDD_HIP_CHECK(hipEventRecord(e1.h, nullptr));
    MDD_HIP_CHECK(hipEventSynchronize(e1.h));
    MDD_HIP_CHECK(hipEventElapsedTime(ms, e0.h, e1.h));
    *ms /= (float)reps;
    return MDD_OK;
}
// `reps` launches timed one by one, the first (cold) one left out of the mean where there is another; before(r) / after(r) run untimed
// around launch r
template <class F, class B, class A> static int time_each(int reps, float *mean, F launch, B before, A after) {
    float tot = 0.f;
    for (int r = 0; r < reps; r++) {
        float t = 0.f;
        if (int rc = before(r)) return rc;
        if (int rc = time_launches(0, 1, &t, launch)) return rc;
        if (r > 0 || reps == 1) tot += t;
        if (int rc = after(r)) return rc;
    }
    *mean = tot / (float)(reps > 1 ? reps - 1 : 1);
    return MDD_OK;
}
static int nothing(int) { return MDD_OK; }

}  // namespace mdd

using namespace mdd;

// Race screen for the 8-phase kernel (tests/test_gpu_parity.py): the same pseudo-random split operands through the single-barrier kernel
// and through the production 8-phase kernel, `reps` times each; returns the number of C words of the 8-phase kernel that ever differed
// from the single-barrier kernel's (both perform the same arithmetic per element, so it must be 0).
// ms_out (nullable, 16 floats; the slots not named here are left alone): [0] single-barrier, [1] 8-phase: mean kernel time, HIP events;
// MDD_GEMM_STAMP: [3..6] the 8-phase kernel's phase stamps, mean cycles per K-tile and wave; MDD_GEMM_T128: [14] the 128x128 kernel (two
// workgroups per CU) on the same problem.
extern "C" int mdd_diag_gemm_ph8(int M, int N, int K, int reps, unsigned seed, unsigned *mismatches_out, float *ms_out) {
    if (M <= 0 || N <= 0 || K < 32 || K % 32 || !mismatches_out || reps < 1) { set_error("mdd_diag_gemm_ph8: bad shape"); return MDD_ERR_ARG; }
    static OncePerDevice attr;
    if (int rc = once_per_device(attr, init_gemm_attributes)) return rc;
    const size_t na = (size_t)M * K, nw = (size_t)N * K, nc = (size_t)M * N;
    DeviceArray<unsigned short> Ap, Wp;
    DeviceBuf C1, C2;
    DeviceArray<unsigned> cnt;
    if (int rc = Ap.need(2 * na)) return rc;
    if (int rc = Wp.need(2 * nw)) return rc;
    if (int rc = C1.need(nc)) return rc;
    if (int rc = C2.need(nc)) return rc;
    if (int rc = cnt.need(1)) return rc;
    MDD_HIP_CHECK(hipMemset(cnt.p, 0, 4));
    if (int rc = fill(Ap.p, 2 * na, seed, SmallBf16())) return rc;
    if (int rc = fill(Wp.p, 2 * nw, seed * 7919u + 13u, SmallBf16())) return rc;
    const SplitOperand A{.p = {Ap.p, Ap.p + na}, .ld = K}, W{.p = {Wp.p, Wp.p + nw}, .ld = K};
    float ms[2] = {0.f, 0.f};
    if (int rc = time_each(reps, &ms[0], [&] { return launch_gemm_bf16x3_256(X3Form::SingleBarrier, A, W, C1.p, N, M, N, K, nullptr); }, nothing, nothing)) return rc;
    if (int rc = time_each(reps, &ms[1], [&] { return launch_gemm_bf16x3_256(X3Form::Phase8, A, W, C2.p, N, M, N, K, nullptr); },
                           [&](int) -> int { MDD_HIP_CHECK(hipMemsetAsync(C2.p, 0xff, nc * 4, nullptr)); return MDD_OK; },
                           [&](int) -> int {
                               hipLaunchKernelGGL(diag_diff_kernel, dim3(1024), dim3(256), 0, nullptr, reinterpret_cast<const unsigned *>(C1.p),
                                                  reinterpret_cast<const unsigned *>(C2.p), nc, cnt.p);
                               MDD_LAUNCH_CHECK();
                               return MDD_OK;
                           })) return rc;
    MDD_HIP_CHECK(hipMemcpy(mismatches_out, cnt.p, 4, hipMemcpyDeviceToHost));
    if (!ms_out) return MDD_OK;
    ms_out[0] = ms[0]; ms_out[1] = ms[1];
    if (getenv("MDD_GEMM_T128")) {
        const auto t128 = [&] { return launch_gemm_bf16x3(A, W, C2.p, nullptr, N, M, N, K, nullptr, {}, /* tile128 */ true); };
        if (int rc = time_each(reps, &ms_out[14], t128, nothing, nothing)) return rc;
    }
    if (getenv("MDD_GEMM_STAMP")) {
        const int nwg = std::min(256, ((M + 255) / 256) * ((N + 255) / 256));
        DeviceArray<long long> sd;
        std::vector<long long> hs((size_t)256 * 8 * 4);
        if (int rc = sd.need(hs.size())) return rc;
        MDD_HIP_CHECK(hipMemset(sd.p, 0, hs.size() * 8));
        if (int rc = launch_gemm_bf16x3_256(X3Form::Phase8Stamped, A, W, C2.p, N, M, N, K, nullptr, nullptr, sd.p)) return rc;
        MDD_HIP_CHECK(hipMemcpy(hs.data(), sd.p, hs.size() * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < 4; i++) {
            double tot = 0;
            for (int w = 0; w < nwg * 8; w++) tot += (double)hs[(size_t)w * 4 + i];
            ms_out[3 + i] = (float)(tot / (nwg * 8) / (K / 32));
        }
    }
    return MDD_OK;
}

extern "C" int mdd_diag_gates(const float *x_dev, float *sig_dev, float *tanh_dev, int64_t n, void *stream) {
    if (!x_dev || !sig_dev || !tanh_dev || n <= 0) { set_error("mdd_diag_gates: bad arguments"); return MDD_ERR_ARG; }
    hipLaunchKernelGGL(diag_gates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev, sig_dev, tanh_dev, (long long)n);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// One GEMM through a chosen arithmetic, fp32 operands and result on the device; synchronises.  The f32x6 launches of this entry and of the
// two below take their tile walk from MDD_GEMM_X6_RASTER and their tile from MDD_GEMM_X6_RT as they stand at the call (plan.h).
//   mode 0: exact fp32 MFMA (gemm_nt_f32_kernel)   1: split-bf16 x3 (operands split here)   3: the f32x6 kernel (three planes, split here)
extern "C" int mdd_diag_gemm(int mode, const float *A_dev, const float *W_dev, float *C_dev, int M, int N, int K, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!A_dev || !W_dev || !C_dev || M <= 0 || N <= 0 || K <= 0 || K % 32) { set_error("mdd_diag_gemm: bad arguments"); return MDD_ERR_ARG; }
    if (mode != 0 && mode != 1 && mode != 3) { set_error("mdd_diag_gemm: mode %d (0 exact fp32, 1 split-bf16 x3, 3 f32x6)", mode); return MDD_ERR_ARG; }
    if (mode == 0) return launch_gemm_nt({.p = A_dev, .ld = K}, {.p = W_dev, .ld = K}, C_dev, N, M, N, K, st);
    const size_t na = (size_t)M * K, nw = (size_t)N * K;
    const int planes = mode == 1 ? 2 : 3;
    X6Raster raster;
    if (int rc = diag_raster("mdd_diag_gemm", &raster)) return rc;
    int rt;
    if (int rc = diag_rt("mdd_diag_gemm", &rt)) return rc;
    DeviceArray<unsigned short> pa, pw;     // freed on return, behind the synchronisation
    if (pa.need(planes * na) || pw.need(planes * nw)) { set_error("mdd_diag_gemm: out of memory"); return MDD_ERR_NOMEM; }
    int rc;
    if (mode == 1) {
        const SplitPtr a{pa.p, pa.p + na}, w{pw.p, pw.p + nw};
        if (!(rc = launch_split(A_dev, na, a, st)) && !(rc = launch_split(W_dev, nw, w, st)))
            rc = launch_gemm_bf16x3({.p = a, .ld = K}, {.p = w, .ld = K}, C_dev, nullptr, N, M, N, K, st);
    } else {
        static OncePerDevice attr;
        rc = once_per_device(attr, init_gemm_x6_attributes);
        if (!rc) rc = launch_split3(A_dev, M, K, K, pa.p, st);
        if (!rc) rc = launch_split3(W_dev, N, K, K, pw.p, st);
        if (!rc) rc = launch_gemm_f32x6(pa.p, na, pw.p, nw, nullptr, C_dev, M, N, K, N, st, raster, nullptr, rt);
    }
    (void)hipStreamSynchronize(st);
    return rc;
}

extern "C" int mdd_diag_gemm_ops(int mode, int ta, int tb, const float *A_dev, int lda, const float *B_dev, int ldb, float *C_dev, int ldc, int M, int N, int K,
                                 int splits, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!A_dev || !B_dev || !C_dev || M <= 0 || N <= 0 || K <= 0 || splits < 1 || lda < (ta ? M : K) || ldb < (tb ? N : K) || ldc < N) {
        set_error("mdd_diag_gemm_ops: bad arguments"); return MDD_ERR_ARG;
    }
    if (mode != 0 && mode != 3) { set_error("mdd_diag_gemm_ops: mode %d (0 exact fp32, 3 f32x6)", mode); return MDD_ERR_ARG; }
    const GemmOperand A{A_dev, lda, ta != 0}, B{B_dev, ldb, tb != 0};
    X6Raster raster;
    if (int rc = diag_raster("mdd_diag_gemm_ops", &raster)) return rc;
    int rt;
    if (int rc = diag_rt("mdd_diag_gemm_ops", &rt, 3)) return rc;   // unset: the training step's tile
    DeviceBuf xa, xb, part;     // freed on return, behind the synchronisation
    int rc;
    if (mode == 0) rc = launch_gemm_f32(A, B, C_dev, ldc, M, N, K, st);
    else if (!(rc = init_gemm_x6_attributes())) rc = gemm_f32x6_ops(A, B, nullptr, C_dev, ldc, M, N, K, splits, xa, xb, part, st, raster, rt);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) { set_error("mdd_diag_gemm_ops: the stream failed"); rc = MDD_ERR_HIP; }
    return rc;
}

// Timing aid: two warm and `reps` timed launches of one GEMM kernel (operands resident and pre-split; events on the null stream) -> mean ms.
//   mode 0 exact fp32 MFMA, 1 split-bf16 x3, 3 f32x6
// MDD_GEMM_STAMP (mode 3): one extra launch of the stamped instantiation; per-K-tile cycle means of the first 1024 workgroups are printed
// mhz_out (nullable, mode 3): the clock the chip held inside the kernel, from one launch of the stamped instantiation enqueued straight behind
// the timed ones and ten more: the median over workgroups of shader-clock ticks / 100 MHz constant-clock ticks around the tile loop, x 100.
// `reps` long enough (2 s) for the clock to have settled is the caller's business.
static int gemm_time(const char *entry, int mode, int M, int N, int K, int reps, float *ms_out, float *mhz_out);
extern "C" int mdd_diag_gemm_time(int mode, int M, int N, int K, int reps, float *ms_out) { return gemm_time("mdd_diag_gemm_time", mode, M, N, K, reps, ms_out, nullptr); }
extern "C" int mdd_diag_gemm_clock(int M, int N, int K, int reps, float *ms_out, float *mhz_out) {
    if (!mhz_out) { set_error("mdd_diag_gemm_clock: bad arguments"); return MDD_ERR_ARG; }
    return gemm_time("mdd_diag_gemm_clock", 3, M, N, K, reps, ms_out, mhz_out);
}
static int gemm_time(const char *entry, int mode, int M, int N, int K, int reps, float *ms_out, float *mhz_out) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 32 || reps < 1 || !ms_out) { set_error("%s: bad arguments", entry); return MDD_ERR_ARG; }
    if (mode != 0 && mode != 1 && mode != 3) { set_error("%s: mode %d", entry, mode); return MDD_ERR_ARG; }
    X6Raster raster;
    if (int rc = diag_raster(entry, &raster)) return rc;
    int rt;
    if (int rc = diag_rt(entry, &rt)) return rc;
    const size_t na = (size_t)M * K, nw = (size_t)N * K, nc = (size_t)M * N;
    DeviceBuf A, W, Cm;
    DeviceArray<unsigned short> pa, pw;
    if (A.need(na) || W.need(nw) || Cm.need(nc) || pa.need(3 * na) || pw.need(3 * nw)) { set_error("%s: out of memory", entry); return MDD_ERR_NOMEM; }
    if (int rc = fill(A.p, na, 1u, TwoScales())) return rc;
    if (int rc = fill(W.p, nw, 2u, TwoScales())) return rc;
    const SplitPtr a{pa.p, pa.p + na}, w{pw.p, pw.p + nw};
    if (mode == 1) {
        if (int rc = launch_split(A.p, na, a, nullptr)) return rc;
        if (int rc = launch_split(W.p, nw, w, nullptr)) return rc;
    }
    if (mode == 3) {
        if (int rc = init_gemm_x6_attributes()) return rc;
        if (int rc = launch_split3(A.p, M, K, K, pa.p, nullptr)) return rc;
        if (int rc = launch_split3(W.p, N, K, K, pw.p, nullptr)) return rc;
    }
    const auto x6 = [&](long long *stamps) { return launch_gemm_f32x6(pa.p, na, pw.p, nw, nullptr, Cm.p, M, N, K, N, nullptr, raster, stamps, rt); };
    const size_t ns = X6_STAMP_WORDS;
    DeviceArray<long long> sd;
    if (mode == 3 && (mhz_out || getenv("MDD_GEMM_STAMP"))) {
        if (int rc = sd.need(ns)) return rc;
        MDD_HIP_CHECK(hipMemset(sd.p, 0, ns * 8));
    }
    if (int rc = time_launches(2, reps, ms_out, [&] {
            if (mode == 0) return launch_gemm_nt({.p = A.p, .ld = K}, {.p = W.p, .ld = K}, Cm.p, N, M, N, K, nullptr);
            if (mode == 1) return launch_gemm_bf16x3({.p = a, .ld = K}, {.p = w, .ld = K}, Cm.p, nullptr, N, M, N, K, nullptr);
            return x6(nullptr);
        })) return rc;
    if (mode == 3 && mhz_out) {
        for (int r = 0; r < 10; r++) if (int rc = x6(nullptr)) return rc;
        if (int rc = x6(sd.p)) return rc;
        std::vector<long long> h(ns);
        MDD_HIP_CHECK(hipMemcpy(h.data(), sd.p, ns * 8, hipMemcpyDeviceToHost));
        std::vector<double> mhz;
        for (size_t g = 0; g < (size_t)X6_STAMP_WGS; g++) {
            const long long clk = h[X6_STAMP_PHASE_WORDS + g * 2], rt = h[X6_STAMP_PHASE_WORDS + g * 2 + 1];
            if (clk > 0 && rt > 0) mhz.push_back((double)clk / (double)rt * 100.0);
        }
        if (mhz.empty()) { set_error("%s: no workgroup stamped", entry); return MDD_ERR_STATE; }
        std::nth_element(mhz.begin(), mhz.begin() + mhz.size() / 2, mhz.end());
        *mhz_out = (float)mhz[mhz.size() / 2];
    }
    if (mode == 3 && getenv("MDD_GEMM_STAMP")) {
        std::vector<long long> h(ns);
        MDD_HIP_CHECK(hipMemset(sd.p, 0, ns * 8));
        if (int rc = x6(sd.p)) return rc;
        MDD_HIP_CHECK(hipMemcpy(h.data(), sd.p, ns * 8, hipMemcpyDeviceToHost));
        double sum[4] = {0, 0, 0, 0}; size_t cnt = 0;
        for (size_t w_ = 0; w_ < 1024 * 4; w_++) if (h[w_ * 4 + 0] > 0) { for (int i = 0; i < 4; i++) sum[i] += (double)h[w_ * 4 + i]; cnt++; }
        const double d = (double)cnt * (K / 32);
        if (cnt) printf("  f32x6 stamps, cycles per K-tile and wave: MFMA stream %.0f (ideal %d), memory wait %.0f, barrier %.0f\n",
                        sum[0] / d, x6_choose_tile(M, x6_ceil_div(N, 128), raster, rt).rt * 8 * 6 * 16, sum[1] / d, sum[2] / d);
        fflush(stdout);
    }
    return MDD_OK;
}

// Timing aid: two warm and `reps` timed launches of the f32x6 conv front end on pseudo-random features and weights ([B, T, 243] -> T/2 * B
// rows) between events -> mean ms.  which: 0 the default kernel, 1 the row-at-a-time kernel.  phases (nullable, which = 0 only): one extra
// launch of the stamped instantiation; phases[wave * 10 + phase] receives the mean cycles per workgroup (over the first 512) of that wave in
// that phase.  mismatch (nullable) receives the number of output words in which the two kernels differ.
extern "C" int mdd_diag_conv_time(int B, int T, int reps, int which, float *ms_out, double *phases, long long *mismatch) {
    if (B <= 0 || T < 2 || reps < 1 || which < 0 || which > 1 || !ms_out) { set_error("mdd_diag_conv_time: bad arguments"); return MDD_ERR_ARG; }
    const int Tp = T / 2;
    const size_t nx = (size_t)B * T * 243, nout = (size_t)3 * Tp * B * 1952;
    DeviceBuf xb, wb;              // wb: w0 [288] | sc0 [32] | sh0 [32] | sc1 [32] | sh1 [32] | w1 [32 * 288]
    DeviceArray<unsigned short> w13, out, out2;
    DeviceArray<long long> sd;
    if (int rc = init_conv_attributes()) return rc;
    if (xb.need(nx) || wb.need(416 + 32 * 288) || w13.need(3 * 32 * 288) || out.need(nout) || (mismatch && out2.need(nout)) ||
        (phases && sd.need((size_t)512 * 8 * CM_NPH))) return MDD_ERR_HIP;
    const struct { float *p; size_t n; Affine value; } fills[] = {
        {xb.p, nx, {2.f, 0.f}}, {wb.p, 288, {0.4f, 0.f}}, {wb.p + 288, 32, {0.2f, 1.f}}, {wb.p + 320, 32, {0.3f, 0.1f}},
        {wb.p + 352, 32, {0.2f, 1.f}}, {wb.p + 384, 32, {0.3f, 0.1f}}, {wb.p + 416, (size_t)32 * 288, {0.1f, 0.f}}};
    unsigned seed = 0;
    for (const auto &f : fills) if (int rc = fill(f.p, f.n, ++seed, f.value)) return rc;
    if (int rc = launch_split3_rowmajor(wb.p + 416, 32 * 288, w13.p, nullptr)) return rc;
    auto run = [&](int w, unsigned short *o, long long *stp) {
        return launch_conv_fused3(xb.p, wb.p, wb.p + 288, wb.p + 320, w13.p, wb.p + 352, wb.p + 384, o, nullptr, B, T, 0, 0, w == 1, stp);
    };
    if (int rc = time_launches(2, reps, ms_out, [&] { return run(which, out.p, nullptr); })) return rc;
    if (phases) {
        const size_t ns = (size_t)512 * 8 * CM_NPH;
        MDD_HIP_CHECK(hipMemset(sd.p, 0, ns * 8));
        if (int rc = run(0, out.p, sd.p)) return rc;
        std::vector<long long> h(ns);
        MDD_HIP_CHECK(hipMemcpy(h.data(), sd.p, ns * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < 8 * CM_NPH; i++) phases[i] = 0.0;
        size_t cnt = 0;
        for (size_t g = 0; g < 512; g++) {
            long long any = 0;
            for (int i = 0; i < 8 * CM_NPH; i++) any |= h[g * 8 * CM_NPH + i];
            if (!any) continue;
            for (int i = 0; i < 8 * CM_NPH; i++) phases[i] += (double)h[g * 8 * CM_NPH + i];
            cnt++;
        }
        if (cnt) for (int i = 0; i < 8 * CM_NPH; i++) phases[i] /= (double)cnt;
    }
    if (mismatch) {
        if (int rc = run(0, out.p, nullptr)) return rc;
        if (int rc = run(1, out2.p, nullptr)) return rc;
        std::vector<unsigned short> a(nout), b(nout);
        MDD_HIP_CHECK(hipMemcpy(a.data(), out.p, nout * 2, hipMemcpyDeviceToHost));
        MDD_HIP_CHECK(hipMemcpy(b.data(), out2.p, nout * 2, hipMemcpyDeviceToHost));
        long long bad = 0;
        for (size_t i = 0; i < nout; i++) bad += a[i] != b[i];
        *mismatch = bad;
    }
    return MDD_OK;
}

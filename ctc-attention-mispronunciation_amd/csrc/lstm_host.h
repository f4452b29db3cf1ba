// The host shape of a persistent BiLSTM layer launch (lstm_granule.hip, lstm_bwd.hip, lstm_f32.hip, lstm_x6.hip), host code only:
//   1. refuse   bad arguments, each launcher its own, before any HIP call;
//   2. zero     the sync words (the abort word among them);
//   3. zero     the live bytes of the exchange buffer: tag 0 is never valid, so a replay cannot see a previous launch's state;
//   4. launch   kPersistGrid x 256 with the family's LDS size;
//   5. check    hipGetLastError.
// Steps 2 to 5 are launch_persistent().  A family writes its template instantiations down ONCE, as a struct: List, the (H, row tiles per team)
// pairs as an InstList (a pair marked DBG also exists as a stamped instantiation); kernel<H, N, DBG>(); lds(H, N), its dynamic LDS bytes; and
// built(H, N), the filter of a development build on that list.  The attribute initialisation (init_persistent_attributes) and the dispatch from
// the runtime (H, tiles) (launch_instantiation) both walk that one list: a launcher cannot reach an instantiation whose LDS attribute was not
// set.  (Everything here has internal linkage: the library exports what it did.)
#pragma once
#include <type_traits>

#include "lstm_persist.h"

namespace mdd {

static constexpr int kPersistLdsLimit = 156 * 1024;   // hipFuncAttributeMaxDynamicSharedMemorySize of every persistent layer kernel

// The fields of PersistArgs that every family fills from LstmStepArgs the same way; the rest is zero.  oshift is null when oscale is null:
// the kernels test oscale alone.
static inline PersistArgs persist_args(const LstmStepArgs &s, unsigned short *hx, unsigned int *sync, int *err_flag, long long *stamps) {
    PersistArgs a{};
    a.gx = s.gx; a.hx = hx; a.sync = sync; a.err_flag = err_flag; a.dbg = stamps; a.seqlen = s.seqlen;
    a.out = s.out; a.out_raw = s.out_raw; a.oscale = s.oscale; a.oshift = s.oscale ? s.oshift : nullptr;
    a.T = s.T; a.B = s.B; a.BGr = (s.B + 15) / 16; a.BG = granule_bg(s.B);
    return a;
}

template <class Args>
static int launch_persistent(void (*kernel)(Args), size_t lds, Args a, void *hx, size_t hx_live, unsigned int *sync, hipStream_t st) {
    if (int rc = launch_zero_fill(sync, kPersistSyncWords * sizeof(unsigned int), st)) return rc;
    if (int rc = launch_zero_fill(hx, hx_live, st)) return rc;   // by a kernel, not a memset node: see launch_zero_fill (lstm_persist.hip)
    hipLaunchKernelGGL(kernel, dim3(kPersistGrid), dim3(256), lds, st, a);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

template <int H_, int N_, bool DBG_ = false> struct Inst { static constexpr int H = H_, N = N_; static constexpr bool DBG = DBG_; };
template <class... I> struct InstList {};
struct PersistFamily { static constexpr bool built(int, int) { return true; } };   // what a family derives from: every pair of its list is compiled

// f(Inst) for every built pair of the family's list, until one returns non-zero: that value, else 0
template <class Fam, class F, class... I> static int for_each_instantiation(InstList<I...>, F f) {
    int rc = 0;
    auto visit = [&](auto i) { if constexpr (Fam::built(decltype(i)::H, decltype(i)::N)) rc = f(i); return rc; };
    (void)(visit(I{}) || ...);
    return rc;
}

template <class Fam> static int init_persistent_attributes() {
    return for_each_instantiation<Fam>(typename Fam::List{}, [](auto i) -> int {
        using I = decltype(i);
        MDD_HIP_CHECK(hipFuncSetAttribute((const void *)Fam::template kernel<I::H, I::N, false>(), hipFuncAttributeMaxDynamicSharedMemorySize, kPersistLdsLimit));
        if constexpr (I::DBG) MDD_HIP_CHECK(hipFuncSetAttribute((const void *)Fam::template kernel<I::H, I::N, true>(), hipFuncAttributeMaxDynamicSharedMemorySize, kPersistLdsLimit));
        return MDD_OK;
    });
}

// Steps 2 to 5 through the family's instantiation for (H, tiles) -- the stamped one where dbg is set and the pair has it.  kNoInstantiation: the
// list has none (the launcher says which of its limits that is); else the launch's status.
static constexpr int kNoInstantiation = 1;   // (no mdd_status is positive)
template <class Fam, class Args>
static int launch_instantiation(int H, int tiles, bool dbg, const Args &a, void *hx, size_t hx_live, unsigned int *sync, hipStream_t st) {
    int rc = kNoInstantiation;
    for_each_instantiation<Fam>(typename Fam::List{}, [&](auto i) -> int {
        using I = decltype(i);
        if (I::H != H || I::N != tiles) return 0;
        auto kernel = Fam::template kernel<I::H, I::N, false>();
        if constexpr (I::DBG) { if (dbg) kernel = Fam::template kernel<I::H, I::N, true>(); }
        rc = launch_persistent(kernel, Fam::lds(I::H, I::N), a, hx, hx_live, sync, st);
        return 1;   // found: the walk ends
    });
    return rc;
}

}  // namespace mdd

// The host shape of a CTC lattice entry (mdd_ctc_loss, mdd_ctc_align, mdd_ctc_variants, mdd_ctc_confnet, mdd_ctc_confnet_best, the beam entries), host code only:
//   1. refuse    every bad argument by name, then a caller workspace that is too small (refuse_workspace) -- before any HIP call;
//   2. attributes the kernels' LDS budgets, once per device (once_per_device, mdd_internal.h);
//   3. workspace the caller's, or one allocated on the stream for the call (StreamWorkspace);
//   4. launch;
//   5. check     hipGetLastError, with the workspace still in scope: its free is enqueued behind the last launch on every return path.
#pragma once
#include "mdd_internal.h"

namespace mdd {

// Scratch for one call: the caller's pointer when one is given, else `need` bytes allocated stream-ordered (none for need == 0) and freed
// on the same stream by the destructor.  Declare it in front of the launches and let it live to the entry's return: the free then follows
// the last launch whichever return is taken.
class StreamWorkspace {
public:
    StreamWorkspace() = default;
    StreamWorkspace(const StreamWorkspace &) = delete;
    StreamWorkspace &operator=(const StreamWorkspace &) = delete;
    StreamWorkspace(StreamWorkspace &&o) noexcept : p_(o.p_), owned_(o.owned_), st_(o.st_) { o.p_ = o.owned_ = nullptr; }
    ~StreamWorkspace() { if (owned_) (void)hipFreeAsync(owned_, st_); }
    __attribute__((visibility("hidden"))) int acquire(void *caller, int64_t need, hipStream_t st) {   // (hidden: where it is not inlined it is no new export)
        p_ = caller;
        if (caller || need <= 0) return MDD_OK;
        MDD_HIP_CHECK(hipMallocAsync(&owned_, (size_t)need, st));
        p_ = owned_;
        st_ = st;
        return MDD_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p_); }

private:
    void *p_ = nullptr, *owned_ = nullptr;
    hipStream_t st_ = nullptr;
};

// The refusal of a caller workspace of `given` bytes where `bytes_fn` asks for `need`
inline int refuse_workspace(const char *entry, const char *bytes_fn, int64_t given, int64_t need) {
    set_error("%s: workspace_bytes %lld, need %lld (%s)", entry, (long long)given, (long long)need, bytes_fn);
    return MDD_ERR_ARG;
}

// ctc_labels_per_lane(Lmax), the consecutive labels a lane owns in the wave forms of the lattice, is plan.h's (through mdd_internal.h): the
// host-only plan of mdd_ctc_nbest reads it too.

}  // namespace mdd

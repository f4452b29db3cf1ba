// What the two sweeps over an error network share (ctc_confnet.hip: sum-product, ctc_confnet_best.hip: max-product): the launch shape and
// the LDS budget that bounds the slots (mdd_ctc_confnet_max_slots), so that a network one entry takes, the other takes.
#pragma once
#include <hip/hip_runtime.h>

namespace mdd {

static constexpr int CN_WAVES = 16;
static constexpr size_t CN_LDS_LIMIT = 159 * 1024;       // dynamic LDS; the last KB of the CU's 160 stays with the kernel's static 256 bytes

// doubles of LDS for J slots: three [J, C] rows, what the waves publish of their blocks ([waves, C] and [waves]), skip / all / apre [J],
// pre / tail / end [J + 1]
static inline size_t confnet_lds_doubles(int C, int J) { return (size_t)3 * J * C + (size_t)CN_WAVES * (C + 1) + (size_t)6 * J + 8; }

}  // namespace mdd

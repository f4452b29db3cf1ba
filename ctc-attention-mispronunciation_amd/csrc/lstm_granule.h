// The inline-asm MFMAs of the split-bf16 persistent kernels (lstm_granule.hip, lstm_bwd.hip), their wait states, and the sched-barrier speed hint.
#pragma once
#include "lstm_persist.h"

namespace mdd {

// acc += A.B with A taken straight from an accumulation-file register (half of the resident weight fragments live
// there: the compiler would otherwise copy each one to a VGPR with four v_accvgpr_read per MFMA, on every step)
__device__ __forceinline__ void mfma_a(f32x4 &acc, const bf16x8 &a_agpr, const bf16x8 &b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "a"(a_agpr), "v"(b));
}
// The other two products of a k-step in the same form.  ALL MFMAs of the persistent kernels' product loops are asm volatile, so that
// their issue order is the source order (product-major: a k-step's three products over the RTW row tiles, i.e. an accumulator is
// written again RTW >= 2 MFMAs later), whatever the scheduler does around them.  Round 2 mixed builtin MFMAs with the asm one: the
// compiler cannot see that an asm MFMA reads its accumulator, inserts no wait state in front of it, and -- once the
// __builtin_amdgcn_sched_barrier calls that happened to pin the product-major order were removed -- scheduled
//     v_mfma a[152:155], v[98:101], v[182:185], 0 ; v_mfma a[152:155], a[96:99], v[178:181], a[152:155]
// back to back: the second read a[152:155] before the first had written it, and results moved by 1.7e-4 (profiles/round3_lstm_ordering.txt).
// The sched barriers are a speed hint now (MDD_NO_SCHED_HINT builds give identical bits).  The accumulators' readers after the loop
// are vector instructions the compiler cannot order behind an asm MFMA either: mfma_drain() supplies their wait states.
__device__ __forceinline__ void mfma_v(f32x4 &acc, const bf16x8 &a, const bf16x8 &b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_v0(f32x4 &acc, const bf16x8 &a, const bf16x8 &b) {   // first product of a tile: from a literal zero
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_drain() { asm volatile("s_nop 7\n\ts_nop 7" ::: "memory"); }
// The B operands of a k-step are made by vector instructions (tag masks, register moves) just before its MFMAs.  "VALU writes a VGPR ->
// MFMA reads it" needs two wait states, which the compiler supplies for builtin MFMAs and cannot for asm ones (the first all-asm build was
// wrong in the 1-, 3- and 4-tile forms, whose schedules put a v_and directly in front of the first MFMA): this statement takes both
// operands as read-write, so every instruction that produces them sits in front of it, and its s_nop 1 is the two wait states.
// The A fragments of the k-step go through it too: under register pressure (three and four tiles) the compiler parks some of the "resident"
// VGPR fragments in the accumulation file and copies them back (v_accvgpr_read = a VALU write) right in front of their MFMA.
// tools/check_mfma_hazards.py scans the built ISA for exactly these patterns (tests/test_host.py::test_asm_mfma_hazards).
template <int N>
__device__ __forceinline__ void mfma_operands_ready(bf16x8 &bh, bf16x8 &bl, bf16x8 (&a)[N]) {
    static_assert(N == 2 || N == 3, "row tiles per wave");
    if (N == 3) asm volatile("s_nop 1" : "+v"(bh), "+v"(bl), "+v"(a[0]), "+v"(a[1]), "+v"(a[2]));
    else asm volatile("s_nop 1" : "+v"(bh), "+v"(bl), "+v"(a[0]), "+v"(a[1]));
}
#ifdef MDD_NO_SCHED_HINT
#define MDD_SCHED_HINT() do { } while (0)
#else
#define MDD_SCHED_HINT() __builtin_amdgcn_sched_barrier(0)
#endif

}  // namespace mdd

// fp32 -> bf16 planes on the device: the one pair of conversions and the two- and three-plane splits built on them (the kernels of
// split.hip, the split-output epilogue of gemm_bf16x3.hip, the diagnostics).  Two planes: hi = bf16(x), lo = bf16(x - hi), 16 significand
// bits together.  Three planes: hi, mid = bf16(x - hi), lo = bf16(x - hi - mid), with hi + mid + lo == x exactly (finite x; overflow and
// NaN land in hi).
#pragma once
#include <hip/hip_runtime.h>

namespace mdd {

__device__ __forceinline__ unsigned short bf16_bits(float x) {   // round-to-nearest-even, NaN-preserving cast
    __bf16 b = (__bf16)x;
    return *reinterpret_cast<unsigned short *>(&b);
}
__device__ __forceinline__ float bf16_to_f32(unsigned short b) { return __uint_as_float((unsigned)b << 16); }

__device__ __forceinline__ void split_store(float v, unsigned short *hi, unsigned short *lo, size_t i) {
    const unsigned short h = bf16_bits(v), l = bf16_bits(v - bf16_to_f32(h));
    hi[i] = h;
    lo[i] = l;
}

__device__ __forceinline__ void split3(float v, unsigned short &h, unsigned short &m, unsigned short &l) {
    h = bf16_bits(v);
    const float r1 = v - bf16_to_f32(h);
    m = bf16_bits(r1);
    l = bf16_bits(r1 - bf16_to_f32(m));
}

// eight consecutive values -> 16 bytes at element `off` of each of three planes plane_elems apart
__device__ __forceinline__ void split3_store8(const float (&f)[8], unsigned short *planes, size_t plane_elems, size_t off) {
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    u16x8 h, m, l;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        unsigned short hk, mk, lk;
        split3(f[k], hk, mk, lk);
        h[k] = hk; m[k] = mk; l[k] = lk;
    }
    *reinterpret_cast<u16x8 *>(planes + off) = h;
    *reinterpret_cast<u16x8 *>(planes + plane_elems + off) = m;
    *reinterpret_cast<u16x8 *>(planes + 2 * plane_elems + off) = l;
}

}  // namespace mdd

// What every persistent BiLSTM layer launch shares on the host (lstm_host.h): the zero fill in front of it.
#include "lstm_host.h"

namespace mdd {

__global__ void zero_fill_kernel(u32x4 *p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = (u32x4){0u, 0u, 0u, 0u};
}
// The persistent layer kernels need their exchange buffer's tags and their abort word zeroed before every launch.  Inside a captured graph a
// hipMemsetAsync becomes a memset NODE, and replays of such graphs were measured to let a layer kernel start on the previous launch's
// contents (tools/fused_repro3.py, exact-fp32 mode, small batches: the second and later mdd_forward_fused calls gave wrong layer-0 outputs,
// up to 2e-2, in 7 of 12 and 4 of 14 processes; in none of 12 with MDD_GRAPH=0; in none of 14 with this kernel in the memset's place).
// A kernel node orders like every other kernel of the chain.
int launch_zero_fill(void *p, size_t n, hipStream_t st) {
    if (n % 16 || reinterpret_cast<uintptr_t>(p) % 16) { set_error("zero fill: %zu bytes at %p (a multiple of 16 bytes at a 16-byte aligned address)", n, p); return MDD_ERR_ARG; }
    const size_t n16 = n / 16;
    const int blocks = (int)std::min<size_t>((n16 + 255) / 256, 2048);
    hipLaunchKernelGGL(zero_fill_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, reinterpret_cast<u32x4 *>(p), n16);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

}  // namespace mdd

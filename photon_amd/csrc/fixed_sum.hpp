// fixed_sum.hpp - dot products whose bits depend on the grid size alone: what the iterative solvers (photon_density.hip,
// photon_tomo.hip) share.  A launch of at most kMaxBlocks blocks of kThreads threads strides over the elements; every block
// leaves one partial (block_sum), and whoever needs the total sums the partial array itself (sum_parts): every block of
// every later launch holds the same bits, so a scalar such as CG's alpha never has to leave the device.  The host's look at
// a total (the residual, every few iterations) is read_sum.
#pragma once
#include <hip/hip_runtime.h>

namespace photon {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;            // the partial arrays hold at most this many values (4 per thread to sum)

// Fixed-order block sum: a butterfly inside each wave (every lane ends with the same bits: a + b == b + a), then the wave
// totals in wave order.  blockDim.x == kThreads.
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
    for (int i = 1; i < kThreads / 64; i++) v += red[i];
    return v;
}

// the sum of a partial array of n <= kMaxBlocks values, the same bits in every block
__device__ __forceinline__ double sum_parts(const double *__restrict__ part, int n, double *red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) s += part[i];
    return block_sum(s, red);
}

// the same total for the host's check: one block.  Internal linkage: every unit that includes this has its own.
static __global__ __launch_bounds__(kThreads) void sum_parts_kernel(const double *__restrict__ part, int n_parts,
                                                                    double *__restrict__ out) {
    __shared__ double red[kThreads / 64];
    const double s = sum_parts(part, n_parts, red);
    if (threadIdx.x == 0) *out = s;
}

// *out = the sum of part[0 .. n_parts) by way of the device scalar d_scalar; synchronises the stream
static inline hipError_t read_sum(const double *part, int n_parts, double *d_scalar, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(kThreads), 0, stream, part, n_parts, d_scalar);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_scalar, sizeof(double), hipMemcpyDeviceToHost, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}

}  // namespace photon

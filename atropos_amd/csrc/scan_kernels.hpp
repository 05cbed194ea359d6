// scan_kernels.hpp -- the exclusive prefix sum over 64-bit values that the FASTA index (fasta_kernels.hip) and the BAM
// decode (bam_kernels.hip) lay their outputs out with: a block scan, the blocks' totals scanned by one block, the add.
// No atomics: equal input gives equal sums.  Included by the kernel files; every one gets kernels of its own.
#ifndef ATR_SCAN_KERNELS_HPP
#define ATR_SCAN_KERNELS_HPP

#include <hip/hip_runtime.h>

namespace atr {
namespace {

typedef unsigned long long u64;

constexpr int SCAN_BLOCK = 1024;                          // threads (and elements) per block of the prefix sums
inline long long scan_blocks(long long n) { return (n + SCAN_BLOCK - 1) / SCAN_BLOCK; }

// inclusive prefix sum of one value per thread over a block of THREADS; *total = the block's sum
template <int THREADS>
__device__ __forceinline__ u64 scan_block(u64 v, u64 *s_part, u64 *total) {
    constexpr int WAVES = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) s_part[wave] = x;
    __syncthreads();
    if (wave == 0) {
        u64 w = lane < WAVES ? s_part[lane] : 0ull;
#pragma unroll
        for (int off = 1; off < WAVES; off <<= 1) {
            const u64 y = __shfl_up(w, off, 64);
            if (lane >= off) w += y;
        }
        if (lane < WAVES) s_part[lane] = w;
    }
    __syncthreads();
    *total = s_part[WAVES - 1];
    return x + (wave ? s_part[wave - 1] : 0ull);
}

// out[i] = exclusive prefix of v inside its block, sums[b] = the block's total
__global__ __launch_bounds__(SCAN_BLOCK) void scan_local_kernel(const u64 *__restrict__ v, long long n, u64 *__restrict__ out,
                                                                u64 *__restrict__ sums) {
    __shared__ u64 s_part[SCAN_BLOCK / 64];
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const u64 x = i < n ? v[i] : 0ull;
    u64 total;
    const u64 inc = scan_block<SCAN_BLOCK>(x, s_part, &total);
    if (i < n) out[i] = inc - x;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// exclusive prefix of the nb block totals in place (one block, a run per thread); out[n] = the grand total
__global__ __launch_bounds__(SCAN_BLOCK) void scan_sums_kernel(u64 *__restrict__ sums, long long nb, u64 *__restrict__ out,
                                                               long long n) {
    __shared__ u64 s_part[SCAN_BLOCK / 64];
    const long long per = (nb + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const long long lo = min(nb, per * (long long)threadIdx.x), hi = min(nb, lo + per);
    u64 mine = 0;
    for (long long i = lo; i < hi; ++i) mine += sums[i];
    u64 total;
    const u64 inc = scan_block<SCAN_BLOCK>(mine, s_part, &total);
    u64 run = inc - mine;
    for (long long i = lo; i < hi; ++i) { const u64 t = sums[i]; sums[i] = run; run += t; }
    if (threadIdx.x == 0) out[n] = total;
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_add_kernel(u64 *__restrict__ out, long long n, const u64 *__restrict__ sums) {
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    if (i < n) out[i] += sums[blockIdx.x];
}

__global__ void scan_set_kernel(long long *p, long long v) { *p = v; }

// out[0 .. n] = exclusive prefix sums of v[0 .. n), out[n] the total; sums: scan_blocks(n) words
void device_scan(const u64 *v, long long n, u64 *out, u64 *sums, hipStream_t st) {
    if (n == 0) {
        hipLaunchKernelGGL(scan_set_kernel, dim3(1), dim3(1), 0, st, (long long *)out, 0ll);
        return;
    }
    const long long nb = scan_blocks(n);
    hipLaunchKernelGGL(scan_local_kernel, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, v, n, out, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_BLOCK), 0, st, sums, nb, out, n);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, out, n, (const u64 *)sums);
}

}  // namespace
}  // namespace atr
#endif

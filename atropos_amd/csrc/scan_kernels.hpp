// scan_kernels.hpp -- the exclusive prefix sum that every text kernel file lays its outputs out with (the line index
// and the formatters of fastq_kernels.hip, fastq_emit_kernels.hip and pairtext_kernels.hip, the FASTA index, the BAM
// decode): a block scan, the blocks' totals scanned by one block, the add.  The input is 32- or 64-bit words, the
// sums are 64-bit.  No atomics: equal input gives equal sums, input order is kept.  Included by the kernel files;
// every one gets kernels of its own.
#ifndef ATR_SCAN_KERNELS_HPP
#define ATR_SCAN_KERNELS_HPP

#include <hip/hip_runtime.h>

#include "launch_util.hpp"

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
template <typename V>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_local_kernel(const V *__restrict__ v, long long n, u64 *__restrict__ out,
                                                                u64 *__restrict__ sums) {
    __shared__ u64 s_part[SCAN_BLOCK / 64];
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const u64 x = i < n ? (u64)v[i] : 0ull;
    u64 total;
    const u64 inc = scan_block<SCAN_BLOCK>(x, s_part, &total);
    if (i < n) out[i] = inc - x;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// exclusive prefix of the nb block totals in place (one block, a run per thread); *total_out = the grand total
__global__ __launch_bounds__(SCAN_BLOCK) void scan_sums_kernel(u64 *__restrict__ sums, long long nb, u64 *__restrict__ total_out) {
    __shared__ u64 s_part[SCAN_BLOCK / 64];
    const long long per = (nb + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const long long lo = min(nb, per * (long long)threadIdx.x), hi = min(nb, lo + per);
    u64 mine = 0;
    for (long long i = lo; i < hi; ++i) mine += sums[i];
    u64 total;
    const u64 inc = scan_block<SCAN_BLOCK>(mine, s_part, &total);
    u64 run = inc - mine;
    for (long long i = lo; i < hi; ++i) { const u64 t = sums[i]; sums[i] = run; run += t; }
    if (threadIdx.x == 0 && total_out) *total_out = total;
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_add_kernel(u64 *__restrict__ out, long long n, const u64 *__restrict__ sums) {
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    if (i < n) out[i] += sums[blockIdx.x];
}

__global__ void set_i64_kernel(long long *p, long long v) { *p = v; }

// out[0 .. n) = exclusive prefix sums of v[0 .. n); *total, where one is given, = the sum of all of v (0 for n == 0,
// which writes nothing else).  `total` may be out + n, and need not be: an array of exactly n words stays inside
// its bounds.  sums: scan_blocks(n) words.
template <typename V>
void device_scan(const V *v, long long n, u64 *out, u64 *sums, u64 *total, hipStream_t st) {
    if (n == 0) {
        if (total) hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)total, 0ll);
        return;
    }
    const long long nb = scan_blocks(n);
    hipLaunchKernelGGL(scan_local_kernel<V>, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, v, n, out, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_BLOCK), 0, st, sums, nb, total);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, out, n, (const u64 *)sums);
}

// the workspace of one "sizes -> offsets" step: [sizes V x n][sums u64 x (scan_blocks(n) + spare)]
template <typename V>
struct ScanWork {
    V *sizes;
    u64 *sums;
};

template <typename V>
ScanWork<V> scan_work(Workspace &ws, long long n, int spare = 0) {
    ScanWork<V> w;
    w.sizes = ws.take<V>((size_t)n);
    w.sums = ws.take<u64>((size_t)scan_blocks(n) + spare);
    return w;
}

template <typename V>
size_t scan_work_bytes(long long n, int spare = 0) {
    Workspace ws(nullptr);
    scan_work<V>(ws, n, spare);
    return ws.bytes();
}

}  // namespace
}  // namespace atr
#endif

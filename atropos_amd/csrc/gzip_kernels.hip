// gzip_kernels.hip -- the .gz output compressed on the device: FASTQ text in HBM -> a stream of BGZF members
// (one per 65 280 bytes of text; every gzip reader takes the stream, bgzip / htslib read it in parallel).
//
//   gz_blocks_kernel   a workgroup of 512 lanes per block, the blocks of a launch dealt round-robin to at most
//                      GZ_MAX_GRID workgroups.  The block (64 KiB), the position table (64 KiB: 2^14 words, entered with
//                      ds_max_u32; later a length byte per position), the token bitmap (8 KiB) and the code tables live
//                      in LDS -- 145 KiB, one workgroup per CU.  The phases and everything they compute: deflate_core.hpp.
//                      Each member is written into its own 64 KiB slot of the work buffer.
//   gz_scan_kernel     one workgroup: the running sum of the member sizes -> member offsets and the total.
//   gz_gather_kernel   a workgroup per member: slot -> its place in the compacted stream.
// No inline assembly; every byte written to memory goes out through vector stores or integer atomics.
#include <hip/hip_runtime.h>

#include "atropos_hip.h"
#include "deflate_core.hpp"
#include "launch_util.hpp"

namespace atr {

__global__ __launch_bounds__(GZ_NT) void gz_blocks_kernel(const uint8_t *__restrict__ text, long long n, long long nblocks,
                                                          uint8_t *slots, uint32_t *sizes, uint32_t *match) {
    __shared__ GzLds lds;
    GzCtx c;
    c.L = &lds;
    c.m = match + (size_t)blockIdx.x * GZ_SLOT;
    for (long long b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const long long at = b * GZ_BLOCK;
        c.src = text + at;
        c.n = (uint32_t)(n - at < GZ_BLOCK ? n - at : GZ_BLOCK);
        c.slot = (uint32_t *)(slots + (size_t)b * GZ_SLOT);
        c.size = sizes + b;
        gz_encode_block(c);
    }
}

__global__ __launch_bounds__(1024) void gz_scan_kernel(const uint32_t *__restrict__ sizes, long long nblocks, long long *offsets,
                                                       long long *member_offsets, long long *total) {
    __shared__ long long part[1024];
    const long long per = (nblocks + 1023) / 1024, lo = threadIdx.x * per, hi = lo + per < nblocks ? lo + per : nblocks;
    long long sum = 0;
    for (long long i = lo; i < hi; ++i) sum += sizes[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < 1024; ++i) { const long long v = part[i]; part[i] = run; run += v; }
        *total = run;
        offsets[nblocks] = run;
        if (member_offsets) member_offsets[nblocks] = run;
    }
    __syncthreads();
    long long run = part[threadIdx.x];
    for (long long i = lo; i < hi; ++i) {
        offsets[i] = run;
        if (member_offsets) member_offsets[i] = run;
        run += sizes[i];
    }
}

__global__ __launch_bounds__(256) void gz_gather_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                        const long long *__restrict__ offsets, uint8_t *__restrict__ out) {
    const uint8_t *src = slots + (size_t)blockIdx.x * GZ_SLOT;
    uint8_t *dst = out + offsets[blockIdx.x];
    const uint32_t size = sizes[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < size; i += 256) dst[i] = src[i];
}

}  // namespace atr

using namespace atr;

extern "C" {

int64_t atr_gzip_bound(int64_t n_bytes) { return n_bytes < 0 ? (int64_t)ATR_ERR_INVALID : gz_bound(n_bytes); }

size_t atr_gzip_work_bytes(int64_t n_bytes) { return n_bytes < 0 ? 0 : (size_t)gz_work_bytes(n_bytes); }

int atr_gzip_eof(uint8_t *buf28) {
    if (!buf28) return ATR_ERR_INVALID;
    gz_eof_member(buf28);
    return 28;
}

int atr_gzip_blocks(const uint8_t *d_text, int64_t n_bytes, uint8_t *d_out, int64_t out_capacity, int64_t *d_total,
                    int64_t *d_member_offsets, void *d_work, void *stream) {
    if (n_bytes < 0 || out_capacity < 0) return ATR_ERR_INVALID;
    if (n_bytes >= ((int64_t)1 << 32)) return ATR_ERR_UNSUPPORTED;
    if (out_capacity < gz_bound(n_bytes)) return ATR_ERR_INVALID;      // (before any pointer is looked at)
    if (!d_total) return ATR_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (n_bytes == 0) {
        hipError_t e = hipMemsetAsync(d_total, 0, 8, s);
        if (e == hipSuccess && d_member_offsets) e = hipMemsetAsync(d_member_offsets, 0, 8, s);
        return e == hipSuccess ? ATR_OK : hip_fail(e, "atr_gzip_blocks memset");
    }
    if (!d_text || !d_out || !d_work) return ATR_ERR_INVALID;
    const long long nblocks = gz_nblocks(n_bytes);
    uint8_t *work = (uint8_t *)d_work;
    uint32_t *sizes = (uint32_t *)(work + gz_work_sizes_at(n_bytes));
    long long *offsets = (long long *)(work + gz_work_offsets_at(n_bytes));
    uint32_t *match = (uint32_t *)(work + gz_work_match_at(n_bytes));
    hipLaunchKernelGGL(gz_blocks_kernel, dim3((unsigned)gz_grid(n_bytes)), dim3(GZ_NT), 0, s, d_text, (long long)n_bytes,
                       nblocks, work, sizes, match);
    int rc = launched("atr_gzip_blocks launch");
    if (rc) return rc;
    hipLaunchKernelGGL(gz_scan_kernel, dim3(1), dim3(1024), 0, s, sizes, nblocks, offsets, (long long *)d_member_offsets,
                       (long long *)d_total);
    rc = launched("atr_gzip_blocks scan launch");
    if (rc) return rc;
    hipLaunchKernelGGL(gz_gather_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, work, sizes, offsets, d_out);
    return launched("atr_gzip_blocks gather launch");
}

}  // extern "C"

// fasta_kernels.hip -- the device-resident FASTA batch: line index, line classes, record descriptors,
// the gather of wrapped sequences into a tail behind the text, and the FASTA formatter (see
// include/atropos_hip.h, "device-resident FASTA batch"; the per-line and per-record code is fasta_core.hpp).
//
// Byte streaming throughout, like fastq_kernels.hip.  The order of the work:
//   1. line ends (the caller has their number from atr_fastq_count_lines): 16 bytes per thread, counted per block,
//      placed by a prefix sum (input order, no atomics);
//   2. a thread per line strips and classifies it;
//   3. ONE exclusive prefix sum over the lines -- sequence bytes in the low half, headers in the high half --
//      gives every line its record and its place inside the record's sequence, and every record its length as a
//      difference of two prefix values: a record may span any number of blocks;
//   4. a thread per record decides whether it needs unwrapping; a prefix sum over the records lays the tail out;
//   5. a thread per record writes its descriptor, a wave per sequence line copies the line into the tail.
// The only atomic is the minimum of the error word.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "atropos_hip.h"
#include "fasta_core.hpp"

#include "launch_util.hpp"
#include "scan_kernels.hpp"

namespace atr {
namespace {

constexpr int FA_NL = 256, FA_NL_BYTES = FA_NL * 16;      // line index: threads per block, bytes per block

// ------------------------------------------------------------------------- line index
// bit i set <=> byte off + i ends a line (is_line_end of fastq_core.hpp; the byte behind the text counts as 0)
__device__ __forceinline__ uint32_t fa_line_end_mask16(const uint8_t *bytes, long long off, long long nbytes) {
    if (off >= nbytes) return 0u;
    const uint4 v = *(const uint4 *)(bytes + off);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint8_t after = off + 16 < nbytes ? bytes[off + 16] : (uint8_t)0;
    const int valid = (int)min<long long>(16, nbytes - off);
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint8_t c = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        const uint8_t next = k == 15 ? after : (k + 1 < valid ? (uint8_t)(w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) : (uint8_t)0);
        if (k < valid && is_line_end(c, next)) mask |= 1u << k;
    }
    return mask;
}

__global__ __launch_bounds__(FA_NL) void fa_count_kernel(const uint8_t *__restrict__ bytes, long long nbytes,
                                                         u64 *__restrict__ block_counts) {
    __shared__ uint32_t s_cnt[FA_NL / 64];
    const long long off = ((long long)blockIdx.x * FA_NL + threadIdx.x) * 16;
    uint32_t c = __popc(fa_line_end_mask16(bytes, off, nbytes));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < FA_NL / 64; ++w) t += s_cnt[w];
        block_counts[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(FA_NL) void fa_line_ends_kernel(const uint8_t *__restrict__ bytes, long long nbytes,
                                                             const u64 *__restrict__ block_base, long long nlines,
                                                             uint32_t *__restrict__ line_ends) {
    __shared__ u64 s_part[FA_NL / 64];
    const long long off = ((long long)blockIdx.x * FA_NL + threadIdx.x) * 16;
    uint32_t mask = fa_line_end_mask16(bytes, off, nbytes);
    const u64 c = __popc(mask);
    u64 total;
    const u64 inc = scan_block<FA_NL>(c, s_part, &total);
    long long slot = (long long)(block_base[blockIdx.x] + inc - c);
    while (mask) {
        const int b = __ffs((int)mask) - 1;
        mask &= mask - 1;
        if (slot < nlines) line_ends[slot] = (uint32_t)(off + b);     // (nlines is the count of this very text)
        ++slot;
    }
}

// ------------------------------------------------------------------------- lines and records
__global__ __launch_bounds__(256) void fa_classify_kernel(const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ line_ends,
                                                          long long nlines, uint8_t *__restrict__ cls, uint32_t *__restrict__ at,
                                                          uint32_t *__restrict__ len, u64 *__restrict__ value) {
    const long long L = (long long)blockIdx.x * 256 + threadIdx.x;
    if (L >= nlines) return;
    const uint32_t start = L ? line_ends[L - 1] + 1u : 0u;
    uint32_t a, n;
    const int c = fasta_line_one(bytes, start, line_ends[L], a, n);
    cls[L] = (uint8_t)c;
    at[L] = a;
    len[L] = n;
    value[L] = fasta_line_value(c, n);
}

// header lines take their place in head_line; a sequence line in front of the first header is the error
__global__ __launch_bounds__(256) void fa_heads_kernel(const uint8_t *__restrict__ cls, const u64 *__restrict__ pre, long long nlines,
                                                       uint32_t *__restrict__ head_line, u64 *__restrict__ error) {
    const long long L = (long long)blockIdx.x * 256 + threadIdx.x;
    if (L >= nlines) return;
    const int c = cls[L];
    if (c == FASTA_HEADER) head_line[fasta_pre_headers(pre[L])] = (uint32_t)L;
    else if (c == FASTA_SEQ && fasta_pre_headers(pre[L]) == 0)
        atomicMin(error, (u64)(L + 1) * 8ull + (u64)ATR_FASTA_ERR_HEADER);
}

// what every record needs in the tail (0 for the slots beyond the last record: the grid covers nlines)
__global__ __launch_bounds__(256) void fa_gather_sizes_kernel(const uint32_t *__restrict__ line_ends, const uint8_t *__restrict__ cls,
                                                              const uint32_t *__restrict__ at, const uint32_t *__restrict__ len,
                                                              const u64 *__restrict__ pre, const uint32_t *__restrict__ head_line,
                                                              long long nlines, u64 *__restrict__ need) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nlines) return;
    const FastaLines ln = {line_ends, cls, at, len, pre, head_line, nlines, fasta_pre_headers(pre[nlines])};
    need[r] = r < ln.nrec ? (u64)fasta_record_gather(ln, r) : 0ull;
}

__global__ void fa_info_kernel(const u64 *__restrict__ pre, const u64 *__restrict__ tail_pre, long long nlines,
                               long long *__restrict__ info) {
    info[0] = fasta_pre_headers(pre[nlines]);
    info[1] = (long long)tail_pre[nlines];
}

__global__ __launch_bounds__(256) void fa_records_kernel(const uint32_t *__restrict__ line_ends, const uint8_t *__restrict__ cls,
                                                         const uint32_t *__restrict__ at, const uint32_t *__restrict__ len,
                                                         const u64 *__restrict__ pre, const uint32_t *__restrict__ head_line,
                                                         long long nlines, long long nrec, const u64 *__restrict__ tail_pre,
                                                         uint32_t tail_off, FastqRecord *__restrict__ records,
                                                         uint32_t *__restrict__ record_ends) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec) return;
    const FastaLines ln = {line_ends, cls, at, len, pre, head_line, nlines, nrec};
    FastqRecord rec;
    uint32_t rec_end;
    fasta_record_one(ln, tail_pre, tail_off, r, rec, rec_end);
    records[r] = rec;
    record_ends[r] = rec_end;
}

// One wave per sequence line of a record that is unwrapped: the line's bytes to their place in the tail, 16 bytes
// per lane where source and target share their alignment, else a byte per lane.
__global__ __launch_bounds__(256) void fa_gather_kernel(uint8_t *bytes, const uint32_t *__restrict__ line_ends,
                                                        const uint8_t *__restrict__ cls, const uint32_t *__restrict__ at,
                                                        const uint32_t *__restrict__ len, const u64 *__restrict__ pre,
                                                        const uint32_t *__restrict__ head_line, long long nlines, long long nrec,
                                                        const u64 *__restrict__ tail_pre, uint32_t tail_off, uint32_t tail_bytes) {
    const int lane = threadIdx.x & 63;
    const long long L = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);          // wave-uniform
    if (L >= nlines) return;
    const FastaLines ln = {line_ends, cls, at, len, pre, head_line, nlines, nrec};
    uint32_t to;
    if (!fasta_line_target(ln, tail_pre, L, to)) return;
    const uint32_t n = len[L];
    if ((u64)to + n > (u64)tail_bytes) return;                                    // (never: the caller sized the tail)
    const uint8_t *src = bytes + at[L];
    uint8_t *dst = bytes + tail_off + to;
    uint32_t k = 0;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15u) == 0 && n >= 64u) {
        const uint32_t head = (16u - ((uint32_t)(uintptr_t)dst & 15u)) & 15u;
        if ((uint32_t)lane < head) dst[lane] = src[lane];
        const uint32_t blocks = (n - head) >> 4;
        for (uint32_t b = (uint32_t)lane; b < blocks; b += 64u)
            *(uint4 *)(dst + head + 16u * b) = *(const uint4 *)(src + head + 16u * b);
        k = head + 16u * blocks;
    }
    for (uint32_t o = k + (uint32_t)lane; o < n; o += 64u) dst[o] = src[o];
}

// ------------------------------------------------------------------------- formatter
__global__ __launch_bounds__(256) void fa_emit_sizes_kernel(const FastqRecord *__restrict__ records, const int32_t *__restrict__ begin,
                                                            const int32_t *__restrict__ end, const uint8_t *__restrict__ dest,
                                                            int which, long long n, u64 *__restrict__ sizes) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    u64 s = 0;
    if (!dest || dest[r] == which) s = fasta_record_bytes(records[r], max(0, end[r] - begin[r]));
    sizes[r] = s;
}

// EMIT_LANES lanes per record, 64 / EMIT_LANES records per wave at a time: a record of a few hundred bytes keeps
// its lanes busy for a handful of steps, and a wave's records are neighbours in the input and in the output.
constexpr int FA_EMIT_LANES = 16;
__global__ __launch_bounds__(256) void fa_emit_kernel(const uint8_t *__restrict__ bytes, const FastqRecord *__restrict__ records,
                                                      const int32_t *__restrict__ begin, const int32_t *__restrict__ end,
                                                      const int32_t *__restrict__ ubegin, const int32_t *__restrict__ uend,
                                                      const uint8_t *__restrict__ dest, int which, long long n,
                                                      const long long *__restrict__ offsets, uint8_t *__restrict__ out) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / FA_EMIT_LANES;
    const int part = threadIdx.x % FA_EMIT_LANES;
    if (r >= n || (dest && dest[r] != which)) return;
    const int a = begin[r], b = max(a, end[r]);
    fasta_format_record(out + offsets[r], bytes, records[r], a, b, ubegin ? ubegin[r] : a, uend ? uend[r] : b, part, FA_EMIT_LANES);
}

// work of the index: [cls u8 x nlines][at u32 x nlines][len u32 x nlines][head_line u32 x nlines]
//                    [value u64 x nlines][pre u64 x (nlines + 1)][tail_pre u64 x (nlines + 1)][sums u64 x blocks]
// in front of it, for the line ends: [counts u64 x nblk][base u64 x (nblk + 1)][sums u64 x blocks]
struct FaWork {
    u64 *counts, *base, *csums;                               // the line ends' part
    uint8_t *cls;
    uint32_t *at, *len, *head_line;
    u64 *value, *pre, *tail_pre, *sums;
    size_t bytes;
};

FaWork fa_work(const void *work, long long nbytes, long long nlines) {
    FaWork w;
    Workspace ws(work);
    const long long nblk = blocks(nbytes, FA_NL_BYTES);
    w.counts = ws.take<u64>((size_t)nblk);
    w.base = ws.take<u64>((size_t)nblk + 1);
    w.csums = ws.take<u64>((size_t)scan_blocks(nblk) + 1);
    w.cls = ws.take<uint8_t>((size_t)nlines);
    w.at = ws.take<uint32_t>((size_t)nlines);
    w.len = ws.take<uint32_t>((size_t)nlines);
    w.head_line = ws.take<uint32_t>((size_t)nlines);
    w.value = ws.take<u64>((size_t)nlines);
    w.pre = ws.take<u64>((size_t)nlines + 1);
    w.tail_pre = ws.take<u64>((size_t)nlines + 1);
    w.sums = ws.take<u64>((size_t)scan_blocks(nlines) + 1);
    w.bytes = ws.bytes();
    return w;
}

}  // namespace
}  // namespace atr

using namespace atr;

extern "C" {

size_t atr_fasta_work_bytes(int64_t nbytes, int64_t nlines) {
    if (nbytes < 0 || nlines < 0) return 0;
    return fa_work(nullptr, nbytes, nlines).bytes;
}

int atr_fasta_scan(const uint8_t *d_bytes, int64_t nbytes, uint32_t *d_line_ends, int64_t nlines, void *d_work,
                   int64_t *d_info, void *stream) {
    if (nbytes < 0 || nbytes >= (int64_t)0xFFFFFFF0ll || nlines < 0 || nlines > nbytes || !d_info) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_info + 2, (long long)LLONG_MAX);
    if (nlines == 0) {
        hipError_t e = hipMemsetAsync(d_info, 0, 16, st);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
        return launched("fasta scan launch");
    }
    if (!d_bytes || !d_work || !d_line_ends || ((uintptr_t)d_bytes & 15)) return ATR_ERR_INVALID;
    const FaWork w = fa_work(d_work, nbytes, nlines);
    const long long nblk = blocks(nbytes, FA_NL_BYTES);
    // (the blocks' line counts: atr_fastq_count_lines keeps its own to itself)
    hipLaunchKernelGGL(fa_count_kernel, dim3((unsigned)nblk), dim3(FA_NL), 0, st, d_bytes, (long long)nbytes, w.counts);
    device_scan(w.counts, nblk, w.base, w.csums, w.base + nblk, st);
    hipLaunchKernelGGL(fa_line_ends_kernel, dim3((unsigned)nblk), dim3(FA_NL), 0, st, d_bytes, (long long)nbytes,
                       (const u64 *)w.base, (long long)nlines, d_line_ends);
    hipLaunchKernelGGL(fa_classify_kernel, dim3(grid256(nlines)), dim3(256), 0, st, d_bytes, (const uint32_t *)d_line_ends,
                       (long long)nlines, w.cls, w.at, w.len, w.value);
    device_scan(w.value, nlines, w.pre, w.sums, w.pre + nlines, st);
    hipLaunchKernelGGL(fa_heads_kernel, dim3(grid256(nlines)), dim3(256), 0, st, (const uint8_t *)w.cls, (const u64 *)w.pre,
                       (long long)nlines, w.head_line, (u64 *)d_info + 2);
    hipLaunchKernelGGL(fa_gather_sizes_kernel, dim3(grid256(nlines)), dim3(256), 0, st, (const uint32_t *)d_line_ends,
                       (const uint8_t *)w.cls, (const uint32_t *)w.at, (const uint32_t *)w.len, (const u64 *)w.pre,
                       (const uint32_t *)w.head_line, (long long)nlines, w.value);
    device_scan(w.value, nlines, w.tail_pre, w.sums, w.tail_pre + nlines, st);
    hipLaunchKernelGGL(fa_info_kernel, dim3(1), dim3(1), 0, st, (const u64 *)w.pre, (const u64 *)w.tail_pre, (long long)nlines,
                       (long long *)d_info);
    return launched("fasta scan launch");
}

int atr_fasta_index(uint8_t *d_bytes, int64_t nbytes, const uint32_t *d_line_ends, int64_t nlines, const void *d_work,
                    int64_t nrec, int64_t tail_off, int64_t tail_bytes, atr_fastq_record *d_records,
                    uint32_t *d_record_ends, void *stream) {
    if (nbytes < 0 || nbytes >= (int64_t)0xFFFFFFF0ll || nlines < 0 || nrec < 0 || nrec > nlines || tail_bytes < 0 ||
        tail_off < nbytes || (tail_off & 15) || tail_off + tail_bytes >= (int64_t)0xFFFFFFF0ll)
        return ATR_ERR_INVALID;
    if (nrec == 0) return ATR_OK;
    if (!d_bytes || !d_work || !d_line_ends || !d_records || !d_record_ends || ((uintptr_t)d_bytes & 15)) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const FaWork w = fa_work(d_work, nbytes, nlines);
    hipLaunchKernelGGL(fa_records_kernel, dim3(grid256(nrec)), dim3(256), 0, st, d_line_ends, (const uint8_t *)w.cls,
                       (const uint32_t *)w.at, (const uint32_t *)w.len, (const u64 *)w.pre, (const uint32_t *)w.head_line,
                       (long long)nlines, (long long)nrec, (const u64 *)w.tail_pre, (uint32_t)tail_off, (FastqRecord *)d_records,
                       d_record_ends);
    if (tail_bytes > 0)
        hipLaunchKernelGGL(fa_gather_kernel, dim3((unsigned)blocks(nlines, 4)), dim3(256), 0, st, d_bytes, d_line_ends,
                           (const uint8_t *)w.cls, (const uint32_t *)w.at, (const uint32_t *)w.len, (const u64 *)w.pre,
                           (const uint32_t *)w.head_line, (long long)nlines, (long long)nrec, (const u64 *)w.tail_pre,
                           (uint32_t)tail_off, (uint32_t)tail_bytes);
    return launched("fasta index launch");
}

// work layout: scan_work of 64-bit sizes, a spare word behind the sums
size_t atr_fasta_emit_work_bytes(int64_t n) { return n < 0 ? 0 : scan_work_bytes<u64>(n, 1); }

int atr_fasta_emit(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                   const int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end,
                   const uint8_t *d_dest, int dest, int64_t n, int record_bytes_hint, int64_t *d_offsets, void *d_work,
                   uint8_t *d_out, void *stream) {
    (void)record_bytes_hint;
    if (n < 0 || !d_offsets || ((d_unmasked_begin == nullptr) != (d_unmasked_end == nullptr))) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (!d_out) hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, st, (long long *)d_offsets, 0ll);
        return launched("fasta emit launch");
    }
    if (!d_bytes || !d_records || !d_begin || !d_end || !d_work) return ATR_ERR_INVALID;
    if (!d_out) {
        Workspace ws(d_work);
        const ScanWork<u64> w = scan_work<u64>(ws, n, 1);
        hipLaunchKernelGGL(fa_emit_sizes_kernel, dim3(grid256(n)), dim3(256), 0, st, (const FastqRecord *)d_records, d_begin,
                           d_end, d_dest, dest, (long long)n, w.sizes);
        device_scan(w.sizes, n, (u64 *)d_offsets, w.sums, (u64 *)d_offsets + n, st);
        return launched("fasta emit sizes launch");
    }
    hipLaunchKernelGGL(fa_emit_kernel, dim3((unsigned)blocks(n * FA_EMIT_LANES, 256)), dim3(256), 0, st, d_bytes,
                       (const FastqRecord *)d_records, d_begin, d_end, d_unmasked_begin, d_unmasked_end, d_dest, dest,
                       (long long)n, (const long long *)d_offsets, d_out);
    return launched("fasta emit launch");
}

}  // extern "C"

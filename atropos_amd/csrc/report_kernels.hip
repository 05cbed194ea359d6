// report_kernels.hip -- the trim report: what the reference's modifiers, filters and formatters count while they work
// (summary['trim'], commands/trim/__init__.py:129-137), added to a counter block that stays on the device for the
// whole run (layout and per-lane arithmetic: report_core.hpp).
//
//   rep_intervals_kernel  a lane per read, after a trimmer stage: the bases the stage counts as trimmed, summed over
//                         the wave with __shfl_xor, one 64-bit atomic per wave into the stage's slot.
//   rep_adapters_kernel   a lane per read, once per adapter round: the match's (side, length, errors) bin of its
//                         adapter and the base before a 3' match, `weight` each.  When the table of the round's longest
//                         read fits the block's LDS the bins are 32-bit LDS atomics and every block adds its non-zero
//                         words to the resident table once; else 64-bit global atomics per match.
//   rep_outputs_kernel    a lane per read, after the filters: records and written bases per destination, input
//                         records and bases, reads with an adapter; 32-bit sums per lane, a ballot per word decides
//                         whether the wave reduces it at all (__shfl_xor), one 64-bit atomic per wave and word
//                         that is not zero.
// Integer sums only: the block does not depend on launch shape or order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "atropos_hip.h"
#include "launch_util.hpp"
#include "fastq_core.hpp"
#include "report_core.hpp"

namespace atr {

typedef unsigned long long u64;

struct ReportHandle {
    RepLayout L;
};

__device__ __forceinline__ long long rep_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ unsigned rep_wave_sum32(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void rep_intervals_kernel(const FastqRecord *__restrict__ recs,
                                                            const int32_t *__restrict__ b0, const int32_t *__restrict__ e0,
                                                            const int32_t *__restrict__ b1, const int32_t *__restrict__ e1,
                                                            long long n, int mode, int front, int back, u64 *slot) {
    long long sum = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        sum += rep_trimmed_bases(mode, b0[i], e0[i], b1[i], e1[i], front, back, (int)recs[i].seq_len);
    sum = rep_wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(slot, (u64)sum);
}

__global__ __launch_bounds__(256) void rep_adapters_kernel(RepLayout G, int lds_len, const uint8_t *__restrict__ bytes,
                                                           const FastqRecord *__restrict__ recs,
                                                           const uint8_t *__restrict__ took, const int16_t *__restrict__ best,
                                                           const long long *__restrict__ which,
                                                           const uint8_t *__restrict__ front, int default_front,
                                                           const int32_t *__restrict__ begin, const int32_t *__restrict__ end,
                                                           long long n, unsigned weight, u64 *counters) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rep_lds[];
    const bool in_lds = lds_len >= 0;
    RepLayout S = G;                                                   // the layout the bins are counted in
    if (in_lds) S.max_len = lds_len;
    const int lds_words = in_lds ? (int)(S.nadapters * rep_adapter_words(S)) : 0;
    if (in_lds) {
        for (int w = threadIdx.x; w < lds_words; w += 256) rep_lds[w] = 0;
        __syncthreads();
    }
    u64 *table = counters + REP_HDR;
    long long overflow = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if (!took[i]) continue;
        const int b = begin[i], len = end[i] - b;
        const RepHit h = rep_adapter_hit(best + i * 8, len, front ? (int)front[i] : default_front,
                                         bytes + (size_t)recs[i].seq_off + b);
        const long long a = which[i];
        if (!rep_hit_fits(S, h, a)) { ++overflow; continue; }
        const long long bin = rep_hist_word(S, (int)a, h.back, h.length, h.errors);
        if (in_lds) {
            atomicAdd(&rep_lds[bin], weight);
            if (h.adj >= 0) atomicAdd(&rep_lds[rep_adj_word(S, (int)a, h.adj)], weight);
        } else {
            atomicAdd(&table[bin], (u64)weight);
            if (h.adj >= 0) atomicAdd(&table[rep_adj_word(S, (int)a, h.adj)], (u64)weight);
        }
    }
    overflow = rep_wave_sum(overflow);
    if ((threadIdx.x & 63) == 0 && overflow) atomicAdd(&counters[REP_OVERFLOW], (u64)overflow);
    if (in_lds) {
        __syncthreads();
        for (int w = threadIdx.x; w < lds_words; w += 256) {
            const uint32_t v = rep_lds[w];
            if (v) atomicAdd(&table[rep_rebase_word(S, G, w)], (u64)v);
        }
    }
}

// Per-lane and per-wave sums are 32-bit: a chunk is below 4 GiB of text (atr_fastq_index), so no sum of read lengths
// over a part of it reaches 2^32; the block's words are 64-bit.
__global__ __launch_bounds__(256) void rep_outputs_kernel(const FastqRecord *__restrict__ recs,
                                                          const int32_t *__restrict__ begin, const int32_t *__restrict__ end,
                                                          const uint8_t *__restrict__ matched, const uint8_t *__restrict__ dest,
                                                          long long n, u64 *counters) {
    unsigned records = 0, bases = 0, adapters = 0;
    unsigned dn[REP_DESTS], dbp[REP_DESTS];
#pragma unroll
    for (int d = 0; d < REP_DESTS; ++d) dn[d] = dbp[d] = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned len = end[i] > begin[i] ? (unsigned)(end[i] - begin[i]) : 0u;   // (a masked read is written whole)
        const int mine = dest[i] < REP_DESTS ? dest[i] : REP_DESTS - 1;
        ++records;
        bases += recs[i].seq_len;
        adapters += matched[i] != 0;
#pragma unroll
        for (int d = 0; d < REP_DESTS; ++d) {
            dn[d] += mine == d;
            dbp[d] += mine == d ? len : 0u;
        }
    }
    const bool first = (threadIdx.x & 63) == 0;
    if (__ballot(records != 0) == 0) return;                            // (wave-uniform: a wave beyond the batch)
    records = rep_wave_sum32(records); bases = rep_wave_sum32(bases);
    if (first) atomicAdd(&counters[REP_IN_RECORDS], (u64)records);
    if (first && bases) atomicAdd(&counters[REP_IN_BASES], (u64)bases);
    if (__ballot(adapters != 0)) {
        adapters = rep_wave_sum32(adapters);
        if (first) atomicAdd(&counters[REP_WITH_ADAPTERS], (u64)adapters);
    }
#pragma unroll
    for (int d = 0; d < REP_DESTS; ++d) {
        if (__ballot(dn[d] != 0) == 0) continue;                        // most waves see one or two destinations
        const unsigned c = rep_wave_sum32(dn[d]), bp = rep_wave_sum32(dbp[d]);
        if (first) atomicAdd(&counters[REP_DEST + d], (u64)c);
        if (first && bp) atomicAdd(&counters[REP_DEST_BP + d], (u64)bp);
    }
}

}  // namespace atr

using namespace atr;

static inline unsigned rep_grid(long long n) {
    return (unsigned)std::max<long long>(1, std::min<long long>((n + 1023) / 1024, 1024));
}

extern "C" {

int atr_report_create(int n_adapters, int max_read_len, int max_errors, void **out) {
    if (!out) return ATR_ERR_INVALID;
    *out = nullptr;
    const RepLayout L = {n_adapters, max_read_len, max_errors};
    const int rc = rep_layout_check(L);
    if (rc) return rc == -1 ? ATR_ERR_INVALID : ATR_ERR_UNSUPPORTED;
    ReportHandle *h = new (std::nothrow) ReportHandle();
    if (!h) return ATR_ERR_NOMEM;
    h->L = L;
    *out = h;
    return ATR_OK;
}

void atr_report_destroy(void *report) { delete (ReportHandle *)report; }

int64_t atr_report_counters(const void *report) {
    const ReportHandle *h = (const ReportHandle *)report;
    return h ? rep_words(h->L) : ATR_ERR_INVALID;
}

int atr_report_intervals(const void *report, const atr_fastq_record *d_records, const int32_t *d_begin0,
                         const int32_t *d_end0, const int32_t *d_begin1, const int32_t *d_end1, int64_t n, int mode, int front,
                         int back, int slot, void *d_counters, void *stream) {
    if (!report || n < 0 || mode < REP_SUBSEQ || mode > REP_NEND || front < 0 || back < 0 || slot < 0 || slot >= REP_SLOTS)
        return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_records || !d_begin0 || !d_end0 || !d_begin1 || !d_end1 || !d_counters) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(rep_intervals_kernel, dim3(rep_grid(n)), dim3(256), 0, (hipStream_t)stream,
                       (const FastqRecord *)d_records, d_begin0, d_end0, d_begin1, d_end1, (long long)n, mode, front, back,
                       (u64 *)d_counters + REP_TRIM + slot);
    return launched("atr_report_intervals launch");
}

int atr_report_adapters(const void *report, const uint8_t *d_bytes, const atr_fastq_record *d_records, const uint8_t *d_took,
                        const int16_t *d_best, const int64_t *d_which, const uint8_t *d_front, int default_front,
                        const int32_t *d_begin, const int32_t *d_end, int64_t n, int longest, int weight, int variant,
                        void *d_counters, void *stream) {
    const ReportHandle *h = (const ReportHandle *)report;
    if (!h || n < 0 || longest < 0 || weight < 1 || weight > 2 || default_front < 0 || default_front > 2 ||
        variant < ATR_REPORT_AUTO || variant > ATR_REPORT_GLOBAL)
        return ATR_ERR_INVALID;
    if (longest > h->L.max_len) return ATR_ERR_UNSUPPORTED;             // before anything is launched or counted
    RepLayout S = h->L;
    S.max_len = longest;
    const bool fits = S.nadapters * rep_adapter_words(S) <= REP_LDS_WORDS;
    if (variant == ATR_REPORT_LDS && !fits) return ATR_ERR_UNSUPPORTED;
    if (n == 0 || h->L.nadapters == 0) return ATR_OK;
    if (!d_bytes || !d_records || !d_took || !d_best || !d_which || !d_begin || !d_end || !d_counters) return ATR_ERR_INVALID;
    const bool in_lds = variant == ATR_REPORT_LDS || (variant == ATR_REPORT_AUTO && fits);
    const size_t lds = in_lds ? (size_t)(S.nadapters * rep_adapter_words(S)) * 4 : 0;
    hipLaunchKernelGGL(rep_adapters_kernel, dim3(rep_grid(n)), dim3(256), lds, (hipStream_t)stream, h->L,
                       in_lds ? longest : -1, d_bytes, (const FastqRecord *)d_records, d_took, d_best,
                       (const long long *)d_which, d_front, default_front, d_begin, d_end, (long long)n, (unsigned)weight,
                       (u64 *)d_counters);
    return launched("atr_report_adapters launch");
}

int atr_report_outputs(const void *report, const atr_fastq_record *d_records, const int32_t *d_begin, const int32_t *d_end,
                       const uint8_t *d_matched, const uint8_t *d_dest, int64_t n, void *d_counters, void *stream) {
    if (!report || n < 0) return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_records || !d_begin || !d_end || !d_matched || !d_dest || !d_counters) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(rep_outputs_kernel, dim3(rep_grid(n)), dim3(256), 0, (hipStream_t)stream,
                       (const FastqRecord *)d_records, d_begin, d_end, d_matched, d_dest, (long long)n, (u64 *)d_counters);
    return launched("atr_report_outputs launch");
}

int atr_report_read(const void *report, const void *d_counters, int64_t *out, void *stream) {
    if (!report || !d_counters || !out) return ATR_ERR_INVALID;
    hipError_t e = hipMemcpyAsync(out, d_counters, (size_t)atr_report_counters(report) * 8, hipMemcpyDeviceToHost,
                                  (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? ATR_OK : hip_fail(e, "atr_report_read");
}

}  // extern "C"

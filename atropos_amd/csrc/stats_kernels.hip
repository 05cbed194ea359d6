// stats_kernels.hip -- read statistics over a device-resident FASTQ chunk (ReadStatistics.collect_record,
// commands/stats.py:194-255): counts, length / GC% / mean-quality histograms with the first read of every bin, and
// the per-position byte tables, added into a caller-owned block of uint64 counters (stats_core.hpp) so that any
// number of chunks accumulates on the device without a host round trip.
//
// Both kernels take the reads in groups of 64: every lane loads the descriptor and kept interval of one read of
// the group (one coalesced step), then the wave walks the group's selected reads four at a time, whose byte loads
// are independent of each other (a read at a time left one dependent chain of record load -> byte load per read:
// latency bound at 3.5 % of HBM bandwidth).  Integer adds and max only: the counts do not depend on launch shape
// or order.
//   stats_scalar_kernel    count, length bin (a lane per read); per read, lanes over consecutive positions: GC
//                          count and quality sum by wave reduction; the three histograms and their first-read
//                          indices in per-block LDS (lengths beyond ST_LEN_LDS straight to the global bins).
//   stats_position_kernel  grid.y = windows of 64 positions, lane = position: A C G T N counted in registers
//                          across all the wave's reads, qualities '!'..'~' in a per-block LDS table [64][94] with
//                          an odd row pitch (rows of the 64 lanes fall into different banks), anything else with a
//                          global atomic.  Every block flushes its non-zero counters once, one atomic per bin.
//                          Every window reads the descriptors of the whole chunk: a chunk with one very long read
//                          among short ones pays a descriptor pass (32 B per read) per 64 positions of that read.
#include <hip/hip_runtime.h>
#include <limits.h>

#include <algorithm>

#include "atropos_hip.h"
#include "launch_util.hpp"
#include "fastq_core.hpp"
#include "stats_core.hpp"

namespace atr {

constexpr int ST_WIN = 64;             // positions per window of the position kernel (one per lane)
constexpr int ST_QSYM = 94;            // quality bytes '!' .. '~' kept in LDS
constexpr int ST_QPITCH = 95;          // odd row pitch of the LDS quality table
constexpr int ST_LEN_LDS = 1024;       // read lengths binned in LDS by the scalar kernel
constexpr int ST_ILP = 4;              // reads of a group in flight at once

typedef unsigned long long u64;

struct StatsArgs {
    u64 *st;
    int max_len, longest, quality_base;
    const uint8_t *bytes;
    const FastqRecord *records;
    const int32_t *begin, *end, *ubegin, *uend;
    const uint8_t *dest;
    int which;
    long long n;
    u64 index_base;                    // index of the chunk's first record in the stream (first-seen order)
};

// one read of a group: the kept interval [a, a + len) as atr_fastq_emit writes it, the unmasked part [ub, ue)
struct StView {
    uint32_t so, qo;
    int a, len, ub, ue, hasq;
    bool sel;                          // selected (in range, destination) and within `longest`
    bool skip;                         // selected but longer than `longest`
};

__device__ __forceinline__ StView st_view(const StatsArgs &A, long long r) {
    StView v{0u, 0u, 0, 0, INT_MIN, INT_MAX, 0, false, false};
    if (r >= A.n || (A.dest && A.dest[r] != A.which)) return v;
    const FastqRecord rec = A.records[r];
    v.so = rec.seq_off; v.qo = rec.qual_off; v.hasq = rec.qual_len > 0;
    v.a = A.begin ? A.begin[r] : 0;
    const int b = A.end ? max(v.a, A.end[r]) : (int)rec.seq_len;
    v.len = b - v.a;
    if (A.ubegin) { v.ub = A.ubegin[r]; v.ue = A.uend[r]; }
    v.sel = v.len <= A.longest;
    v.skip = !v.sel;
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the next ST_ILP set bits of a wave-uniform mask (lane numbers; ok[u] = false once it runs out)
__device__ __forceinline__ void take_lanes(u64 &mask, int (&j)[ST_ILP], bool (&ok)[ST_ILP]) {
#pragma unroll
    for (int u = 0; u < ST_ILP; ++u) {
        ok[u] = mask != 0;
        j[u] = ok[u] ? __ffsll((long long)mask) - 1 : 0;
        if (ok[u]) mask &= mask - 1;
    }
}

__global__ __launch_bounds__(256) void stats_scalar_kernel(StatsArgs A) {
    __shared__ uint32_t s_len[ST_LEN_LDS], s_gc[ST_GC_BINS], s_mq[ST_MQ_BINS], s_hdr[4];
    __shared__ u64 f_len[ST_LEN_LDS], f_gc[ST_GC_BINS], f_mq[ST_MQ_BINS];      // ~first read index, 0 = none
    for (int i = threadIdx.x; i < ST_LEN_LDS; i += 256) { s_len[i] = 0; f_len[i] = 0; }
    for (int i = threadIdx.x; i < ST_MQ_BINS; i += 256) { s_mq[i] = 0; f_mq[i] = 0; }
    if (threadIdx.x < ST_GC_BINS) { s_gc[threadIdx.x] = 0; f_gc[threadIdx.x] = 0; }
    if (threadIdx.x < 4) s_hdr[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long nw = (long long)gridDim.x * 4;
    const long long L = A.max_len;
    u64 *glen = A.st + st_len_off(A.max_len), *gfirst = A.st + st_first_off(A.max_len);
    for (long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); g * 64 < A.n; g += nw) {
        const long long r = g * 64 + lane;
        const StView v = st_view(A, r);
        const u64 tag = ~(A.index_base + (u64)r);
        if (v.skip) atomicAdd(&s_hdr[ST_SKIPPED], 1u);
        if (v.sel) {
            atomicAdd(&s_hdr[ST_COUNT], 1u);
            if (v.len < ST_LEN_LDS) {
                atomicAdd(&s_len[v.len], 1u);
                if (f_len[v.len] < tag) atomicMax(&f_len[v.len], tag);
            } else {
                atomicAdd(&glen[v.len], 1ull);
                atomicMax(&gfirst[v.len], tag);
            }
        }
        u64 mask = __ballot(v.sel && v.len > 0);
        while (mask) {
            int j[ST_ILP];
            bool ok[ST_ILP];
            take_lanes(mask, j, ok);
            int len[ST_ILP], a[ST_ILP], ub[ST_ILP], ue[ST_ILP], hq[ST_ILP], gc[ST_ILP], qs[ST_ILP];
            uint32_t so[ST_ILP], qo[ST_ILP];
            int most = 0;
#pragma unroll
            for (int u = 0; u < ST_ILP; ++u) {
                len[u] = ok[u] ? __shfl(v.len, j[u], 64) : 0;
                a[u] = __shfl(v.a, j[u], 64); ub[u] = __shfl(v.ub, j[u], 64); ue[u] = __shfl(v.ue, j[u], 64);
                hq[u] = __shfl(v.hasq, j[u], 64);
                so[u] = __shfl(v.so, j[u], 64); qo[u] = __shfl(v.qo, j[u], 64);
                gc[u] = 0; qs[u] = 0;
                most = max(most, len[u]);
            }
            for (int k = lane; k - lane < most; k += 64) {
                uint8_t c[ST_ILP], q[ST_ILP];
#pragma unroll
                for (int u = 0; u < ST_ILP; ++u) {            // the loads of the four reads first
                    const int pos = a[u] + k;
                    const bool in = k < len[u];
                    c[u] = (in && pos >= ub[u] && pos < ue[u]) ? A.bytes[(size_t)so[u] + pos] : (uint8_t)'N';
                    q[u] = (in && hq[u]) ? A.bytes[(size_t)qo[u] + pos] : (uint8_t)0;
                }
#pragma unroll
                for (int u = 0; u < ST_ILP; ++u) {
                    gc[u] += (k < len[u]) & ((c[u] == 'C') | (c[u] == 'G'));
                    qs[u] += q[u];
                }
            }
#pragma unroll
            for (int u = 0; u < ST_ILP; ++u) { gc[u] = wave_sum(gc[u]); qs[u] = wave_sum(qs[u]); }
            if (lane < ST_ILP) {
                int mylen = 0, mygc = 0, myqs = 0, myhq = 0, myj = 0;
                bool myok = false;
#pragma unroll
                for (int u = 0; u < ST_ILP; ++u)
                    if (lane == u) { myok = ok[u]; mylen = len[u]; mygc = gc[u]; myqs = qs[u]; myhq = hq[u]; myj = j[u]; }
                if (myok) {
                    const u64 t = ~(A.index_base + (u64)(g * 64 + myj));
                    const int gb = st_div_round_even(100 * mygc, mylen);
                    atomicAdd(&s_gc[gb], 1u);
                    if (f_gc[gb] < t) atomicMax(&f_gc[gb], t);
                    atomicMax(&s_hdr[ST_LONGEST], (uint32_t)mylen);
                    if (myhq) {
                        atomicAdd(&s_hdr[ST_WITHQ], 1u);
                        const int mb = st_div_round_even(myqs - A.quality_base * mylen, mylen) + A.quality_base;
                        atomicAdd(&s_mq[mb], 1u);
                        if (f_mq[mb] < t) atomicMax(&f_mq[mb], t);
                    }
                }
            }
        }
    }
    __syncthreads();
    const int lmax = min(ST_LEN_LDS - 1, A.longest);
    for (int i = threadIdx.x; i <= lmax; i += 256) {
        if (s_len[i]) atomicAdd(&glen[i], (u64)s_len[i]);
        if (f_len[i]) atomicMax(&gfirst[i], f_len[i]);
    }
    for (int i = threadIdx.x; i < ST_MQ_BINS; i += 256) {
        if (s_mq[i]) atomicAdd(&A.st[st_mq_off(A.max_len) + i], (u64)s_mq[i]);
        if (f_mq[i]) atomicMax(&gfirst[L + 1 + ST_GC_BINS + i], f_mq[i]);
    }
    if (threadIdx.x < ST_GC_BINS) {
        if (s_gc[threadIdx.x]) atomicAdd(&A.st[st_gc_off(A.max_len) + threadIdx.x], (u64)s_gc[threadIdx.x]);
        if (f_gc[threadIdx.x]) atomicMax(&gfirst[L + 1 + threadIdx.x], f_gc[threadIdx.x]);
    }
    if (threadIdx.x == 0) {
        if (s_hdr[ST_COUNT]) atomicAdd(&A.st[ST_COUNT], (u64)s_hdr[ST_COUNT]);
        if (s_hdr[ST_WITHQ]) atomicAdd(&A.st[ST_WITHQ], (u64)s_hdr[ST_WITHQ]);
        if (s_hdr[ST_SKIPPED]) atomicAdd(&A.st[ST_SKIPPED], (u64)s_hdr[ST_SKIPPED]);
        if (s_hdr[ST_LONGEST]) atomicMax(&A.st[ST_LONGEST], (u64)s_hdr[ST_LONGEST]);
    }
}

__global__ __launch_bounds__(256) void stats_position_kernel(StatsArgs A) {
    __shared__ uint32_t s_q[ST_WIN * ST_QPITCH];
    __shared__ uint32_t s_b[5 * ST_WIN];
    for (int i = threadIdx.x; i < ST_WIN * ST_QPITCH; i += 256) s_q[i] = 0;
    for (int i = threadIdx.x; i < 5 * ST_WIN; i += 256) s_b[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w0 = (int)blockIdx.y * ST_WIN;                   // first position of the window
    const int p = w0 + lane;
    const long long nw = (long long)gridDim.x * 4;
    u64 *gseq = A.st + st_seq_off(A.max_len) + (long long)p * 256;
    u64 *gqual = A.st + st_qual_off(A.max_len) + (long long)p * 256;
    uint32_t cA = 0, cC = 0, cG = 0, cT = 0, cN = 0;
    uint32_t *myq = s_q + lane * ST_QPITCH;
    for (long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); g * 64 < A.n; g += nw) {
        const StView v = st_view(A, g * 64 + lane);
        u64 mask = __ballot(v.sel && v.len > w0);              // the group's reads that reach this window
        while (mask) {
            int j[ST_ILP];
            bool ok[ST_ILP];
            take_lanes(mask, j, ok);
            uint8_t c[ST_ILP];
            uint32_t q[ST_ILP];
            bool in[ST_ILP], hq[ST_ILP];
#pragma unroll
            for (int u = 0; u < ST_ILP; ++u) {                  // the loads of the four reads first
                const int len = __shfl(v.len, j[u], 64), a = __shfl(v.a, j[u], 64);
                const int ub = __shfl(v.ub, j[u], 64), ue = __shfl(v.ue, j[u], 64);
                const uint32_t so = __shfl(v.so, j[u], 64), qo = __shfl(v.qo, j[u], 64);
                hq[u] = __shfl(v.hasq, j[u], 64) != 0;
                in[u] = ok[u] && p < len;
                const int pos = a + p;
                c[u] = (in[u] && pos >= ub && pos < ue) ? A.bytes[(size_t)so + pos] : (uint8_t)'N';
                q[u] = (in[u] && hq[u]) ? A.bytes[(size_t)qo + pos] : 0u;
            }
#pragma unroll
            for (int u = 0; u < ST_ILP; ++u) {
                if (!in[u]) continue;
                const uint8_t b = c[u];
                cA += b == 'A'; cC += b == 'C'; cG += b == 'G'; cT += b == 'T'; cN += b == 'N';
                if (b != 'A' && b != 'C' && b != 'G' && b != 'T' && b != 'N') atomicAdd(&gseq[b], 1ull);
                if (hq[u]) {
                    if (q[u] - 33u < (uint32_t)ST_QSYM) atomicAdd(&myq[q[u] - 33u], 1u);
                    else atomicAdd(&gqual[q[u]], 1ull);
                }
            }
        }
    }
    if (cA) atomicAdd(&s_b[0 * ST_WIN + lane], cA);
    if (cC) atomicAdd(&s_b[1 * ST_WIN + lane], cC);
    if (cG) atomicAdd(&s_b[2 * ST_WIN + lane], cG);
    if (cT) atomicAdd(&s_b[3 * ST_WIN + lane], cT);
    if (cN) atomicAdd(&s_b[4 * ST_WIN + lane], cN);
    __syncthreads();
    const int npos = min(ST_WIN, A.longest - w0);              // positions of this window the table has
    u64 *seq0 = A.st + st_seq_off(A.max_len) + (long long)w0 * 256;
    u64 *qual0 = A.st + st_qual_off(A.max_len) + (long long)w0 * 256;
    for (int i = threadIdx.x; i < 5 * ST_WIN; i += 256) {
        const int k = i / ST_WIN, j = i % ST_WIN;
        if (j < npos && s_b[i]) atomicAdd(&seq0[(long long)j * 256 + "ACGTN"[k]], (u64)s_b[i]);
    }
    for (int i = threadIdx.x; i < ST_WIN * ST_QSYM; i += 256) {
        const int j = i / ST_QSYM, s = i % ST_QSYM;
        const uint32_t v = s_q[j * ST_QPITCH + s];
        if (j < npos && v) atomicAdd(&qual0[(long long)j * 256 + 33 + s], (u64)v);
    }
}

// dst += src, both blocks laid out for their own capacity (dst_L >= src_L); src's reads come after dst's:
// its first-read indices are shifted by `offset`
__global__ __launch_bounds__(256) void stats_merge_kernel(u64 *__restrict__ dst, int dst_L, const u64 *__restrict__ src,
                                                          int src_L, u64 offset) {
    const long long total = st_words(src_L);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const u64 v = src[i];
        if (!v) continue;
        long long j;
        if (i < ST_HDR) {
            if (i == ST_LONGEST) { dst[i] = max(dst[i], v); continue; }
            j = i;
        } else if (i < st_gc_off(src_L)) j = i;                                   // lengths: same offset
        else if (i < st_seq_off(src_L)) j = i - st_gc_off(src_L) + st_gc_off(dst_L);
        else if (i < st_qual_off(src_L)) j = i - st_seq_off(src_L) + st_seq_off(dst_L);
        else if (i < st_first_off(src_L)) j = i - st_qual_off(src_L) + st_qual_off(dst_L);
        else {                                                                    // first-read indices: the earlier
            const long long k = i - st_first_off(src_L);                         // read wins (~index: the larger)
            j = k <= src_L ? st_first_off(dst_L) + k : k - (src_L + 1) + st_first_off(dst_L) + dst_L + 1;
            dst[j] = max(dst[j], v - offset);
            continue;
        }
        dst[j] += v;                                          // one thread per word: no other writer
    }
}

}  // namespace atr

using namespace atr;

static inline int st_check_len(int max_len) {
    if (max_len < 1) return ATR_ERR_INVALID;
    if (max_len > ATR_MAX_LONG_READ_LEN) return ATR_ERR_UNSUPPORTED;
    return ATR_OK;
}

extern "C" {

int64_t atr_read_stats_bytes(int max_len) {
    const int rc = st_check_len(max_len);
    return rc ? rc : (int64_t)st_words(max_len) * 8;
}

int atr_read_stats_clear(void *d_stats, int max_len, void *stream) {
    const int rc = st_check_len(max_len);
    if (rc) return rc;
    if (!d_stats) return ATR_ERR_INVALID;
    hipError_t e = hipMemsetAsync(d_stats, 0, (size_t)st_words(max_len) * 8, (hipStream_t)stream);
    return e == hipSuccess ? ATR_OK : hip_fail(e, "atr_read_stats_clear");
}

int atr_read_stats_batch(void *d_stats, int max_len, int longest, int quality_base, const uint8_t *d_bytes,
                         const atr_fastq_record *d_records, const int32_t *d_begin, const int32_t *d_end,
                         const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end, const uint8_t *d_dest,
                         int which, int64_t n, int64_t index_base, void *stream) {
    const int rc = st_check_len(max_len);
    if (rc) return rc;
    if (!d_stats || n < 0 || index_base < 0 || longest < 0 || longest > max_len || quality_base < 0 || quality_base > 255)
        return ATR_ERR_INVALID;
    if ((d_begin == nullptr) != (d_end == nullptr) || (d_unmasked_begin == nullptr) != (d_unmasked_end == nullptr) ||
        (d_unmasked_begin && !d_begin))
        return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!d_bytes || !d_records) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    StatsArgs A{(u64 *)d_stats, max_len, longest, quality_base, d_bytes, (const FastqRecord *)d_records, d_begin, d_end,
                d_unmasked_begin, d_unmasked_end, d_dest, which, (long long)n, (u64)index_base};
    const long long blocks = (n + 255) / 256;                 // a wave per group of 64 reads, four waves per block
    hipLaunchKernelGGL(stats_scalar_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>(blocks, 2048))),
                       dim3(256), 0, st, A);
    if (longest > 0) {
        // a wave per read and window; the windows of one block column share their reads (L2)
        const int nwin = (longest + ST_WIN - 1) / ST_WIN;
        const long long gx = std::max<long long>(1, std::min<long long>(blocks, std::max(64, 3072 / nwin)));
        hipLaunchKernelGGL(stats_position_kernel, dim3((unsigned)gx, (unsigned)nwin), dim3(256), 0, st, A);
    }
    return launched("atr_read_stats_batch launch");
}

int atr_read_stats_merge(void *d_dst, int dst_max_len, const void *d_src, int src_max_len, int64_t index_offset,
                         void *stream) {
    int rc = st_check_len(dst_max_len);
    if (!rc) rc = st_check_len(src_max_len);
    if (rc) return rc;
    if (!d_dst || !d_src || src_max_len > dst_max_len || index_offset < 0) return ATR_ERR_INVALID;
    const long long total = st_words(src_max_len);
    hipLaunchKernelGGL(stats_merge_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096)), dim3(256), 0,
                       (hipStream_t)stream, (u64 *)d_dst, dst_max_len, (const u64 *)d_src, src_max_len, (u64)index_offset);
    return launched("atr_read_stats_merge launch");
}

}  // extern "C"

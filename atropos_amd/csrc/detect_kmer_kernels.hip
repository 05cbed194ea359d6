// detect_kmer_kernels.hip -- de-novo adapter discovery over the representatives of the distinct pass (the
// reference's HeuristicDetector._get_contaminants, commands/detect/__init__.py:568-619; layouts, keys and decisions:
// detect_kmer_core.hpp).  Integer counting over resident reads: the caller sorts 64-bit keys (torch.sort, as the
// distinct pass does), the kernels make the keys and turn sorted runs into classes.
//
//   kmer_slots_kernel   a wave per representative: its row of the table, the read of each of its slots, level = k0
//   kmer_pair_kernel    a thread per slot: the key of the (a + b)-mer from the classes of its a-mer and its b-mer
//   kmer_heads_kernel / the shared prefix sum / kmer_rank_kernel
//                       sorted keys -> the class of every entry (scattered back to its slot) and, per class, its run
//                       in the sorted order (count = end - begin) and the smallest slot that holds it (an atomic
//                       minimum: the first occurrence in record order, whatever order the entries came in)
//   kmer_level_kernel   a thread per surviving slot of level k: its class is over-represented when its run is longer
//                       than min_count; then its read is in S_{k+1} (level[read] = k + 1; every writer stores the
//                       same value) and the slot the class names appends the candidate row.  A read of exactly k
//                       bases whose only k-mer is over-represented flags the candidates of its two (k - 1)-mers
//                       (the reference's `seq in cur`, :603-605).
//   kmer_next_kernel    in a later launch: the slots of the reads of S_{k+1} with room for k + 1 bytes, compacted
//                       (a wave takes its places with one atomic add; the order is not kept and nothing depends on
//                       it), with their level keys
//   kmer_gather_kernel  a wave per candidate: its text into one byte buffer
//   kmer_support_kernel a wave per representative, patterns and the read staged in LDS, lanes over start offsets:
//                       the reads that hold a pattern (abundance) and, over the reads of S_len(pattern), the smallest
//                       (first index, record) -- the longest-match rule.  LDS atomics per block, one flush.
// Sums, minima and ranks of integers only: the candidate table as a set, level[], abundance and the longest-match
// word do not depend on launch shape or run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "atropos_hip.h"
#include "launch_util.hpp"
#include "detect_kmer_core.hpp"
#include "fastq_core.hpp"
#include "scan_kernels.hpp"

namespace atr {

__global__ __launch_bounds__(256) void kmer_slots_kernel(const FastqRecord *__restrict__ recs, const int32_t *__restrict__ kept,
                                                         const long long *__restrict__ reps, const long long *__restrict__ start,
                                                         long long nrep, long long total, int k0, KmerRep *__restrict__ tab,
                                                         int32_t *__restrict__ slot_rep, int32_t *__restrict__ level) {
    const int lane = threadIdx.x & 63;
    for (long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); j < nrep; j += (long long)gridDim.x * 4) {
        const long long r = reps[j], s = start[j];
        const int kl = min(max(kept[r], 0), KMER_MAX_READ);
        if (lane == 0) {
            KmerRep R;
            R.start = s; R.off = recs[r].seq_off; R.kept = kl; R.rec = r;
            tab[j] = R;
            level[j] = k0;
        }
        for (int o = lane; o < kl; o += 64)
            if (s + o < total) slot_rep[s + o] = (int32_t)j;
    }
}

__global__ __launch_bounds__(256) void kmer_pair_kernel(const KmerRep *__restrict__ tab, const int32_t *__restrict__ slot_rep,
                                                        long long total, const uint8_t *__restrict__ bytes,
                                                        const int32_t *__restrict__ id_a, int a, const int32_t *__restrict__ id_b,
                                                        int b, long long *__restrict__ keys) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const KmerRep R = tab[slot_rep[p]];
    const int o = (int)(p - R.start);
    long long key = KMER_NO_KEY;
    if (R.kept - o >= a + b) {
        const int32_t ia = id_a ? id_a[p] : (int32_t)bytes[(size_t)R.off + o];
        const int32_t ib = id_b ? id_b[p + a] : (int32_t)bytes[(size_t)R.off + o + a];
        key = kmer_pair_key(ia, ib);
    }
    keys[p] = key;
}

__global__ __launch_bounds__(256) void kmer_heads_kernel(const long long *__restrict__ keys, long long n, uint32_t *__restrict__ v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long key = keys[i];
    v[i] = (key != KMER_NO_KEY && (i == 0 || keys[i - 1] != key)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void kmer_rank_kernel(const long long *__restrict__ keys, const long long *__restrict__ idx,
                                                        const int32_t *__restrict__ list, long long n,
                                                        const uint32_t *__restrict__ v, const u64 *__restrict__ excl,
                                                        int32_t *__restrict__ cls, int32_t *__restrict__ begin,
                                                        int32_t *__restrict__ end, int32_t *__restrict__ head) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long key = keys[i], at = idx[i];
    const int32_t slot = list ? list[at] : (int32_t)at;
    if (key == KMER_NO_KEY) { cls[slot] = KMER_NO_CLASS; return; }
    const int32_t rank = (int32_t)(excl[i] + v[i]) - 1;
    cls[slot] = rank;
    if (v[i]) begin[rank] = (int32_t)i;
    atomicMin(&head[rank], slot);                                      // (the caller set head to all 0x7f)
    if (i + 1 == n || keys[i + 1] != key) end[rank] = (int32_t)(i + 1);
}

__global__ __launch_bounds__(256) void kmer_level_kernel(const KmerRep *__restrict__ tab, const int32_t *__restrict__ slot_rep,
                                                         const int32_t *__restrict__ list, long long n,
                                                         const int32_t *__restrict__ cls, const int32_t *__restrict__ cls_prev,
                                                         const int32_t *__restrict__ begin, const int32_t *__restrict__ end,
                                                         const int32_t *__restrict__ head, int32_t *__restrict__ cand_of,
                                                         const int32_t *__restrict__ cand_of_prev, int k, long long min_count,
                                                         int32_t *__restrict__ level, int32_t *__restrict__ cand,
                                                         long long capacity, long long *__restrict__ state) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t slot = list ? list[i] : (int32_t)i;
    const int32_t c = cls[slot];
    if (c < 0) return;
    const int32_t rep = slot_rep[slot];
    const KmerRep R = tab[rep];
    const int o = (int)(slot - R.start);
    const long long count = (long long)end[c] - begin[c];
    const bool over = kmer_over(count, min_count);
    if (head[c] == slot) {
        int32_t row = -1;
        if (over) {
            const long long at = (long long)atomicAdd((u64 *)&state[KMER_S_CANDIDATES], 1ull);
            atomicAdd((u64 *)&state[KMER_S_OVER + k], 1ull);
            if (at < capacity) {
                row = (int32_t)at;
                int32_t *w = cand + (size_t)at * KMER_C_WORDS;
                w[KMER_C_LEVEL] = k; w[KMER_C_COUNT] = (int32_t)count; w[KMER_C_REP] = rep; w[KMER_C_OFFSET] = o;
                w[KMER_C_QUIRK] = 0;
            }
        }
        cand_of[c] = row;
    }
    if (!over) return;
    level[rep] = k + 1;
    if (cls_prev && cand_of_prev && o == 0 && R.kept == k) {
        // the whole read is an over-represented k-mer: its two (k - 1)-mers are dropped from the results
        for (int d = 0; d < 2; ++d) {
            const int32_t cp = cls_prev[slot + d];
            const int32_t row = cp >= 0 ? cand_of_prev[cp] : -1;
            if (row >= 0 && row < capacity) cand[(size_t)row * KMER_C_WORDS + KMER_C_QUIRK] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void kmer_next_kernel(const KmerRep *__restrict__ tab, const int32_t *__restrict__ slot_rep,
                                                        const int32_t *__restrict__ list, long long n,
                                                        const int32_t *__restrict__ cls, const uint8_t *__restrict__ bytes,
                                                        const int32_t *__restrict__ level, int k, int32_t *__restrict__ list_next,
                                                        long long *__restrict__ keys_next, long long *__restrict__ state) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool take = false;
    int32_t slot = 0;
    long long key = 0;
    if (i < n) {
        slot = list ? list[i] : (int32_t)i;
        const int32_t c = cls[slot];
        const int32_t rep = slot_rep[slot];
        const KmerRep R = tab[rep];
        const int o = (int)(slot - R.start);
        if (c >= 0 && level[rep] == k + 1 && R.kept - o >= k + 1) {
            take = true;
            key = kmer_level_key(c, bytes[(size_t)R.off + o + k]);
        }
    }
    const u64 mask = __ballot(take);
    if (!mask) return;
    const int leader = __builtin_ctzll(mask);
    u64 base = 0;
    if (lane == leader) base = atomicAdd((u64 *)&state[KMER_S_SURVIVORS], (u64)__popcll(mask));
    base = (u64)__shfl((unsigned long long)base, leader, 64);
    if (take) {
        const u64 at = base + (u64)__popcll(mask & ((1ull << lane) - 1ull));
        if (at < (u64)n) { list_next[at] = slot; keys_next[at] = key; }
    }
}

__global__ __launch_bounds__(256) void kmer_gather_kernel(const KmerRep *__restrict__ tab, const uint8_t *__restrict__ bytes,
                                                          const int32_t *__restrict__ cand, const long long *__restrict__ text_off,
                                                          long long ncand, long long nrep, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); c < ncand; c += (long long)gridDim.x * 4) {
        const int32_t *w = cand + (size_t)c * KMER_C_WORDS;
        const int32_t rep = w[KMER_C_REP], o = w[KMER_C_OFFSET];
        const long long at = text_off[c], len = text_off[c + 1] - at;
        if (rep < 0 || rep >= nrep || o < 0) continue;
        const KmerRep R = tab[rep];
        for (int j = lane; j < len && o + j < R.kept; j += 64) out[at + j] = bytes[(size_t)R.off + o + j];
    }
}

constexpr int KMER_TEXT_STAGE = KMER_MAX_READ + 64;

__global__ __launch_bounds__(256) void kmer_support_kernel(const KmerRep *__restrict__ tab, long long nrep,
                                                           const uint8_t *__restrict__ bytes, const int32_t *__restrict__ level,
                                                           const uint8_t *__restrict__ patterns, const int32_t *__restrict__ pat_len,
                                                           int npat, u64 *__restrict__ abundance, u64 *__restrict__ longest) {
    __shared__ uint8_t s_pat[KMER_MAX_PATTERNS * KMER_MAX_READ];
    __shared__ uint8_t s_text[4][KMER_TEXT_STAGE];
    __shared__ int s_len[KMER_MAX_PATTERNS];
    __shared__ unsigned s_ab[KMER_MAX_PATTERNS];
    __shared__ u64 s_min[KMER_MAX_PATTERNS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < npat * KMER_MAX_READ; i += 256) s_pat[i] = patterns[i];
    for (int i = threadIdx.x; i < npat; i += 256) {
        const int L = pat_len[i];
        s_len[i] = (L >= 1 && L <= KMER_MAX_READ) ? L : 0;             // (0: matches nothing)
        s_ab[i] = 0; s_min[i] = ~0ull;
    }
    __syncthreads();
    uint8_t *text = s_text[wave];
    for (long long j = (long long)blockIdx.x * 4 + wave; j < nrep; j += (long long)gridDim.x * 4) {
        const KmerRep R = tab[j];
        const int kl = R.kept, lv = level[j];
        for (int o = lane; o < kl; o += 64) text[o] = bytes[(size_t)R.off + o];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int p = 0; p < npat; ++p) {
            const int L = s_len[p];
            if (L == 0 || L > kl) continue;
            const uint8_t *pat = s_pat + p * KMER_MAX_READ;
            int first = -1;
            for (int base = 0; base + L <= kl; base += 64) {
                const int o = base + lane;
                const bool hit = o + L <= kl && kmer_same(text + o, pat, L);
                const u64 m = __ballot(hit);
                if (m) { first = base + __builtin_ctzll(m); break; }
            }
            if (first >= 0 && lane == 0) {
                atomicAdd(&s_ab[p], 1u);
                if (lv >= L) atomicMin(&s_min[p], kmer_support_word(first, R.rec));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    for (int p = threadIdx.x; p < npat; p += 256) {
        if (s_ab[p]) atomicAdd(&abundance[p], (u64)s_ab[p]);
        if (s_min[p] != ~0ull) atomicMin(&longest[p], s_min[p]);
    }
}

struct KmerRankWork {
    uint32_t *v;
    u64 *excl, *sums;
};

static KmerRankWork kmer_rank_work(Workspace &ws, long long n) {
    KmerRankWork w;
    w.v = ws.take<uint32_t>((size_t)n);
    w.excl = ws.take<u64>((size_t)n);
    w.sums = ws.take<u64>((size_t)scan_blocks(n) + 1);
    return w;
}

}  // namespace atr

using namespace atr;

static inline unsigned kmer_wave_grid(long long waves) {
    return (unsigned)std::max<long long>(1, std::min<long long>((waves + 3) / 4, 8192));
}

extern "C" {

int atr_detect_kmer_slots(const atr_fastq_record *d_records, const int32_t *d_kept, const int64_t *d_reps,
                          const int64_t *d_start, int64_t nrep, int64_t total, int kmer_size, void *d_reptab,
                          int32_t *d_slot_rep, int32_t *d_level, void *stream) {
    const int rc = kmer_check_slots(nrep, total, kmer_size);
    if (rc) return rc;
    if (nrep == 0) return ATR_OK;
    if (!d_records || !d_kept || !d_reps || !d_start || !d_reptab || !d_level || (total && !d_slot_rep)) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(kmer_slots_kernel, dim3(kmer_wave_grid(nrep)), dim3(256), 0, (hipStream_t)stream,
                       (const FastqRecord *)d_records, d_kept, (const long long *)d_reps, (const long long *)d_start,
                       (long long)nrep, (long long)total, kmer_size, (KmerRep *)d_reptab, d_slot_rep, d_level);
    return launched("atr_detect_kmer_slots launch");
}

int atr_detect_kmer_pair_keys(const void *d_reptab, const int32_t *d_slot_rep, int64_t total, const uint8_t *d_bytes,
                              const int32_t *d_id_a, int a, const int32_t *d_id_b, int b, int64_t *d_keys, void *stream) {
    if (a < 1 || b < 1) return ATR_ERR_INVALID;
    const int rc = kmer_check_len(total, a + b);
    if (rc) return rc;
    if ((a == 1) != (d_id_a == nullptr) || (b == 1) != (d_id_b == nullptr)) return ATR_ERR_INVALID;
    if (total == 0) return ATR_OK;
    if (!d_reptab || !d_slot_rep || !d_bytes || !d_keys) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(kmer_pair_kernel, dim3(grid256(total)), dim3(256), 0, (hipStream_t)stream, (const KmerRep *)d_reptab,
                       d_slot_rep, (long long)total, d_bytes, d_id_a, a, d_id_b, b, (long long *)d_keys);
    return launched("atr_detect_kmer_pair_keys launch");
}

size_t atr_detect_kmer_rank_work_bytes(int64_t n) {
    if (n < 0 || n > KMER_MAX_SLOTS) return 0;
    Workspace ws(nullptr);
    kmer_rank_work(ws, n);
    return ws.bytes();
}

int atr_detect_kmer_rank(const int64_t *d_keys, const int64_t *d_idx, const int32_t *d_list, int64_t n, int32_t *d_cls,
                         int32_t *d_begin, int32_t *d_end, int32_t *d_head, int64_t *d_nclasses, void *d_work,
                         size_t work_bytes, void *stream) {
    if (n < 0 || !d_nclasses) return ATR_ERR_INVALID;
    if (n > KMER_MAX_SLOTS) return ATR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (n && (!d_keys || !d_idx || !d_cls || !d_begin || !d_end || !d_head || !d_work ||
              work_bytes < atr_detect_kmer_rank_work_bytes(n)))
        return ATR_ERR_INVALID;
    Workspace ws(d_work);
    const KmerRankWork w = kmer_rank_work(ws, n);
    if (n) {
        hipError_t e = hipMemsetAsync(d_head, 0x7f, (size_t)n * 4, st);
        if (e != hipSuccess) return hip_fail(e, "atr_detect_kmer_rank");
    }
    if (n) hipLaunchKernelGGL(kmer_heads_kernel, dim3(grid256(n)), dim3(256), 0, st, (const long long *)d_keys, (long long)n, w.v);
    device_scan<uint32_t>(w.v, (long long)n, w.excl, w.sums, (u64 *)d_nclasses, st);
    if (n)
        hipLaunchKernelGGL(kmer_rank_kernel, dim3(grid256(n)), dim3(256), 0, st, (const long long *)d_keys,
                           (const long long *)d_idx, d_list, (long long)n, (const uint32_t *)w.v, (const u64 *)w.excl, d_cls,
                           d_begin, d_end, d_head);
    return launched("atr_detect_kmer_rank launch");
}

int atr_detect_kmer_level(const void *d_reptab, const int32_t *d_slot_rep, const int32_t *d_list, int64_t n,
                          const int32_t *d_cls, const int32_t *d_cls_prev, const int32_t *d_begin, const int32_t *d_end,
                          const int32_t *d_head, int32_t *d_cand_of, const int32_t *d_cand_of_prev, int k, int64_t min_count,
                          int32_t *d_level, int32_t *d_cand, int64_t capacity, int64_t *d_state, void *stream) {
    const int rc = kmer_check_level(n, k, capacity);
    if (rc) return rc;
    if (n == 0) return ATR_OK;
    if (!d_reptab || !d_slot_rep || !d_cls || !d_begin || !d_end || !d_head || !d_cand_of || !d_level || !d_state ||
        (capacity && !d_cand) || ((d_cls_prev == nullptr) != (d_cand_of_prev == nullptr)))
        return ATR_ERR_INVALID;
    hipLaunchKernelGGL(kmer_level_kernel, dim3(grid256(n)), dim3(256), 0, (hipStream_t)stream, (const KmerRep *)d_reptab,
                       d_slot_rep, d_list, (long long)n, d_cls, d_cls_prev, d_begin, d_end, d_head, d_cand_of, d_cand_of_prev, k,
                       (long long)min_count, d_level, d_cand, (long long)capacity, (long long *)d_state);
    return launched("atr_detect_kmer_level launch");
}

int atr_detect_kmer_next(const void *d_reptab, const int32_t *d_slot_rep, const int32_t *d_list, int64_t n,
                         const int32_t *d_cls, const uint8_t *d_bytes, const int32_t *d_level, int k, int32_t *d_list_next,
                         int64_t *d_keys_next, int64_t *d_state, void *stream) {
    const int rc = kmer_check_level(n, k, 0);
    if (rc) return rc;
    if (!d_state) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_state + KMER_S_SURVIVORS, 0, 8, st);
    if (e != hipSuccess) return hip_fail(e, "atr_detect_kmer_next");
    if (n == 0) return ATR_OK;
    if (!d_reptab || !d_slot_rep || !d_cls || !d_bytes || !d_level || !d_list_next || !d_keys_next) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(kmer_next_kernel, dim3(grid256(n)), dim3(256), 0, st, (const KmerRep *)d_reptab, d_slot_rep, d_list,
                       (long long)n, d_cls, d_bytes, d_level, k, d_list_next, (long long *)d_keys_next, (long long *)d_state);
    return launched("atr_detect_kmer_next launch");
}

int atr_detect_kmer_gather(const void *d_reptab, int64_t nrep, const uint8_t *d_bytes, const int32_t *d_cand,
                           const int64_t *d_text_off, int64_t ncand, uint8_t *d_out, void *stream) {
    if (ncand < 0 || nrep < 0) return ATR_ERR_INVALID;
    if (ncand > KMER_MAX_CANDIDATES) return ATR_ERR_UNSUPPORTED;
    if (ncand == 0) return ATR_OK;
    if (!d_reptab || !d_bytes || !d_cand || !d_text_off || !d_out) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(kmer_gather_kernel, dim3(kmer_wave_grid(ncand)), dim3(256), 0, (hipStream_t)stream,
                       (const KmerRep *)d_reptab, d_bytes, d_cand, (const long long *)d_text_off, (long long)ncand,
                       (long long)nrep, d_out);
    return launched("atr_detect_kmer_gather launch");
}

int atr_detect_kmer_support(const void *d_reptab, int64_t nrep, const uint8_t *d_bytes, const int32_t *d_level,
                            const uint8_t *d_patterns, const int32_t *d_pat_len, int npat, int64_t *d_abundance,
                            uint64_t *d_longest, void *stream) {
    const int rc = kmer_check_support(nrep, npat);
    if (rc) return rc;
    if (npat == 0) return ATR_OK;
    if (!d_patterns || !d_pat_len || !d_abundance || !d_longest) return ATR_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_abundance, 0, (size_t)npat * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_longest, 0xFF, (size_t)npat * 8, st);
    if (e != hipSuccess) return hip_fail(e, "atr_detect_kmer_support");
    if (nrep == 0) return ATR_OK;
    if (!d_reptab || !d_bytes || !d_level) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(kmer_support_kernel, dim3(kmer_wave_grid(nrep)), dim3(256), 0, st, (const KmerRep *)d_reptab,
                       (long long)nrep, d_bytes, d_level, d_patterns, d_pat_len, npat, (u64 *)d_abundance, (u64 *)d_longest);
    return launched("atr_detect_kmer_support launch");
}

}  // extern "C"

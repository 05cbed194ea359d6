// detect_kernels.hip -- known-contaminant detection over a device-resident FASTQ chunk (the reference's
// KnownContaminantDetector, commands/detect/__init__.py:495-549; tables and per-read arithmetic: detect_core.hpp).
//
// Three passes, a wavefront per read in the first and the last (lanes over consecutive bases: coalesced loads):
//   det_filter_kernel  base counts, the complexity decision from the host's table (double adds only), the
//                      past-end cut and the length tests -> kept length per read (0 = dropped) and the hash of
//                      the kept bytes.  The past-end expression works on ballot masks of "base == B" (five
//                      64-bit words per past-end base, wave-uniform): a run of >= 8 is three shifted ANDs, the
//                      trailing run is the highest clear bit.  No LDS.
//   det_mark_kernel    a lane per kept read in hash order (the caller sorts): the first read of every run of
//                      equal hashes is a representative; any other compares its bytes with that one and, only
//                      when they differ (a hash collision), with every earlier read of the run.  Exact.
//   det_match_kernel   a wave per representative: codes of the read staged in LDS, every lane packs the k-mer at
//                      its position, tests it against the bloom bits in LDS and looks the few that pass up in the
//                      global table; postings set bits in the wave's LDS bit sets (known sequence x strand x
//                      k-mer).  A match of a known sequence's first k-mer triggers the byte compare of the whole
//                      sequence (abundance).  Then a lane per known sequence: popcounts, n = max(fw, rv), LDS
//                      atomics into the block's counters; every block flushes its non-zero counters once with
//                      global atomics.  Integer sums and maxima only: the result does not depend on launch
//                      shape or order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "atropos_hip.h"
#include "launch_util.hpp"
#include "detect_core.hpp"
#include "fastq_core.hpp"

namespace atr {

typedef unsigned long long u64;

struct DetDev {
    const u64 *keys;
    const uint32_t *vals, *postings, *bloom, *thr, *seq_off;
    const uint8_t *seq_bytes, *enc, *comp_ok;
    const double *cx;
    int nseq, k, bits, words, min_k, npast, max_len;
    uint32_t mask;
    uint8_t past[DET_MAX_PAST_END];
};

struct DetectHandle {
    DetectTables T;
    DetDev D;
    void *blob = nullptr;
    size_t lds = 0;
};

__device__ __forceinline__ void det_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int det_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ u64 det_wave_sum64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (u64)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void det_filter_kernel(DetDev D, const uint8_t *__restrict__ bytes,
                                                         const FastqRecord *__restrict__ recs, long long n,
                                                         int32_t *__restrict__ kept, long long *__restrict__ hashes,
                                                         u64 *counters) {
    const int lane = threadIdx.x & 63;
    const u64 p64 = det_pow(64);
    const u64 plane = det_pow((uint32_t)lane);
    unsigned nkept = 0, nlong = 0;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (long long)gridDim.x * 4) {
        const FastqRecord rec = recs[r];
        const int len = (int)rec.seq_len;
        if (rec.seq_len > (uint32_t)D.max_len) {                       // (the entry point refuses such a chunk)
            if (lane == 0) { kept[r] = 0; hashes[r] = 0; }
            ++nlong;
            continue;
        }
        uint64_t m[DET_MAX_PAST_END][DET_CHUNKS], valid[DET_CHUNKS];
        uint8_t c[DET_CHUNKS];
        int ca = 0, cc = 0, cg = 0, ct = 0;
#pragma unroll
        for (int t = 0; t < DET_CHUNKS; ++t) {
            const int j = t * 64 + lane;
            const bool in = j < len;
            c[t] = in ? bytes[(size_t)rec.seq_off + j] : (uint8_t)0;
            const uint8_t u = det_upper(c[t]);
            ca += in & (u == 'A'); cc += in & (u == 'C'); cg += in & (u == 'G'); ct += in & (u == 'T');
            valid[t] = __ballot(in);
#pragma unroll
            for (int p = 0; p < DET_MAX_PAST_END; ++p) m[p][t] = p < D.npast ? __ballot(in && c[t] == D.past[p]) : 0ull;
        }
        ca = det_wave_sum(ca); cc = det_wave_sum(cc); cg = det_wave_sum(cg); ct = det_wave_sum(ct);
        int cut = len;
#pragma unroll
        for (int p = 0; p < DET_MAX_PAST_END; ++p)
            if (p < D.npast) cut = min(cut, det_past_end_cut(m[p], valid, len));
        const int kl = det_low_complexity(D.cx, D.max_len + 1, len, ca, cc, cg, ct) ? 0 : det_kept_len(len, cut, D.k, D.min_k);
        u64 sum = 0, pw = plane;
#pragma unroll
        for (int t = 0; t < DET_CHUNKS; ++t) {
            if (t * 64 + lane < kl) sum += (u64)(c[t] + 1u) * pw;
            pw *= p64;
        }
        sum = det_wave_sum64(sum);
        if (lane == 0) {
            kept[r] = kl;
            hashes[r] = (long long)det_hash_finish(sum, kl);
        }
        nkept += kl > 0;
    }
    if (lane == 0) {
        if (nkept) atomicAdd(&counters[DET_KEPT], (u64)nkept);
        if (nlong) atomicAdd(&counters[DET_OVERLONG], (u64)nlong);
    }
}

__device__ __forceinline__ bool det_same(const uint8_t *bytes, const FastqRecord *recs, const int32_t *kept, long long a,
                                         long long b) {
    const int len = kept[a];
    if (len != kept[b]) return false;
    const uint8_t *pa = bytes + recs[a].seq_off, *pb = bytes + recs[b].seq_off;
    for (int j = 0; j < len; ++j)
        if (pa[j] != pb[j]) return false;
    return true;
}

__global__ __launch_bounds__(256) void det_mark_kernel(const uint8_t *__restrict__ bytes, const FastqRecord *__restrict__ recs,
                                                       const int32_t *__restrict__ kept, const long long *__restrict__ order,
                                                       const long long *__restrict__ head, long long m,
                                                       uint8_t *__restrict__ rep, u64 *counters) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool is_rep = false;
    if (i < m) {
        const long long hd = head[i], r = order[i];
        is_rep = true;
        if (hd != i) {
            if (det_same(bytes, recs, kept, r, order[hd])) is_rep = false;
            else
                for (long long j = hd + 1; j < i; ++j)
                    if (det_same(bytes, recs, kept, r, order[j])) { is_rep = false; break; }
        }
        rep[i] = is_rep ? 1 : 0;
    }
    const u64 b = __ballot(is_rep);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counters[DET_DISTINCT], (u64)__popcll(b));
}

__global__ __launch_bounds__(256) void det_match_kernel(DetDev D, const uint8_t *__restrict__ bytes,
                                                        const FastqRecord *__restrict__ recs, const int32_t *__restrict__ kept,
                                                        const long long *__restrict__ order, const uint8_t *__restrict__ rep,
                                                        long long m, u64 *counters) {
    extern __shared__ __attribute__((aligned(16))) uint8_t det_lds[];
    const int S = D.nseq, W = D.words, stride = 2 * W + 1;
    uint32_t *bloom = (uint32_t *)det_lds;
    u64 *a_matches = (u64 *)(bloom + DET_BLOOM_WORDS);
    uint32_t *a_hits = (uint32_t *)(a_matches + S), *a_max = a_hits + S, *a_ab = a_max + S;
    uint32_t *all_bits = a_ab + S;
    uint8_t *enc = (uint8_t *)(all_bits + (size_t)4 * S * stride);
    uint8_t *all_codes = enc + 256;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *bits = all_bits + (size_t)wave * S * stride;
    uint8_t *codes = all_codes + wave * DET_STAGE;
    for (int i = threadIdx.x; i < DET_BLOOM_WORDS; i += 256) bloom[i] = D.bloom[i];
    for (int i = threadIdx.x; i < S; i += 256) { a_matches[i] = 0; a_hits[i] = 0; a_max[i] = 0; a_ab[i] = 0; }
    enc[threadIdx.x] = D.enc[threadIdx.x];
    __syncthreads();
    unsigned ninvalid = 0;
    for (long long i = (long long)blockIdx.x * 4 + wave; i < m; i += (long long)gridDim.x * 4) {
        if (!rep[i]) continue;
        const long long r = order[i];
        const int kl = kept[r];
        const uint8_t *seq = bytes + recs[r].seq_off;
        bool bad = false;
        for (int j = lane; j < kl && j < DET_MAX_READ; j += 64) {
            const uint8_t c = seq[j];
            codes[j] = enc[c];
            bad |= !D.comp_ok[c];
        }
        if (__any(bad)) { ++ninvalid; continue; }                      // no reverse complement: the caller raises
        for (int w = lane; w < S * stride; w += 64) bits[w] = 0;
        det_wave_sync();
        for (int j = lane; j + D.k <= kl; j += 64) {
            u64 key = 0;
            bool ok = true;
            for (int q = 0; q < D.k; ++q) {
                const uint8_t code = codes[j + q];
                ok &= code != DET_OTHER;
                key = (key << D.bits) | code;
            }
            if (!ok) continue;
            const u64 h = det_mix(key);
            const uint32_t bit = det_bloom_bit(h);
            if (!((bloom[bit >> 5] >> (bit & 31)) & 1u)) continue;
            const uint32_t v = det_lookup((const uint64_t *)D.keys, D.vals, D.mask, key, h);
            if (v == DET_EMPTY) continue;
            const uint32_t first = v >> 12, count = v & 4095u;
            for (uint32_t e = 0; e < count; ++e) {
                const uint32_t p = D.postings[first + e];
                const int s = p & 4095u, strand = (p >> 12) & 1u, kidx = (p >> 13) & 255u;
                atomicOr(&bits[s * stride + strand * W + (kidx >> 5)], 1u << (kidx & 31));
                if (kidx == 0 && strand == 0) {                        // the known sequence may start here
                    const int off = (int)D.seq_off[s], L = (int)D.seq_off[s + 1] - off;
                    bool same = j + L <= kl;
                    for (int x = 0; same && x < L; ++x) same = seq[j + x] == D.seq_bytes[off + x];
                    if (same) atomicOr(&bits[s * stride + 2 * W], 1u);
                }
            }
        }
        det_wave_sync();
        for (int s = lane; s < S; s += 64) {
            const uint32_t *b = bits + s * stride;
            int fw = 0, rv = 0;
            for (int w = 0; w < W; ++w) { fw += __popc(b[w]); rv += __popc(b[W + w]); }
            const uint32_t nn = (uint32_t)(fw >= rv ? fw : rv);
            if (nn) atomicAdd(&a_matches[s], (u64)nn);
            if (nn >= D.thr[s]) { atomicAdd(&a_hits[s], 1u); atomicMax(&a_max[s], nn); }
            if (b[2 * W]) atomicAdd(&a_ab[s], 1u);
        }
        det_wave_sync();
    }
    if (lane == 0 && ninvalid) atomicAdd(&counters[DET_INVALID], (u64)ninvalid);
    __syncthreads();
    u64 *g = counters + DET_HDR;
    for (int s = threadIdx.x; s < S; s += 256) {
        if (a_matches[s]) atomicAdd(&g[s], a_matches[s]);
        if (a_hits[s]) atomicAdd(&g[S + s], (u64)a_hits[s]);
        if (a_max[s]) atomicMax(&g[2 * S + s], (u64)a_max[s]);
        if (a_ab[s]) atomicAdd(&g[3 * S + s], (u64)a_ab[s]);
    }
}

}  // namespace atr

using namespace atr;

static inline unsigned det_grid(long long waves) {
    return (unsigned)std::max<long long>(1, std::min<long long>((waves + 3) / 4, 4096));
}

extern "C" {

int atr_detect_create(const uint8_t *seqs, const int32_t *lens, int nseq, int kmer_size, const uint8_t *past_end_bases,
                      int n_past_end, const int32_t *thresholds, const double *complexity, int max_len, void **out) {
    if (!out) return ATR_ERR_INVALID;
    *out = nullptr;
    DetectHandle *h = new (std::nothrow) DetectHandle();
    if (!h) return ATR_ERR_NOMEM;
    int rc = det_build(h->T, seqs, lens, nseq, kmer_size, past_end_bases, n_past_end, thresholds, complexity, max_len);
    if (rc) { delete h; return rc; }
    const DetectTables &T = h->T;
    h->lds = det_lds_bytes(nseq, T.words);
    // one allocation, every table 16-byte aligned
    struct Part { const void *src; size_t bytes; size_t off; };
    Part parts[] = {{T.keys.data(), T.keys.size() * 8, 0},         {T.complexity.data(), T.complexity.size() * 8, 0},
                    {T.vals.data(), T.vals.size() * 4, 0},         {T.postings.data(), T.postings.size() * 4, 0},
                    {T.bloom.data(), T.bloom.size() * 4, 0},       {T.thresholds.data(), T.thresholds.size() * 4, 0},
                    {T.seq_off.data(), T.seq_off.size() * 4, 0},   {T.seq_bytes.data(), T.seq_bytes.size(), 0},
                    {T.enc, 256, 0},                               {T.comp_ok, 256, 0}};
    size_t total = 0;
    for (Part &p : parts) { p.off = total; total += (p.bytes + 15) / 16 * 16; }
    hipError_t e = hipMalloc(&h->blob, std::max<size_t>(total, 16));
    if (e != hipSuccess) { delete h; return e == hipErrorOutOfMemory ? ATR_ERR_NOMEM : hip_fail(e, "atr_detect_create"); }
    for (const Part &p : parts) {
        if (!p.bytes) continue;
        e = hipMemcpy((uint8_t *)h->blob + p.off, p.src, p.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(h->blob); delete h; return hip_fail(e, "atr_detect_create"); }
    }
    const uint8_t *b = (const uint8_t *)h->blob;
    DetDev &D = h->D;
    D.keys = (const u64 *)(b + parts[0].off); D.cx = (const double *)(b + parts[1].off);
    D.vals = (const uint32_t *)(b + parts[2].off); D.postings = (const uint32_t *)(b + parts[3].off);
    D.bloom = (const uint32_t *)(b + parts[4].off); D.thr = (const uint32_t *)(b + parts[5].off);
    D.seq_off = (const uint32_t *)(b + parts[6].off); D.seq_bytes = b + parts[7].off;
    D.enc = b + parts[8].off; D.comp_ok = b + parts[9].off;
    D.nseq = T.nseq; D.k = T.kmer_size; D.bits = T.bits; D.words = T.words; D.min_k = T.min_k; D.npast = T.npast;
    D.max_len = T.max_len; D.mask = T.mask;
    for (int i = 0; i < DET_MAX_PAST_END; ++i) D.past[i] = T.past[i];
    *out = h;
    return ATR_OK;
}

void atr_detect_destroy(void *handle) {
    DetectHandle *h = (DetectHandle *)handle;
    if (!h) return;
    if (h->blob) (void)hipFree(h->blob);
    delete h;
}

int64_t atr_detect_counter_bytes(const void *handle) {
    const DetectHandle *h = (const DetectHandle *)handle;
    return h ? (int64_t)(DET_HDR + 4 * (int64_t)h->T.nseq) * 8 : ATR_ERR_INVALID;
}

int atr_detect_clear(const void *handle, void *d_counters, void *stream) {
    if (!handle || !d_counters) return ATR_ERR_INVALID;
    hipError_t e = hipMemsetAsync(d_counters, 0, (size_t)atr_detect_counter_bytes(handle), (hipStream_t)stream);
    return e == hipSuccess ? ATR_OK : hip_fail(e, "atr_detect_clear");
}

int atr_detect_filter_batch(const void *handle, const uint8_t *d_bytes, const atr_fastq_record *d_records, int64_t n,
                            int longest, int32_t *d_kept, int64_t *d_hashes, void *d_counters, void *stream) {
    const DetectHandle *h = (const DetectHandle *)handle;
    if (!h || n < 0 || longest < 0) return ATR_ERR_INVALID;
    if (longest > h->T.max_len) return ATR_ERR_UNSUPPORTED;
    if (n == 0) return ATR_OK;
    if (!d_bytes || !d_records || !d_kept || !d_hashes || !d_counters) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(det_filter_kernel, dim3(det_grid(n)), dim3(256), 0, (hipStream_t)stream, h->D, d_bytes,
                       (const FastqRecord *)d_records, (long long)n, d_kept, (long long *)d_hashes, (u64 *)d_counters);
    return launched("atr_detect_filter_batch launch");
}

int atr_detect_mark_batch(const void *handle, const uint8_t *d_bytes, const atr_fastq_record *d_records,
                          const int32_t *d_kept, const int64_t *d_order, const int64_t *d_head, int64_t m, uint8_t *d_rep,
                          void *d_counters, void *stream) {
    if (!handle || m < 0) return ATR_ERR_INVALID;
    if (m == 0) return ATR_OK;
    if (!d_bytes || !d_records || !d_kept || !d_order || !d_head || !d_rep || !d_counters) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(det_mark_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_bytes,
                       (const FastqRecord *)d_records, d_kept, (const long long *)d_order, (const long long *)d_head,
                       (long long)m, d_rep, (u64 *)d_counters);
    return launched("atr_detect_mark_batch launch");
}

int atr_detect_batch(const void *handle, const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_kept,
                     const int64_t *d_order, const uint8_t *d_rep, int64_t m, void *d_counters, void *stream) {
    const DetectHandle *h = (const DetectHandle *)handle;
    if (!h || m < 0) return ATR_ERR_INVALID;
    if (h->T.nseq == 0) return ATR_ERR_UNSUPPORTED;                    // a detector without known sequences: no match pass
    if (m == 0) return ATR_OK;
    if (!d_bytes || !d_records || !d_kept || !d_order || !d_rep || !d_counters) return ATR_ERR_INVALID;
    hipLaunchKernelGGL(det_match_kernel, dim3(det_grid(m)), dim3(256), h->lds, (hipStream_t)stream, h->D, d_bytes,
                       (const FastqRecord *)d_records, d_kept, (const long long *)d_order, d_rep, (long long)m,
                       (u64 *)d_counters);
    return launched("atr_detect_batch launch");
}

int atr_detect_read(const void *handle, const void *d_counters, uint64_t *out, void *stream) {
    if (!handle || !d_counters || !out) return ATR_ERR_INVALID;
    hipError_t e = hipMemcpyAsync(out, d_counters, (size_t)atr_detect_counter_bytes(handle), hipMemcpyDeviceToHost,
                                  (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? ATR_OK : hip_fail(e, "atr_detect_read");
}

}  // extern "C"

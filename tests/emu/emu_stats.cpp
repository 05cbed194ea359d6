// TEST INFRASTRUCTURE: CPU twin of atropos_amd/csrc/stats_kernels.hip (atr_read_stats_*), over the product's block
// layout and rounding (stats_core.hpp) with -DATR_HOST_EMU.  One loop iteration of emu_read_stats_batch = one read,
// counted as stats_scalar_kernel and stats_position_kernel count it together; the counters are sums and maxima, so
// the order does not matter.
// NOTE: unlike the other twins this one RESTATES the per-read counting of stats_kernels.hip (the kernels have no
// per-lane header to compile here); only the layout and the rounding are shared code.  What pins it: the plain Python
// model of tests/_stats_kernels_common.py (which shares neither), block for block -- tests/test_stats_kernels_host.py
// compares this twin with it on the CPU, tests/test_gpu_stats_kernels.py the kernels, case for case the same.  A
// change to what the kernels count fails the second; the same change made here fails the first.
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "emu_abi.hpp"
#define ATR_HD static inline
#include "fastq_core.hpp"
#include "stats_core.hpp"

using namespace atr;

typedef unsigned long long u64;

static int st_check_len(int max_len) {
    if (max_len < 1) return ATR_ERR_INVALID;
    if (max_len > ATR_MAX_LONG_READ_LEN) return ATR_ERR_UNSUPPORTED;
    return ATR_OK;
}

extern "C" {

int64_t emu_read_stats_bytes(int max_len) {
    const int rc = st_check_len(max_len);
    return rc ? rc : (int64_t)st_words(max_len) * 8;
}
EMU_TWIN(read_stats_bytes);

int emu_read_stats_clear(void *stats, int max_len, void *) {
    const int rc = st_check_len(max_len);
    if (rc) return rc;
    if (!stats) return ATR_ERR_INVALID;
    memset(stats, 0, (size_t)st_words(max_len) * 8);
    return ATR_OK;
}
EMU_TWIN(read_stats_clear);

int emu_read_stats_batch(void *stats, int max_len, int longest, int quality_base, const uint8_t *bytes,
                         const atr_fastq_record *records, const int32_t *begin, const int32_t *end, const int32_t *ubegin,
                         const int32_t *uend, const uint8_t *dest, int which, int64_t n, int64_t index_base, void *) {
    const int rc = st_check_len(max_len);
    if (rc) return rc;
    if (!stats || n < 0 || index_base < 0 || longest < 0 || longest > max_len || quality_base < 0 || quality_base > 255)
        return ATR_ERR_INVALID;
    if ((begin == nullptr) != (end == nullptr) || (ubegin == nullptr) != (uend == nullptr) || (ubegin && !begin))
        return ATR_ERR_INVALID;
    if (n == 0) return ATR_OK;
    if (!bytes || !records) return ATR_ERR_INVALID;
    u64 *st = (u64 *)stats;
    const int L = max_len;
    u64 *first = st + st_first_off(L);
    for (int64_t r = 0; r < n; ++r) {
        if (dest && dest[r] != which) continue;
        const FastqRecord &rec = *(const FastqRecord *)&records[r];
        const int a = begin ? begin[r] : 0;
        const int b = end ? std::max(a, end[r]) : (int)rec.seq_len;
        const int len = b - a;
        const int ub = ubegin ? ubegin[r] : INT_MIN, ue = ubegin ? uend[r] : INT_MAX;
        const bool hasq = rec.qual_len > 0;
        if (len > longest) { st[ST_SKIPPED] += 1; continue; }
        const u64 tag = ~((u64)index_base + (u64)r);
        st[ST_COUNT] += 1;
        st[st_len_off(L) + len] += 1;
        first[len] = std::max(first[len], tag);
        if (len == 0) continue;
        int gc = 0, qs = 0;
        for (int p = 0; p < len; ++p) {
            const int pos = a + p;
            const uint8_t c = (pos >= ub && pos < ue) ? bytes[(size_t)rec.seq_off + pos] : (uint8_t)'N';
            gc += (c == 'C') | (c == 'G');
            st[st_seq_off(L) + (long long)p * 256 + c] += 1;
            if (hasq) {
                const uint8_t q = bytes[(size_t)rec.qual_off + pos];
                qs += q;
                st[st_qual_off(L) + (long long)p * 256 + q] += 1;
            }
        }
        const int gb = st_div_round_even(100 * gc, len);
        st[st_gc_off(L) + gb] += 1;
        first[L + 1 + gb] = std::max(first[L + 1 + gb], tag);
        st[ST_LONGEST] = std::max(st[ST_LONGEST], (u64)len);
        if (hasq) {
            st[ST_WITHQ] += 1;
            const int mb = st_div_round_even(qs - quality_base * len, len) + quality_base;
            st[st_mq_off(L) + mb] += 1;
            first[L + 1 + ST_GC_BINS + mb] = std::max(first[L + 1 + ST_GC_BINS + mb], tag);
        }
    }
    return ATR_OK;
}
EMU_TWIN(read_stats_batch);

int emu_read_stats_merge(void *d_dst, int dst_L, const void *d_src, int src_L, int64_t index_offset, void *) {
    int rc = st_check_len(dst_L);
    if (!rc) rc = st_check_len(src_L);
    if (rc) return rc;
    if (!d_dst || !d_src || src_L > dst_L || index_offset < 0) return ATR_ERR_INVALID;
    u64 *dst = (u64 *)d_dst;
    const u64 *src = (const u64 *)d_src;
    const u64 offset = (u64)index_offset;
    for (long long i = 0; i < st_words(src_L); ++i) {
        const u64 v = src[i];
        if (!v) continue;
        long long j;
        if (i < ST_HDR) {
            if (i == ST_LONGEST) { dst[i] = std::max(dst[i], v); continue; }
            j = i;
        } else if (i < st_gc_off(src_L)) j = i;
        else if (i < st_seq_off(src_L)) j = i - st_gc_off(src_L) + st_gc_off(dst_L);
        else if (i < st_qual_off(src_L)) j = i - st_seq_off(src_L) + st_seq_off(dst_L);
        else if (i < st_first_off(src_L)) j = i - st_qual_off(src_L) + st_qual_off(dst_L);
        else {
            const long long k = i - st_first_off(src_L);
            j = k <= src_L ? st_first_off(dst_L) + k : k - (src_L + 1) + st_first_off(dst_L) + dst_L + 1;
            dst[j] = std::max(dst[j], v - offset);
            continue;
        }
        dst[j] += v;
    }
    return ATR_OK;
}
EMU_TWIN(read_stats_merge);

}  // extern "C"

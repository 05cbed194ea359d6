// TEST INFRASTRUCTURE: CPU twin of detect_kernels.hip, built from the product's detect_core.hpp with
// -DATR_HOST_EMU (tables, look-up, hash, complexity decision, the past-end cut on position masks).  The three passes
// walk the reads one after the other; what the kernels spread over lanes (ballots, wave sums, LDS bit sets) is a
// plain loop here.  A harness for the CPU tier, not parity evidence for the kernels.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "emu_abi.hpp"
#include "detect_core.hpp"
#include "fastq_core.hpp"

using namespace atr;

extern "C" {

int emu_detect_create(const uint8_t *seqs, const int32_t *lens, int nseq, int kmer_size, const uint8_t *past, int npast,
                      const int32_t *thresholds, const double *complexity, int max_len, void **out) {
    if (!out) return -1;
    *out = nullptr;
    DetectTables *T = new DetectTables();
    const int rc = det_build(*T, seqs, lens, nseq, kmer_size, past, npast, thresholds, complexity, max_len);
    if (rc) { delete T; return rc; }
    *out = T;
    return 0;
}
EMU_TWIN(detect_create);

void emu_detect_destroy(void *h) { delete (DetectTables *)h; }
EMU_TWIN(detect_destroy);

int64_t emu_detect_counter_bytes(const void *h) { return 8 * (DET_HDR + 4 * (int64_t)((const DetectTables *)h)->nseq); }
EMU_TWIN(detect_counter_bytes);

int emu_detect_clear(const void *h, void *counters, void *) {
    memset(counters, 0, (size_t)emu_detect_counter_bytes(h));
    return 0;
}
EMU_TWIN(detect_clear);

int emu_detect_read(const void *h, const void *counters, uint64_t *out, void *) {
    memcpy(out, counters, (size_t)emu_detect_counter_bytes(h));
    return 0;
}
EMU_TWIN(detect_read);

// test hook, != 0: every read gets the same hash (the distinct pass must still be exact)
int emu_detect_force_hash = 0;

int emu_detect_filter_batch(const void *h, const uint8_t *bytes, const atr_fastq_record *records, int64_t n, int longest,
                            int32_t *kept, int64_t *hashes, void *d_counters, void *) {
    const FastqRecord *recs = (const FastqRecord *)records;
    uint64_t *counters = (uint64_t *)d_counters;
    const int force_hash = emu_detect_force_hash;
    const DetectTables &T = *(const DetectTables *)h;
    if (n < 0 || longest < 0) return -1;
    if (longest > T.max_len) return -2;
    for (int64_t r = 0; r < n; ++r) {
        const int len = (int)recs[r].seq_len;
        const uint8_t *seq = bytes + recs[r].seq_off;
        if (len > T.max_len) { kept[r] = 0; hashes[r] = 0; ++counters[DET_OVERLONG]; continue; }
        int cnt[4] = {0, 0, 0, 0};
        uint64_t valid[DET_CHUNKS] = {0}, m[DET_MAX_PAST_END][DET_CHUNKS] = {{0}};
        for (int j = 0; j < len; ++j) {
            const uint8_t u = det_upper(seq[j]);
            cnt[0] += u == 'A'; cnt[1] += u == 'C'; cnt[2] += u == 'G'; cnt[3] += u == 'T';
            valid[j >> 6] |= 1ull << (j & 63);
            for (int p = 0; p < T.npast; ++p)
                if (seq[j] == T.past[p]) m[p][j >> 6] |= 1ull << (j & 63);
        }
        int cut = len;
        for (int p = 0; p < T.npast; ++p) {
            const int c = det_past_end_cut(m[p], valid, len);
            if (c < cut) cut = c;
        }
        const int kl = det_low_complexity(T.complexity.data(), T.max_len + 1, len, cnt[0], cnt[1], cnt[2], cnt[3])
                           ? 0 : det_kept_len(len, cut, T.kmer_size, T.min_k);
        uint64_t sum = 0;
        for (int j = 0; j < kl; ++j) sum += (uint64_t)(seq[j] + 1u) * det_pow((uint32_t)j);
        kept[r] = kl;
        hashes[r] = force_hash ? 42 : (int64_t)det_hash_finish(sum, kl);
        counters[DET_KEPT] += kl > 0;
    }
    return 0;
}
EMU_TWIN(detect_filter_batch);

static bool same(const uint8_t *bytes, const FastqRecord *recs, const int32_t *kept, int64_t a, int64_t b) {
    return kept[a] == kept[b] && memcmp(bytes + recs[a].seq_off, bytes + recs[b].seq_off, (size_t)kept[a]) == 0;
}

int emu_detect_mark_batch(const void *, const uint8_t *bytes, const atr_fastq_record *records, const int32_t *kept,
                          const int64_t *order, const int64_t *head, int64_t m, uint8_t *rep, void *d_counters, void *) {
    const FastqRecord *recs = (const FastqRecord *)records;
    uint64_t *counters = (uint64_t *)d_counters;
    for (int64_t i = 0; i < m; ++i) {
        bool is_rep = true;
        const int64_t hd = head[i], r = order[i];
        if (hd != i) {
            if (same(bytes, recs, kept, r, order[hd])) is_rep = false;
            else
                for (int64_t j = hd + 1; j < i; ++j)
                    if (same(bytes, recs, kept, r, order[j])) { is_rep = false; break; }
        }
        rep[i] = is_rep;
        counters[DET_DISTINCT] += is_rep;
    }
    return 0;
}
EMU_TWIN(detect_mark_batch);

int emu_detect_batch(const void *h, const uint8_t *bytes, const atr_fastq_record *records, const int32_t *kept,
                     const int64_t *order, const uint8_t *rep, int64_t m, void *d_counters, void *) {
    const FastqRecord *recs = (const FastqRecord *)records;
    uint64_t *counters = (uint64_t *)d_counters;
    const DetectTables &T = *(const DetectTables *)h;
    const int S = T.nseq, W = T.words, stride = 2 * W + 1;
    std::vector<uint32_t> bits((size_t)S * stride);
    std::vector<uint8_t> codes(DET_MAX_READ);
    uint64_t *g = counters + DET_HDR;
    for (int64_t i = 0; i < m; ++i) {
        if (!rep[i]) continue;
        const int64_t r = order[i];
        const int kl = kept[r];
        const uint8_t *seq = bytes + recs[r].seq_off;
        bool bad = false;
        for (int j = 0; j < kl; ++j) { codes[j] = T.enc[seq[j]]; bad |= !T.comp_ok[seq[j]]; }
        if (bad) { ++counters[DET_INVALID]; continue; }
        std::fill(bits.begin(), bits.end(), 0u);
        for (int j = 0; j + T.kmer_size <= kl; ++j) {
            uint64_t key = 0;
            bool ok = true;
            for (int q = 0; q < T.kmer_size; ++q) { ok &= codes[j + q] != DET_OTHER; key = (key << T.bits) | codes[j + q]; }
            if (!ok) continue;
            const uint64_t hh = det_mix(key);
            const uint32_t bit = det_bloom_bit(hh);
            if (!((T.bloom[bit >> 5] >> (bit & 31)) & 1u)) continue;
            const uint32_t v = det_lookup(T.keys.data(), T.vals.data(), T.mask, key, hh);
            if (v == DET_EMPTY) continue;
            for (uint32_t e = 0; e < (v & 4095u); ++e) {
                const uint32_t p = T.postings[(v >> 12) + e];
                const int s = p & 4095u, strand = (p >> 12) & 1u, kidx = (p >> 13) & 255u;
                bits[s * stride + strand * W + (kidx >> 5)] |= 1u << (kidx & 31);
                if (kidx == 0 && strand == 0) {
                    const int off = (int)T.seq_off[s], L = (int)T.seq_off[s + 1] - off;
                    if (j + L <= kl && memcmp(seq + j, T.seq_bytes.data() + off, (size_t)L) == 0) bits[s * stride + 2 * W] = 1u;
                }
            }
        }
        for (int s = 0; s < S; ++s) {
            const uint32_t *b = bits.data() + s * stride;
            int fw = 0, rv = 0;
            for (int w = 0; w < W; ++w) { fw += __builtin_popcount(b[w]); rv += __builtin_popcount(b[W + w]); }
            const uint32_t nn = (uint32_t)(fw >= rv ? fw : rv);
            g[s] += nn;
            if (nn >= T.thresholds[s]) { g[S + s] += 1; if (nn > g[2 * S + s]) g[2 * S + s] = nn; }
            if (b[2 * W]) g[3 * S + s] += 1;
        }
    }
    return 0;
}
EMU_TWIN(detect_batch);

}  // extern "C"

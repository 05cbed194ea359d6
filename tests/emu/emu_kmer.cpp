// TEST INFRASTRUCTURE: CPU twin of detect_kmer_kernels.hip, built from the product's detect_kmer_core.hpp with
// -DATR_HOST_EMU (layouts, keys, the over-representation test, the support word, the argument checks).  What the
// kernels spread over threads and waves is a plain loop here; the compaction keeps slot order (the kernels do not, and
// nothing may depend on it).  A harness for the CPU tier, not parity evidence for the kernels.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emu_abi.hpp"
#include "detect_kmer_core.hpp"
#include "fastq_core.hpp"

using namespace atr;

extern "C" {

int emu_detect_kmer_slots(const atr_fastq_record *records, const int32_t *kept, const int64_t *reps, const int64_t *start,
                          int64_t nrep, int64_t total, int kmer_size, void *reptab, int32_t *slot_rep, int32_t *level, void *) {
    const int rc = kmer_check_slots(nrep, total, kmer_size);
    if (rc) return rc;
    if (nrep == 0) return 0;
    if (!records || !kept || !reps || !start || !reptab || !level || (total && !slot_rep)) return -1;
    const FastqRecord *recs = (const FastqRecord *)records;
    KmerRep *tab = (KmerRep *)reptab;
    for (int64_t j = 0; j < nrep; ++j) {
        const int64_t r = reps[j];
        int kl = kept[r] < 0 ? 0 : kept[r];
        if (kl > KMER_MAX_READ) kl = KMER_MAX_READ;
        tab[j].start = start[j]; tab[j].off = recs[r].seq_off; tab[j].kept = kl; tab[j].rec = r;
        level[j] = kmer_size;
        for (int o = 0; o < kl; ++o)
            if (start[j] + o < total) slot_rep[start[j] + o] = (int32_t)j;
    }
    return 0;
}
EMU_TWIN(detect_kmer_slots);

int emu_detect_kmer_pair_keys(const void *reptab, const int32_t *slot_rep, int64_t total, const uint8_t *bytes,
                              const int32_t *id_a, int a, const int32_t *id_b, int b, int64_t *keys, void *) {
    if (a < 1 || b < 1) return -1;
    const int rc = kmer_check_len(total, a + b);
    if (rc) return rc;
    if ((a == 1) != (id_a == nullptr) || (b == 1) != (id_b == nullptr)) return -1;
    if (total == 0) return 0;
    if (!reptab || !slot_rep || !bytes || !keys) return -1;
    const KmerRep *tab = (const KmerRep *)reptab;
    for (int64_t p = 0; p < total; ++p) {
        const KmerRep &R = tab[slot_rep[p]];
        const int o = (int)(p - R.start);
        long long key = KMER_NO_KEY;
        if (R.kept - o >= a + b)
            key = kmer_pair_key(id_a ? id_a[p] : (int32_t)bytes[(size_t)R.off + o],
                                id_b ? id_b[p + a] : (int32_t)bytes[(size_t)R.off + o + a]);
        keys[p] = key;
    }
    return 0;
}
EMU_TWIN(detect_kmer_pair_keys);

size_t emu_detect_kmer_rank_work_bytes(int64_t n) { return (n < 0 || n > KMER_MAX_SLOTS) ? 0 : 16; }
EMU_TWIN(detect_kmer_rank_work_bytes);

int emu_detect_kmer_rank(const int64_t *keys, const int64_t *idx, const int32_t *list, int64_t n, int32_t *cls, int32_t *begin,
                         int32_t *end, int32_t *head, int64_t *nclasses, void *work, size_t work_bytes, void *) {
    if (n < 0 || !nclasses) return -1;
    if (n > KMER_MAX_SLOTS) return -2;
    if (n && (!keys || !idx || !cls || !begin || !end || !head || !work || work_bytes < emu_detect_kmer_rank_work_bytes(n))) return -1;
    int32_t rank = -1;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t slot = list ? list[idx[i]] : (int32_t)idx[i];
        if (keys[i] == KMER_NO_KEY) { cls[slot] = KMER_NO_CLASS; continue; }
        if (i == 0 || keys[i - 1] != keys[i]) { ++rank; begin[rank] = (int32_t)i; head[rank] = slot; }
        if (slot < head[rank]) head[rank] = slot;
        cls[slot] = rank;
        end[rank] = (int32_t)(i + 1);
    }
    *nclasses = rank + 1;
    return 0;
}
EMU_TWIN(detect_kmer_rank);

int emu_detect_kmer_level(const void *reptab, const int32_t *slot_rep, const int32_t *list, int64_t n, const int32_t *cls,
                          const int32_t *cls_prev, const int32_t *begin, const int32_t *end, const int32_t *head,
                          int32_t *cand_of, const int32_t *cand_of_prev, int k, int64_t min_count, int32_t *level, int32_t *cand,
                          int64_t capacity, int64_t *state, void *) {
    const int rc = kmer_check_level(n, k, capacity);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!reptab || !slot_rep || !cls || !begin || !end || !head || !cand_of || !level || !state || (capacity && !cand) ||
        ((cls_prev == nullptr) != (cand_of_prev == nullptr)))
        return -1;
    const KmerRep *tab = (const KmerRep *)reptab;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t slot = list ? list[i] : (int32_t)i;
        const int32_t c = cls[slot];
        if (c < 0) continue;
        const int32_t rep = slot_rep[slot];
        const KmerRep &R = tab[rep];
        const int o = (int)(slot - R.start);
        const long long count = (long long)end[c] - begin[c];
        const bool over = kmer_over(count, min_count);
        if (head[c] == slot) {
            int32_t row = -1;
            if (over) {
                const int64_t at = state[KMER_S_CANDIDATES]++;
                ++state[KMER_S_OVER + k];
                if (at < capacity) {
                    row = (int32_t)at;
                    int32_t *w = cand + (size_t)at * KMER_C_WORDS;
                    w[KMER_C_LEVEL] = k; w[KMER_C_COUNT] = (int32_t)count; w[KMER_C_REP] = rep; w[KMER_C_OFFSET] = o;
                    w[KMER_C_QUIRK] = 0;
                }
            }
            cand_of[c] = row;
        }
        if (!over) continue;
        level[rep] = k + 1;
    }
    // (the quirk reads cand_of_prev, which the previous call completed; a second loop keeps the rows' own writes first)
    for (int64_t i = 0; i < n && cls_prev; ++i) {
        const int32_t slot = list ? list[i] : (int32_t)i;
        const int32_t c = cls[slot];
        if (c < 0 || !kmer_over((long long)end[c] - begin[c], min_count)) continue;
        const KmerRep &R = tab[slot_rep[slot]];
        if (slot != R.start || R.kept != k) continue;
        for (int d = 0; d < 2; ++d) {
            const int32_t cp = cls_prev[slot + d];
            const int32_t row = cp >= 0 ? cand_of_prev[cp] : -1;
            if (row >= 0 && row < capacity) cand[(size_t)row * KMER_C_WORDS + KMER_C_QUIRK] = 1;
        }
    }
    return 0;
}
EMU_TWIN(detect_kmer_level);

int emu_detect_kmer_next(const void *reptab, const int32_t *slot_rep, const int32_t *list, int64_t n, const int32_t *cls,
                         const uint8_t *bytes, const int32_t *level, int k, int32_t *list_next, int64_t *keys_next,
                         int64_t *state, void *) {
    const int rc = kmer_check_level(n, k, 0);
    if (rc) return rc;
    if (!state) return -1;
    state[KMER_S_SURVIVORS] = 0;
    if (n == 0) return 0;
    if (!reptab || !slot_rep || !cls || !bytes || !level || !list_next || !keys_next) return -1;
    const KmerRep *tab = (const KmerRep *)reptab;
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t slot = list ? list[i] : (int32_t)i;
        const int32_t c = cls[slot], rep = slot_rep[slot];
        const KmerRep &R = tab[rep];
        const int o = (int)(slot - R.start);
        if (c < 0 || level[rep] != k + 1 || R.kept - o < k + 1) continue;
        list_next[at] = slot;
        keys_next[at] = kmer_level_key(c, bytes[(size_t)R.off + o + k]);
        ++at;
    }
    state[KMER_S_SURVIVORS] = at;
    return 0;
}
EMU_TWIN(detect_kmer_next);

int emu_detect_kmer_gather(const void *reptab, int64_t nrep, const uint8_t *bytes, const int32_t *cand, const int64_t *text_off,
                           int64_t ncand, uint8_t *out, void *) {
    if (ncand < 0 || nrep < 0) return -1;
    if (ncand > KMER_MAX_CANDIDATES) return -2;
    if (ncand == 0) return 0;
    if (!reptab || !bytes || !cand || !text_off || !out) return -1;
    const KmerRep *tab = (const KmerRep *)reptab;
    for (int64_t c = 0; c < ncand; ++c) {
        const int32_t *w = cand + (size_t)c * KMER_C_WORDS;
        const int32_t rep = w[KMER_C_REP], o = w[KMER_C_OFFSET];
        const int64_t at = text_off[c], len = text_off[c + 1] - at;
        if (rep < 0 || rep >= nrep || o < 0) continue;
        for (int j = 0; j < len && o + j < tab[rep].kept; ++j) out[at + j] = bytes[(size_t)tab[rep].off + o + j];
    }
    return 0;
}
EMU_TWIN(detect_kmer_gather);

int emu_detect_kmer_support(const void *reptab, int64_t nrep, const uint8_t *bytes, const int32_t *level, const uint8_t *patterns,
                            const int32_t *pat_len, int npat, int64_t *abundance, uint64_t *longest, void *) {
    const int rc = kmer_check_support(nrep, npat);
    if (rc) return rc;
    if (npat == 0) return 0;
    if (!patterns || !pat_len || !abundance || !longest) return -1;
    for (int p = 0; p < npat; ++p) { abundance[p] = 0; longest[p] = ~0ull; }
    if (nrep == 0) return 0;
    if (!reptab || !bytes || !level) return -1;
    const KmerRep *tab = (const KmerRep *)reptab;
    for (int64_t j = 0; j < nrep; ++j) {
        const KmerRep &R = tab[j];
        const uint8_t *text = bytes + R.off;
        for (int p = 0; p < npat; ++p) {
            const int L = pat_len[p];
            if (L < 1 || L > KMER_MAX_READ || L > R.kept) continue;
            for (int o = 0; o + L <= R.kept; ++o) {
                if (!kmer_same(text + o, patterns + (size_t)p * KMER_MAX_READ, L)) continue;
                ++abundance[p];
                const unsigned long long w = kmer_support_word(o, R.rec);
                if (level[j] >= L && w < longest[p]) longest[p] = w;
                break;
            }
        }
    }
    return 0;
}
EMU_TWIN(detect_kmer_support);

}  // extern "C"

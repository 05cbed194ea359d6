// TEST INFRASTRUCTURE: CPU twin of report_kernels.hip, built from the product's report_core.hpp with -DATR_HOST_EMU
// (the layout of the counter block, what a trimmer stage counts, the bin of a match).  The three passes walk the reads
// one after the other; what the kernels do with wave sums and a table in LDS is a plain loop here -- the LDS variant
// counts into a table of the round's length and rebases it, as the kernel's flush does.  A harness for the CPU tier,
// not parity evidence for the kernels.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emu_abi.hpp"
#include "fastq_core.hpp"
#include "report_core.hpp"

using namespace atr;

extern "C" {

int emu_report_create(int n_adapters, int max_read_len, int max_errors, void **out) {
    if (!out) return -1;
    *out = nullptr;
    const RepLayout L = {n_adapters, max_read_len, max_errors};
    const int rc = rep_layout_check(L);
    if (rc) return rc;
    *out = new RepLayout(L);
    return 0;
}
EMU_TWIN(report_create);

void emu_report_destroy(void *h) { delete (RepLayout *)h; }
EMU_TWIN(report_destroy);

int64_t emu_report_counters(const void *h) { return h ? rep_words(*(const RepLayout *)h) : -1; }
EMU_TWIN(report_counters);

int emu_report_read(const void *h, const void *counters, int64_t *out, void *) {
    if (!h) return -1;
    memcpy(out, counters, 8 * (size_t)emu_report_counters(h));
    return 0;
}
EMU_TWIN(report_read);

int emu_report_intervals(const void *h, const atr_fastq_record *records, const int32_t *b0, const int32_t *e0, const int32_t *b1,
                         const int32_t *e1, int64_t n, int mode, int front, int back, int slot, void *d_counters, void *) {
    const FastqRecord *recs = (const FastqRecord *)records;
    int64_t *counters = (int64_t *)d_counters;
    if (!h || n < 0 || mode < REP_SUBSEQ || mode > REP_NEND || front < 0 || back < 0 || slot < 0 || slot >= REP_SLOTS) return -1;
    for (int64_t i = 0; i < n; ++i)
        counters[REP_TRIM + slot] += rep_trimmed_bases(mode, b0[i], e0[i], b1[i], e1[i], front, back, (int)recs[i].seq_len);
    return 0;
}
EMU_TWIN(report_intervals);

int emu_report_adapters(const void *h, const uint8_t *bytes, const atr_fastq_record *records, const uint8_t *took,
                        const int16_t *best, const int64_t *which, const uint8_t *front, int default_front,
                        const int32_t *begin, const int32_t *end, int64_t n, int longest, int weight, int variant,
                        void *d_counters, void *) {
    const FastqRecord *recs = (const FastqRecord *)records;
    int64_t *counters = (int64_t *)d_counters;
    if (!h || n < 0 || longest < 0 || weight < 1 || weight > 2 || variant < 0 || variant > 2) return -1;
    const RepLayout G = *(const RepLayout *)h;
    if (longest > G.max_len) return -2;
    RepLayout S = G;
    S.max_len = longest;
    const bool fits = S.nadapters * rep_adapter_words(S) <= REP_LDS_WORDS;
    if (variant == ATR_REPORT_LDS && !fits) return -2;
    const bool in_lds = variant == ATR_REPORT_LDS || (variant == ATR_REPORT_AUTO && fits);
    if (!in_lds) S = G;
    std::vector<uint32_t> lds(in_lds ? (size_t)(S.nadapters * rep_adapter_words(S)) : 0);
    int64_t *table = counters + REP_HDR;
    for (int64_t i = 0; i < n; ++i) {
        if (!took[i]) continue;
        const int b = begin[i], len = end[i] - b;
        const RepHit hit = rep_adapter_hit(best + i * 8, len, front ? (int)front[i] : default_front, bytes + recs[i].seq_off + b);
        if (!rep_hit_fits(S, hit, which[i])) { ++counters[REP_OVERFLOW]; continue; }
        const int64_t bin = rep_hist_word(S, (int)which[i], hit.back, hit.length, hit.errors);
        const int64_t adj = hit.adj >= 0 ? rep_adj_word(S, (int)which[i], hit.adj) : -1;
        if (in_lds) {
            lds[bin] += weight;
            if (adj >= 0) lds[adj] += weight;
        } else {
            table[bin] += weight;
            if (adj >= 0) table[adj] += weight;
        }
    }
    for (size_t w = 0; w < lds.size(); ++w)
        if (lds[w]) table[rep_rebase_word(S, G, (int64_t)w)] += lds[w];
    return 0;
}
EMU_TWIN(report_adapters);

int emu_report_outputs(const void *h, const atr_fastq_record *records, const int32_t *begin, const int32_t *end,
                       const uint8_t *matched, const uint8_t *dest, int64_t n, void *d_counters, void *) {
    const FastqRecord *recs = (const FastqRecord *)records;
    int64_t *counters = (int64_t *)d_counters;
    if (!h || n < 0) return -1;
    for (int64_t i = 0; i < n; ++i) {
        const int d = dest[i] < REP_DESTS ? dest[i] : REP_DESTS - 1;
        counters[REP_IN_RECORDS] += 1;
        counters[REP_IN_BASES] += recs[i].seq_len;
        counters[REP_WITH_ADAPTERS] += matched[i] != 0;
        counters[REP_DEST + d] += 1;
        counters[REP_DEST_BP + d] += end[i] > begin[i] ? end[i] - begin[i] : 0;
    }
    return 0;
}
EMU_TWIN(report_outputs);

}  // extern "C"

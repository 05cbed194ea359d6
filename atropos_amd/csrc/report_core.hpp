// report_core.hpp -- the trim report's counter block and its per-lane arithmetic: what the reference counts while it
// trims (Trimmer.trimmed_bases, commands/trim/modifiers.py:54-82; Adapter._trimmed_front / _trimmed_back,
// adapters/__init__.py:411-436; the formatters' written / bp counters, io/seqio.py:716-764), shared by the device
// kernels (report_kernels.hip) and the CPU twin of the test-suite (tests/emu/emu_report.cpp, -DATR_HOST_EMU).
//
// The block is int64 words, one block per read of the layout (read 1 / read 2):
//   [REP_IN_RECORDS] [REP_IN_BASES]  records and bases as read
//   [REP_WITH_ADAPTERS]              reads an adapter round matched (AdapterCutter.with_adapters)
//   [REP_OVERFLOW]                   matches outside the table (length, errors or adapter index): the caller raises
//   [REP_DEST + d]  [REP_DEST_BP + d]  records sent to destination d and the bases of their final intervals
//   [REP_TRIM + s]                   trimmed_bases of trimmer slot s
//   from REP_HDR, per adapter: adjacent[8] (A C G T other; three words of padding), then the histogram
//   [front | back][length 0 .. max_len][errors 0 .. max_errors].
// Sums of integers only: the block does not depend on launch shape or order.
#ifndef ATR_REPORT_CORE_HPP
#define ATR_REPORT_CORE_HPP

#include <stdint.h>

#ifdef ATR_HOST_EMU
#define REP_HD static inline
#else
#define REP_HD __host__ __device__ __forceinline__
#endif

namespace atr {

enum { REP_IN_RECORDS = 0, REP_IN_BASES = 1, REP_WITH_ADAPTERS = 2, REP_OVERFLOW = 3, REP_DEST = 8, REP_DEST_BP = 16,
       REP_TRIM = 24, REP_HDR = 32, REP_SLOTS = 8, REP_DESTS = 8, REP_ADJ = 8 };
// how a trimmer stage counts: Trimmer.subseq (what the interval lost), Trimmer.clip with fixed lengths
// (UnconditionalCutter), Trimmer.clip with MinCutter's lengths (what is still missing at either end), NEndTrimmer's
// subseq (a read of nothing but N counts twice)
enum { REP_SUBSEQ = 0, REP_CLIP = 1, REP_MINCUT = 2, REP_NEND = 3 };
enum { REP_MAX_ADAPTERS = 64, REP_MAX_WORDS = 1 << 22, REP_LDS_WORDS = 12288 };   // 32 MiB of counters; 48 KiB of LDS

struct RepLayout {
    int nadapters, max_len, max_errors;
};

REP_HD int64_t rep_adapter_words(const RepLayout &L) { return REP_ADJ + 2 * (int64_t)(L.max_len + 1) * (L.max_errors + 1); }
REP_HD int64_t rep_words(const RepLayout &L) { return REP_HDR + L.nadapters * rep_adapter_words(L); }
// word of an adapter's table, relative to REP_HDR
REP_HD int64_t rep_adj_word(const RepLayout &L, int adapter, int adj) { return adapter * rep_adapter_words(L) + adj; }
REP_HD int64_t rep_hist_word(const RepLayout &L, int adapter, int back, int length, int errors) {
    return adapter * rep_adapter_words(L) + REP_ADJ + ((int64_t)back * (L.max_len + 1) + length) * (L.max_errors + 1) + errors;
}
// the word of layout G that word w of the (shorter) layout S counts into; both relative to REP_HDR
REP_HD int64_t rep_rebase_word(const RepLayout &S, const RepLayout &G, int64_t w) {
    const int64_t per = rep_adapter_words(S);
    const int adapter = (int)(w / per);
    int64_t r = w % per;
    if (r < REP_ADJ) return rep_adj_word(G, adapter, (int)r);
    r -= REP_ADJ;
    const int errors = (int)(r % (S.max_errors + 1));
    r /= S.max_errors + 1;
    return rep_hist_word(G, adapter, (int)(r / (S.max_len + 1)), (int)(r % (S.max_len + 1)), errors);
}

// Bases a trimmer stage adds to trimmed_bases for one read: [b0, e0) before the stage, [b1, e1) after it, `total`
// the read's length in the file.  clip counts the lengths it was ASKED to remove, and nothing for an empty read
// (modifiers.py:77); subseq counts what went (begin + len - end, io/_seqio.pyx:62-73), an empty read loses nothing.
REP_HD int64_t rep_trimmed_bases(int mode, int b0, int e0, int b1, int e1, int front, int back, int total) {
    if (e0 <= b0) return 0;
    if (mode == REP_CLIP) return (int64_t)front + back;
    if (mode == REP_MINCUT) {
        const int f = front - b0, b = back - (total - e0);              // MinCutter.to_trim: what is already gone counts
        return (int64_t)(f > 0 ? f : 0) + (b > 0 ? b : 0);
    }
    const int after = e1 > b1 ? e1 - b1 : 0;
    // NEndTrimmer on a read that is all N: ^N+ ends at len and N+$ starts at 0, subseq(len, 0) counts len + (len - 0)
    if (mode == REP_NEND && after == 0) return 2 * (int64_t)(e0 - b0);
    return (int64_t)(e0 - b0) - after;
}

struct RepHit {
    int back, length, errors, adj;       // adj: 0..3 = A C G T, 4 = anything else or no base; -1 for a 5' match
};

// What Adapter.trimmed counts for one match (record: astart, astop, rstart, rstop, matches, errors) on a read of
// `len` bases whose first base is seq[0].  code: the adapter's side (0 back, 1 front, 2 = Match._guess_is_front:
// front when rstart == 0).  The adjacent base is the byte as it stands in the read: 'a' is not 'A'.
REP_HD RepHit rep_adapter_hit(const int16_t *rec, int len, int code, const uint8_t *seq) {
    RepHit h;
    const int rstart = rec[2], rstop = rec[3];
    const bool front = code == 2 ? rstart == 0 : code == 1;
    h.back = front ? 0 : 1;
    h.errors = rec[5];
    h.adj = -1;
    if (front) {
        h.length = rstop;
    } else {
        h.length = len - rstart;
        const uint8_t c = rstart > 0 && rstart <= len ? seq[rstart - 1] : (uint8_t)0;
        h.adj = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
    }
    return h;
}

REP_HD bool rep_hit_fits(const RepLayout &L, const RepHit &h, long long adapter) {
    return adapter >= 0 && adapter < L.nadapters && h.length >= 0 && h.length <= L.max_len && h.errors >= 0 &&
           h.errors <= L.max_errors;
}

// ATR_OK-style check of a layout: 0 fine, -1 invalid, -2 beyond the table bound
REP_HD int rep_layout_check(const RepLayout &L) {
    if (L.nadapters < 0 || L.max_len < 0 || L.max_errors < 0) return -1;
    if (L.nadapters > REP_MAX_ADAPTERS || L.max_len > (1 << 20) || L.max_errors > (1 << 10)) return -2;
    return rep_words(L) > REP_MAX_WORDS ? -2 : 0;
}

}  // namespace atr
#endif

// pairtext_core.hpp -- per-pair arithmetic of the interleaved FASTQ writer (atr_fastq_emit_pairs).
//
// The reference's InterleavedFormatter (io/seqio.py:740-749) is FastqFormat.format_entry of read 1
// followed by format_entry of read 2, pair after pair, into one file.  A pair here is two record
// descriptors -- in one chunk (an interleaved input) or in two -- with a kept interval and an optional
// unmasked interval each; its text is the two records' texts of fastq_core.hpp back to back.  What a
// record's text is (name2, the mask) is decided there and nowhere else.
//
// Compiled for gfx950 and, with -DATR_HOST_EMU, for the CPU test emulation (tests/emu).
#ifndef ATR_PAIRTEXT_CORE_HPP
#define ATR_PAIRTEXT_CORE_HPP

#include "fastq_core.hpp"

namespace atr {

// One read of a pair as the formatter sees it: its chunk, descriptor, kept interval [a, b) and the part
// [ub, ue) of it the 'mask' action left (a, b: no mask).
struct MateText {
    const uint8_t *bytes;
    FastqRecord rec;
    int a, b, ub, ue;
};

// record r of one mate's arrays; ubegin / uend may be NULL
ATR_DEV MateText mate_text(const uint8_t *bytes, const FastqRecord *records, const int32_t *begin, const int32_t *end,
                           const int32_t *ubegin, const int32_t *uend, long long r) {
    MateText m;
    m.bytes = bytes;
    m.rec = records[r];
    m.a = begin[r];
    m.b = end[r] > m.a ? end[r] : m.a;
    m.ub = ubegin ? ubegin[r] : m.a;
    m.ue = uend ? uend[r] : m.b;
    return m;
}

ATR_DEV uint32_t mate_text_bytes(const MateText &m) { return fastq_record_bytes(m.rec, m.b - m.a); }

// Bytes of a formatted pair: read 1's record, then read 2's
ATR_DEV uint32_t pair_text_bytes(const MateText &m1, const MateText &m2) { return mate_text_bytes(m1) + mate_text_bytes(m2); }

// One read's record of the pair's text at o: `before` bytes into it (0 for read 1, mate_text_bytes(read 1) for
// read 2), written by `nl` cooperating lanes.
ATR_DEV void pair_format_mate(uint8_t *o, const MateText &m, uint32_t before, int lane, int nl) {
    fastq_format_record(o + before, m.bytes, m.rec, m.a, m.b, m.ub, m.ue, lane, nl);
}

// The pair's text at o, pair_text_bytes(m1, m2) bytes, written by `nl` cooperating lanes (the emulation
// passes 0, 1).
ATR_DEV void pair_format(uint8_t *o, const MateText &m1, const MateText &m2, int lane, int nl) {
    pair_format_mate(o, m1, 0u, lane, nl);
    pair_format_mate(o, m2, mate_text_bytes(m1), lane, nl);
}

// A record a wave may format out of a staged copy of the span [lo, hi) of its chunk: it lies inside the
// span in file order (name, bases, qualities), its kept interval lies inside its lines, and its '+' text is
// its own name (a rewritten name sits behind the chunk: flag bit 1).
ATR_DEV bool mate_stageable(const MateText &m, uint32_t lo, uint32_t hi) {
    const FastqRecord &r = m.rec;
    const uint32_t rec_lo = r.name_off - 1u, rec_hi = r.qual_off + r.qual_len;
    return rec_lo >= lo && rec_hi <= hi && rec_hi >= rec_lo && r.name_off >= 1u && r.seq_off >= rec_lo &&
           r.name_off + r.name_len <= r.seq_off && r.seq_off + r.seq_len <= r.qual_off && !(r.flags & 2u) && m.a >= 0 &&
           (uint32_t)m.b <= r.seq_len && (m.b == m.a || (uint32_t)m.b <= r.qual_len);
}

// ---- OverwriteRead (commands/trim/modifiers.py:511-563; op-order letter W) ------------------------------
// 0: the pair stays; 1: read 1 is overwritten with read 2's reverse complement; 2: read 2 with read 1's.
// q1 / q2: the kept qualities.  mean < lowq <=> sum < lowq * window, mean >= highq <=> sum >= highq * window,
// in integers (a window is at most a read long, a quality at most 255: no overflow).
ATR_DEV int overwrite_which(const uint8_t *q1, int len1, const uint8_t *q2, int len2, int base, int lowq, int highq,
                            int window) {
    if (len1 < window || len2 < window) return 0;
    long long s1 = 0, s2 = 0;
    for (int k = 0; k < window; ++k) { s1 += (int)q1[k] - base; s2 += (int)q2[k] - base; }
    const long long lo = (long long)lowq * window, hi = (long long)highq * window;
    if (s1 < lo && s2 >= hi) return 1;
    if (s2 < lo && s1 >= hi) return 2;
    return 0;
}

// Bytes a chunk grows by for the clone of `better`'s kept bases: name + bases + qualities, 16-byte padded
ATR_DEV uint32_t overwrite_clone_bytes(const FastqRecord &better, int kept) {
    return (better.name_len + 2u * (uint32_t)kept + 15u) & ~15u;
}

// The descriptor of a clone written at offset `at` of the overwritten read's chunk: name | bases | qualities
ATR_DEV FastqRecord overwrite_clone_record(const FastqRecord &better, int kept, uint32_t at) {
    FastqRecord r = {at, better.name_len, at + better.name_len, (uint32_t)kept, at + better.name_len + (uint32_t)kept,
                     (uint32_t)kept, better.flags & 1u, 0u};
    return r;
}

// Writes the clone of m (the better read, kept interval [a, b)) at dst: its name, its bases complemented (comp[c],
// 0: no complement) in reverse order, its qualities reversed; `nl` cooperating lanes, each WRITING forward
// (consecutive lanes, consecutive bytes) and reading backward.  Returns false if this lane met a base without a
// complement.
ATR_DEV bool overwrite_clone_write(uint8_t *dst, const MateText &m, const uint8_t *comp, int lane, int nl) {
    const uint32_t kept = (uint32_t)(m.b - m.a);
    lanes_copy(dst, m.bytes + m.rec.name_off, m.rec.name_len, lane, nl);
    uint8_t *s = dst + m.rec.name_len, *q = s + kept;
    const uint8_t *bases = m.bytes + m.rec.seq_off + m.a, *quals = m.bytes + m.rec.qual_off + m.a;
    bool ok = true;
    for (uint32_t k = (uint32_t)lane; k < kept; k += (uint32_t)nl) {
        const uint8_t c = comp[bases[kept - 1u - k]];
        ok = ok && c != 0;
        s[k] = c;
        q[k] = quals[kept - 1u - k];
    }
    return ok;
}

}  // namespace atr

#endif

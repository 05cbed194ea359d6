// fasta_core.hpp -- per-line and per-record arithmetic of the device-resident FASTA batch: line
// classification, record descriptors over the line sums, and the FASTA formatter.
//
// The reference reads FASTA line by line (FastaReader, atropos/io/seqio.py:233-280): every line is
// strip()ped, blank lines and lines that start with '#' are skipped anywhere, a line that starts with
// '>' opens a record whose name is the rest of the line, every other line is a piece of the current
// record's sequence; the pieces are joined.  It writes '>' name '\n' sequence '\n' (FastaFormat,
// io/seqio.py:1008-1067; the command line never asks for wrapping).
//
// Here a batch is the file's bytes plus one FastqRecord per record (qual_off = qual_len = flags = 0).
// A record with at most one sequence line is used in place; the lines of any other record are gathered
// into a tail behind the text, so that every later stage sees one contiguous sequence.  All sums are
// differences of ONE exclusive prefix sum over the lines (low half: stripped sequence bytes, high
// half: headers), so a record may span any number of thread blocks and no sum depends on scheduling.
//
// One difference from the reference: it decodes the file as UTF-8, where U+0085 and U+00A0 are
// whitespace for strip(); here whitespace is the ASCII set " \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f" and
// bytes >= 0x80 never are.
//
// Compiled for gfx950 and, with -DATR_HOST_EMU, for the CPU test emulation (tests/emu).
#ifndef ATR_FASTA_CORE_HPP
#define ATR_FASTA_CORE_HPP

#include "fastq_core.hpp"

namespace atr {

enum { FASTA_SKIP = 0, FASTA_HEADER = 1, FASTA_SEQ = 2 };

// str.strip()'s whitespace among the bytes below 0x80
ATR_DEV bool fasta_is_space(uint8_t c) { return c == 32u || (c >= 9u && c <= 13u) || (c >= 28u && c <= 31u); }

// The line [start, end] (end: the last byte of its terminator) stripped: `at` its first byte that is not
// whitespace, `len` the bytes up to its last one.  Returns the line's class.
ATR_DEV int fasta_line_one(const uint8_t *bytes, uint32_t start, uint32_t end, uint32_t &at, uint32_t &len) {
    uint32_t lo = start, hi = end + 1u;                           // (a chunk is smaller than 2^32 - 16 bytes)
    while (lo < hi && fasta_is_space(bytes[lo])) ++lo;
    while (hi > lo && fasta_is_space(bytes[hi - 1u])) --hi;
    at = lo;
    len = hi - lo;
    if (len == 0u || bytes[lo] == '#') return FASTA_SKIP;
    return bytes[lo] == '>' ? FASTA_HEADER : FASTA_SEQ;
}

// what a line adds to the prefix sum: a header counts in the high half, a sequence line's bytes in the low
ATR_DEV unsigned long long fasta_line_value(int cls, uint32_t len) {
    return cls == FASTA_HEADER ? (1ull << 32) : (cls == FASTA_SEQ ? (unsigned long long)len : 0ull);
}
ATR_DEV uint32_t fasta_pre_bytes(unsigned long long pre) { return (uint32_t)(pre & 0xFFFFFFFFull); }
ATR_DEV long long fasta_pre_headers(unsigned long long pre) { return (long long)(pre >> 32); }

// The lines of a batch as the index keeps them between its two calls.  pre[L]: the exclusive prefix sum of
// fasta_line_value over the lines, pre[nlines] the total; head_line[r]: the header line of record r.
struct FastaLines {
    const uint32_t *line_ends;
    const uint8_t *cls;
    const uint32_t *at, *len;
    const unsigned long long *pre;
    const uint32_t *head_line;
    long long nlines, nrec;
};

ATR_DEV long long fasta_next_head(const FastaLines &ln, long long r) { return r + 1 < ln.nrec ? (long long)ln.head_line[r + 1] : ln.nlines; }

// Sequence bytes of record r and its first sequence line (-1: none).  The walk to that line passes blank and '#'
// lines only.
ATR_DEV uint32_t fasta_record_sum(const FastaLines &ln, long long r, long long &first) {
    const long long h = ln.head_line[r], next = fasta_next_head(ln, r);
    const uint32_t total = fasta_pre_bytes(ln.pre[next]) - fasta_pre_bytes(ln.pre[h]);
    first = -1;
    if (total) {
        first = h + 1;
        while (ln.cls[first] != FASTA_SEQ) ++first;               // (total > 0: there is one in front of `next`)
    }
    return total;
}

// Bytes record r needs in the tail: its sequence if it has more than one sequence line (every such line
// holds at least one byte, so "more than one" is "more bytes than the first")
ATR_DEV uint32_t fasta_record_gather(const FastaLines &ln, long long r) {
    long long first;
    const uint32_t total = fasta_record_sum(ln, r, first);
    return (total && total > ln.len[first]) ? total : 0u;
}

// Descriptor of record r.  tail_pre[r]: the exclusive prefix sum of fasta_record_gather, tail_off: where the
// tail begins in the chunk.  rec_end: the last byte of the line end of the record's last line (the line in
// front of the next header, skipped lines included).
ATR_DEV void fasta_record_one(const FastaLines &ln, const unsigned long long *tail_pre, uint32_t tail_off, long long r,
                              FastqRecord &rec, uint32_t &rec_end) {
    const long long h = ln.head_line[r], next = fasta_next_head(ln, r);
    rec.name_off = ln.at[h] + 1u;                                 // the stripped line after '>'
    rec.name_len = ln.len[h] - 1u;
    long long first;
    rec.seq_len = fasta_record_sum(ln, r, first);
    if (first < 0) rec.seq_off = rec.name_off + rec.name_len;
    else if (rec.seq_len > ln.len[first]) rec.seq_off = tail_off + (uint32_t)tail_pre[r];
    else rec.seq_off = ln.at[first];
    rec.qual_off = rec.qual_len = 0u;
    rec.flags = rec.reserved = 0u;
    rec_end = ln.line_ends[next - 1];
}

// Where sequence line L goes in the tail, or false if its record stays in place.
ATR_DEV bool fasta_line_target(const FastaLines &ln, const unsigned long long *tail_pre, long long L, uint32_t &to) {
    if (ln.cls[L] != FASTA_SEQ) return false;
    const long long r = fasta_pre_headers(ln.pre[L]) - 1;
    if (r < 0 || tail_pre[r + 1] == tail_pre[r]) return false;
    to = (uint32_t)tail_pre[r] + (fasta_pre_bytes(ln.pre[L]) - fasta_pre_bytes(ln.pre[ln.head_line[r]]));
    return true;
}

// Bytes of a formatted record: '>' name '\n' seq '\n'
ATR_DEV uint32_t fasta_record_bytes(const FastqRecord &rec, int kept) { return 1u + rec.name_len + 1u + (uint32_t)kept + 1u; }

// The record's text at o, written by `nl` cooperating lanes (the emulation passes 0, 1); the arguments of
// fastq_format_record.  Reads the name and the sequence only: a FASTQ record is formatted just as well.
ATR_DEV void fasta_format_record(uint8_t *o, const uint8_t *bytes, const FastqRecord &rec, int a, int b, int ub, int ue,
                                 int lane, int nl) {
    const uint32_t kept = (uint32_t)(b - a);
    if (lane == 0) o[0] = '>';
    lanes_copy(o + 1, bytes + rec.name_off, rec.name_len, lane, nl);
    o += 1 + rec.name_len;
    if (lane == 0) o[0] = '\n';
    o += 1;
    if (ub > a || ue < b) {
        for (uint32_t k = (uint32_t)lane; k < kept; k += (uint32_t)nl) o[k] = masked_base(bytes + rec.seq_off, a + (int)k, ub, ue);
    } else {
        lanes_copy(o, bytes + rec.seq_off + a, kept, lane, nl);
    }
    if (lane == 0) o[kept] = '\n';
}

}  // namespace atr
#endif

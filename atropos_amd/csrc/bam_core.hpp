// bam_core.hpp -- per-record and per-tile code of unaligned BAM input: the record walk over the inflated bytes of
// a BAM stream and the decode of its records into FASTQ text.
//
// A BAM stream behind its header is a run of records, each `block_size` (int32) followed by block_size bytes:
//   refID i32 | pos i32 | l_read_name u8 | mapq u8 | bin u16 | n_cigar_op u16 | flag u16 | l_seq i32 | next_refID i32 |
//   next_pos i32 | tlen i32 | read_name (NUL-terminated) | cigar u32 x n_cigar_op | seq, 4 bits a base, high nibble
//   first | qual u8 x l_seq | tags.                       (SAM/BAM specification, section 4.2; all little-endian)
// A record says only where the next one begins, so the walk of a chunk is a chain of dependent loads.  It is split
// the way the stream gunzip splits a deflate stream (inflate_stream_core.hpp): the bytes are cut into tiles, every
// tile guesses its first record start from what a record looks like (bam_plausible_chain) and walks from there to
// its end (bam_tile_walk), and ONE serial pass over the tiles (bam_resolve_tile) follows the true chain from the
// chunk's entry: a tile whose guess is the chain's start in it keeps its result, any other is walked again from the
// true start until that walk meets a start the speculative walk visited as well.  The result is the serial walk's
// for any byte content: a guess only ever saves work.
//
// The walk (bam_step) stops at the first record that is not whole inside the chunk, or that cannot be one:
// block_size below what its own fields need, above the cap a carried-over record may have, or a negative l_seq.
//
// Compiled for gfx950 and, with -DATR_HOST_EMU, for the CPU test emulation (tests/emu).
#ifndef ATR_BAM_CORE_HPP
#define ATR_BAM_CORE_HPP

#include "fastq_core.hpp"

namespace atr {

enum { BAM_OK = 0, BAM_SMALL = 1, BAM_BIG = 2, BAM_LSEQ = 3, BAM_TRUNCATED = 4, BAM_PARTIAL = 5 };   // 1 .. 4: ATR_BAM_ERR_*
enum { BAM_REC_LSEQ0 = 1, BAM_REC_QUAL = 2, BAM_REC_NAME = 3, BAM_REC_PAIR_NAME = 4, BAM_REC_PAIR_FLAGS = 5 };  // ATR_BAM_REC_*
enum { BAM_FIXED = 36, BAM_LOOKAHEAD = 3 };               // block_size + the 32 fixed bytes; records a guess must chain over
constexpr uint32_t BAM_NONE = 0xFFFFFFFFu;                // no start (a chunk is smaller than 2^32 - 16 bytes)
constexpr long long BAM_FAR = 0x7FFFFFFFFFFFFFFFll;

// records start at any byte: the fields are put together from bytes
ATR_DEV uint32_t bam_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
ATR_DEV int32_t bam_i32(const uint8_t *p) {
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// what the fields of a record need of block_size (l_seq >= 0)
ATR_DEV long long bam_min_block(uint32_t l_read_name, uint32_t n_cigar, int32_t l_seq) {
    return 32ll + l_read_name + 4ll * n_cigar + ((long long)l_seq + 1) / 2 + l_seq;
}

// One step of the serial walk: the record at `at` (0 <= at <= n) of bytes[0 .. n).  BAM_OK: it is whole, the next one
// begins at `next`; BAM_PARTIAL: the chunk ends in it (or at it); else what is wrong with it.  Reads bytes below n only.
ATR_DEV int bam_step(const uint8_t *bytes, long long n, long long at, long long cap, long long &next) {
    if (n - at < 4) return BAM_PARTIAL;
    const long long bs = bam_i32(bytes + at);
    if (bs < 32) return BAM_SMALL;
    if (bs > cap) return BAM_BIG;
    if (at + 4 + bs > n) return BAM_PARTIAL;
    const int32_t l_seq = bam_i32(bytes + at + 20);
    if (l_seq < 0) return BAM_LSEQ;
    if (bs < bam_min_block(bytes[at + 12], bam_u16(bytes + at + 16), l_seq)) return BAM_SMALL;
    next = at + 4 + bs;
    return BAM_OK;
}

// Does a record plausibly begin at `at` (at + BAM_FIXED <= n)?  Stricter than bam_step: a name that ends in NUL and
// reference ids the header knows.  The name's end is looked at where the chunk holds it.
ATR_DEV bool bam_plausible(const uint8_t *bytes, long long n, long long at, int32_t n_ref, long long cap, long long &next) {
    const uint8_t *p = bytes + at;
    const long long bs = bam_i32(p);
    const int32_t ref = bam_i32(p + 4), l_seq = bam_i32(p + 20), mate_ref = bam_i32(p + 24);
    const uint32_t l_name = p[12];
    if (l_seq < 0 || l_name < 1u) return false;
    if (ref < -1 || ref >= n_ref || mate_ref < -1 || mate_ref >= n_ref) return false;
    if (bs < bam_min_block(l_name, bam_u16(p + 16), l_seq) || bs > cap) return false;
    const long long nul = at + BAM_FIXED + l_name - 1;
    if (nul < n && bytes[nul] != 0) return false;
    next = at + 4 + bs;
    return true;
}

// A candidate start: a plausible record whose next BAM_LOOKAHEAD - 1 records, as far as the chunk holds their fixed
// bytes, are plausible too.
ATR_DEV bool bam_plausible_chain(const uint8_t *bytes, long long n, long long at, int32_t n_ref, long long cap) {
    for (int k = 0; k < BAM_LOOKAHEAD; ++k) {
        if (at + BAM_FIXED > n) return k > 0;
        long long next;
        if (!bam_plausible(bytes, n, at, n_ref, cap, next)) return false;
        at = next;
    }
    return true;
}

// What a tile knows of itself after the speculative pass: its guess (BAM_NONE: no candidate), the whole records the
// walk from the guess found with their start inside the tile, where that walk left the tile (status BAM_OK: the first
// start at or beyond the tile's end) or stopped (status: why, exit: at which record).
struct BamTile {
    uint32_t guess, exit, count, status;
};

// The walk from `from` (inside the tile) to the tile's end.
ATR_DEV BamTile bam_tile_walk(const uint8_t *bytes, long long n, long long from, long long tile_end, long long cap) {
    BamTile t = {(uint32_t)from, 0u, 0u, (uint32_t)BAM_OK};
    long long at = from;
    while (at < tile_end) {
        long long next;
        const int st = bam_step(bytes, n, at, cap, next);
        if (st != BAM_OK) { t.status = (uint32_t)st; break; }
        ++t.count;
        at = next;
    }
    t.exit = (uint32_t)at;
    return t;
}

// The true chain as the serial pass carries it from tile to tile.
struct BamChain {
    long long at;                 // the next record start of the chain (while status == BAM_OK)
    int status;                   // BAM_OK, or why the chain stopped at `at`
    unsigned long long count, repaired;
};

ATR_DEV void bam_chain_take(BamChain &c, const BamTile &t) {
    c.at = t.exit;
    c.status = (int)t.status;
}

// Tile [.., tile_end) of the chain: `entry` = the chain's first start inside it (BAM_NONE: it has none -- the tile
// lies inside one record, behind the chain's end or behind the chunk's last byte), `base` = the records in front of it.
ATR_DEV void bam_resolve_tile(const uint8_t *bytes, long long n, long long cap, long long tile_end, const BamTile &spec,
                              BamChain &c, uint32_t &entry, uint32_t &base) {
    base = (uint32_t)c.count;
    entry = BAM_NONE;
    if (c.status != BAM_OK || c.at >= tile_end || c.at >= n) return;
    entry = (uint32_t)c.at;
    if (spec.guess == entry) {
        c.count += spec.count;
        bam_chain_take(c, spec);
        return;
    }
    // the guess was wrong, or there was none: the true walk p and the speculative walk s side by side, the one that
    // is behind steps, until they stand on the same start
    ++c.repaired;
    long long p = c.at, s = spec.guess == BAM_NONE ? BAM_FAR : (long long)spec.guess;
    uint32_t p_count = 0, s_count = 0;
    for (;;) {
        if (p >= tile_end) { c.at = p; c.count += p_count; return; }
        if (s != BAM_FAR && s >= tile_end) s = BAM_FAR;
        if (p == s) {
            c.count += p_count + (spec.count - s_count);
            bam_chain_take(c, spec);
            return;
        }
        long long next = 0;
        if (p < s) {
            const int st = bam_step(bytes, n, p, cap, next);
            if (st != BAM_OK) { c.at = p; c.status = st; c.count += p_count; return; }
            ++p_count;
            p = next;
        } else {
            if (bam_step(bytes, n, s, cap, next) == BAM_OK) { ++s_count; s = next; }
            else s = BAM_FAR;
        }
    }
}

// the words of atr_bam_walk's result once the chain has passed the last tile
ATR_DEV void bam_chain_result(const BamChain &c, long long n, int final, long long *result) {
    const long long consumed = c.at < n ? c.at : n;       // (a chain that runs to the end stands at n)
    long long error = BAM_FAR;
    if (c.status >= BAM_SMALL && c.status <= BAM_LSEQ) error = consumed * 8 + c.status;
    else if (final && consumed != n) error = consumed * 8 + BAM_TRUNCATED;
    result[0] = (long long)c.count;
    result[1] = consumed;
    result[2] = error;
    result[3] = (long long)c.repaired;
}

// ---------------------------------------------------------------------------------------------- decode
struct BamFields {
    uint32_t l_name, n_cigar, flag;
    int32_t l_seq;
    uint32_t name, seq, qual;     // byte offsets
};

ATR_DEV BamFields bam_fields(const uint8_t *bytes, uint32_t at) {
    BamFields f;
    f.l_name = bytes[at + 12];
    f.n_cigar = bam_u16(bytes + at + 16);
    f.flag = bam_u16(bytes + at + 18);
    f.l_seq = bam_i32(bytes + at + 20);
    f.name = at + BAM_FIXED;
    f.seq = f.name + f.l_name + 4u * f.n_cigar;
    f.qual = f.seq + ((uint32_t)f.l_seq + 1u) / 2u;
    return f;
}

ATR_DEV uint32_t bam_name_len(const BamFields &f) { return f.l_name ? f.l_name - 1u : 0u; }

// '@' name '\n' seq '\n' '+' '\n' qual '\n'
ATR_DEV unsigned long long bam_text_bytes(const BamFields &f) { return (unsigned long long)bam_name_len(f) + 2ull * (uint32_t)f.l_seq + 6ull; }

// Output slot j of a paired decode takes record bam_pair_source: records 2i and 2i + 1 are a pair, read 1 first
// (flag 0x40) or read 2 first, which swaps them (PairedEndSAMReader, io/seqio.py:634-638).  `error`: what is wrong
// with the pair (checked for every slot alike, reported by the even one).
ATR_DEV long long bam_pair_source(const uint8_t *bytes, const uint32_t *starts, long long j, int &error) {
    const long long i = j & ~1ll;
    const BamFields a = bam_fields(bytes, starts[i]), b = bam_fields(bytes, starts[i + 1]);
    error = 0;
    bool same = a.l_name == b.l_name;
    for (uint32_t k = 0; same && k < a.l_name; ++k) same = bytes[a.name + k] == bytes[b.name + k];
    const bool first_is_read1 = (a.flag & 0x40u) != 0u;
    if (!same) error = BAM_REC_PAIR_NAME;
    else if (!(b.flag & (first_is_read1 ? 0x80u : 0x40u))) error = BAM_REC_PAIR_FLAGS;
    return first_is_read1 ? j : (j ^ 1ll);
}

// what can be said of a record without its name and qualities
ATR_DEV int bam_record_check(const BamFields &f) {
    if (f.l_seq == 0) return BAM_REC_LSEQ0;
    if (f.l_name == 0u) return BAM_REC_NAME;
    return 0;
}

ATR_DEV uint8_t bam_base(uint32_t nibble) {
    return (uint8_t)"=ACMGRSVTWYHKDBN"[nibble & 15u];
}

// The record's FASTQ text at o, written by `nl` cooperating lanes (the emulation passes 0, 1).  Returns what this
// lane saw wrong in the name or the qualities (0: nothing).
ATR_DEV int bam_format_record(uint8_t *o, const uint8_t *bytes, const BamFields &f, int lane, int nl) {
    const uint32_t name_len = bam_name_len(f), l_seq = (uint32_t)f.l_seq;
    int error = 0;
    if (lane == 0) o[0] = '@';
    for (uint32_t k = (uint32_t)lane; k < name_len; k += (uint32_t)nl) {
        const uint8_t c = bytes[f.name + k];
        if (c == '\n' || c == '\r') error = BAM_REC_NAME;
        o[1u + k] = c;
    }
    o += 1u + name_len;
    if (lane == 0) o[0] = '\n';
    o += 1;
    for (uint32_t k = (uint32_t)lane; k < (l_seq + 1u) / 2u; k += (uint32_t)nl) {      // a byte, two bases, per step
        const uint32_t pair = bytes[f.seq + k];
        o[2u * k] = bam_base(pair >> 4);
        if (2u * k + 1u < l_seq) o[2u * k + 1u] = bam_base(pair);
    }
    o += l_seq;
    if (lane == 0) { o[0] = '\n'; o[1] = '+'; o[2] = '\n'; }
    o += 3;
    for (uint32_t k = (uint32_t)lane; k < l_seq; k += (uint32_t)nl) {
        const uint32_t q = bytes[f.qual + k];
        if (q > 93u) error = BAM_REC_QUAL;                  // (the smaller kind: what the minimum over the lanes keeps)
        o[k] = (uint8_t)(q + 33u);
    }
    if (lane == 0) o[l_seq] = '\n';
    return error;
}

// ---------------------------------------------------------------------------------------------- header (host)
// "BAM\1" | l_text i32 | text | n_ref i32 | n_ref x (l_name i32 | name | l_ref i32).  Returns 0 with the header's
// length and n_ref, 1 when buf[0 .. n) ends inside the header, -1 when it is none.
static inline long long bam_host_i32(const uint8_t *p) {
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

static inline int bam_header_parse(const uint8_t *buf, long long n, long long *header_bytes, int *n_ref) {
    static const uint8_t magic[4] = {'B', 'A', 'M', 1};
    for (long long k = 0; k < 4 && k < n; ++k)
        if (buf[k] != magic[k]) return -1;
    if (n < 8) return 1;
    const long long l_text = bam_host_i32(buf + 4);
    if (l_text < 0) return -1;
    long long at = 8 + l_text;
    if (at + 4 > n) return 1;
    const long long refs = bam_host_i32(buf + at);
    if (refs < 0) return -1;
    at += 4;
    for (long long r = 0; r < refs; ++r) {
        if (at + 4 > n) return 1;
        const long long l_name = bam_host_i32(buf + at);
        if (l_name < 0) return -1;
        at += 4 + l_name + 4;
        if (at > n) return 1;
    }
    *header_bytes = at;
    *n_ref = (int)refs;
    return 0;
}

}  // namespace atr
#endif

// inflate_core.hpp -- per-member arithmetic of the device gunzip (gunzip_kernels.hip): one BGZF member (RFC 1952 with
// the 'BC' extra subfield, an RFC 1951 body of any number of stored / fixed / dynamic blocks) -> its text.
//
// A member is worked on by ONE WAVE of INF_NT = 64 lanes.  The bit reader and the Huffman decode are UNIFORM: every
// lane holds the same bit position and takes the same branches.  The lanes share
//   the input     64 words of the member sit in one register per lane (InfWave::chunk); the reader picks two of them
//                 by lane index; a reload every 252 bytes is one coalesced load
//   the decode    canonical codes, no table walk: lane l (1 .. 15) holds the left-aligned end of the codes of length l,
//                 one compare + ballot + count-trailing-zeros gives a code's length, a lane read its base into the
//                 symbols sorted by (length, symbol) in LDS
//   the tables    counting and sorting the code lengths of a block: a lane per length
//   the copies    a match of length n at distance d: lane k writes out[pos + k] = out[pos - d + k % d], k = lane, lane + 64, ...
//                 -- every source byte lies BEFORE pos, so a distance below the length (or the lane count) gives the serial
//                 result without any order among the lanes
//   the CRC       1024 positions per lane, folded with the fixed multipliers of deflate_core.hpp
//   the output    the member's text is decoded into LDS (64 KiB) and copied to its place in the text tensor only after
//                 ISIZE and the CRC were found right: the only stores to global memory, all inside the member's range.
// Lanes exchange data through LDS only, and between a store and a load of it by another lane stands INF_SYNC() (the
// barrier of the one-wave workgroup, which is also the fence the compiler needs); out[] is written once per position.
//
// Bounds: every store to out[] is checked against the member's text size before it is made, whatever the bits say;
// no byte is loaded from outside the member's range of the stream (reads beyond it give zero bits), and the bit
// position is checked against the trailer after every code.  A member that breaks a rule gets a nonzero INF_E_* status.
//
// Compiled for gfx950 and, with -DATR_HOST_EMU, for the CPU twin (tests/emu/emu_gunzip.cpp): INF_LANES is then a loop
// over the lanes and a per-lane register an array.
#ifndef ATR_INFLATE_CORE_HPP
#define ATR_INFLATE_CORE_HPP

#include <stdint.h>

#include "deflate_core.hpp"

namespace atr {

enum {
    INF_NT = 64,                 // lanes of a member: one wave
    INF_MAX_TEXT = 65536,        // ISIZE of a BGZF member is at most this
    INF_MAX_MEMBER = 65536,      // BSIZE + 1 is at most this
    INF_MAX_MEMBERS = 1 << 22,   // members of one call: the grid (a workgroup each) stays far inside what a launch takes
    INF_LL = 288, INF_D = 32, INF_CL = 19,
    INF_RANGE = INF_MAX_TEXT / INF_NT,     // positions a lane checksums
};

// status of a member (0: its text is in place)
enum {
    INF_OK = 0,
    INF_E_RANGE = 1,        // member_at / text_at: negative, decreasing, beyond the stream or the capacity, above 64 KiB
    INF_E_HEADER = 2,       // magic, CM, FLG, no 'BC' subfield of SLEN 2, no room for the trailer
    INF_E_BSIZE = 3,        // BSIZE + 1 is not the member's range
    INF_E_ISIZE = 4,        // ISIZE is not the text range, or the blocks end short of it
    INF_E_BTYPE = 5,        // BTYPE 11
    INF_E_STORED = 6,       // LEN / NLEN
    INF_E_LENGTHS = 7,      // HLIT > 286, HDIST > 30, an over-subscribed or incomplete code
    INF_E_NO_EOB = 8,       // no code for end-of-block
    INF_E_REPEAT = 9,       // symbol 16 with nothing before it, a repeat past HLIT + HDIST
    INF_E_SYMBOL = 10,      // bits that are no code, literal/length symbol 286 / 287, distance symbol 30 / 31
    INF_E_DISTANCE = 11,    // a distance that reaches before the member's first byte
    INF_E_OVERRUN = 12,     // output past ISIZE
    INF_E_INPUT = 13,       // input that runs into the trailer, or ends before it
    INF_E_CRC = 14,
    INF_E_SHORT = 100,      // (inf_header only: the header is not wholly there)
};

#ifdef ATR_HOST_EMU
#define INF_LANES(...) for (int lane = 0; lane < INF_NT; ++lane) { __VA_ARGS__; }
#define INF_LANE0(...) { __VA_ARGS__; }
#define INF_SYNC()
#define INF_REG(name) uint32_t name[INF_NT]
#define INF_R(reg) reg[lane]
#define INF_GET(reg, idx) (reg[(idx)])
#define INF_UNIFORM(x) (x)
#else
#define INF_LANES(...) { const int lane = (int)threadIdx.x; __VA_ARGS__; }
#define INF_LANE0(...) if (threadIdx.x == 0) { __VA_ARGS__; }
#define INF_SYNC() __syncthreads()
#define INF_REG(name) uint32_t name
#define INF_R(reg) reg
#define INF_GET(reg, idx) ((uint32_t)__builtin_amdgcn_readlane((int)(reg), (int)(idx)))
#define INF_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#endif

GZ_HD uint32_t inf_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
GZ_HD uint32_t inf_le32(const uint8_t *p) { return inf_le16(p) | inf_le16(p + 2) << 16; }

// The gzip header of a BGZF member at p, of which `avail` bytes may be read: magic, CM 8, FEXTRA (FTEXT is let pass,
// every other flag would put fields behind the extra field), the walk over the extra subfields to 'BC' with SLEN 2.
// -> INF_OK and where the deflate data starts and BSIZE; INF_E_SHORT: the header is longer than avail; INF_E_HEADER.
GZ_HD int inf_header(const uint8_t *p, uint32_t avail, uint32_t *data_at, uint32_t *bsize) {
    if (avail < 12) return INF_E_SHORT;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4) || (p[3] & 0xfa)) return INF_E_HEADER;
    const uint32_t end = 12 + inf_le16(p + 10);
    if (end > avail) return INF_E_SHORT;
    for (uint32_t at = 12; at + 4 <= end;) {
        const uint32_t slen = inf_le16(p + at + 2);
        if (p[at] == 'B' && p[at + 1] == 'C') {
            if (slen != 2 || at + 6 > end) return INF_E_HEADER;
            *bsize = inf_le16(p + at + 4);
            *data_at = end;
            return INF_OK;
        }
        at += 4 + slen;
    }
    return INF_E_HEADER;
}

// The whole members at the front of buf[0 .. n): member_at[0 .. k] and text_at[0 .. k] (the running sum of ISIZE), at
// most max_members of them; *covered: the bytes they take.  Stops at the first member that is not whole.
// -> 0, or -1 at a header that is not a BGZF member (k and *covered then tell which).
GZ_HD int inf_scan(const uint8_t *buf, int64_t n, int64_t max_members, int64_t *member_at, int64_t *text_at, int64_t *n_members,
                   int64_t *covered) {
    int64_t at = 0, text = 0, k = 0;
    int rc = 0;
    member_at[0] = 0;
    text_at[0] = 0;
    while (k < max_members && at < n) {
        const uint32_t avail = (uint32_t)(n - at < INF_MAX_MEMBER ? n - at : INF_MAX_MEMBER);
        uint32_t data_at = 0, bsize = 0;
        const int st = inf_header(buf + at, avail, &data_at, &bsize);
        if (st == INF_E_SHORT) break;
        if (st || bsize + 1 < data_at + 8) { rc = -1; break; }
        if (at + bsize + 1 > n) break;
        const uint32_t isize = inf_le32(buf + at + bsize + 1 - 4);
        if (isize > INF_MAX_TEXT) { rc = -1; break; }
        at += bsize + 1;
        text += isize;
        ++k;
        member_at[k] = at;
        text_at[k] = text;
    }
    *n_members = k;
    *covered = at;
    return rc;
}

// ---------------------------------------------------------------------------------------------- the member
struct InfTables {                         // what the codes of a block take (shared with inflate_stream_core.hpp)
    uint32_t crc_tab[256];
    uint32_t lane_a[INF_NT];               // per lane: the CRC of its positions
    uint32_t cnt[16];                      // codes per length of the code being built
    uint16_t sym[3][INF_LL];               // symbols sorted by (length, symbol): literal/length, distance, code-length
    uint8_t seq[INF_LL + INF_D];           // the code lengths of a block: HLIT of them, then HDIST
    uint8_t cl_len[INF_CL + 1];
};

struct InfLds : InfTables {
    uint32_t out[INF_MAX_TEXT / 4];        // the member's text
};

enum { INF_T_LL = 0, INF_T_D = 1, INF_T_CL = 2 };
enum { INF_B_COMPLETE = 0, INF_B_OVER = 1, INF_B_INCOMPLETE = 2, INF_B_SINGLE = 3, INF_B_EMPTY = 4 };

struct InfWave {
    INF_REG(chunk);          // word cbase + lane of the member
    INF_REG(lim[3]);         // lane l, 1 .. 15: (first code of length l + their count) << (15 - l); 0 in the other lanes
    INF_REG(base[3]);        // lane l: index of the first symbol of length l in sym[] - first code of length l
    uint32_t cbase;
};

struct InfCtx {
    InfTables *L;            // (inf_member: an InfLds)
    const uint8_t *src;      // the member
    uint32_t msize;          // 26 .. INF_MAX_MEMBER
    uint8_t *dst;            // its text
    uint32_t n_out;          // 0 .. INF_MAX_TEXT
};

ATR_DEV uint32_t inf_rev15(uint32_t v) {                    // the low 15 bits of v, reversed
#if defined(__clang__)
    return __builtin_bitreverse32(v) >> 17;
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    return ((v >> 16) | (v << 16)) >> 17;
#endif
}

// the 32 bits at bitpos (least significant first); bits beyond the member are zero
ATR_DEV uint32_t inf_peek(const InfCtx &c, InfWave &W, uint32_t bitpos) {
    const uint32_t w = bitpos >> 5;
    if (w < W.cbase || w + 1 >= W.cbase + INF_NT) {
        W.cbase = w;
        INF_LANES(
            const uint32_t b = 4u * (w + (uint32_t)lane);
            uint32_t v = 0;
            for (uint32_t k = 0; k < 4; ++k)
                if (b + k < c.msize) v |= (uint32_t)c.src[b + k] << (8 * k);
            INF_R(W.chunk) = v;
        )
    }
    const uint32_t i = w - W.cbase;
    const uint64_t two = ((uint64_t)INF_GET(W.chunk, i + 1) << 32) | INF_GET(W.chunk, i);
    return (uint32_t)(two >> (bitpos & 31u));
}

// length of the code that the 15 reversed bits start with; 0: none
#ifdef ATR_HOST_EMU
#define INF_FIND(limreg, code15, len) { len = 0; for (int l_ = 1; l_ <= 15; ++l_) if ((code15) < limreg[l_]) { len = (uint32_t)l_; break; } }
#else
#define INF_FIND(limreg, code15, len) { const unsigned long long m_ = __ballot((code15) < limreg) & 0xfffeull; \
                                        len = m_ ? (uint32_t)__builtin_ctzll(m_) : 0u; }
#endif

// next symbol of code t at bitpos: -> symbol, or 0xffff for bits that are no code; len: its bits
#define INF_DECODE(t, v, S_, N_) { const uint32_t c15_ = inf_rev15(v); INF_FIND(W.lim[t], c15_, N_) \
    const uint32_t i_ = N_ ? INF_GET(W.base[t], N_) + (c15_ >> (15u - N_)) : (uint32_t)INF_LL; \
    S_ = i_ < INF_LL ? INF_UNIFORM(L->sym[t][i_]) : 0xffffu; }

// The canonical code over lens[0 .. n): counts per length (a lane per length), the Kraft sum, every lane's lim / base,
// the symbols in (length, symbol) order (a lane per length).  -> INF_B_*
ATR_DEV int inf_build(InfTables *L, InfWave &W, int t, const uint8_t *lens, uint32_t n) {
    INF_SYNC();                                            // (lens[] written, the table before it read)
    INF_LANES(
        if (lane < 16) {
            uint32_t k = 0;
            for (uint32_t i = 0; i < n; ++i) k += lens[i] == (uint32_t)lane;
            L->cnt[lane] = k;
        }
    )
    INF_SYNC();
    int left = 1, maxlen = 0;
    for (int l = 1; l <= 15; ++l) {
        const int k = (int)INF_UNIFORM(L->cnt[l]);
        left = 2 * left - k;
        if (left < 0) return INF_B_OVER;
        if (k) maxlen = l;
    }
    INF_LANES(
        uint32_t first = 0, off = 0, lim = 0, base = 0, mine = 0;
        for (int l = 1; l <= 15; ++l) {
            const uint32_t k = L->cnt[l];
            if (l == lane) { lim = (first + k) << (15 - l); base = off - first; mine = off; }
            first = (first + k) << 1;
            off += k;
        }
        INF_R(W.lim[t]) = lim;
        INF_R(W.base[t]) = base;
        if (lane >= 1 && lane <= 15)
            for (uint32_t i = 0; i < n; ++i)
                if (lens[i] == (uint32_t)lane) L->sym[t][mine++] = (uint16_t)i;
    )
    INF_SYNC();
    return left == 0 ? INF_B_COMPLETE : maxlen == 0 ? INF_B_EMPTY : maxlen == 1 ? INF_B_SINGLE : INF_B_INCOMPLETE;
}

// the header of a dynamic block: the code-length code, then HLIT + HDIST code lengths into seq[]
ATR_DEV int inf_dynamic(const InfCtx &c, InfWave &W, uint32_t &bitpos, uint32_t endbits, uint32_t &hlit, uint32_t &hdist) {
    InfTables *L = c.L;
    const uint8_t order[INF_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v = inf_peek(c, W, bitpos);
    hlit = (v & 31u) + 257u;
    hdist = ((v >> 5) & 31u) + 1u;
    const uint32_t hclen = ((v >> 10) & 15u) + 4u;
    bitpos += 14;
    if (hlit > 286 || hdist > 30) return INF_E_LENGTHS;
    INF_SYNC();
    for (uint32_t i = 0; i < INF_CL; ++i) {
        uint32_t x = 0;
        if (i < hclen) { x = inf_peek(c, W, bitpos) & 7u; bitpos += 3; }
        const uint32_t at = order[i];
        INF_LANE0(L->cl_len[at] = (uint8_t)x)
    }
    if (bitpos > endbits) return INF_E_INPUT;
    if (inf_build(L, W, INF_T_CL, L->cl_len, INF_CL) != INF_B_COMPLETE) return INF_E_LENGTHS;
    const uint32_t total = hlit + hdist;
    uint32_t prev = 0;
    for (uint32_t i = 0; i < total;) {
        v = inf_peek(c, W, bitpos);
        uint32_t s, len;
        INF_DECODE(INF_T_CL, v, s, len)
        if (s > 18) return INF_E_LENGTHS;
        bitpos += len;
        v >>= len;
        uint32_t rep = 1, val = s;
        if (s == 16) {
            if (i == 0) return INF_E_REPEAT;
            rep = 3 + (v & 3u); bitpos += 2; val = prev;
        } else if (s == 17) {
            rep = 3 + (v & 7u); bitpos += 3; val = 0;
        } else if (s == 18) {
            rep = 11 + (v & 127u); bitpos += 7; val = 0;
        }
        if (i + rep > total) return INF_E_REPEAT;
        if (bitpos > endbits) return INF_E_INPUT;
        INF_LANES(for (uint32_t k = (uint32_t)lane; k < rep; k += INF_NT) L->seq[i + k] = (uint8_t)val)
        prev = val;
        i += rep;
    }
    INF_SYNC();
    if (INF_UNIFORM(L->seq[GZ_EOB]) == 0) return INF_E_NO_EOB;
    return INF_OK;
}

// the codes of a fixed block as code lengths: 288 literal/length, then 32 distance
ATR_DEV void inf_fixed(InfTables *L) {
    INF_SYNC();
    INF_LANES(
        for (uint32_t i = (uint32_t)lane; i < INF_LL + INF_D; i += INF_NT)
            L->seq[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    )
}

// the tokens of a coded block, up to its end-of-block
ATR_DEV int inf_tokens(const InfCtx &c, InfWave &W, uint32_t &bitpos, uint32_t endbits, uint32_t &pos) {
    InfLds *L = static_cast<InfLds *>(c.L);
    uint8_t *out = (uint8_t *)L->out;
    for (;;) {
        uint32_t v = inf_peek(c, W, bitpos);
        uint32_t s, len;
        INF_DECODE(INF_T_LL, v, s, len)
        bitpos += len;
        if (bitpos > endbits) return INF_E_INPUT;
        if (s < 256) {
            if (pos >= c.n_out) return INF_E_OVERRUN;
            INF_LANE0(out[pos] = (uint8_t)s)
            ++pos;
            continue;
        }
        if (s == GZ_EOB) return INF_OK;
        if (s >= 286) return INF_E_SYMBOL;                 // (0xffff: no code)
        v >>= len;
        uint32_t n;                                        // the length, 3 .. 258
        if (s < 265) n = s - 254;
        else if (s == 285) n = 258;
        else {
            const uint32_t eb = (s - 261) >> 2;
            n = 3 + ((4 + ((s - 261) & 3u)) << eb) + (v & ((1u << eb) - 1u));
            bitpos += eb;
        }
        v = inf_peek(c, W, bitpos);
        INF_DECODE(INF_T_D, v, s, len)
        if (s >= 30) return INF_E_SYMBOL;
        bitpos += len;
        v >>= len;
        uint32_t d = s + 1;                                // the distance, 1 .. 32768
        if (s >= 4) {
            const uint32_t eb = (s >> 1) - 1;
            d = 1 + ((2 + (s & 1u)) << eb) + (v & ((1u << eb) - 1u));
            bitpos += eb;
        }
        if (bitpos > endbits) return INF_E_INPUT;
        if (d > pos) return INF_E_DISTANCE;
        if (n > c.n_out - pos) return INF_E_OVERRUN;
        INF_SYNC();                                        // (the bytes before pos are stored)
        const uint32_t from = pos - d;
        if (d >= n) {
            INF_LANES(for (uint32_t k = (uint32_t)lane; k < n; k += INF_NT) out[pos + k] = out[from + k])
        } else {
            INF_LANES(for (uint32_t k = (uint32_t)lane; k < n; k += INF_NT) out[pos + k] = out[from + k % d])
        }
        pos += n;
    }
}

ATR_DEV void inf_crc_table(InfTables *L) {
    INF_LANES(for (uint32_t i = (uint32_t)lane; i < 256; i += INF_NT) L->crc_tab[i] = gz_crc_entry(i))
    INF_SYNC();
}

// CRC-32 of out[0 .. n): the text taken as the LAST n bytes of INF_MAX_TEXT (zero bytes in front of a message leave a
// register that starts at zero unchanged), INF_RANGE positions per lane, folded pairwise (deflate_core.hpp: gz_p_crc)
ATR_DEV uint32_t inf_crc(InfLds *L, uint32_t n) {
    const uint8_t *out = (const uint8_t *)L->out;
    const uint32_t off = INF_MAX_TEXT - n;
    INF_SYNC();
    INF_LANES(
        uint32_t v = (uint32_t)lane * INF_RANGE;
        const uint32_t end = v + INF_RANGE;
        uint32_t crc = 0;
        if (v < off) v = off;
        for (; v < end; ++v) crc = L->crc_tab[(crc ^ out[v - off]) & 0xffu] ^ (crc >> 8);
        L->lane_a[lane] = crc;
    )
    INF_SYNC();
    for (int j = 0; j < 6; ++j) {
        const int stride = 1 << j;
        INF_LANES(
            if ((lane & (2 * stride - 1)) == 0) L->lane_a[lane] = gz_mulmod(gz_x8(10 + j), L->lane_a[lane]) ^ L->lane_a[lane + stride];
        )
        INF_SYNC();
    }
    return INF_UNIFORM(L->lane_a[0]) ^ gz_crc_advance(0xffffffffu, n) ^ 0xffffffffu;
}

// One member: header, blocks, ISIZE, CRC, and only then its text into dst[0 .. n_out).  L->crc_tab is filled.
// Every lane of the wave calls it (device), or the emulation calls it once.  -> INF_OK or INF_E_*
ATR_DEV int inf_member(const InfCtx &c) {
    InfLds *L = static_cast<InfLds *>(c.L);
    InfWave W;
    W.cbase = 0xffffffffu;
    uint32_t data_at = 0, bsize = 0;
    if (inf_header(c.src, c.msize, &data_at, &bsize) != INF_OK) return INF_E_HEADER;
    if (bsize + 1 != c.msize) return INF_E_BSIZE;
    if (data_at + 8 > c.msize) return INF_E_HEADER;
    const uint32_t end_byte = c.msize - 8, endbits = 8 * end_byte;
    const uint32_t crc_want = inf_le32(c.src + end_byte), isize = inf_le32(c.src + end_byte + 4);
    if (isize != c.n_out) return INF_E_ISIZE;
    uint8_t *out = (uint8_t *)L->out;
    uint32_t bitpos = 8 * data_at, pos = 0;
    for (;;) {
        uint32_t v = inf_peek(c, W, bitpos);
        bitpos += 3;
        if (bitpos > endbits) return INF_E_INPUT;
        const uint32_t bfinal = v & 1u, btype = (v >> 1) & 3u;
        if (btype == 3) return INF_E_BTYPE;
        if (btype == 0) {
            bitpos = (bitpos + 7u) & ~7u;
            v = inf_peek(c, W, bitpos);
            bitpos += 32;
            if (bitpos > endbits) return INF_E_INPUT;
            const uint32_t len = v & 0xffffu, at = bitpos >> 3;
            if ((v >> 16) != (~len & 0xffffu)) return INF_E_STORED;
            if (len > end_byte - at) return INF_E_INPUT;
            if (len > c.n_out - pos) return INF_E_OVERRUN;
            INF_LANES(for (uint32_t k = (uint32_t)lane; k < len; k += INF_NT) out[pos + k] = c.src[at + k])
            pos += len;
            bitpos += 8 * len;
        } else {
            uint32_t hlit = INF_LL, hdist = INF_D;
            if (btype == 1) inf_fixed(L);
            else {
                const int st = inf_dynamic(c, W, bitpos, endbits, hlit, hdist);
                if (st) return st;
            }
            int b = inf_build(L, W, INF_T_LL, L->seq, hlit);
            if (b == INF_B_OVER || b == INF_B_INCOMPLETE) return INF_E_LENGTHS;
            b = inf_build(L, W, INF_T_D, L->seq + hlit, hdist);
            if (b == INF_B_OVER || b == INF_B_INCOMPLETE) return INF_E_LENGTHS;
            const int st = inf_tokens(c, W, bitpos, endbits, pos);
            if (st) return st;
        }
        if (bfinal) break;
    }
    bitpos = (bitpos + 7u) & ~7u;
    if (bitpos != endbits) return INF_E_INPUT;
    if (pos != c.n_out) return INF_E_ISIZE;
    if (inf_crc(L, c.n_out) != crc_want) return INF_E_CRC;
    INF_LANES(for (uint32_t k = (uint32_t)lane; k < c.n_out; k += INF_NT) c.dst[k] = out[k])
    return INF_OK;
}

// the ranges of member m: -> false when they are no ranges a member can have
GZ_HD bool inf_ranges_ok(int64_t a0, int64_t a1, int64_t t0, int64_t t1, int64_t n_stream, int64_t capacity) {
    return a0 >= 0 && a1 >= a0 && a1 <= n_stream && a1 - a0 <= INF_MAX_MEMBER && t0 >= 0 && t1 >= t0 && t1 <= capacity &&
           t1 - t0 <= INF_MAX_TEXT;
}

}  // namespace atr
#endif

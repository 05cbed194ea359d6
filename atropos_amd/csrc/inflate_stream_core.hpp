// inflate_stream_core.hpp -- per-wave code of the speculative two-pass gunzip (gunzip_stream_kernels.hip): a slab of ONE
// ordinary deflate stream (RFC 1951, no member table) -> its text.  The method of pugz / rapidgzip:
//
//   find     the slab is cut into chunks of chunk_bytes; in every chunk but the first the lanes probe bit offsets for the
//            header of a non-final dynamic block (ist_probe: BTYPE, HLIT, HDIST, a complete code-length code), and the
//            wave decodes the header of every survivor with the uniform code of inflate_core.hpp (ist_verify: the code
//            lengths, an end-of-block code, a complete literal/length code, a distance code inflate would take).  The
//            first offset that passes is the chunk's candidate; chunk 0 starts at start_bit.
//   decode   a wave per chunk decodes from its candidate with an UNKNOWN window: the window is a ring of 16-bit symbols
//            in LDS, a symbol is a byte or the marker 0x8000 | (distance behind the chunk's start - 1), and every symbol
//            is written through to the chunk's room in the workspace.  It stops behind the block that ends exactly on
//            a later chunk's candidate, behind the final block, at the end of the input or of its room, or at an error
//            -- and what counts is the last block boundary before that (ist_run).
//   chain    ONE wave walks the chain from chunk 0: a chunk is confirmed when the chain's bit position is its
//            candidate; its place in the text is the running sum; its last 32 KiB are resolved against the text before
//            it and stored, so that the window behind it is final.  Where the chain breaks -- no chunk starts on this
//            bit, a chunk made no progress or does not fit -- the same wave decodes on from here with the KNOWN window
//            (ist_run again: the ring is loaded with the text, the symbols go to the text as bytes) up to a block
//            boundary from which the chain goes on.  Errors and the two ends (input, room) are found by this wave only.
//   resolve  every confirmed chunk replaces the markers in front of its last 32 KiB from the final text before it.
//   crc      pieces of IST_PIECE bytes of the final text are checksummed a wave each and folded behind crc_in.
// Speculation costs time, never correctness: nothing that a chunk decoded is used unless the chain reached its first bit.
//
// Bounds: a symbol is stored only below the room it is decoded into (the chunk's room, or the text capacity); reads of
// the stream beyond n_stream give zero bits, and a decision that took such bits is "the input ends here", never an
// error; every loop of the decode advances the bit position or ends.
//
// Compiled for gfx950 and, with -DATR_HOST_EMU, for the CPU twin (tests/emu/emu_gunzip_stream.cpp).
#ifndef ATR_INFLATE_STREAM_CORE_HPP
#define ATR_INFLATE_STREAM_CORE_HPP

#include <stdint.h>

#include "inflate_core.hpp"

namespace atr {

enum {
    IST_WINDOW = 32768,
    IST_RING = 32768 + 512,         // slots of the ring: a match of 258 never meets its own source (32768 + 258 at the least)
    IST_PIECE = 16384,              // bytes of text per CRC piece: 256 per lane
    IST_MIN_CHUNK = 64, IST_MAX_CHUNK = 1 << 24,
    IST_MAX_STREAM = 1 << 28,       // bytes of a slab: bit positions stay below 2^31
    IST_NEED_INPUT = 101,           // status: not one block ends inside the slab
    IST_NEED_ROOM = 102,            // status: not one block's text fits text_capacity
    IST_S_INPUT = 200, IST_S_ROOM = 201, IST_S_HANDOFF = 202, IST_S_FINAL = 203,    // (how a run ended; never a status)
    IST_F_FINAL = 1, IST_F_INPUT = 2,
    IST_R_STATUS = 0, IST_R_END_BIT, IST_R_TEXT_LEN, IST_R_FINAL, IST_R_CRC, IST_R_CHUNKS, IST_R_CONFIRMED, IST_R_REDECODED,
    IST_R_WORDS = 8, IST_W_BAD = 8, IST_STATE_WORDS = 16,
    IST_SLACK = 1024,               // symbols of room every chunk has beyond its share
};
#define IST_NONE 0xffffffffu

struct IstLds : InfTables {
    uint16_t ring[IST_RING];
};

// where everything lies in the workspace
struct IstPlan {
    int64_t n_max;           // chunks the arrays hold
    int64_t sym_cap;         // symbols the chunks share in proportion to their bits: twice the text capacity
    int64_t n_pieces;
    int64_t cand_at, end_at, len_at, flags_at, place_at, base_at, piece_at, sym_at, bytes;
};

GZ_HD IstPlan ist_plan(int64_t n_stream, int64_t chunk_bytes, int64_t capacity) {
    IstPlan p;
    p.n_max = n_stream / chunk_bytes + 2;
    p.sym_cap = 2 * capacity;
    p.n_pieces = capacity / IST_PIECE + 1;
    const int64_t words = (p.n_max * 4 + 15) / 16 * 16;
    p.cand_at = IST_STATE_WORDS * 8;
    p.end_at = p.cand_at + words;
    p.len_at = p.end_at + words;
    p.flags_at = p.len_at + words;
    p.place_at = p.flags_at + words;
    p.base_at = p.place_at + 2 * words;
    p.piece_at = p.base_at + 2 * words;
    p.sym_at = p.piece_at + (p.n_pieces * 4 + 15) / 16 * 16;
    p.bytes = p.sym_at + (p.sym_cap + p.n_max * IST_SLACK) * 2;
    return p;
}

// chunks of a call: chunk i begins at bit start_bit + i * 8 * chunk_bytes
GZ_HD int64_t ist_chunks(int64_t n_stream, int64_t start_bit, int64_t chunk_bytes) {
    const int64_t bits = 8 * n_stream - start_bit, cbits = 8 * chunk_bytes;
    return bits <= 0 ? 1 : (bits + cbits - 1) / cbits;
}

// what a call is given, and its arrays in the workspace
struct IstCall {
    const uint8_t *src;
    uint32_t n_stream, start_bit, cbits, n_chunks;
    const uint8_t *window;
    uint32_t window_len, capacity;
    uint64_t sym_cap;
    uint8_t *text;
    int64_t *state;
    uint32_t *cand, *end_bit, *len, *flags, *piece;
    int64_t *place, *base;
    uint16_t *sym;
};

GZ_HD IstCall ist_call(const uint8_t *src, int64_t n_stream, int64_t start_bit, const uint8_t *window, int32_t window_len,
                       uint8_t *text, int64_t capacity, int64_t chunk_bytes, void *workspace) {
    const IstPlan p = ist_plan(n_stream, chunk_bytes, capacity);
    uint8_t *w = (uint8_t *)workspace;
    IstCall c;
    c.src = src;
    c.n_stream = (uint32_t)n_stream;
    c.start_bit = (uint32_t)start_bit;
    c.cbits = (uint32_t)(8 * chunk_bytes);
    c.n_chunks = (uint32_t)ist_chunks(n_stream, start_bit, chunk_bytes);
    c.window = window;
    c.window_len = (uint32_t)window_len;
    c.capacity = (uint32_t)capacity;
    c.sym_cap = (uint64_t)p.sym_cap;
    c.text = text;
    c.state = (int64_t *)w;
    c.cand = (uint32_t *)(w + p.cand_at);
    c.end_bit = (uint32_t *)(w + p.end_at);
    c.len = (uint32_t *)(w + p.len_at);
    c.flags = (uint32_t *)(w + p.flags_at);
    c.place = (int64_t *)(w + p.place_at);
    c.base = (int64_t *)(w + p.base_at);
    c.piece = (uint32_t *)(w + p.piece_at);
    c.sym = (uint16_t *)(w + p.sym_at);
    return c;
}

// ---------------------------------------------------------------------------------------------- find
// the 32 bits at bitpos, least significant first, read byte by byte (a lane of its own); zero beyond the stream
ATR_DEV uint32_t ist_bits(const uint8_t *src, uint32_t n, uint32_t bitpos) {
    const uint32_t b = bitpos >> 3;
    uint64_t v = 0;
    for (uint32_t k = 0; k < 5; ++k)
        if (b + k < n) v |= (uint64_t)src[b + k] << (8 * k);
    return (uint32_t)(v >> (bitpos & 7u));
}

// May a non-final dynamic block begin at this bit?  BFINAL 0, BTYPE 10, HLIT <= 286, HDIST <= 30, the header inside the
// stream, and the Kraft sum of the code-length code exactly one.
ATR_DEV bool ist_probe(const uint8_t *src, uint32_t n, uint32_t bit) {
    uint32_t v = ist_bits(src, n, bit);
    if ((v & 7u) != 4u) return false;
    if (((v >> 3) & 31u) > 29u || ((v >> 8) & 31u) > 29u) return false;
    const uint32_t hclen = ((v >> 13) & 15u) + 4u;
    if (bit + 17u + 3u * hclen > 8u * n) return false;
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        if (i % 8 == 0) v = ist_bits(src, n, bit + 17u + 3u * i);
        const uint32_t l = v & 7u;
        v >>= 3;
        if (l) kraft += 128u >> l;
    }
    return kraft == 128u;
}

// the wave reads the header at `bit` as the decoder would: the code lengths, an end-of-block code, a complete
// literal/length code (zlib never writes another), a distance code that is complete, single or empty
ATR_DEV bool ist_verify(InfTables *L, const InfCtx &c, InfWave &W, uint32_t bit) {
    uint32_t bitpos = bit + 3, hlit = 0, hdist = 0;
    if (inf_dynamic(c, W, bitpos, 8u * c.msize, hlit, hdist)) return false;
    if (inf_build(L, W, INF_T_LL, L->seq, hlit) != INF_B_COMPLETE) return false;
    const int b = inf_build(L, W, INF_T_D, L->seq + hlit, hdist);
    return b != INF_B_OVER && b != INF_B_INCOMPLETE;
}

// chunk i: its arrays are reset and its candidate is looked for
ATR_DEV void ist_find(InfTables *L, const IstCall &k, uint32_t i) {
    INF_LANE0(k.end_bit[i] = 0; k.len[i] = 0; k.flags[i] = 0; k.place[i] = -1; if (i == 0) k.state[IST_W_BAD] = 0)
    uint32_t found = IST_NONE;
    if (i == 0) found = k.start_bit;
    else {
        InfCtx c;
        c.L = L;
        c.src = k.src;
        c.msize = k.n_stream;
        c.dst = 0;
        c.n_out = 0;
        InfWave W;
        W.cbase = 0xffffffffu;
        const uint32_t endbits = 8u * k.n_stream, lo = k.start_bit + i * k.cbits;
        const uint32_t hi = endbits - lo < k.cbits ? endbits : lo + k.cbits;
        for (uint32_t base = lo; base < hi && found == IST_NONE; base += INF_NT) {
            unsigned long long mask = 0;
#ifdef ATR_HOST_EMU
            INF_LANES(if (base + (uint32_t)lane < hi && ist_probe(k.src, k.n_stream, base + (uint32_t)lane)) mask |= 1ull << lane)
#else
            INF_LANES(mask = __ballot(base + (uint32_t)lane < hi && ist_probe(k.src, k.n_stream, base + (uint32_t)lane)))
#endif
            while (mask) {
                const uint32_t b = (uint32_t)__builtin_ctzll(mask);
                mask &= mask - 1;
                if (ist_verify(L, c, W, base + b)) { found = base + b; break; }
            }
        }
    }
    INF_LANE0(k.cand[i] = found)
}

// ---------------------------------------------------------------------------------------------- decode
struct IstOut {
    uint16_t *sym;           // the symbols go here (speculative) ...
    uint8_t *bytes;          // ... or, not null: the window is known, they are bytes and go here
    uint32_t room;           // at most this many
    uint32_t lo;             // known window: ring positions below this hold no text (IST_WINDOW - bytes of text before)
};

#define IST_PUT(o, p, s) { if ((o).bytes) (o).bytes[p] = (uint8_t)(s); else (o).sym[p] = (uint16_t)(s); }

// The tokens of a coded block up to its end-of-block.  pos: symbols so far; ring position = pos + IST_WINDOW, so that
// the positions below IST_WINDOW are the window before the run: markers, or (known) the text loaded there.
// -> INF_OK, INF_E_*, IST_S_INPUT (bits from beyond the stream were taken), IST_S_ROOM
ATR_DEV int ist_tokens(IstLds *L, const InfCtx &c, InfWave &W, const IstOut &o, uint32_t &bitpos, uint32_t endbits, uint32_t &pos) {
    for (;;) {
        uint32_t v = inf_peek(c, W, bitpos);
        uint32_t s, len;
        INF_DECODE(INF_T_LL, v, s, len)
        bitpos += len;
        if (bitpos > endbits || (s == 0xffffu && bitpos == endbits)) return IST_S_INPUT;
        if (s < 256) {
            if (pos >= o.room) return IST_S_ROOM;
            INF_LANE0(L->ring[(pos + IST_WINDOW) % IST_RING] = (uint16_t)s; IST_PUT(o, pos, s))
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
        bitpos += len;
        if (bitpos > endbits || (s == 0xffffu && bitpos == endbits)) return IST_S_INPUT;
        if (s >= 30) return INF_E_SYMBOL;
        v >>= len;
        uint32_t d = s + 1;                                // the distance, 1 .. 32768
        if (s >= 4) {
            const uint32_t eb = (s >> 1) - 1;
            d = 1 + ((2 + (s & 1u)) << eb) + (v & ((1u << eb) - 1u));
            bitpos += eb;
        }
        if (bitpos > endbits) return IST_S_INPUT;
        const uint32_t q = pos + IST_WINDOW, from = q - d;
        if (from < o.lo) return INF_E_DISTANCE;
        if (n > o.room - pos) return IST_S_ROOM;
        INF_SYNC();                                        // (the symbols before pos are stored)
        const bool known = o.bytes != 0;
        INF_LANES(
            for (uint32_t k = (uint32_t)lane; k < n; k += INF_NT) {
                const uint32_t at = from + (d >= n ? k : k % d);
                const uint32_t x = at < IST_WINDOW && !known ? 0x8000u | (IST_WINDOW - 1u - at) : L->ring[at % IST_RING];
                L->ring[(q + k) % IST_RING] = (uint16_t)x;
                IST_PUT(o, pos + k, x)
            }
        )
        pos += n;
    }
}

// Blocks from bit0 on.  self: the chunk that decodes (a later chunk whose candidate is the bit behind a block ends the
// run), or IST_NONE: the chain's own decode (that chunk must also have got on from there).
// end_bit / len: the last block boundary and the symbols before it; -> IST_S_*, or the INF_E_* of the block behind it.
ATR_DEV int ist_run(IstLds *L, const IstCall &k, const IstOut &o, uint32_t bit0, uint32_t self, uint32_t &end_bit, uint32_t &len) {
    InfCtx c;
    c.L = L;
    c.src = k.src;
    c.msize = k.n_stream;
    c.dst = 0;
    c.n_out = 0;
    InfWave W;
    W.cbase = 0xffffffffu;
    const uint32_t endbits = 8u * k.n_stream;
    uint32_t bitpos = bit0, pos = 0;
    end_bit = bit0;
    len = 0;
    for (;;) {
        uint32_t v = inf_peek(c, W, bitpos);
        bitpos += 3;
        if (bitpos > endbits) return IST_S_INPUT;
        const uint32_t bfinal = v & 1u, btype = (v >> 1) & 3u;
        if (btype == 3) return INF_E_BTYPE;
        if (btype == 0) {
            bitpos = (bitpos + 7u) & ~7u;
            v = inf_peek(c, W, bitpos);
            bitpos += 32;
            if (bitpos > endbits) return IST_S_INPUT;
            const uint32_t n = v & 0xffffu, at = bitpos >> 3;
            if ((v >> 16) != (~n & 0xffffu)) return INF_E_STORED;
            if (n > k.n_stream - at) return IST_S_INPUT;
            if (n > o.room - pos) return IST_S_ROOM;
            INF_SYNC();
            INF_LANES(
                for (uint32_t j = (uint32_t)lane; j < n; j += INF_NT) {
                    const uint32_t x = k.src[at + j];
                    L->ring[(pos + IST_WINDOW + j) % IST_RING] = (uint16_t)x;
                    IST_PUT(o, pos + j, x)
                }
            )
            pos += n;
            bitpos += 8 * n;
        } else {
            uint32_t hlit = INF_LL, hdist = INF_D;
            if (btype == 1) inf_fixed(L);
            else {
                const int st = inf_dynamic(c, W, bitpos, endbits, hlit, hdist);
                if (st) return bitpos > endbits ? (int)IST_S_INPUT : st;
            }
            int b = inf_build(L, W, INF_T_LL, L->seq, hlit);
            if (b == INF_B_OVER || b == INF_B_INCOMPLETE) return INF_E_LENGTHS;
            b = inf_build(L, W, INF_T_D, L->seq + hlit, hdist);
            if (b == INF_B_OVER || b == INF_B_INCOMPLETE) return INF_E_LENGTHS;
            const int st = ist_tokens(L, c, W, o, bitpos, endbits, pos);
            if (st) return st;
        }
        end_bit = bitpos;
        len = pos;
        if (bfinal) return IST_S_FINAL;
        const uint32_t j = (bitpos - k.start_bit) / k.cbits;
        if (j < k.n_chunks && j != self && k.cand[j] == bitpos && (self != IST_NONE || k.end_bit[j] > bitpos)) return IST_S_HANDOFF;
    }
}

// Chunk i decodes from its candidate into its room.  The rooms follow the bits: the symbols are shared out in proportion
// to the distance to the next candidate (twice the text capacity over the whole slab), IST_SLACK on top for each.
ATR_DEV void ist_decode(IstLds *L, const IstCall &k, uint32_t i) {
    const uint32_t bit0 = k.cand[i];
    if (bit0 == IST_NONE) return;
    const uint32_t endbits = 8u * k.n_stream;
    uint32_t next = endbits;
    for (uint32_t j = i + 1; j < k.n_chunks; ++j)
        if (k.cand[j] != IST_NONE) { next = k.cand[j]; break; }
    const uint64_t total = endbits > k.start_bit ? endbits - k.start_bit : 1u;
    const uint64_t b0 = (uint64_t)(bit0 - k.start_bit) * k.sym_cap / total + (uint64_t)i * IST_SLACK;
    const uint64_t b1 = (uint64_t)(next - k.start_bit) * k.sym_cap / total + (uint64_t)i * IST_SLACK + IST_SLACK;
    IstOut o;
    o.sym = k.sym + b0;
    o.bytes = 0;
    o.room = b1 - b0 < 0x7fffffffu ? (uint32_t)(b1 - b0) : 0x7fffffffu;
    o.lo = 0;
    uint32_t end_bit, len;
    const int st = ist_run(L, k, o, bit0, i, end_bit, len);
    INF_LANE0(k.base[i] = (int64_t)b0; k.end_bit[i] = end_bit; k.len[i] = len; k.flags[i] = st == IST_S_FINAL ? IST_F_FINAL : st == IST_S_INPUT ? IST_F_INPUT : 0)
}

// ---------------------------------------------------------------------------------------------- chain
// the byte `dist` before text position t (dist <= t + window_len)
ATR_DEV uint32_t ist_before(const IstCall &k, uint32_t t, uint32_t dist) {
    return dist <= t ? k.text[t - dist] : k.window[k.window_len - (dist - t)];
}

// symbols [p0, p1) of confirmed chunk j, whose text begins at t, as bytes into the text; -> a marker reached before the text
ATR_DEV bool ist_resolve(const IstCall &k, uint32_t j, uint32_t t, uint32_t p0, uint32_t p1, int lane) {
    const uint16_t *sym = k.sym + k.base[j];
    bool bad = false;
    for (uint32_t p = p0 + (uint32_t)lane; p < p1; p += INF_NT) {
        uint32_t x = sym[p];
        if (x & 0x8000u) {
            const uint32_t dist = (x & 0x7fffu) + 1u;
            if (dist > t + k.window_len) { bad = true; x = 0; }
            else x = ist_before(k, t, dist);
        }
        k.text[t + p] = (uint8_t)x;
    }
    return bad;
}

ATR_DEV void ist_chain(IstLds *L, const IstCall &k) {
    uint32_t E = k.start_bit, T = 0, confirmed = 0, redecoded = 0, final = 0;
    bool zero = false;                                     // (chunk 0 is confirmed by definition, used or not)
    int status = INF_OK;
    for (;;) {
        const uint32_t j = (E - k.start_bit) / k.cbits;
        if (j < k.n_chunks && k.cand[j] == E && k.end_bit[j] > E && k.len[j] <= k.capacity - T) {
            const uint32_t n = k.len[j], tail = n < IST_WINDOW ? n : (uint32_t)IST_WINDOW;
            INF_SYNC();
            INF_LANE0(k.place[j] = T; L->cnt[0] = 0)
            INF_SYNC();
            INF_LANES(if (ist_resolve(k, j, T, n - tail, n, lane)) L->cnt[0] = 1)
            INF_SYNC();                                    // (the window behind the chunk is final text)
            ++confirmed;
            zero |= j == 0;
            if (INF_UNIFORM(L->cnt[0])) { status = INF_E_DISTANCE; break; }
            T += n;
            E = k.end_bit[j];
            if (k.flags[j] & IST_F_FINAL) { final = 1; break; }
            if (k.flags[j] & IST_F_INPUT) break;           // (the block at E does not end inside the slab)
            continue;
        }
        // nothing usable starts here: decode on with the window that is known
        const uint32_t have = T + k.window_len < IST_WINDOW ? T + k.window_len : (uint32_t)IST_WINDOW;
        INF_SYNC();
        INF_LANES(for (uint32_t t = (uint32_t)lane; t < have; t += INF_NT) L->ring[IST_WINDOW - have + t] = (uint16_t)ist_before(k, T, have - t))
        INF_SYNC();
        IstOut o;
        o.sym = 0;
        o.bytes = k.text + T;
        o.room = k.capacity - T;
        o.lo = IST_WINDOW - have;
        uint32_t e2, n2;
        const int st = ist_run(L, k, o, E, IST_NONE, e2, n2);
        INF_SYNC();
        if (e2 > E) ++redecoded;
        T += n2;
        E = e2;
        if (st == IST_S_FINAL) { final = 1; break; }
        if (st == IST_S_HANDOFF) continue;
        if (st == IST_S_INPUT || st == IST_S_ROOM) {
            if (E == k.start_bit) status = st == IST_S_INPUT ? IST_NEED_INPUT : IST_NEED_ROOM;
            break;
        }
        status = st;
        break;
    }
    INF_LANE0(
        k.state[IST_R_STATUS] = status; k.state[IST_R_END_BIT] = E; k.state[IST_R_TEXT_LEN] = T; k.state[IST_R_FINAL] = final;
        k.state[IST_R_CHUNKS] = k.n_chunks; k.state[IST_R_CONFIRMED] = confirmed + (zero ? 0 : 1); k.state[IST_R_REDECODED] = redecoded;
    )
}

// ---------------------------------------------------------------------------------------------- resolve, crc
// chunk j, if confirmed: the symbols in front of its last 32 KiB
ATR_DEV void ist_resolve_chunk(const IstCall &k, uint32_t j) {
    const int64_t t = k.place[j];
    if (t < 0 || k.len[j] <= IST_WINDOW) return;
    INF_LANES(if (ist_resolve(k, j, (uint32_t)t, 0, k.len[j] - IST_WINDOW, lane)) k.state[IST_W_BAD] = 1)
}

// piece i of the text: its CRC register from zero, taken as the LAST bytes of IST_PIECE (inflate_core.hpp: inf_crc)
ATR_DEV void ist_crc_piece(InfTables *L, const IstCall &k, uint32_t i) {
    const int64_t total = k.state[IST_R_TEXT_LEN];
    const int64_t lo = (int64_t)i * IST_PIECE;
    if (k.state[IST_R_STATUS] != INF_OK || lo >= total) return;
    const uint32_t n = total - lo < IST_PIECE ? (uint32_t)(total - lo) : (uint32_t)IST_PIECE, off = IST_PIECE - n;
    const uint8_t *text = k.text + lo;
    enum { RANGE = IST_PIECE / INF_NT };
    INF_LANES(
        uint32_t v = (uint32_t)lane * RANGE;
        const uint32_t end = v + RANGE;
        uint32_t crc = 0;
        if (v < off) v = off;
        for (; v < end; ++v) crc = L->crc_tab[(crc ^ text[v - off]) & 0xffu] ^ (crc >> 8);
        L->lane_a[lane] = crc;
    )
    INF_SYNC();
    for (int j = 0; j < 6; ++j) {
        const int stride = 1 << j;
        INF_LANES(
            if ((lane & (2 * stride - 1)) == 0) L->lane_a[lane] = gz_mulmod(gz_x8(8 + j), L->lane_a[lane]) ^ L->lane_a[lane + stride];
        )
        INF_SYNC();
    }
    INF_LANE0(k.piece[i] = L->lane_a[0])
}

// the result words: the state, a marker that resolve found before the text, the pieces folded behind crc_in
ATR_DEV void ist_finish(const IstCall &k, uint32_t crc_in, int64_t *result) {
    int64_t status = k.state[IST_R_STATUS];
    if (status == INF_OK && k.state[IST_W_BAD]) status = INF_E_DISTANCE;
    uint32_t reg = crc_in ^ 0xffffffffu;
    if (status == INF_OK) {
        const int64_t total = k.state[IST_R_TEXT_LEN];
        for (int64_t i = 0; i * IST_PIECE < total; ++i) {
            const int64_t n = total - i * IST_PIECE < IST_PIECE ? total - i * IST_PIECE : (int64_t)IST_PIECE;
            reg = gz_crc_advance(reg, (uint32_t)n) ^ k.piece[i];
        }
    }
    for (int w = 0; w < IST_R_WORDS; ++w) result[w] = k.state[w];
    result[IST_R_STATUS] = status;
    result[IST_R_CRC] = reg ^ 0xffffffffu;
}

// the arguments of a call: -> ATR_OK (0), -1 invalid, -2 outside the envelope
GZ_HD int ist_args(int64_t n_stream, int64_t start_bit, int32_t window_len, int64_t capacity, int64_t chunk_bytes) {
    if (n_stream < 0 || start_bit < 0 || start_bit > 8 * n_stream || window_len < 0 || window_len > IST_WINDOW || capacity < 0 ||
        chunk_bytes < IST_MIN_CHUNK)
        return -1;
    if (n_stream >= IST_MAX_STREAM || capacity >= ((int64_t)1 << 31) || chunk_bytes > IST_MAX_CHUNK) return -2;
    return 0;
}

}  // namespace atr
#endif

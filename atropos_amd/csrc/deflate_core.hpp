// deflate_core.hpp -- per-block arithmetic of the device gzip compressor (gzip_kernels.hip): one BGZF member
// (RFC 1952 with the 6-byte 'BC' extra field, RFC 1951 body) per 65 280 bytes of text.
//
// A block is worked on by GZ_NT lanes in PHASES; inside a phase the lanes are independent of each other, between
// two phases stands a barrier.  gz_encode_block() is the one list of phases: the kernel runs it with a lane per
// thread and __syncthreads() as the barrier, the CPU emulation (tests/emu/emu_gzip.cpp, -DATR_HOST_EMU) runs every
// phase as a loop over the lanes.  What a phase leaves behind does not depend on the order of its lanes (the only
// concurrent updates are integer max / add / or), so the member's bytes are a function of the text alone.
//
//   load      text -> LDS, tables cleared, the member's 64 KiB slot zeroed
//   crc       a table CRC per lane over 128 bytes, folded pairwise with the fixed "advance by 128 * 2^j bytes" multipliers
//   match     tiles of GZ_NT positions: every lane looks its 4-byte hash up in the position table AS IT STOOD AFTER THE
//             TILE BEFORE and extends the candidate, and probes distance 1 (quality runs) | barrier | every lane
//             enters its position with an integer max | barrier
//   parse     greedy, a lane per 512-byte segment (a match ends at its segment's end): token starts and the
//             literal/length histogram; the distance histogram in a pass over all positions
//   codes     rank sort, Moffat-Katajainen code lengths, the limit (15 / 7), canonical codes, the code-length code
//             and the block header
//   layout    bits per lane range, their running sum, coded or stored
//   pack      every lane writes the tokens of its 128 positions at its bit offset: whole words with plain stores,
//             the two words it shares with its neighbours with an integer or
//
// Compiled for gfx950 and, with -DATR_HOST_EMU, for the CPU test emulation (tests/emu).
#ifndef ATR_DEFLATE_CORE_HPP
#define ATR_DEFLATE_CORE_HPP

#include <stdint.h>

#ifdef ATR_HOST_EMU
#ifndef ATR_DEV
#define ATR_DEV static inline
#endif
#define GZ_HD static inline
#define GZ_ATOMIC_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define GZ_ATOMIC_ADD(p, v) (*(p) += (v))
#define GZ_ATOMIC_OR(p, v) (*(p) |= (v))
#define GZ_PHASE(body) for (int lane = 0; lane < GZ_NT; ++lane) { body; }
#else
#ifndef ATR_DEV
#define ATR_DEV __device__ __forceinline__
#endif
#define GZ_HD __host__ __device__ static inline
#define GZ_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define GZ_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define GZ_ATOMIC_OR(p, v) atomicOr((p), (v))
#define GZ_PHASE(body) { const int lane = (int)threadIdx.x; body; } __syncthreads();
#endif

namespace atr {

enum {
    GZ_BLOCK = 0xff00,        // input bytes per member (bgzip's block size)
    GZ_SLOT = 65536,          // a member is at most this long; the work buffer holds one slot per member
    GZ_NT = 512,              // lanes per block
    GZ_RANGE = GZ_SLOT / GZ_NT,   // positions a lane packs
    GZ_SEG = 512,             // positions a lane parses; a match does not cross a segment's end
    GZ_HASH_BITS = 14,
    GZ_WINDOW = 32768,
    GZ_MIN_MATCH = 3,
    GZ_MAX_MATCH = 258,
    GZ_HEADER = 18,           // 12 bytes of gzip header with FEXTRA + the 6-byte BC subfield
    GZ_TRAILER = 8,           // CRC32, ISIZE
    GZ_STORED_OVERHEAD = GZ_HEADER + 5 + GZ_TRAILER,     // 31: what a stored member adds to its input
    GZ_LL = 288, GZ_D = 32, GZ_SYMS = GZ_LL + GZ_D, GZ_EOB = 256,
    GZ_MAX_GRID = 512,        // workgroups of a launch; each owns one match array
};

GZ_HD int64_t gz_nblocks(int64_t n) { return (n + GZ_BLOCK - 1) / GZ_BLOCK; }
GZ_HD int64_t gz_bound(int64_t n) { return n + gz_nblocks(n) * GZ_STORED_OVERHEAD; }
GZ_HD int64_t gz_grid(int64_t n) { const int64_t nb = gz_nblocks(n); return nb < GZ_MAX_GRID ? (nb > 0 ? nb : 1) : GZ_MAX_GRID; }
// work buffer: [slots][sizes u32][offsets i64][match arrays u32 x 65536 per workgroup]
GZ_HD int64_t gz_work_sizes_at(int64_t n) { return gz_nblocks(n) * GZ_SLOT; }
GZ_HD int64_t gz_work_offsets_at(int64_t n) { return gz_work_sizes_at(n) + (gz_nblocks(n) * 4 + 15) / 16 * 16; }
GZ_HD int64_t gz_work_match_at(int64_t n) { return gz_work_offsets_at(n) + (gz_nblocks(n) + 1) * 8 + 8; }
GZ_HD int64_t gz_work_bytes(int64_t n) { return gz_work_match_at(n) + gz_grid(n) * (int64_t)GZ_SLOT * 4; }

// the 28-byte BGZF end-of-file member
GZ_HD void gz_eof_member(uint8_t *out) {
    const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 28; ++i) out[i] = eof[i];
}

// ---------------------------------------------------------------------------------------------- CRC32
// Reflected CRC-32 (0xEDB88320).  A register value is a polynomial over GF(2), bit 31 = x^0.
ATR_DEV uint32_t gz_crc_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i >> 1) ^ (0xedb88320u & (0u - (i & 1u)));
    return i;
}

ATR_DEV uint32_t gz_mulmod(uint32_t a, uint32_t b) {          // a * b mod P
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (0xedb88320u & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 * 2^k) mod P: "advance the register by 2^k bytes" is a multiplication by entry k (made on the host, once)
ATR_DEV uint32_t gz_x8(int k) {
    static const uint32_t t[17] = {0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u, 0xed627daeu,
                                   0x88d14467u, 0xd7bbfe6au, 0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u,
                                   0x09fe548fu, 0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u, 0x31fec169u};
    return t[k];
}

ATR_DEV uint32_t gz_crc_advance(uint32_t v, uint32_t nbytes) {
    for (int k = 0; nbytes; ++k, nbytes >>= 1)
        if (nbytes & 1u) v = gz_mulmod(gz_x8(k), v);
    return v;
}

// ---------------------------------------------------------------------------------------------- symbols
ATR_DEV uint32_t gz_len_sym(uint32_t len, uint32_t &ebits, uint32_t &eval) {      // len 3 .. 258
    const uint32_t t = len - 3;
    if (len == 258) { ebits = 0; eval = 0; return 285; }
    if (t < 8) { ebits = 0; eval = 0; return 257 + t; }
    const uint32_t eb = (31u - (uint32_t)__builtin_clz(t)) - 2u;
    ebits = eb;
    eval = t & ((1u << eb) - 1u);
    return 261 + 4 * eb + ((t >> eb) & 3u);
}

ATR_DEV uint32_t gz_dist_sym(uint32_t dist, uint32_t &ebits, uint32_t &eval) {    // dist 1 .. 32768
    const uint32_t t = dist - 1;
    if (t < 4) { ebits = 0; eval = 0; return t; }
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(t);
    ebits = hb - 1;
    eval = t & ((1u << (hb - 1)) - 1u);
    return 2 * hb + ((t >> (hb - 1)) & 1u);
}

ATR_DEV uint32_t gz_bitrev(uint32_t v, uint32_t nbits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < nbits; ++i) r |= ((v >> i) & 1u) << (nbits - 1 - i);
    return r;
}

// ---------------------------------------------------------------------------------------------- code lengths
// Minimum-redundancy code lengths (Moffat & Katajainen, in place) over the n frequencies key[] in ascending order,
// then limited to maxbits by moving codes down the length histogram until the Kraft sum is exactly one.
// sym[i]: the symbol of key[i]; len_out[symbol] is written for the n symbols; blc[1 .. maxbits]: codes per length.
ATR_DEV void gz_build_lengths(uint32_t *key, const uint16_t *sym, int n, int maxbits, uint8_t *len_out, uint32_t *blc) {
    for (int i = 0; i < 16; ++i) blc[i] = 0;
    if (n == 0) return;
    if (n == 1) { len_out[sym[0]] = 1; blc[1] = 1; return; }
    key[0] += key[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || key[root] < key[leaf]) { key[next] = key[root]; key[root++] = (uint32_t)next; }
        else key[next] = key[leaf++];
        if (leaf >= n || (root < next && key[root] < key[leaf])) { key[next] += key[root]; key[root++] = (uint32_t)next; }
        else key[next] += key[leaf++];
    }
    key[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) key[next] = key[key[next]] + 1;
    int avbl = 1, used = 0, dpth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && (int)key[root] == dpth) { ++used; --root; }
        while (avbl > used) { key[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
    for (int i = 0; i < n; ++i) blc[key[i] > (uint32_t)maxbits ? (uint32_t)maxbits : key[i]]++;
    uint32_t total = 0;
    for (int i = maxbits; i > 0; --i) total += blc[i] << (maxbits - i);
    while (total != (1u << maxbits)) {
        blc[maxbits]--;
        for (int i = maxbits - 1; i > 0; --i)
            if (blc[i]) { blc[i]--; blc[i + 1] += 2; break; }
        --total;
    }
    int j = n;
    for (int i = 1; i <= maxbits; ++i)
        for (uint32_t l = blc[i]; l > 0; --l) len_out[sym[--j]] = (uint8_t)i;
}

// canonical code of a symbol with `len` bits that has `before` lower symbols of its length, bit-reversed for an
// LSB-first bit stream
ATR_DEV uint32_t gz_canonical(const uint32_t *blc, uint32_t len, uint32_t before) {
    uint32_t code = 0;
    for (uint32_t bits = 1; bits <= len; ++bits) code = (code + (bits > 1 ? blc[bits - 1] : 0u)) << 1;
    return gz_bitrev(code + before, len);
}

// ---------------------------------------------------------------------------------------------- bit writer
// Appends bits, least significant first, to 32-bit words that start out zero.  A word that the writer fills
// completely is stored; the words at its two ends, which it may share with other writers, are or-ed in.
struct GzWriter {
    uint32_t *w;
    uint64_t acc;
    uint32_t nacc, wpos, shared;
};

ATR_DEV void gzw_init(GzWriter &s, uint32_t *words, uint32_t bitpos) {
    s.w = words;
    s.acc = 0;
    s.nacc = bitpos & 31u;
    s.wpos = bitpos >> 5;
    s.shared = s.nacc != 0;
}

ATR_DEV void gzw_put(GzWriter &s, uint32_t v, uint32_t nbits) {   // nbits <= 32, v < 2^nbits
    s.acc |= (uint64_t)v << s.nacc;
    s.nacc += nbits;
    if (s.nacc >= 32) {
        if (s.shared) GZ_ATOMIC_OR(&s.w[s.wpos], (uint32_t)s.acc);
        else s.w[s.wpos] = (uint32_t)s.acc;
        s.shared = 0;
        s.wpos++;
        s.acc >>= 32;
        s.nacc -= 32;
    }
}

ATR_DEV void gzw_flush(GzWriter &s) {
    if (s.nacc) GZ_ATOMIC_OR(&s.w[s.wpos], (uint32_t)s.acc);
    s.acc = 0;
    s.nacc = 0;
    s.shared = 1;
}

// ---------------------------------------------------------------------------------------------- the block
struct GzLds {
    uint32_t text[GZ_SLOT / 4];          // the block, zero beyond its end
    uint32_t tab[GZ_SLOT / 4];           // position + 1 by hash; after the match tiles: a length byte per position
    uint32_t flags[GZ_SLOT / 32];        // bit p: a token starts at p
    uint32_t crc_tab[256];
    uint32_t lane_a[GZ_NT];              // per lane: CRC, then bits of its range, then its bit offset
    uint32_t freq[GZ_SYMS];              // 0 .. 287 literal/length, 288 .. 319 distance
    uint32_t skey[GZ_SYMS];              // frequencies in ascending order (per alphabet, at its base)
    uint32_t rle[GZ_SYMS];               // the code lengths as code-length symbols: symbol | extra << 8
    uint32_t hdr[160];                   // the deflate block header, as bits
    uint32_t blc[3][16];                 // codes per length: literal/length, distance, code-length
    uint32_t cl_freq[19];
    uint32_t s[16];                      // scalars, GZ_S_*
    uint16_t ssym[GZ_SYMS];
    uint16_t code[GZ_SYMS];
    uint16_t cl_code[20];
    uint8_t len[GZ_SYMS];
    uint8_t cl_len[20];
};

enum { GZ_S_CRC, GZ_S_NLL, GZ_S_ND, GZ_S_HDR_BITS, GZ_S_STORED, GZ_S_SIZE, GZ_S_NRLE };

struct GzCtx {
    GzLds *L;
    const uint8_t *src;      // the block's text
    uint32_t n;              // 1 .. GZ_BLOCK
    uint32_t *m;             // per position: length << 16 | distance of its match, or 0
    uint32_t *slot;          // the member, GZ_SLOT bytes
    uint32_t *size;          // its length
};

ATR_DEV uint32_t gz_byte(const GzLds *L, uint32_t p) { return ((const uint8_t *)L->text)[p]; }

ATR_DEV uint32_t gz_load32(const GzLds *L, uint32_t p) {      // the four bytes at p, any alignment
    const uint32_t w = p >> 2, sh = (p & 3u) * 8u;
    return (uint32_t)((((uint64_t)L->text[w + 1] << 32) | L->text[w]) >> sh);
}

ATR_DEV uint32_t gz_hash(uint32_t key) { return (key * 2654435761u) >> (32 - GZ_HASH_BITS); }

// bytes that text[a ..] and text[b ..] have in common, at most maxlen
ATR_DEV uint32_t gz_extend(const GzLds *L, uint32_t a, uint32_t b, uint32_t maxlen) {
    uint32_t k = 0;
    while (k < maxlen) {
        const uint32_t x = gz_load32(L, a + k) ^ gz_load32(L, b + k);
        if (x) { k += (uint32_t)__builtin_ctz(x) >> 3; break; }
        k += 4;
    }
    return k < maxlen ? k : maxlen;
}

// A hashed match pays for its distance's extra bits only when it is long enough.
ATR_DEV bool gz_worth(uint32_t len, uint32_t dist) {
    return len >= 4u + (dist > 256u) + (dist > 4096u) + (dist > 16384u);
}

ATR_DEV void gz_p_load(const GzCtx &c, int lane) {
    GzLds *L = c.L;
    const bool aligned = ((uintptr_t)c.src & 3u) == 0;
    for (uint32_t w = (uint32_t)lane; w < GZ_SLOT / 4; w += GZ_NT) {
        const uint32_t base = 4 * w;
        uint32_t v = 0;
        if (base + 4 <= c.n && aligned) v = *(const uint32_t *)(c.src + base);
        else
            for (uint32_t k = 0; k < 4 && base + k < c.n; ++k) v |= (uint32_t)c.src[base + k] << (8 * k);
        L->text[w] = v;
        L->tab[w] = 0;
        c.slot[w] = 0;
    }
    for (uint32_t w = (uint32_t)lane; w < GZ_SLOT / 32; w += GZ_NT) L->flags[w] = 0;
    if (lane < GZ_SYMS) { L->freq[lane] = 0; L->len[lane] = 0; L->code[lane] = 0; }
    if (lane < 256) L->crc_tab[lane] = gz_crc_entry((uint32_t)lane);
}

// The block is taken as the LAST n bytes of GZ_SLOT: zero bytes in front of a message leave a register that starts
// at zero unchanged, so every lane's 128 bytes sit a fixed number of bytes before the end.
ATR_DEV void gz_p_crc(const GzCtx &c, int lane) {
    const GzLds *L = c.L;
    const uint32_t off = GZ_SLOT - c.n;
    uint32_t v = (uint32_t)lane * GZ_RANGE, end = v + GZ_RANGE, crc = 0;
    if (v < off) v = off;
    for (; v < end; ++v) crc = L->crc_tab[(crc ^ gz_byte(L, v - off)) & 0xffu] ^ (crc >> 8);
    c.L->lane_a[lane] = crc;
}

ATR_DEV void gz_p_crc_level(const GzCtx &c, int lane, int j) {
    GzLds *L = c.L;
    const int stride = 1 << j;
    if ((lane & (2 * stride - 1)) == 0) L->lane_a[lane] = gz_mulmod(gz_x8(7 + j), L->lane_a[lane]) ^ L->lane_a[lane + stride];
}

ATR_DEV void gz_p_lookup(const GzCtx &c, uint32_t p) {
    const GzLds *L = c.L;
    if (p >= c.n) return;
    const uint32_t room = c.n - p, maxlen = room < GZ_MAX_MATCH ? room : (uint32_t)GZ_MAX_MATCH;
    uint32_t best_len = 0, best_dist = 0;
    if (maxlen >= 4) {
        const uint32_t key = gz_load32(L, p), cand = L->tab[gz_hash(key)];
        if (cand) {
            const uint32_t at = cand - 1, dist = p - at;
            if (dist <= GZ_WINDOW && gz_load32(L, at) == key) {
                const uint32_t len = gz_extend(L, at, p, maxlen);
                if (gz_worth(len, dist)) { best_len = len; best_dist = dist; }
            }
        }
    }
    if (p >= 1 && maxlen >= GZ_MIN_MATCH && gz_byte(L, p - 1) == gz_byte(L, p)) {
        const uint32_t len = gz_extend(L, p - 1, p, maxlen);
        if (len >= GZ_MIN_MATCH && len >= best_len) { best_len = len; best_dist = 1; }
    }
    c.m[p] = best_len ? (best_len << 16) | best_dist : 0u;
}

ATR_DEV void gz_p_insert(const GzCtx &c, uint32_t p) {
    if (p + 4 <= c.n) GZ_ATOMIC_MAX(&c.L->tab[gz_hash(gz_load32(c.L, p))], p + 1);
}

// the table's memory becomes a byte per position: 0 no match, else min(length - 2, 255)
ATR_DEV void gz_p_lenb(const GzCtx &c, int lane) {
    uint8_t *lenb = (uint8_t *)c.L->tab;
    for (uint32_t p = (uint32_t)lane; p < c.n; p += GZ_NT) {
        const uint32_t len = c.m[p] >> 16;
        lenb[p] = (uint8_t)(len ? (len - 2 < 255 ? len - 2 : 255) : 0);
    }
}

// the match token at p, cut at the end of p's segment: its length, or 0 for a literal
ATR_DEV uint32_t gz_token_len(const GzCtx &c, uint32_t p) {
    const uint32_t v = ((const uint8_t *)c.L->tab)[p];
    if (!v) return 0;
    uint32_t len = v < 255 ? v + 2 : c.m[p] >> 16;
    uint32_t end = (p / GZ_SEG + 1) * GZ_SEG;
    if (end > c.n) end = c.n;
    if (len > end - p) len = end - p;
    return len >= GZ_MIN_MATCH ? len : 0;
}

ATR_DEV void gz_p_parse(const GzCtx &c, int lane) {
    GzLds *L = c.L;
    uint32_t p = (uint32_t)lane * GZ_SEG;
    if (p >= c.n) return;
    const uint32_t end = p + GZ_SEG < c.n ? p + GZ_SEG : c.n;
    if (lane == 0) GZ_ATOMIC_ADD(&L->freq[GZ_EOB], 1u);
    uint32_t word = 0, wi = p >> 5;                 // (a segment's flag words are its lane's own)
    while (p < end) {
        if ((p >> 5) != wi) { L->flags[wi] = word; word = 0; wi = p >> 5; }
        word |= 1u << (p & 31u);
        const uint32_t len = gz_token_len(c, p);
        if (len) {
            uint32_t eb, ev;
            GZ_ATOMIC_ADD(&L->freq[gz_len_sym(len, eb, ev)], 1u);
            p += len;
        } else {
            GZ_ATOMIC_ADD(&L->freq[gz_byte(L, p)], 1u);
            ++p;
        }
    }
    L->flags[wi] = word;
}

ATR_DEV bool gz_starts(const GzLds *L, uint32_t p) { return (L->flags[p >> 5] >> (p & 31u)) & 1u; }

ATR_DEV void gz_p_dist_hist(const GzCtx &c, int lane) {
    GzLds *L = c.L;
    for (uint32_t p = (uint32_t)lane; p < c.n; p += GZ_NT)
        if (gz_starts(L, p) && gz_token_len(c, p)) {
            uint32_t eb, ev;
            GZ_ATOMIC_ADD(&L->freq[GZ_LL + gz_dist_sym(c.m[p] & 0xffffu, eb, ev)], 1u);
        }
}

// rank sort: a lane per symbol counts the used symbols of its alphabet that come before it (frequency, then symbol)
ATR_DEV void gz_p_rank(const GzCtx &c, int lane) {
    GzLds *L = c.L;
    if (lane >= GZ_SYMS) return;
    const int base = lane < GZ_LL ? 0 : GZ_LL, count = lane < GZ_LL ? GZ_LL : GZ_D;
    const uint32_t f = L->freq[lane];
    uint32_t rank = 0, used = 0;
    for (int t = base; t < base + count; ++t) {
        const uint32_t g = L->freq[t];
        used += g != 0;
        rank += g != 0 && (g < f || (g == f && t < lane));
    }
    if (f) { L->skey[base + rank] = f; L->ssym[base + rank] = (uint16_t)lane; }
    if (lane == base) L->s[base ? GZ_S_ND : GZ_S_NLL] = used;
}

ATR_DEV void gz_p_lengths(const GzCtx &c, int lane) {
    GzLds *L = c.L;
    if (lane == 0) gz_build_lengths(L->skey, L->ssym, (int)L->s[GZ_S_NLL], 15, L->len, L->blc[0]);
    if (lane == 64) gz_build_lengths(L->skey + GZ_LL, L->ssym + GZ_LL, (int)L->s[GZ_S_ND], 15, L->len, L->blc[1]);
}

ATR_DEV void gz_p_codes(const GzCtx &c, int lane) {
    GzLds *L = c.L;
    if (lane >= GZ_SYMS) return;
    const uint32_t len = L->len[lane];
    if (!len) return;
    const int base = lane < GZ_LL ? 0 : GZ_LL;
    uint32_t before = 0;
    for (int t = base; t < lane; ++t) before += L->len[t] == len;
    L->code[lane] = (uint16_t)gz_canonical(L->blc[base ? 1 : 0], len, before);
}

// One lane: the code lengths of both alphabets as code-length symbols (runs of zeros as 17 / 18, repeats as 16),
// their code (at most 7 bits, complete), and the block header's bits.
ATR_DEV void gz_p_header(const GzCtx &c, int lane) {
    GzLds *L = c.L;
    if (lane != 0) return;
    int hlit = GZ_LL - 2, hdist = 30;                      // (286 and 30 symbols exist)
    while (hlit > 257 && !L->len[hlit - 1]) --hlit;
    while (hdist > 1 && !L->len[GZ_LL + hdist - 1]) --hdist;
    const int total = hlit + hdist;
    for (int i = 0; i < 19; ++i) { L->cl_freq[i] = 0; L->cl_len[i] = 0; L->cl_code[i] = 0; }
    int nrle = 0;
    for (int i = 0; i < total;) {
        const uint32_t v = L->len[i < hlit ? i : GZ_LL + (i - hlit)];
        int run = 1;
        while (i + run < total && L->len[(i + run) < hlit ? (i + run) : GZ_LL + (i + run - hlit)] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int r = run < 138 ? run : 138; L->rle[nrle++] = 18u | (uint32_t)(r - 11) << 8; run -= r; }
            if (run >= 3) { L->rle[nrle++] = 17u | (uint32_t)(run - 3) << 8; run = 0; }
        } else {
            L->rle[nrle++] = v;
            --run;
            while (run >= 3) { const int r = run < 6 ? run : 6; L->rle[nrle++] = 16u | (uint32_t)(r - 3) << 8; run -= r; }
        }
        while (run-- > 0) L->rle[nrle++] = v;
    }
    for (int i = 0; i < nrle; ++i) L->cl_freq[L->rle[i] & 0xffu]++;
    // sorted by (frequency, symbol); a lone symbol gets a partner, because the code-length code must be complete
    uint32_t key[19];
    uint16_t sym[19];
    int n = 0;
    for (int s = 0; s < 19; ++s) n += L->cl_freq[s] != 0;
    if (n == 1) L->cl_freq[L->cl_freq[0] ? 1 : 0] = 1;
    n = 0;
    for (int s = 0; s < 19; ++s) {
        const uint32_t f = L->cl_freq[s];
        if (!f) continue;
        int at = n++;
        while (at > 0 && key[at - 1] > f) { key[at] = key[at - 1]; sym[at] = sym[at - 1]; --at; }
        key[at] = f;
        sym[at] = (uint16_t)s;
    }
    gz_build_lengths(key, sym, n, 7, L->cl_len, L->blc[2]);
    for (int s = 0; s < 19; ++s) {
        const uint32_t len = L->cl_len[s];
        if (!len) continue;
        uint32_t before = 0;
        for (int t = 0; t < s; ++t) before += L->cl_len[t] == len;
        L->cl_code[s] = (uint16_t)gz_canonical(L->blc[2], len, before);
    }
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 19;
    while (hclen > 4 && !L->cl_len[order[hclen - 1]]) --hclen;
    for (int i = 0; i < 160; ++i) L->hdr[i] = 0;
    GzWriter w;
    gzw_init(w, L->hdr, 0);
    gzw_put(w, 5u, 3);                                     // BFINAL = 1, BTYPE = 10
    gzw_put(w, (uint32_t)(hlit - 257), 5);
    gzw_put(w, (uint32_t)(hdist - 1), 5);
    gzw_put(w, (uint32_t)(hclen - 4), 4);
    uint32_t bits = 17;
    for (int i = 0; i < hclen; ++i) gzw_put(w, L->cl_len[order[i]], 3);
    bits += 3u * (uint32_t)hclen;
    for (int i = 0; i < nrle; ++i) {
        const uint32_t s = L->rle[i] & 0xffu, extra = L->rle[i] >> 8;
        gzw_put(w, L->cl_code[s], L->cl_len[s]);
        bits += L->cl_len[s];
        const uint32_t eb = s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u;
        if (eb) { gzw_put(w, extra, eb); bits += eb; }
    }
    gzw_flush(w);
    L->s[GZ_S_HDR_BITS] = bits;
}

ATR_DEV uint32_t gz_token_bits(const GzCtx &c, uint32_t p) {
    const GzLds *L = c.L;
    const uint32_t len = gz_token_len(c, p);
    if (!len) return L->len[gz_byte(L, p)];
    uint32_t eb, ev, db, dv;
    const uint32_t ls = gz_len_sym(len, eb, ev), ds = gz_dist_sym(c.m[p] & 0xffffu, db, dv);
    return L->len[ls] + eb + L->len[GZ_LL + ds] + db;
}

ATR_DEV void gz_p_cost(const GzCtx &c, int lane) {
    const GzLds *L = c.L;
    uint32_t p = (uint32_t)lane * GZ_RANGE, bits = 0;
    const uint32_t end = p + GZ_RANGE < c.n ? p + GZ_RANGE : c.n;
    for (; p < end; ++p)
        if (gz_starts(L, p)) bits += gz_token_bits(c, p);
    c.L->lane_a[lane] = bits;
}

// One lane: every lane's bit offset, and whether the coded member is smaller than the stored one.
ATR_DEV void gz_p_layout(const GzCtx &c, int lane) {
    GzLds *L = c.L;
    if (lane != 0) return;
    uint32_t at = GZ_HEADER * 8 + L->s[GZ_S_HDR_BITS];
    for (int i = 0; i < GZ_NT; ++i) { const uint32_t b = L->lane_a[i]; L->lane_a[i] = at; at += b; }
    at += L->len[GZ_EOB];
    const uint32_t coded = (at + 7) / 8 + GZ_TRAILER, stored = c.n + GZ_STORED_OVERHEAD;
    L->s[GZ_S_STORED] = coded >= stored;
    L->s[GZ_S_SIZE] = coded >= stored ? stored : coded;
    *c.size = L->s[GZ_S_SIZE];
}

ATR_DEV void gz_p_crc_final(const GzCtx &c, int lane) {
    if (lane == 0) c.L->s[GZ_S_CRC] = c.L->lane_a[0] ^ gz_crc_advance(0xffffffffu, c.n) ^ 0xffffffffu;
}

ATR_DEV void gz_put_header(GzWriter &w, uint32_t member_size) {
    const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) gzw_put(w, h[i], 8);
    gzw_put(w, (member_size - 1) & 0xffffu, 16);
}

ATR_DEV void gz_p_pack(const GzCtx &c, int lane) {
    const GzLds *L = c.L;
    const bool stored = L->s[GZ_S_STORED] != 0;
    GzWriter w;
    if (lane == 0) {
        gzw_init(w, c.slot, 0);
        gz_put_header(w, L->s[GZ_S_SIZE]);
        if (stored) {
            gzw_put(w, 1u, 8);                             // BFINAL = 1, BTYPE = 00, padding
            gzw_put(w, c.n, 16);
            gzw_put(w, ~c.n & 0xffffu, 16);
        } else {
            const uint32_t bits = L->s[GZ_S_HDR_BITS];
            for (uint32_t i = 0; i < bits / 32; ++i) gzw_put(w, L->hdr[i], 32);
            if (bits & 31u) gzw_put(w, L->hdr[bits / 32] & ((1u << (bits & 31u)) - 1u), bits & 31u);
        }
        gzw_flush(w);
    }
    uint32_t p = (uint32_t)lane * GZ_RANGE;
    if (p > c.n) p = c.n;
    const uint32_t end = p + GZ_RANGE < c.n ? p + GZ_RANGE : c.n;
    if (stored) {
        gzw_init(w, c.slot, (GZ_HEADER + 5 + p) * 8);
        for (; p < end; ++p) gzw_put(w, gz_byte(L, p), 8);
    } else {
        gzw_init(w, c.slot, L->lane_a[lane]);
        for (; p < end; ++p) {
            if (!gz_starts(L, p)) continue;
            const uint32_t len = gz_token_len(c, p);
            if (!len) {
                const uint32_t b = gz_byte(L, p);
                gzw_put(w, L->code[b], L->len[b]);
                continue;
            }
            uint32_t eb, ev, db, dv;
            const uint32_t ls = gz_len_sym(len, eb, ev), ds = GZ_LL + gz_dist_sym(c.m[p] & 0xffffu, db, dv);
            gzw_put(w, L->code[ls] | ev << L->len[ls], L->len[ls] + eb);
            gzw_put(w, L->code[ds] | dv << L->len[ds], L->len[ds] + db);
        }
    }
    if (lane == GZ_NT - 1) {
        if (!stored) {
            gzw_put(w, L->code[GZ_EOB], L->len[GZ_EOB]);
            if (w.nacc & 7u) gzw_put(w, 0u, 8u - (w.nacc & 7u));
        }
        gzw_put(w, L->s[GZ_S_CRC], 32);
        gzw_put(w, c.n, 32);
    }
    gzw_flush(w);
}

// THE list of phases of a block.  Every lane of the block calls it (device), or the emulation calls it once.
ATR_DEV void gz_encode_block(const GzCtx &c) {
    GZ_PHASE(gz_p_load(c, lane))
    GZ_PHASE(gz_p_crc(c, lane))
    for (int j = 0; j < 9; ++j) { GZ_PHASE(gz_p_crc_level(c, lane, j)) }
    const uint32_t ntiles = (c.n + GZ_NT - 1) / GZ_NT;
    for (uint32_t t = 0; t < ntiles; ++t) {
        GZ_PHASE(gz_p_lookup(c, t * GZ_NT + (uint32_t)lane))
        GZ_PHASE(gz_p_insert(c, t * GZ_NT + (uint32_t)lane))
    }
    GZ_PHASE(gz_p_crc_final(c, lane); gz_p_lenb(c, lane))
    GZ_PHASE(gz_p_parse(c, lane))
    GZ_PHASE(gz_p_dist_hist(c, lane))
    GZ_PHASE(gz_p_rank(c, lane))
    GZ_PHASE(gz_p_lengths(c, lane))
    GZ_PHASE(gz_p_codes(c, lane))
    GZ_PHASE(gz_p_header(c, lane))
    GZ_PHASE(gz_p_cost(c, lane))
    GZ_PHASE(gz_p_layout(c, lane))
    GZ_PHASE(gz_p_pack(c, lane))
}

}  // namespace atr
#endif

// detect_core.hpp -- known-contaminant detection (the reference's KnownContaminantDetector,
// commands/detect/__init__.py:495-549): the tables the host builds from the known sequences and the
// per-read arithmetic that the kernels (detect_kernels.hip) and the CPU test emulation (tests/emu/emu_detect.cpp,
// -DATR_HOST_EMU) share.
//
// Per read (Detector._filter_seq): drop it when its complexity is <= 1.0, cut it at the first past-end match
// (`B{8,}.*|B{2,}$` for every past-end base B), drop it when what is left is shorter than kmer_size or than the
// shortest known sequence.  Per DISTINCT kept sequence and known sequence (ContaminantMatcher.match): fw / rv =
// number of distinct k-mers of the known sequence found in the read / in its reverse complement, n = max.
//
// K-mers compare as strings.  Bytes are coded as an index into the alphabet of the known sequences (their bytes
// and the complements of those); any other byte gets DET_OTHER and a k-mer that holds one matches nothing.  A
// k-mer is its codes packed `bits` per base into one 64-bit key.  A k-mer K of a known sequence occurs in the
// reverse complement of a read exactly when revcomp(K) occurs in the read (the complement is an involution on
// its domain; a K with a byte outside that domain never does), so both strands are ONE look-up of the read's
// forward k-mers in one table that holds K and revcomp(K):
//   slots    open addressing, linear probing: key, and (first posting << 12 | postings) or DET_EMPTY
//   postings (known sequence, strand, index of the k-mer among the DISTINCT k-mers of that sequence)
//   bloom    one bit per 16-bit hash prefix of every key: what the match kernel keeps in LDS; the slots and
//            postings stay in global memory and are read only for the few k-mers that pass it
#ifndef ATR_DETECT_CORE_HPP
#define ATR_DETECT_CORE_HPP

#include <stddef.h>
#include <stdint.h>

#ifdef ATR_HOST_EMU
#define DET_HD static inline
#else
#define DET_HD __host__ __device__ __forceinline__
#endif

#include <map>
#include <string>
#include <vector>

namespace atr {

constexpr int DET_MAX_READ = 320;          // longest read (the complexity table is (max_len + 1)^2 doubles)
constexpr int DET_CHUNKS = DET_MAX_READ / 64;
constexpr int DET_MAX_KMERS = 128;         // distinct k-mers per known sequence (bit set of 4 x 32)
constexpr int DET_MAX_SEQS = 2047;         // known sequences a posting can name (the LDS bound below is tighter)
constexpr int DET_MAX_PAST_END = 4;        // past-end bases
constexpr int DET_MIN_K = 4, DET_MAX_K = 32;
constexpr uint8_t DET_OTHER = 255;
constexpr uint32_t DET_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t DET_NEVER = 0xFFFFFFFFu;   // threshold of a known sequence without k-mers
constexpr int DET_BLOOM_WORDS = 2048;      // 65536 bits
constexpr int DET_STAGE = DET_MAX_READ + 32;   // bytes of a wave's code stage in LDS
constexpr int DET_MAX_LDS = 64 * 1024;     // what a block of the match kernel may take

// LDS of a block of the match kernel (four waves): bloom bits, the block's counters (20 bytes per known sequence),
// per wave the bit sets (2 * words + 1 words per known sequence) and the code stage, the byte -> code table.
// With DET_MAX_LDS this bounds the known sequences: 818 with up to 32 distinct k-mers each (words = 1), 556 up to
// 64, 421 up to 96, 339 up to 128.
static inline size_t det_lds_bytes(int nseq, int words) {
    return (size_t)DET_BLOOM_WORDS * 4 + (size_t)nseq * 8 + (size_t)nseq * 3 * 4 + (size_t)4 * nseq * (2 * words + 1) * 4 +
           256 + 4 * DET_STAGE;
}

// counter block: uint64 words; header, then matches[S], hits[S], max_n[S], abundance[S]
constexpr int DET_HDR = 8;
enum { DET_KEPT = 0, DET_DISTINCT = 1, DET_INVALID = 2, DET_OVERLONG = 3 };

// posting: known sequence (bits 0-11), strand (bit 12: 1 = reverse complement), k-mer index (bits 13-20)
DET_HD uint32_t det_posting(int seq, int strand, int kidx) { return (uint32_t)seq | ((uint32_t)strand << 12) | ((uint32_t)kidx << 13); }

DET_HD uint64_t det_mix(uint64_t x) {       // (the 64-bit finaliser of MurmurHash3)
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
DET_HD uint32_t det_bloom_bit(uint64_t h) { return (uint32_t)(h >> 48); }
DET_HD uint32_t det_slot(uint64_t h, uint32_t mask) { return (uint32_t)(h >> 16) & mask; }

// The look-up: (first posting << 12 | count) of `key`, DET_EMPTY if the table does not hold it.
DET_HD uint32_t det_lookup(const uint64_t *keys, const uint32_t *vals, uint32_t mask, uint64_t key, uint64_t h) {
    for (uint32_t s = det_slot(h, mask);; s = (s + 1) & mask) {
        const uint32_t v = vals[s];
        if (v == DET_EMPTY || keys[s] == key) return v;
    }
}

// hash of a kept sequence for the distinct pass: sum of (byte + 1) * P^position (any order), finalised with the
// length.  Equal sequences have equal hashes; the distinct pass compares the bytes of reads that share one.
constexpr uint64_t DET_P = 0x9E3779B97F4A7C15ull;
DET_HD uint64_t det_pow(uint32_t e) {
    uint64_t r = 1, b = DET_P;
    for (; e; e >>= 1, b *= b) if (e & 1) r *= b;
    return r;
}
DET_HD uint64_t det_hash_finish(uint64_t sum, int len) { return det_mix(sum + (uint64_t)len * 0xD6E8FEB86659FD93ull); }

DET_HD uint8_t det_upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }

// sequence_complexity(seq) <= 1.0 from the counts of A, C, G, T (after upper()) and the whole length: f is the
// host's table f[len][count] = (count / len) * log(count / len) / LOG2, added in the reference's order in IEEE
// double (adds only).  A read without any of the four has term 0 and is dropped.
DET_HD bool det_low_complexity(const double *f, int ld, int len, int a, int c, int g, int t) {
    const double *row = f + (long long)len * ld;
    double term = 0.0;
    if (a > 0) term += row[a];
    if (c > 0) term += row[c];
    if (g > 0) term += row[g];
    if (t > 0) term += row[t];
    return -term <= 1.0;
}

// what a read keeps: the cut of the past-end expression, then the length tests.  0 = dropped.
DET_HD int det_kept_len(int len, int cut, int kmer_size, int min_k) {
    const int kept = cut < len ? cut : len;
    return (kept < kmer_size || kept < min_k || kept <= 0) ? 0 : kept;
}

// o = a >> s over the five words as one 320-bit number (bit i of word t is position 64 t + i), 0 < s < 64
DET_HD void det_shr(const uint64_t (&a)[DET_CHUNKS], int s, uint64_t (&o)[DET_CHUNKS]) {
#pragma unroll
    for (int t = 0; t < DET_CHUNKS; ++t) o[t] = (a[t] >> s) | (t + 1 < DET_CHUNKS ? a[t + 1] << (64 - s) : 0ull);
}

// start of the leftmost match of `B{8,}.*|B{2,}$` given m = positions that hold B and v = positions of the read
DET_HD int det_past_end_cut(const uint64_t (&m)[DET_CHUNKS], const uint64_t (&v)[DET_CHUNKS], int len) {
    uint64_t r[DET_CHUNKS], s[DET_CHUNKS];
    det_shr(m, 1, s);
#pragma unroll
    for (int t = 0; t < DET_CHUNKS; ++t) r[t] = m[t] & s[t];
    det_shr(r, 2, s);
#pragma unroll
    for (int t = 0; t < DET_CHUNKS; ++t) r[t] &= s[t];
    det_shr(r, 4, s);
#pragma unroll
    for (int t = 0; t < DET_CHUNKS; ++t) r[t] &= s[t];                 // bit i: positions i .. i + 7 hold B
    int cut = len, last_other = -1;
#pragma unroll
    for (int t = DET_CHUNKS - 1; t >= 0; --t) {
        if (r[t]) cut = t * 64 + __builtin_ffsll((long long)r[t]) - 1;
        const uint64_t other = v[t] & ~m[t];
        if (last_other < 0 && other) last_other = t * 64 + 63 - __builtin_clzll(other);
    }
    const int trail = last_other + 1;                                  // the trailing run of B starts here
    if (len - trail >= 2 && trail < cut) cut = trail;
    return cut;
}

// ------------------------------------------------------------------------------------------------ host side
// complement of BASE_COMPLEMENTS (util/__init__.py:67-88: the IUPAC pairs in both cases), 0 = none
static inline uint8_t det_complement(uint8_t c) {
    static const char *from = "ACGTRYSWKMBDHVNacgtryswkmbdhvn", *to = "TGCAYRSWMKVHDBNtgcayrswmkvhdbn";
    for (int i = 0; from[i]; ++i)
        if ((uint8_t)from[i] == c) return (uint8_t)to[i];
    return 0;
}

struct DetectTables {
    int nseq = 0, kmer_size = 0, bits = 0, words = 1, min_k = 0, npast = 0, max_len = 0;
    uint8_t past[DET_MAX_PAST_END] = {0, 0, 0, 0};
    uint8_t enc[256];                        // byte -> code, DET_OTHER
    uint8_t comp_ok[256];                    // byte has a complement
    uint32_t mask = 0;                       // slots - 1
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals, postings, bloom, thresholds, seq_off, n_kmers;
    std::vector<uint8_t> seq_bytes;          // the known sequences back to back (seq_off[s] .. seq_off[s + 1])
    std::vector<double> complexity;          // [(max_len + 1)][(max_len + 1)]
};

// Returns 0, -1 (invalid) or -2 (outside the envelope).  seqs: the known sequences back to back, lens[nseq].
// nseq == 0 (the heuristic detector's filter: no known list, no shortest-known-sequence test) builds empty tables.
static inline int det_build(DetectTables &T, const uint8_t *seqs, const int32_t *lens, int nseq, int kmer_size,
                            const uint8_t *past, int npast, const int32_t *thresholds, const double *complexity,
                            int max_len) {
    if (nseq < 0 || (nseq && (!seqs || !lens || !thresholds)) || !complexity || npast < 0 || (npast && !past) ||
        kmer_size < 1 || max_len < 1)
        return -1;
    if (nseq > DET_MAX_SEQS || npast > DET_MAX_PAST_END || kmer_size < DET_MIN_K || kmer_size > DET_MAX_K ||
        max_len > DET_MAX_READ)
        return -2;
    T.nseq = nseq; T.kmer_size = kmer_size; T.npast = npast; T.max_len = max_len;
    for (int i = 0; i < npast; ++i) T.past[i] = past[i];
    T.seq_off.assign(1, 0u);
    T.min_k = nseq ? 0x7fffffff : 0;
    for (int s = 0; s < nseq; ++s) {
        if (lens[s] < 0) return -1;
        T.seq_off.push_back(T.seq_off.back() + (uint32_t)lens[s]);
        if (lens[s] < T.min_k) T.min_k = lens[s];
    }
    if (nseq) {
        T.seq_bytes.assign(seqs, seqs + T.seq_off.back());
        T.thresholds.assign(thresholds, thresholds + nseq);
    }
    T.complexity.assign(complexity, complexity + (size_t)(max_len + 1) * (max_len + 1));
    // the alphabet: the bytes of the known sequences and their complements
    bool used[256] = {false};
    for (uint8_t c : T.seq_bytes) {
        used[c] = true;
        if (det_complement(c)) used[det_complement(c)] = true;
    }
    int nalpha = 0;
    for (int c = 0; c < 256; ++c) {
        T.enc[c] = used[c] ? (uint8_t)nalpha++ : DET_OTHER;
        T.comp_ok[c] = det_complement((uint8_t)c) != 0;
    }
    T.bits = 1;
    while ((1 << T.bits) < nalpha) ++T.bits;
    if (T.bits * kmer_size > 64) return -2;
    // distinct k-mers of every sequence, both strands -> key -> postings
    std::map<uint64_t, std::vector<uint32_t>> table;
    T.n_kmers.assign(nseq, 0u);
    int most = 0;
    for (int s = 0; s < nseq; ++s) {
        const uint8_t *q = T.seq_bytes.data() + T.seq_off[s];
        std::map<std::string, int> seen;
        for (int i = 0; i + kmer_size <= lens[s]; ++i) {
            const std::string kmer((const char *)q + i, (size_t)kmer_size);
            if (seen.count(kmer)) continue;
            const int kidx = (int)seen.size();
            seen[kmer] = kidx;
            if (kidx >= DET_MAX_KMERS) return -2;
            uint64_t fw = 0, rv = 0;
            bool has_rv = true;
            for (int j = 0; j < kmer_size; ++j) {
                fw = (fw << T.bits) | T.enc[(uint8_t)kmer[j]];
                const uint8_t c = det_complement((uint8_t)kmer[kmer_size - 1 - j]);
                if (!c) has_rv = false;
                rv = (rv << T.bits) | (c ? T.enc[c] : 0);
            }
            table[fw].push_back(det_posting(s, 0, kidx));
            if (has_rv) table[rv].push_back(det_posting(s, 1, kidx));
        }
        T.n_kmers[s] = (uint32_t)seen.size();
        if ((int)seen.size() > most) most = (int)seen.size();
    }
    T.words = most > 96 ? 4 : most > 64 ? 3 : most > 32 ? 2 : 1;
    if (det_lds_bytes(nseq, T.words) > (size_t)DET_MAX_LDS) return -2;
    uint32_t slots = 1024;
    while (slots < 2 * table.size()) slots *= 2;
    T.mask = slots - 1;
    T.keys.assign(slots, 0ull);
    T.vals.assign(slots, DET_EMPTY);
    T.bloom.assign(DET_BLOOM_WORDS, 0u);
    T.postings.clear();
    for (const auto &kv : table) {
        if (kv.second.size() > 4095 || T.postings.size() + kv.second.size() >= (1u << 20)) return -2;
        const uint64_t h = det_mix(kv.first);
        uint32_t s = det_slot(h, T.mask);
        while (T.vals[s] != DET_EMPTY) s = (s + 1) & T.mask;
        T.keys[s] = kv.first;
        T.vals[s] = (uint32_t)(T.postings.size() << 12) | (uint32_t)kv.second.size();
        T.bloom[det_bloom_bit(h) >> 5] |= 1u << (det_bloom_bit(h) & 31);
        T.postings.insert(T.postings.end(), kv.second.begin(), kv.second.end());
    }
    if (T.postings.empty()) T.postings.push_back(0u);
    return 0;
}

}  // namespace atr
#endif

/*
 * atropos_hip.h -- C ABI of the MI355X (gfx950) adapter-alignment library.
 *
 * This is the drop-in boundary for the one hot path of jdidion/atropos:
 * the Cython module atropos/align/_align.pyx (Aligner.locate, MultiAligner.locate,
 * compare_prefixes) and atropos/align/__init__.py:InsertAligner.match_insert.
 * Each entry point cites the reference interface it replaces.  The reference
 * calls these once per read from Python; this library takes whole batches that
 * are already resident in GPU memory and writes result records back to GPU
 * memory.  No exceptions, no C++ types, no torch types: plain pointers, sizes
 * and integer status codes.  All `d_*` pointers are device pointers on the
 * current HIP device; `stream` is a hipStream_t passed as void* (NULL = the
 * null stream).  Calls are asynchronous with respect to the host.
 *
 * Data layouts
 * ------------
 * ASCII reads   : row-major bytes, read r at d_ascii + r*row_stride, length
 *                 d_lens[r] (or max_len for every read when d_lens is NULL).
 * Packed reads  : 4 bits per base, "tile64" layout.  Reads are grouped in tiles
 *                 of 64 (one wavefront, one read per lane); a read occupies
 *                 nchunks = ceil(max_len/32) chunks of 16 bytes (32 bases);
 *                 chunk c of lane l of tile t lives at byte offset
 *                 ((t*nchunks + c)*64 + l)*16, so one wavefront load of chunk c
 *                 is a single contiguous 1 KiB transaction.  Base j of a read is
 *                 in chunk j/32, little-endian dword (j%32)/8, bits 4*(j%8)..+3.
 *                 Bases past the read's length are 0.  Buffer size:
 *                 atr_packed_bytes().
 * Result record : 8 x int16 = 16 bytes per read (atr_result), refstop == -1
 *                 means "no match" (the reference returns None).
 */
#ifndef ATROPOS_HIP_H
#define ATROPOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (negative = error) */
#define ATR_OK                 0
#define ATR_ERR_INVALID       -1   /* bad argument (the reference raises ValueError) */
#define ATR_ERR_UNSUPPORTED   -2   /* outside the device kernels' envelope, see atr_aligner_create */
#define ATR_ERR_HIP           -3   /* HIP runtime error; atr_last_error() has the text */
#define ATR_ERR_NOMEM         -4   /* the reference raises MemoryError */
#define ATR_ERR_NODEVICE      -5   /* no HIP device visible */

/* alignment flags, atropos/align/__init__.py:17-26 */
#define ATR_START_WITHIN_SEQ1  1
#define ATR_START_WITHIN_SEQ2  2
#define ATR_STOP_WITHIN_SEQ1   4
#define ATR_STOP_WITHIN_SEQ2   8
#define ATR_SEMIGLOBAL        15

/* envelope of the device kernels */
#define ATR_MAX_REF_LEN      128   /* adapter / reference length m of an aligner handle (longer references, up to
                                    * ATR_PAIRS_MAX_LEN: atr_locate_pairs_batch with the same reference on every pair) */
#define ATR_MAX_READ_LEN     736   /* read length n (23 chunks) of the batch pipelines, the per-read calls and the text stages */
#define ATR_MAX_LONG_READ_LEN 32736 /* atr_pack_reads + atr_locate_batch take reads up to here (1023 chunks; the record's
                                    * int16 fields end at 32767): batches with max_len > ATR_MAX_READ_LEN go through the
                                    * full column sweep with a rolling origin base (locate_kernel.hpp) whatever the path */

/* which 256-entry translate table the packed reads must have been built with */
#define ATR_TABLE_DNA15   0   /* equality compare: 15 upper-case IUPAC letters -> their bit codes, rest 0 */
#define ATR_TABLE_ACGT    1   /* _align.pyx:31-44  (_acgt_table)  */
#define ATR_TABLE_IUPAC   2   /* _align.pyx:46-83  (_iupac_table) */
#define ATR_TABLE_CUSTOM  3   /* equality compare over a per-aligner symbol map (arbitrary ASCII reference) */

typedef struct {
    int16_t refstart, refstop, querystart, querystop, matches, errors, aux0, aux1;
} atr_result;

typedef struct atr_aligner atr_aligner;           /* replaces the cdef class Aligner, _align.pyx:121-494 */
typedef struct atr_insert_aligner atr_insert_aligner;   /* replaces InsertAligner, align/__init__.py:178-377 */

/* ---- library / device ---------------------------------------------------- */

int atr_version(void);
int atr_device_count(void);                       /* >= 0, or ATR_ERR_HIP */
const char *atr_last_error(void);                 /* thread-local text of the last ATR_ERR_HIP */

/* ---- translate tables and the 4-bit packer ------------------------------- */

/* Fill `table` with one of the fixed tables above (kind != ATR_TABLE_CUSTOM). */
int atr_translate_table(int kind, uint8_t table[256]);

/* Bytes of a tile64 packed buffer for nreads reads of at most max_len bases. */
size_t atr_packed_bytes(int64_t nreads, int max_len);

/* ASCII -> 4-bit tile64.  `table` is a HOST pointer to the 256-entry translate
 * table (the reference does bytes.translate(table) per read: _align.pyx:243-248,
 * :292-297).  d_lens may be NULL (all reads max_len long).  d_starts may be NULL; otherwise
 * read r is packed from its base d_starts[r] on, i.e. the slice read[start:] of length
 * d_lens[r] - d_starts[r] (what LinkedAdapter.match_to hands to the 3' adapter after
 * removing the 5' match, adapters/__init__.py:683-690).  d_invalid may be NULL;
 * otherwise *d_invalid (device int32, zeroed by the caller) is incremented once per
 * read that contains a byte the table maps to 0 -- the insert aligner needs every base
 * to have a complement (reverse_complement raises KeyError, util/__init__.py:479-482). */
int atr_pack_reads(const uint8_t *d_ascii, int64_t row_stride, const int32_t *d_lens,
                   const int32_t *d_starts, int64_t nreads, int max_len, const uint8_t table[256],
                   uint8_t *d_packed, int32_t *d_invalid, void *stream);

/* Same arguments, same tiles and chunk addresses, but each 16-byte chunk holds the FOUR BIT
 * PLANES of its 32 bases (word p, bit b = bit p of the code of base 32c + b): the layout the
 * insert aligner consumes (atr_insert_match_batch), which compares 32 bases per boolean op. */
int atr_pack_planes(const uint8_t *d_ascii, int64_t row_stride, const int32_t *d_lens,
                   const int32_t *d_starts, int64_t nreads, int max_len, const uint8_t table[256],
                   uint8_t *d_packed, int32_t *d_invalid, void *stream);

/* Counts into *d_count (device int32, zeroed by the caller) the reads of a plane64 buffer whose
 * first min(d_lens[r], d_other_lens[r]) bases hold an uncoded base (a byte the pack table maps
 * to 0).  InsertAligner.match_insert reverse-complements only seq2[:min(len(seq1), len(seq2))]
 * (align/__init__.py:251-259), so that prefix -- not the whole read, which is what d_invalid of
 * the pack calls covers -- is what must have complements.  Either length array may be NULL
 * (max_len). */
int atr_planes_count_uncoded(const uint8_t *d_planes, const int32_t *d_lens, const int32_t *d_other_lens,
                             int64_t nreads, int max_len, int32_t *d_count, void *stream);

/* ---- Aligner (atropos/align/_align.pyx:121-494) -------------------------- */

/* Aligner.__cinit__(reference, max_error_rate, flags, wildcard_ref,
 * wildcard_query, min_overlap, indel_cost)  (_align.pyx:197-208).
 * ATR_ERR_INVALID  : m < 1, min_overlap < 1 or indel_cost < 1 (ValueError, :219-220, :229-230),
 *                    non-ASCII reference byte (UnicodeEncodeError, :243).
 * ATR_ERR_UNSUPPORTED: m > ATR_MAX_REF_LEN, int(e*m) >= 1000, or an indel cost
 *                    large enough to overflow the 12-bit cost field while still
 *                    <= int(e*m) (never the case for the trim command's settings). */
int atr_aligner_create(const char *ref, int m, double max_error_rate, int flags,
                       int wildcard_ref, int wildcard_query, int min_overlap, int indel_cost,
                       atr_aligner **out);
void atr_aligner_destroy(atr_aligner *a);
/* property setters, _align.pyx:214-232 */
int atr_aligner_set_min_overlap(atr_aligner *a, int min_overlap);
int atr_aligner_set_indel_cost(atr_aligner *a, int indel_cost);
/* Which table queries must be packed with (ATR_TABLE_*), and the table itself
 * (meaningful for ATR_TABLE_CUSTOM). */
int atr_aligner_query_table(const atr_aligner *a, uint8_t table[256]);

/* Aligner.locate(query) for a batch (_align.pyx:266-491): d_out[r] receives
 * (refstart, refstop, querystart, querystop, matches, errors) or refstop = -1.
 * d_lens may be NULL.  max_len is the layout parameter the buffer was packed
 * with.  d_work: optional device scratch of atr_locate_work_bytes(nreads) bytes; when
 * given (and the aligner qualifies: START/STOP_WITHIN_SEQ2 set, m <= 64) the filtered
 * pipeline runs -- a bit-parallel pre-pass resolves most reads and the full DP only
 * sweeps a short column window of the rest; results are identical either way.
 * All work is enqueued on `stream` (a hipStream_t; NULL = the default stream) and is complete
 * when the stream reaches the end of the call: the filtered pipeline forks one internal
 * per-thread side stream after its scatter pass and joins it again before it returns (events,
 * no host synchronisation; the pattern is legal inside a stream capture).  d_work must stay
 * valid until then and must not be shared by calls that may overlap. */
size_t atr_locate_work_bytes(int64_t nreads);
/* Diagnostics (bench.py's hard-batch figures; no reference twin): how many reads of the LAST filtered call that used
 * d_work (atr_locate_batch with d_work, atr_locate_planes_batch: n_adapters = 1; atr_linked_match_batch on a long
 * batch: the set's adapter count) the pre-pass left to the exact DP kernels.  Waits for `stream`. */
int atr_locate_work_unresolved(const void *d_work, int64_t nreads, int n_adapters, void *stream, int64_t *out);
int atr_locate_batch(const atr_aligner *a, const uint8_t *d_packed, const int32_t *d_lens,
                     int64_t nreads, int max_len, atr_result *d_out, void *d_work, void *stream);

/* Aligner.locate(query) for a LONG batch of reads that are still ASCII rows (_align.pyx:266-297 takes the string; every
 * real caller starts from text): ONE pre-pass kernel stages a tile's rows through LDS, packs each read into bit planes in
 * registers (the aligner's query table), stores them to d_planes -- atr_packed_bytes(nreads, max_len) bytes, afterwards a
 * complete plane64 batch, e.g. for the next adapter -- and runs the two-pass pre-pass on the registers; then the DP
 * kernels of atr_locate_planes_batch.  Same records as atr_pack_planes + atr_locate_planes_batch, which is also what runs
 * when there is no fused kernel (it exists as a run-time compiled build for this aligner, read length and row stride:
 * no hiprtc, ATR_JIT=0, reads of more than 256 bases, rows wider than 256 bytes).  Envelope: atr_locate_planes_applies.
 * d_work: atr_locate_work_bytes(nreads).  Short batches: atr_locate_ascii_batch. */
int atr_locate_ascii_planes_batch(const atr_aligner *a, const uint8_t *d_ascii, int64_t row_stride, const int32_t *d_lens,
                                  int64_t nreads, int max_len, uint8_t *d_planes, atr_result *d_out, void *d_work, void *stream);

/* Aligner.locate(query) for a batch of reads in the plane64 layout (atr_pack_planes with the aligner's query
 * table; _align.pyx:266-491, same records as atr_locate_batch).  d_lens as in atr_locate_batch (NULL: every read
 * has max_len bases; else the positions of a read past its length must hold code 0, as atr_pack_planes leaves
 * them).  The two-pass pre-pass: exact
 * pieces of the adapter located 32 read positions per boolean op, then Myers' bit-vector sweep over a 64-column
 * window of the flagged reads only, then the exact DP of atr_locate_batch's filtered pipeline on what is left.
 * atr_locate_planes_applies: 1 when this aligner and read length are inside its envelope (3' adapters -- no
 * START_WITHIN_SEQ1 --, up to 40 bases, int(e * m) <= 4, A / C / G / T in the adapter's first 32 bases, reads of
 * 65 .. 320 bases; ragged != 0: a batch with d_lens, max_len the longest read), else 0:
 * pack tile64 and call atr_locate_batch.
 * d_work: atr_locate_work_bytes(nreads) bytes.  ATR_ERR_UNSUPPORTED outside the envelope. */
int atr_locate_planes_applies(const atr_aligner *a, int max_len, int ragged);
/* Build (or load from the code-object cache) the pre-pass kernel SPECIALISED for this aligner and read length: the
 * library compiles its own kernel source once more with the adapter's piece codes, masks and thresholds as
 * constants (hiprtc, found at run time), which removes the per-term scalar dispatch of the generic kernel.  An
 * aligner object of the reference lives for a whole run (adapters/__init__.py:311-322), so the compile (seconds,
 * once per adapter and machine: objects are kept under $ATR_KCACHE_DIR / ~/.cache/atropos_amd) is paid once.
 * atr_locate_planes_batch does this by itself once a handle has seen $ATR_JIT_MIN_READS (2 M) reads; $ATR_JIT=0 turns
 * it off, =1 on for every call.  Same records either way.  ATR_OK: a specialised kernel is ready on the current device;
 * ATR_ERR_UNSUPPORTED: none (outside the envelope, switched off, no hiprtc) -- the generic kernel serves the calls. */
int atr_aligner_prepare(const atr_aligner *a, int max_len, int ragged);
int atr_locate_planes_batch(const atr_aligner *a, const uint8_t *d_planes, const int32_t *d_lens, int64_t nreads,
                            int max_len, atr_result *d_out, void *d_work, void *stream);

/* The same with the kernels named (identical records on every path; for cross-checks and tuning).
 * Short batches -- the 1000 reads the reference's trim command hands over per call
 * (commands/base.py:179), the per-read API -- are bound by the latency of one wavefront, not by
 * throughput: ATR_LOCATE_WAVE gives every read a WAVEFRONT (one DP row per lane, anti-diagonal
 * sweep: n + m steps instead of n * m cells per lane; up to three rows per lane for long references, no scratch). */
#define ATR_LOCATE_AUTO      0   /* what atr_locate_batch does: WAVE for batches of at most 32768 reads where it
                                    applies, else the anchored-prefix band / FILTERED with d_work, else FULL */
#define ATR_LOCATE_FULL      1   /* full-matrix sweep, one read per lane */
#define ATR_LOCATE_FILTERED  2   /* bit-vector pre-pass + window / band DP (needs d_work); FULL where it does not apply */
#define ATR_LOCATE_WAVE      3   /* one read per wavefront */
int atr_locate_batch_path(const atr_aligner *a, const uint8_t *d_packed, const int32_t *d_lens,
                          int64_t nreads, int max_len, atr_result *d_out, void *d_work, int path, void *stream);

/* Short batches straight from ASCII (no atr_pack_reads in between): row r of d_ascii (row_stride bytes apart; base
 * address and stride multiples of four) holds read r, translated inside the wavefront-per-read kernel with the aligner's
 * own query table (_align.pyx:243-248, :292-297).  At most 32768 reads per call (ATR_ERR_UNSUPPORTED beyond: pack the
 * batch and call atr_locate_batch). */
int atr_locate_ascii_batch(const atr_aligner *a, const uint8_t *d_ascii, int64_t row_stride, const int32_t *d_lens,
                           int64_t nreads, int max_len, atr_result *d_out, void *stream);

/* Aligner.locate(query) for ONE read in HOST memory, synchronously: what the module swap of INTEGRATION.md section 1
 * calls per read.  The read goes through a page-locked staging buffer of the calling thread that the kernel reads
 * directly, the record comes back the same way; one launch, one stream synchronisation, no allocation.
 * query: n ASCII bytes (not translated, not terminated); *out: the record (refstop = -1 for None). */
int atr_locate_one(const atr_aligner *a, const char *query, int n, atr_result *out, void *stream);

/* The same for the other two functions the module swap calls once per read pair with the insert aligner
 * (align/__init__.py:250-377): MultiAligner(max_error_rate, flags, min_overlap).locate(ref, query, max_matches)
 * (_align.pyx:593-783; out: up to cap records, *count: the number of hits the reference returns, 0 = None) and
 * compare_prefixes / compare_suffixes(ref, query, wildcard_ref, wildcard_query) (_align.pyx:501-544,
 * align/__init__.py:28-44).  Host strings in, host records out, one launch and one synchronisation each. */
int atr_multi_locate_one(const char *ref, int m, const char *query, int n, double max_error_rate, int flags, int min_overlap,
                         int max_matches, atr_result *out, int cap, int32_t *count, void *stream);
int atr_compare_one(const char *ref, int m, const char *query, int n, int wildcard_ref, int wildcard_query, int suffix,
                    atr_result *out, void *stream);

/* ---- linked adapters: LinkedAdapter.match_to under AdapterCutter._best_match ------------
 * (atropos/adapters/__init__.py:648-690, atropos/commands/trim/modifiers.py:107-122) --------- */

#define ATR_LINKED_MAX_ADAPTERS 4

/* One `-a ^FRONT...BACK` adapter: Adapter(FRONT, PREFIX) and Adapter(BACK, BACK) with what
 * Adapter.match_to wraps around each alignment (adapters/__init__.py:338-400).  The aligners
 * carry sequence, max_error_rate, wildcard flags, min_overlap (Adapter sets aligner.min_overlap
 * = min(min_overlap, len), :285, :313) and indel cost (:316-322).
 *   *_exact_shortcut : the literal startswith / find shortcut is active (`not adapter_wildcards`,
 *                      :351-367): a full-length zero-error occurrence bypasses the acceptance test;
 *   d_*_rmp          : DEVICE table rmp[size * *_rmp_ld + matches] = match_probability(matches, size)
 *                      with its bound *_max_rmp (:393-397), or NULL (max_rmp is None). */
typedef struct {
    const atr_aligner *front;      /* flags == ATR_STOP_WITHIN_SEQ2 (anchored 5') */
    const atr_aligner *back;       /* flags == START_WITHIN_SEQ2 | STOP_WITHIN_SEQ1 | STOP_WITHIN_SEQ2 (regular 3') */
    int front_exact_shortcut, back_exact_shortcut;
    const double *d_front_rmp, *d_back_rmp;
    int front_rmp_ld, back_rmp_ld;
    double front_max_rmp, back_max_rmp;
} atr_linked_adapter;

typedef struct atr_linked_set atr_linked_set;

/* Copies what it needs from the aligners (they may be destroyed afterwards; later setter calls on
 * them are not seen) and uploads one parameter block to the current device.
 * ATR_ERR_UNSUPPORTED: more than ATR_LINKED_MAX_ADAPTERS adapters; a 5' part with m + int(e*m) > 32
 * or int(e*m) > 7; a 3' part outside the filtered pipeline (m > 64) or with START_WITHIN_SEQ1;
 * int(e*m) >= m; aligners that need different translate tables; the literal shortcut together with
 * a wildcard comparison (read wildcards on an ACGT-only adapter).  Callers then match the parts
 * one by one (atr_locate_batch + atr_adapter_postfilter). */
int atr_linked_create(const atr_linked_adapter *adapters, int n_adapters, atr_linked_set **out);
void atr_linked_destroy(atr_linked_set *s);
/* ATR_TABLE_* the reads must be packed with */
int atr_linked_query_table(const atr_linked_set *s);

/* For every read of a tile64 batch (whole reads, packed once): which linked adapter matches, its
 * 5' match and its 3' match on read[front.rstop:].
 *   d_which[2r]     = index of the first adapter whose 5' part matches, or -1 (LinkedAdapter.match_to
 *                     returns None for every adapter);
 *   d_which[2r + 1] = how many 5' parts match (with more than one the reference's _best_match raises
 *                     AttributeError: LinkedMatch has no `matches`, modifiers.py:120);
 *   d_front[r]      = front_match of that adapter as (astart, astop, rstart, rstop, matches, errors);
 *   d_back[r]       = back_match, coordinates relative to read[front.rstop:] as in the reference
 *                     (refstop == -1: None -- also when no 5' part matched).
 * d_work: scratch of atr_linked_work_bytes() bytes; stream semantics as atr_locate_batch. */
size_t atr_linked_work_bytes(const atr_linked_set *s, int64_t nreads);
int atr_linked_match_batch(const atr_linked_set *s, const uint8_t *d_packed, const int32_t *d_lens, int64_t nreads,
                           int max_len, int8_t *d_which, atr_result *d_front, atr_result *d_back, void *d_work,
                           void *stream);

/* The same matches with the anchored 5' parts decided AT PACK TIME (round 6; linked_group.hip).  An anchored 5' part
 * only looks at the read's first m + int(e*m) <= 32 bases, and LinkedAdapter.match_to (adapters/__init__.py:671-690)
 * matches the 3' part of the adapter whose 5' part matched on read[front.rstop:]: atr_linked_group_pack reads the ASCII
 * rows once, decides every read's 5' part (d_which, d_front: as atr_linked_match_batch) and packs read[front.rstop:] as
 * bit planes (plane64) into a sub-batch PER ADAPTER -- group g's reads in batch order on consecutive slots:
 *   d_grouped   atr_linked_group_bytes(nreads, max_len) bytes; d_glens[slot] = len - rstop (0 on the padding slots that
 *               fill a group's last tile); d_perm[slot] = the read (-1: padding); d_slot_of[r] = its slot (-1: no 5'
 *               match, nothing packed); all three int32, nreads + 64 * ATR_LINKED_MAX_ADAPTERS entries for glens / perm;
 *   info (HOST, 8 x int64, written before the call returns -- the call waits for `stream`): [g] = reads of group g,
 *               [4 + g] = first tile of its sub-batch.
 * atr_linked_group_match then runs each group through atr_locate_planes_batch's pipeline with ITS 3' aligner (the pre-pass
 * compiled at run time for that aligner; the groups side by side on internal streams, joined before the call's end on
 * `stream`): d_slab[slot] = the raw Aligner.locate record of the slot's read[rstop:]; with d_back != NULL also
 * d_back[r] = back_match in batch order after Adapter.match_to's acceptance test (:386-398), exactly
 * atr_linked_match_batch's d_back.  atr_linked_group_applies: 1 when every 3' aligner of the set is inside the two-pass
 * pre-pass's envelope for ragged reads of at most max_len bases (else use atr_linked_match_batch).
 * table: the 256-byte translate table of atr_linked_query_table's kind.  d_work: atr_linked_group_work_bytes() bytes,
 * the SAME buffer for the pack and the match call of a batch. */
int atr_linked_group_applies(const atr_linked_set *s, int max_len);
size_t atr_linked_group_bytes(int64_t nreads, int max_len);
size_t atr_linked_group_work_bytes(const atr_linked_set *s, int64_t nreads);
int atr_linked_group_pack(const atr_linked_set *s, const uint8_t *d_ascii, int64_t row_stride, const int32_t *d_lens,
                          int64_t nreads, int max_len, const uint8_t table[256], uint8_t *d_grouped, int32_t *d_glens,
                          int32_t *d_perm, int32_t *d_slot_of, int8_t *d_which, atr_result *d_front, int64_t info[8],
                          void *d_work, void *stream);
int atr_linked_group_match(const atr_linked_set *s, const uint8_t *d_grouped, const int32_t *d_glens, const int64_t info[8],
                           int max_len, const int32_t *d_slot_of, const int8_t *d_which, int64_t nreads, atr_result *d_slab,
                           atr_result *d_back, void *d_work, void *stream);

/* ---- InsertAligner (atropos/align/__init__.py:178-377) -------------------- */

#define ATR_INSERT_MAX_ADAPTER 128   /* adapter length handled by the insert kernel */
#define ATR_INSERT_MAX_READ    320   /* read length handled by the insert kernel */

/* InsertAligner.__init__ arguments (align/__init__.py:206-233) plus the host-built
 * tables.  All pointers are HOST pointers; the library copies what it needs.
 *   rmp_insert[size*rmp_ld + matches]  = match_probability(matches, size, **base_probs)  (:359)
 *   rmp_adapter[size*rmp_ld + matches] = match_probability(matches, size)                (:303-304)
 *   max_mismatch_by_alen[a]            = round(a * max_adapter_mismatch_frac)            (:290)
 * computed by the caller with Python's float/bigint/round semantics (rmp_ld >= ATR_INSERT_MAX_READ + 1,
 * n_mismatch >= ATR_INSERT_MAX_ADAPTER + 1). */
typedef struct {
    const char *adapter1; int alen1;
    const char *adapter2; int alen2;
    double insert_max_rmp, adapter_max_rmp;
    int min_insert_overlap; double max_insert_mismatch_frac;
    int min_adapter_overlap; double max_adapter_mismatch_frac;
    int adapter_check_cutoff;
    int adapter_wildcards, read_wildcards;
    const double *rmp_insert; const double *rmp_adapter; int rmp_ld;
    const int32_t *max_mismatch_by_alen; int n_mismatch;
} atr_insert_config;

/* Allocates two small device tables on the current device (freed by _destroy).
 * ATR_ERR_UNSUPPORTED: an adapter longer than ATR_INSERT_MAX_ADAPTER. */
int atr_insert_aligner_create(const atr_insert_config *cfg, atr_insert_aligner **out);
void atr_insert_aligner_destroy(atr_insert_aligner *a);

/* InsertAligner.match_insert(seq1, seq2) for a batch (align/__init__.py:250-377).
 * Both read sets are PLANE64 buffers (atr_pack_planes) packed with ATR_TABLE_DNA15 and the
 * same max_len (<= ATR_INSERT_MAX_READ).  d_out receives THREE records per pair:
 *   d_out[3p+0] = the insert match tuple (refstop == -1: match_insert returns None),
 *   d_out[3p+1] = Match 1 as (astart, astop, rstart, rstop, matches, errors), astop == -1: None,
 *   d_out[3p+2] = Match 2, likewise. */
int atr_insert_match_batch(const atr_insert_aligner *a, const uint8_t *d_packed1, const int32_t *d_lens1,
                           const uint8_t *d_packed2, const int32_t *d_lens2, int64_t npairs, int max_len,
                           atr_result *d_out, void *stream);

/* The same for SOFT-MASKED reads.  match_insert compares the two reads character by character (lower case is not
 * upper case, _align.pyx:690; reverse_complement keeps the case, util/__init__.py:67-88) but folds the case of
 * the overhangs where compare_prefixes translates them (a wildcard flag set, _align.pyx:521-530).  With
 * ATR_READ_CODES_CASED both reads are packed with atr_case_sensitive_table(): upper-case A C G T N W B D H V keep
 * their DNA15 codes, lower-case a/t, c/g, n take the codes 3/12, 5/10, 6 (closed under the device's complement);
 * M K R Y S have no code in that table.  ATR_ERR_UNSUPPORTED: without wildcard flags an adapter that holds one of
 * M K R Y S or a lower-case letter cannot be told from a soft-masked read base. */
#define ATR_READ_CODES_DNA15 0
#define ATR_READ_CODES_CASED 1
int atr_case_sensitive_table(uint8_t table[256]);
int atr_insert_match_batch_coded(const atr_insert_aligner *a, const uint8_t *d_packed1, const int32_t *d_lens1,
                                 const uint8_t *d_packed2, const int32_t *d_lens2, int64_t npairs, int max_len,
                                 int read_codes, atr_result *d_out, void *stream);

/* InsertAligner.match_insert(seq1, seq2) for ONE pair of reads in host memory, synchronously (the per-pair call of
 * InsertAdapterCutter.__call__, commands/trim/modifiers.py:381-390): n1 / n2 upper-case IUPAC letters each (the caller
 * checks; soft-masked reads take atr_insert_match_batch_coded).  out: the three records of atr_insert_match_batch. */
int atr_insert_match_one(const atr_insert_aligner *a, const char *seq1, int n1, const char *seq2, int n2, atr_result *out,
                         void *stream);

/* ---- MultiAligner.locate, compare_prefixes / compare_suffixes (general) --- */

/* Aligner.enable_debug() / .dpmatrix (_align.pyx:88-119, :259-264, :354-357, :428-431): the DP matrix of
 * ONE locate() call as the reference stores it while debugging -- the costs of exactly the cells its loop
 * computes (Ukkonen's cut-off included), computed with the aligner's true indel cost.  d_packed: one read
 * packed for `a` (tile64, the read is lane 0 of tile 0), n its length.  d_matrix: caller scratch of
 * atr_locate_debug_bytes(a, n) bytes; its first (m + 1) x (n + 1) int32 (row-major, row = reference
 * position) receive the costs, INT32_MIN = never computed (printed as blanks).  d_out: the result record
 * of the same call.  A debugging aid: one lane, not a throughput path. */
size_t atr_locate_debug_bytes(const atr_aligner *a, int n);
int atr_locate_debug(const atr_aligner *a, const uint8_t *d_packed, int n, void *d_matrix, atr_result *d_out,
                     void *stream);

/* MultiAligner(max_error_rate, flags, min_overlap).locate(reference, query, max_matches)
 * (_align.pyx:548-787) for npairs independent pairs of raw ASCII strings (row-major,
 * refs at d_refs + p*ref_stride with length d_ref_lens[p], likewise the queries).
 * d_out holds out_stride records per pair; d_counts[p] receives the number of hits the
 * reference returns (0 == None; hits beyond out_stride are counted but not stored).
 * d_work: caller scratch of atr_multi_locate_work_bytes(npairs, max_ref_len) bytes. */
size_t atr_multi_locate_work_bytes(int64_t npairs, int max_ref_len);
int atr_multi_locate_batch(const uint8_t *d_refs, int64_t ref_stride, const int32_t *d_ref_lens,
                           const uint8_t *d_queries, int64_t query_stride, const int32_t *d_query_lens,
                           int64_t npairs, double max_error_rate, int flags, int min_overlap, int max_matches,
                           int max_ref_len, void *d_work, atr_result *d_out, int32_t *d_counts, int out_stride,
                           void *stream);

/* compare_prefixes(ref, query, wildcard_ref, wildcard_query) (_align.pyx:501-544), or
 * compare_suffixes (align/__init__.py:28-44) when suffix != 0, of ONE reference (host
 * pointer, m <= 1024 raw ASCII bytes) against n queries (device, raw ASCII).  d_lens may
 * be NULL (all queries max_len long). */
int atr_compare_batch(const char *ref, int m, const uint8_t *d_queries, int64_t query_stride,
                      const int32_t *d_lens, int64_t n, int max_len, int wildcard_ref, int wildcard_query,
                      int suffix, atr_result *d_out, void *stream);

/* The same comparison for reads that are already packed for an aligner (tile64, the table of
 * atr_aligner_query_table): `a`'s reference against the first (suffix: last) min(m, len) bases of
 * every read, matching by the aligner's own rule (byte equality without wildcard flags, 4-bit AND
 * with them -- _align.pyx:521-539 picks the same tables as Aligner.__cinit__, :243-248).  This is
 * the branch Adapter.match_to takes for anchored adapters without indels
 * (adapters/__init__.py:370-380); it lets the device pipelines, whose reads only exist packed
 * (FASTQ chunks, the remainders a 5' linked part leaves), run it without an ASCII copy. */
int atr_compare_packed(const atr_aligner *a, const uint8_t *d_packed, const int32_t *d_lens, int64_t nreads,
                       int max_len, int suffix, atr_result *d_out, void *stream);

/* ---- Adapter.match_to post-filter (adapters/__init__.py:386-398) ---------- */

/* Applies, in place on n result records, the acceptance test Adapter.match_to runs on an
 * alignment: size >= min_overlap, errors/size <= max_error_rate (double division) and --
 * when d_rmp is not NULL -- d_rmp[size*rmp_ld + matches] <= max_rmp (d_rmp: DEVICE table of
 * match_probability(matches, size)).  accept_full != 0: a full-length zero-error occurrence
 * (the exact-match shortcut, :351-367) is kept regardless.  Rejected records get refstop -1. */
int atr_adapter_postfilter(atr_result *d_records, int64_t n, int adapter_len, int min_overlap,
                           double max_error_rate, const double *d_rmp, int rmp_ld, double max_rmp,
                           int accept_full, void *stream);

/* ---- ErrorCorrectorMixin.correct_errors (commands/trim/modifiers.py:219-350) ---- */

#define ATR_CORRECT_N             0   /* mismatch_action 'N' */
#define ATR_CORRECT_CONSERVATIVE  1
#define ATR_CORRECT_LIBERAL       2

/* Correct mismatches in the overlap of n read pairs IN PLACE.  d_seq1/d_qual1/d_seq2/
 * d_qual2: raw ASCII, row stride `stride` (qualities may both be NULL); d_insert: 4 x int16
 * per pair = insert_match[0..3]; d_mask (may be NULL) selects the pairs to touch;
 * comp: HOST 256-entry complement table (BASE_COMPLEMENTS; 0 = no complement).
 * d_changed receives 2 x int32 per pair (bases changed in read1, read2; changed[0] == -1:
 * -1 KeyError, -2 IndexError, -3 ValueError: the exception the reference raises), d_newlen the
 * 2 x int32 sequence lengths afterwards (the reference truncates a corrected, longer
 * read 1 to read 2's length when truncate_seqs is set). */
int atr_correct_errors_batch(uint8_t *d_seq1, uint8_t *d_qual1, const int32_t *d_lens1,
                             uint8_t *d_seq2, uint8_t *d_qual2, const int32_t *d_lens2, int64_t stride,
                             const int16_t *d_insert, const uint8_t *d_mask, int64_t n, int max_len,
                             int action, int min_qual_difference, int truncate_seqs, const uint8_t comp[256],
                             int32_t *d_changed, int32_t *d_newlen, void *stream);

/* The correction step of InsertAdapterCutter.__call__ right after the insert match
 * (modifiers.py:397-404): d_insert_records are the 3 records per pair of atr_insert_match_batch;
 * a pair is corrected (correct_errors(read1, read2, insert_match, truncate_seqs=True)) when its
 * insert match exists and has errors > 0.  d_planes1 / d_planes2 (may both be NULL): the plane64
 * buffers the records were computed from (atr_pack_planes, ATR_TABLE_DNA15, layout width
 * planes_max_len) -- with them the kernel finds the disagreeing positions 32 at a time and touches
 * the ASCII matrices only there.  Other arguments as atr_correct_errors_batch. */
int atr_insert_correct_batch(const atr_result *d_insert_records, const uint8_t *d_planes1, const uint8_t *d_planes2,
                             int planes_max_len, uint8_t *d_seq1, uint8_t *d_qual1,
                             const int32_t *d_lens1, uint8_t *d_seq2, uint8_t *d_qual2, const int32_t *d_lens2,
                             int64_t stride, int64_t n, int max_len, int action, int min_qual_difference,
                             const uint8_t comp[256], int32_t *d_changed, int32_t *d_newlen, void *stream);

/* InsertAdapterCutter.__call__'s first two steps as ONE call (modifiers.py:385-404): the insert match of
 * atr_insert_match_batch (records to d_out, 3 per pair) and, for every pair whose insert match has errors > 0,
 * correct_errors(read1, read2, insert_match, truncate_seqs=True) in place on the ASCII matrices -- what
 * atr_insert_match_batch followed by atr_insert_correct_batch(d_out, d_packed1, d_packed2, max_len, ...) computes,
 * bit for bit, but with the reads' planes streamed once: the disagreeing positions are the mask words the match
 * counted.  d_packed1 / d_packed2: plane64 batches (ATR_TABLE_DNA15) of layout width max_len; d_lens1 / d_lens2
 * (may be NULL: every read has max_len bases) are the lengths of BOTH the packed reads and the matrix rows.
 * Batches the fused kernel does not take (more than 256 or fewer than 97 bases of layout width, adapters of
 * more than 64 bases, a row pitch `stride` of 64 MB or more) run the two kernels one after the other inside this call. */
int atr_insert_match_correct_batch(const atr_insert_aligner *a, const uint8_t *d_packed1, const int32_t *d_lens1,
                                   const uint8_t *d_packed2, const int32_t *d_lens2, int64_t npairs, int max_len,
                                   atr_result *d_out, uint8_t *d_seq1, uint8_t *d_qual1, uint8_t *d_seq2,
                                   uint8_t *d_qual2, int64_t stride, int action, int min_qual_difference,
                                   const uint8_t comp[256], int32_t *d_changed, int32_t *d_newlen, void *stream);

/* ---- Aligner.locate with a per-pair reference (MergeOverlapping) ----------- */

/* `Aligner(ref_p, max_error_rate, flags, wildcard_ref, wildcard_query, min_overlap,
 * indel_cost).locate(query_p)` (_align.pyx:197-491) for npairs independent pairs: the
 * aligner MergeOverlapping constructs per read pair with reference = reverse complement of
 * read 2 and query = read 1 (commands/trim/modifiers.py:889-894).  Both sides are 4-bit
 * tile64 batches (atr_pack_reads / atr_pack_records) packed with the tables Aligner would
 * translate with: ATR_TABLE_DNA15 on both sides for the literal compare (every base must be
 * one of the 15 upper-case IUPAC letters), ATR_TABLE_ACGT / ATR_TABLE_IUPAC per wildcard flag
 * otherwise (_align.pyx:243-248, :292-297).  revcomp_ref != 0: the reference of a pair is the
 * reverse complement of the packed sequence (util/__init__.py:479-482).  d_*_lens may be NULL.
 * ATR_ERR_UNSUPPORTED: a side longer than ATR_PAIRS_MAX_LEN (longer than 255 when the flags lack
 * ATR_STOP_WITHIN_SEQ2: only then must the DP cell count matches rather than mismatches) or
 * int(e * m) >= 256. */
#define ATR_PAIRS_MAX_LEN 320
int atr_locate_pairs_batch(const uint8_t *d_ref_packed, const int32_t *d_ref_lens, int ref_max_len, int revcomp_ref,
                           const uint8_t *d_query_packed, const int32_t *d_query_lens, int query_max_len,
                           int64_t npairs, double max_error_rate, int flags, int wildcard_ref, int wildcard_query,
                           int min_overlap, int indel_cost, atr_result *d_out, void *stream);

/* The same for pairs with a side of more than ATR_PAIRS_MAX_LEN bases (up to ATR_MAX_LONG_READ_LEN; the reference has
 * no limit, _align.pyx:266-291): 64-bit cells, the DP column in d_work (atr_locate_pairs_long_work_bytes(npairs,
 * ref_max_len) bytes), one pair per lane over the whole matrix -- a fallback, not a throughput path.  Any lengths
 * are accepted.  ATR_ERR_UNSUPPORTED: max_error_rate * ref_max_len > 32 000. */
size_t atr_locate_pairs_long_work_bytes(int64_t npairs, int ref_max_len);
int atr_locate_pairs_long_batch(const uint8_t *d_ref_packed, const int32_t *d_ref_lens, int ref_max_len, int revcomp_ref,
                                const uint8_t *d_query_packed, const int32_t *d_query_lens, int query_max_len,
                                int64_t npairs, double max_error_rate, int flags, int wildcard_ref, int wildcard_query,
                                int min_overlap, int indel_cost, atr_result *d_out, void *d_work, void *stream);

/* The same with a per-pair lower bound on the alignment's matches (d_need, device, may be NULL = 1 everywhere):
 * MergeOverlapping only looks at an alignment when `matches >= min_overlap` (modifiers.py:896-897, min_overlap
 * from :870-874), so a pair whose reference alignment has fewer matches than d_need[p] may be reported as
 * refstop -1 instead -- which lets the library stop after its cost pass for pairs that cannot overlap that far.
 * Pairs whose alignment has at least d_need[p] matches get the reference's record, bit for bit.
 * With STOP_WITHIN_SEQ2, indel cost 1 and no wildcard flag (both flag sets of MergeOverlapping) the batch runs
 * through: exact costs of all candidate cells by Myers' bit-vector recurrence, the candidates that can still be
 * the reference's choice, and the packed-word DP on the band of diagonals that holds all their optimal paths;
 * other settings -- and pairs outside that pipeline's envelope -- sweep the whole matrix. */
int atr_locate_pairs_need_batch(const uint8_t *d_ref_packed, const int32_t *d_ref_lens, int ref_max_len, int revcomp_ref,
                                const uint8_t *d_query_packed, const int32_t *d_query_lens, int query_max_len,
                                int64_t npairs, double max_error_rate, int flags, int wildcard_ref, int wildcard_query,
                                int min_overlap, int indel_cost, const int32_t *d_need, atr_result *d_out, void *stream);

/* The same with the kernel family named (identical records up to the `need` rule; cross-checks, tuning).  Short
 * batches -- the 1000 pairs MergeOverlapping sees per call of the reference's trim command -- take ATR_PAIRS_WAVE:
 * one pair per wavefront, 64 lanes x up to 5 rows each (references of up to 319 bases), anti-diagonal sweep. */
#define ATR_PAIRS_AUTO  0   /* WAVE for at most 32768 pairs where it applies, else FAST where it pays, else FULL */
#define ATR_PAIRS_FULL  1   /* full-matrix sweep, one pair per lane (atr_locate_pairs_full_batch) */
#define ATR_PAIRS_FAST  2   /* costs by bit-vector, threats, banded payload; FULL for what is outside its envelope */
#define ATR_PAIRS_WAVE  3   /* one pair per wavefront; ATR_ERR_UNSUPPORTED for references of more than 319 bases */
int atr_locate_pairs_path_batch(const uint8_t *d_ref_packed, const int32_t *d_ref_lens, int ref_max_len,
                                int revcomp_ref, const uint8_t *d_query_packed, const int32_t *d_query_lens,
                                int query_max_len, int64_t npairs, double max_error_rate, int flags,
                                int wildcard_ref, int wildcard_query, int min_overlap, int indel_cost,
                                const int32_t *d_need, int path, atr_result *d_out, void *stream);

/* The same for ONE pair in host memory, synchronously -- what MergeOverlapping does per read pair through the module swap
 * (a new Aligner per pair, commands/trim/modifiers.py:889-894) when the reads are longer than an aligner handle's 128
 * bases.  ref_codes / query_codes: the two strings translated to 4-bit codes, one per byte, with the tables named
 * above (what atr_pack_reads would pack); references of up to 319 codes. */
int atr_locate_pair_one(const uint8_t *ref_codes, int m, int revcomp_ref, const uint8_t *query_codes, int n,
                        double max_error_rate, int flags, int wildcard_ref, int wildcard_query, int min_overlap,
                        int indel_cost, atr_result *out, void *stream);
/* atr_locate_pairs_batch by the full-matrix sweep alone (same records; the checker of the pipeline above). */
int atr_locate_pairs_full_batch(const uint8_t *d_ref_packed, const int32_t *d_ref_lens, int ref_max_len, int revcomp_ref,
                                const uint8_t *d_query_packed, const int32_t *d_query_lens, int query_max_len,
                                int64_t npairs, double max_error_rate, int flags, int wildcard_ref, int wildcard_query,
                                int min_overlap, int indel_cost, atr_result *d_out, void *stream);

/* ---- device-resident FASTQ batch (io/_seqio.pyx:163-245, io/seqio.py:686-700) ---- */

/* One chunk of FASTQ text (whole records, < 4 GiB, 16-byte aligned, ending in a line end) is
 * uploaded as raw bytes; the records are found, validated, trimmed and formatted on the
 * device.  Every trimming modifier of the single-end path only clips read ends, so its
 * state is the kept interval [d_begin[r], d_end[r]) of each record's sequence line. */
typedef struct {
    uint32_t name_off, name_len;   /* description after '@', line end stripped (FastqReader, _seqio.pyx:208-216) */
    uint32_t seq_off, seq_len;     /* :217-218 */
    uint32_t qual_off, qual_len;   /* :239-243 */
    uint32_t flags;                /* bit 0: the '+' line repeats the description (name2 = name, :228-236);
                                    * bit 1 (set by a caller that re-pointed name_off at a rewritten name -- LengthTagModifier,
                                    * SuffixRemover, PrefixSuffixAdder, commands/trim/modifiers.py:652-695): the '+' line's text
                                    * is the flags >> 8 bytes at `reserved`, as FastqFormat prints the name2 the file had */
    uint32_t reserved;             /* offset of that text (flags bit 1), else unused */
} atr_fastq_record;

#define ATR_FASTQ_ERR_AT      1    /* FormatError "... expected to start with '@'" (:209-211) */
#define ATR_FASTQ_ERR_PLUS    2    /* "... expected to start with '+'" (:224-227) */
#define ATR_FASTQ_ERR_NAME2   3    /* "Sequence descriptions in the FASTQ file don't match" (:229-235) */
#define ATR_FASTQ_ERR_LENGTH  4    /* "length of quality sequence ... and length of read ... do not match" (:33-43) */

/* Count the lines of the chunk: *d_nlines (device int64).  Line ends follow Python's universal
 * newlines, which is how the reference reads its input (text mode): "\n", "\r\n" and a lone
 * "\r".  d_work: caller scratch of atr_fastq_work_bytes(nbytes) bytes, to be handed unchanged
 * to atr_fastq_index.  The buffer must be readable up to the next multiple of 16 plus one byte. */
size_t atr_fastq_work_bytes(int64_t nbytes);
int atr_fastq_count_lines(const uint8_t *d_bytes, int64_t nbytes, void *d_work, int64_t *d_nlines, void *stream);

/* Positions of the line ends (d_line_ends[nlines], uint32: the last byte of each terminator)
 * and the descriptors of the nlines / 4 records.  *d_error (device int64) receives min over
 * invalid records of (record * 8 + ATR_FASTQ_ERR_*), or INT64_MAX. */
int atr_fastq_index(const uint8_t *d_bytes, int64_t nbytes, const void *d_work, uint32_t *d_line_ends, int64_t nlines,
                    atr_fastq_record *d_records, int64_t *d_error, void *stream);

/* 4-bit tile64 pack (as atr_pack_reads) of sequence[begin:end] of every record; d_begin /
 * d_end may be NULL (the whole sequence line).  d_lens receives the packed lengths.
 * planes != 0: plane64 layout (atr_pack_planes) instead of tile64. */
int atr_pack_records(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                     const int32_t *d_end, int64_t nreads, int max_len, const uint8_t table[256], int planes,
                     uint8_t *d_packed, int32_t *d_lens, int32_t *d_invalid, void *stream);

/* Interval updates, each the device twin of one reference modifier applied to
 * read[begin:end] (records with begin == end are left alone, as `if len(read) == 0`):
 *   atr_clip_batch          UnconditionalCutter.clip(front, back <= 0)   (modifiers.py:565-585, :69-82)
 *   atr_quality_trim_batch  QualityTrimmer / quality_trim_index          (:748-764, _qualtrim.pyx:7-48)
 *                           nextseq != 0: NextseqQualityTrimmer with cutoff_back  (:732-746, _qualtrim.pyx:51-84)
 *   atr_nend_trim_batch     NEndTrimmer                                   (:766-784)
 *                           (d_unmasked_begin/end, may be NULL: AdapterCutter action 'mask' -- the
 *                           bases of [begin, end) outside [unmasked_begin, unmasked_end) read as 'N',
 *                           modifiers.py:155-172; the same pair is honoured by the filter and the writer)
 *   atr_match_trim_batch    Adapter.trimmed(match) for the best match of the round: front != 0
 *                           removes read[:querystop] (adapters/__init__.py:453-457), else keeps
 *                           read[:querystart] (:459-471); d_front[r] selects per read (may be NULL
 *                           = guess rstart == 0, align/__init__.py:108-114 -- 'anywhere' adapters);
 *                           only records with refstop >= 0 and d_active[r] != 0 are touched,
 *                           d_active[r] is cleared for reads without a match (AdapterCutter stops
 *                           at the first failed round, modifiers.py:133-139) and d_matched[r] set. */
int atr_clip_batch(const atr_fastq_record *d_records, int32_t *d_begin, int32_t *d_end, int64_t n, int front,
                   int back, void *stream);
int atr_quality_trim_batch(const uint8_t *d_bytes, const atr_fastq_record *d_records, int32_t *d_begin,
                           int32_t *d_end, int64_t n, int cutoff_front, int cutoff_back, int base, int nextseq,
                           void *stream);
int atr_nend_trim_batch(const uint8_t *d_bytes, const atr_fastq_record *d_records, int32_t *d_begin,
                        int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end, int64_t n,
                        void *stream);
int atr_match_trim_batch(const atr_result *d_matches, const uint8_t *d_front, int default_front, int32_t *d_begin,
                         int32_t *d_end, uint8_t *d_active, uint8_t *d_matched, int64_t n, void *stream);

/* Filters (commands/trim/filters.py:109-184) in the order trim/__init__.py:566-601 installs
 * them; d_dest[r] = the first that fires.  min_len <= 0 / max_len < 0 / max_n < 0: off. */
#define ATR_DEST_KEEP        0
#define ATR_DEST_TOO_SHORT   1
#define ATR_DEST_TOO_LONG    2
#define ATR_DEST_TOO_MANY_N  3
#define ATR_DEST_TRIMMED     4
#define ATR_DEST_UNTRIMMED   5
int atr_read_filter_batch(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                          const int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end,
                          const uint8_t *d_matched, int64_t n, int min_len, int max_len, double max_n,
                          int discard_trimmed, int discard_untrimmed, uint8_t *d_dest, uint8_t *d_fail_mask,
                          void *stream);

/* Paired-end filtering (PairedWrapper, commands/trim/filters.py:66-90): d_fail_mask1/2 are the
 * per-read masks atr_read_filter_batch writes (bit d: the filter with destination d fires;
 * d_dest may be NULL there); a filter fires for the pair when it fires for at least
 * min_affected (1: --pair-filter=any, 2: both) of its reads; d_dest[p] = the first such. */
int atr_pair_filter_batch(const uint8_t *d_fail_mask1, const uint8_t *d_fail_mask2, int64_t n, int min_affected,
                          uint8_t *d_dest, void *stream);

/* InsertAdapterCutter.__call__ after the alignments (commands/trim/modifiers.py:391-496):
 * d_insert = the 3 records per pair of atr_insert_match_batch; d_fallback1/2 = the
 * Adapter.match_to records of read 1 / read 2 (used for pairs without an insert match); the
 * kept intervals of both reads are updated in place, d_matched1/2 receive `read.match is not
 * None`.  symmetric: mirror a lone adapter match onto the other read (:419-446); trim_action:
 * 0 = --no-trim (match only), 1 = trim, 2 = mask (the trimmed end goes to d_unmasked_end*,
 * begin/end stay).  correct_action: -1 = no error correction, else ATR_CORRECT_* -- the
 * overlap of the pairs the reference would correct (:397-446) is corrected IN PLACE in the two
 * FASTQ chunks (bases and qualities, correct_errors(..., truncate_seqs=True), :219-350) before
 * trimming; d_corrected (may be NULL) receives the 2 x int32 changed-base counts per pair and
 * *d_error min over failing pairs of (pair * 8 + code), code 1 KeyError, 2 IndexError,
 * 3 ValueError (the exception the reference raises), or INT64_MAX. */
int atr_insert_plan_batch(const atr_result *d_insert, const atr_result *d_fallback1, const atr_result *d_fallback2,
                          uint8_t *d_bytes1, const atr_fastq_record *d_records1, uint8_t *d_bytes2,
                          const atr_fastq_record *d_records2, int32_t *d_begin1, int32_t *d_end1, int32_t *d_begin2,
                          int32_t *d_end2, int32_t *d_unmasked_end1, int32_t *d_unmasked_end2, int64_t n,
                          int min_insert_len, int symmetric, int trim_action, int correct_action, int min_qual_difference,
                          const uint8_t comp[256], uint8_t *d_matched1, uint8_t *d_matched2, int32_t *d_corrected,
                          int64_t *d_error, void *stream);

/* FastqFormat.format_entry (io/seqio.py:690-699) of every record with d_dest[r] == dest, in
 * input order, into d_out.  First call with d_out == NULL: d_offsets[n + 1] (device int64)
 * receives the exclusive prefix sums of the formatted sizes (d_offsets[n] = total bytes);
 * second call with d_out of that many bytes writes the text.  d_work: scratch of
 * atr_fastq_emit_work_bytes(n) bytes.  record_bytes_hint: average bytes per input record (0:
 * unknown) -- only picks how many records a wave stages at once. */
size_t atr_fastq_emit_work_bytes(int64_t n);
int atr_fastq_emit(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                   const int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end,
                   const uint8_t *d_dest, int dest, int64_t n, int record_bytes_hint, int64_t *d_offsets, void *d_work,
                   uint8_t *d_out, void *stream);

/* Interleaved output (InterleavedFormatter, io/seqio.py:740-749): FastqFormat.format_entry of read 1 and then of
 * read 2 of every pair with d_dest[p] == dest (d_dest NULL: every pair), in pair order, into ONE text.  The two
 * reads have a chunk, a record array, kept intervals and (both or neither) unmasked intervals each; d_bytes1 and
 * d_bytes2 may be the same chunk (an interleaved input) or different ones, and neither needs to start on a 16-byte
 * boundary.
 * PRECONDITION, stricter than atr_fastq_emit's: the kernel loads whole ADDRESS-aligned 16-byte blocks, so up to 15
 * bytes in front of the first '@' a call formats and behind its last quality byte are READ (never written, never
 * used).  They must be readable memory: true for any chunk that lies in one allocation aligned to 16 bytes or more
 * and padded to a multiple of 16 behind its text (what atr_fastq_index asks for already), and for any view into
 * such a chunk; not true for text that ends exactly at the end of a mapping that is not a multiple of 16 long.
 * Two calls, as atr_fastq_emit: with d_out == NULL d_offsets[n + 1] (device int64) receives the exclusive
 * prefix sums of the pairs' formatted sizes (d_offsets[n] = total bytes); with d_out of that many bytes the text is
 * written.  d_work: scratch of atr_fastq_emit_pairs_work_bytes(n) bytes.  pair_bytes_hint: average input bytes per
 * pair (0: unknown) -- only picks how many pairs a wave stages at once.  The offsets are made without global
 * atomics: equal inputs give equal bytes. */
size_t atr_fastq_emit_pairs_work_bytes(int64_t n);
int atr_fastq_emit_pairs(const uint8_t *d_bytes1, const atr_fastq_record *d_records1, const int32_t *d_begin1,
                         const int32_t *d_end1, const int32_t *d_unmasked_begin1, const int32_t *d_unmasked_end1,
                         const uint8_t *d_bytes2, const atr_fastq_record *d_records2, const int32_t *d_begin2,
                         const int32_t *d_end2, const int32_t *d_unmasked_begin2, const int32_t *d_unmasked_end2,
                         const uint8_t *d_dest, int dest, int64_t n, int pair_bytes_hint, int64_t *d_offsets, void *d_work,
                         uint8_t *d_out, void *stream);

/* OverwriteRead (`-w LOWQ,HIGHQ,WINDOW`, commands/trim/modifiers.py:511-563; the W of --op-order), on the kept
 * intervals of the two reads of every pair, in two steps like atr_merge_plan_batch / atr_merge_emit_batch.
 * Plan: d_which[p] = 0 (nothing; also when a read is shorter than the window), 1 (read 1 is overwritten: the sum of
 * read 1's first `window` kept qualities minus the base is < lowq * window and read 2's is >= highq * window) or 2 (the
 * other way round); d_grow1 / d_grow2 [n + 1] (device int64): exclusive prefix sums of the bytes the chunk of read
 * 1 / read 2 must grow by -- name + bases + qualities of every clone, 16-byte padded -- [n] = the total.  d_work:
 * atr_overwrite_work_bytes(n) bytes.  lowq > highq, window < 1: ATR_ERR_INVALID.
 * Apply: the caller has grown the chunks (zeroed) so that the clones of read 1 fit from byte tail1 of d_bytes1 on and
 * those of read 2 from tail2 of d_bytes2 (one chunk for both reads: one tail behind the other); the chunks with
 * their tails must stay below 4 GiB.  Every clone -- the better read's name, its kept bases through comp[] (0: no
 * complement) in reverse order, its kept qualities reversed -- is written there, and the overwritten read's
 * descriptor (flag bit 0 from the better read), begin (0) and end (the clone's length) are re-pointed IN PLACE.
 * *d_error: min over failing pairs of pair * 8 + 1 (a base without a complement, the reference's KeyError), or
 * INT64_MAX. */
size_t atr_overwrite_work_bytes(int64_t n);
int atr_overwrite_plan_batch(const uint8_t *d_bytes1, const atr_fastq_record *d_records1, const int32_t *d_begin1,
                             const int32_t *d_end1, const uint8_t *d_bytes2, const atr_fastq_record *d_records2,
                             const int32_t *d_begin2, const int32_t *d_end2, int64_t n, int lowq, int highq, int window,
                             int quality_base, uint8_t *d_which, int64_t *d_grow1, int64_t *d_grow2, void *d_work,
                             void *stream);
int atr_overwrite_apply_batch(uint8_t *d_bytes1, atr_fastq_record *d_records1, int32_t *d_begin1, int32_t *d_end1,
                              uint8_t *d_bytes2, atr_fastq_record *d_records2, int32_t *d_begin2, int32_t *d_end2, int64_t n,
                              const uint8_t *d_which, const int64_t *d_grow1, const int64_t *d_grow2, int64_t tail1,
                              int64_t tail2, const uint8_t comp[256], int64_t *d_error, void *stream);

/* Demultiplexing (`{name}` in the output path; commands/trim/writers.py:119-154): atr_fastq_emit for many
 * outputs in one pass.  d_group[r] (device int32) is the output of record r, 0 .. n_groups-1; any other value: the
 * record is not written.  The records of output 0 come first in d_out, then those of output 1 ...; inside an
 * output the records keep their input order.  First call with d_out == NULL: d_offsets[n] (device int64) receives
 * the byte position of every written record in d_out (-1 for the others) and d_group_offsets[n_groups + 1] the
 * boundaries of the outputs' segments (d_group_offsets[n_groups] = total bytes); second call with d_out of that
 * many bytes writes the text, every record by the code atr_fastq_emit formats it with.  d_work: scratch of
 * atr_fastq_emit_grouped_work_bytes(n, n_groups) bytes (0: n or n_groups out of range).  record_bytes_hint: as for
 * atr_fastq_emit; the one writing kernel there is takes no hint yet.  The positions are made without global
 * atomics: equal inputs give equal bytes.
 * ATR_ERR_UNSUPPORTED: n_groups > ATR_EMIT_MAX_GROUPS, before anything is launched. */
#define ATR_EMIT_MAX_GROUPS 1024
size_t atr_fastq_emit_grouped_work_bytes(int64_t n, int n_groups);
int atr_fastq_emit_grouped(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                           const int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end,
                           const int32_t *d_group, int n_groups, int64_t n, int record_bytes_hint, int64_t *d_offsets,
                           int64_t *d_group_offsets, void *d_work, uint8_t *d_out, void *stream);

/* The output of every read of a demultiplexed run (Formatters.format, writers.py:138-154): d_group[r] =
 * the output of the adapter of the read's last match (d_adapter_group[d_last_which[r]], device int32 x n_adapters;
 * NULL: the adapter's index) for a read with d_dest[r] == ATR_DEST_KEEP and d_matched[r]; untrimmed_group for a
 * kept read without a match and for ATR_DEST_UNTRIMMED (-1: there is no untrimmed output); -1 for every other read. */
int atr_demux_groups(const uint8_t *d_dest, const uint8_t *d_matched, const int64_t *d_last_which,
                     const int32_t *d_adapter_group, int n_adapters, int untrimmed_group, int64_t n, int32_t *d_group,
                     void *stream);

/* MergeOverlapping.__call__ after the alignment (commands/trim/modifiers.py:864-931), two calls:
 *
 * atr_merge_plan_batch: d_align = one record per pair of Aligner(reverse_complement(read2), error_rate,
 * flags).locate(read1) on the kept intervals (atr_locate_pairs_batch with revcomp_ref; refstop -1 for pairs
 * without an alignment and for pairs that were too short to be aligned, :876-877), d_need[p] = the pair's
 * minimum overlap (:870-874).  d_kind[p] receives 0 (the pair stays a pair) or which of the four shapes
 * of :904-921 the merged read has; d_offsets[n + 1] the exclusive prefix sums of the merged records'
 * formatted sizes (FastqFormat.format_entry of read 1 with the merged sequence; d_offsets[n] = total).
 * *d_error: min over pairs with an "Invalid alignment" (:922-926) of pair * 8 + 4, or INT64_MAX.
 * d_work: scratch of atr_merge_work_bytes(n) bytes.
 *
 * atr_merge_emit_batch: writes the text of the merged records into d_out (d_offsets[n] bytes).
 * correct_action: -1, or ATR_CORRECT_* = MergeOverlapping's mismatch_action: pairs whose alignment has
 * errors and for which d_insert_matched[p] == 0 (may be NULL: none matched; callers also set a non-zero
 * byte for pairs with read.corrected > 0, which correct_errors leaves alone, :232-233) are corrected IN PLACE in
 * the two chunks first (correct_errors(read1, read2, alignment), :900-902) -- except that the mate's
 * bases are the uncorrected ones, as in the reference, which reverse-complements read 2 before (:887).
 * d_corrected (may be NULL): 2 x int32 changed-base counts per pair; *d_error (as initialised by the
 * plan call) additionally receives pair * 8 + {1 KeyError, 2 IndexError, 3 ValueError} of a failing
 * correction. */
size_t atr_merge_work_bytes(int64_t n);
int atr_merge_plan_batch(const atr_result *d_align, const int32_t *d_need, const atr_fastq_record *d_records1,
                         const int32_t *d_begin1, const int32_t *d_end1, const int32_t *d_begin2, const int32_t *d_end2,
                         int64_t n, uint8_t *d_kind, int64_t *d_offsets, void *d_work, int64_t *d_error, void *stream);
int atr_merge_emit_batch(const atr_result *d_align, const uint8_t *d_kind, const uint8_t *d_insert_matched,
                         uint8_t *d_bytes1, const atr_fastq_record *d_records1, uint8_t *d_bytes2,
                         const atr_fastq_record *d_records2, const int32_t *d_begin1, const int32_t *d_end1,
                         const int32_t *d_begin2, const int32_t *d_end2, int64_t n, int correct_action,
                         int min_qual_difference, const uint8_t comp[256], const int64_t *d_offsets, int32_t *d_corrected,
                         int64_t *d_error, uint8_t *d_out, void *stream);


/* Read statistics (ReadStatistics.collect_record, commands/stats.py:194-255; atropos qc, trim --stats, error
 * -a quality) over a device-resident FASTQ chunk.  The statistics live in a caller-allocated block of uint64
 * counters of atr_read_stats_bytes(max_len) bytes: the read count, the longest non-empty read, the number of
 * non-empty reads with qualities, reads skipped because they were longer than `longest`; the length histogram
 * (0 .. max_len), the GC% histogram (101 bins, round((C + G) * 100 / len) half to even), the mean-quality
 * histogram (256 bins, bin = round(sum(q - quality_base) / len) + quality_base), per position below max_len
 * counts of every sequence byte and every quality byte (rows of 256), and for every bin of the three histograms
 * ~(stream index of the first read that landed in it) (0: none; the reference's histograms are dicts in first-seen
 * order, which its median follows).  Counts are integers: the result does not depend on launch shape
 * or on the order of calls.
 *
 * atr_read_stats_bytes: the block size, or ATR_ERR_INVALID (max_len < 1) / ATR_ERR_UNSUPPORTED (max_len >
 * ATR_MAX_LONG_READ_LEN).  atr_read_stats_clear zeroes a block.
 *
 * atr_read_stats_batch adds the records of a chunk (atr_fastq_index) into the block, as atr_fastq_emit would
 * write them: sequence[begin:end], the bases outside [unmasked_begin, unmasked_end) read as 'N'.  d_begin / d_end
 * may be NULL (the whole sequence line), d_unmasked_begin / d_unmasked_end may be NULL (no mask; they need
 * d_begin), d_dest may be NULL (every record; else only those with d_dest[r] == which).  Zero-length reads add
 * to the count and the length histogram only; a record without a quality line (qual_len 0) adds no quality
 * statistics.  longest: an upper bound of the kept lengths, at most max_len; a longer record is not collected
 * but counted among the skipped ones.  quality_base in 0 .. 255.  index_base >= 0: stream index of the chunk's
 * first record (record r is read index_base + r of the stream).
 *
 * atr_read_stats_merge: d_dst += d_src, both blocks laid out for their own max_len (dst_max_len >= src_max_len);
 * d_src's reads follow d_dst's: its read indices are shifted by index_offset >= 0 (d_dst's number of reads).
 * Argument errors are reported before anything is launched. */
int64_t atr_read_stats_bytes(int max_len);
int atr_read_stats_clear(void *d_stats, int max_len, void *stream);
int atr_read_stats_batch(void *d_stats, int max_len, int longest, int quality_base, const uint8_t *d_bytes,
                         const atr_fastq_record *d_records, const int32_t *d_begin, const int32_t *d_end,
                         const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end, const uint8_t *d_dest,
                         int which, int64_t n, int64_t index_base, void *stream);
int atr_read_stats_merge(void *d_dst, int dst_max_len, const void *d_src, int src_max_len, int64_t index_offset,
                         void *stream);


/* Known-contaminant detection (KnownContaminantDetector, commands/detect/__init__.py:495-549; atropos detect
 * --detector known) over a device-resident FASTQ chunk.
 *
 * atr_detect_create builds the detector from nseq known sequences (their bytes back to back in `seqs`, lengths in
 * `lens`): the table of their distinct k-mers and the reverse complements of those.  past_end_bases: n_past_end
 * single bytes B, a read is cut at the leftmost match of `B{8,}.*|B{2,}$`.  thresholds[s]: the smallest n that counts
 * as a hit of sequence s (n / n_kmers > min_kmer_match_frac, evaluated by the caller in the reference's floats;
 * -1 = never).  complexity: doubles [(max_len + 1)][(max_len + 1)], complexity[len][count] = (count / len) *
 * log(count / len) / log(2) as the reference computes it; the device adds the four entries of a read in IEEE double.
 * ATR_ERR_UNSUPPORTED: kmer_size outside 4 .. 32 or too long for a 64-bit key with the alphabet of the known
 * sequences (16 bases at up to 16 letters), more than 128 distinct k-mers in one known sequence, more known sequences
 * than the match kernel's 64 KiB of LDS hold (818 when none has more than 32 distinct k-mers, 556 up to 64, 421 up to
 * 96, 339 up to 128), more than 4 past-end bases, max_len > 320.  Argument errors are
 * reported before the device is touched.
 *
 * The results live in a caller-allocated block of atr_detect_counter_bytes() bytes of uint64 counters (zeroed by
 * atr_detect_clear) that stays on the device across calls: [0] reads kept by the filter, [1] distinct kept
 * sequences, [2] representatives with a byte that has no complement (the reference raises KeyError), [3] reads
 * longer than max_len; from word 8 on, nseq words each of: matches (sum of n over the distinct sequences), hits
 * (distinct sequences with n >= threshold), max_n (largest n among the hits), abundance (distinct sequences that
 * hold the whole known sequence).  All are sums and maxima of integers: independent of launch shape and order.
 *
 * One chunk takes three calls, with a sort by the caller in between:
 *   atr_detect_filter_batch  d_kept[r] = length the read keeps (0 = dropped), d_hashes[r] = hash of the kept bytes.
 *                            longest: upper bound of the read lengths; ATR_ERR_UNSUPPORTED beyond max_len, before
 *                            anything is launched or counted.
 *   atr_detect_mark_batch    d_order[m]: the kept reads sorted by hash, d_head[i]: index in d_order of the first
 *                            read with the hash of entry i.  d_rep[i] = 1 for one read of every distinct kept
 *                            sequence; reads that share a hash are compared byte for byte.
 *   atr_detect_batch         matches the representatives against the known sequences and adds to the counters.
 * Distinctness is per call: a caller that wants it over several chunks puts them into one batch.
 * atr_detect_read copies the block to host memory and waits for the stream. */
int atr_detect_create(const uint8_t *seqs, const int32_t *lens, int nseq, int kmer_size, const uint8_t *past_end_bases,
                      int n_past_end, const int32_t *thresholds, const double *complexity, int max_len, void **out);
void atr_detect_destroy(void *detect);
int64_t atr_detect_counter_bytes(const void *detect);
int atr_detect_clear(const void *detect, void *d_counters, void *stream);
int atr_detect_filter_batch(const void *detect, const uint8_t *d_bytes, const atr_fastq_record *d_records, int64_t n,
                            int longest, int32_t *d_kept, int64_t *d_hashes, void *d_counters, void *stream);
int atr_detect_mark_batch(const void *detect, const uint8_t *d_bytes, const atr_fastq_record *d_records,
                          const int32_t *d_kept, const int64_t *d_order, const int64_t *d_head, int64_t m, uint8_t *d_rep,
                          void *d_counters, void *stream);
int atr_detect_batch(const void *detect, const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_kept,
                     const int64_t *d_order, const uint8_t *d_rep, int64_t m, void *d_counters, void *stream);
int atr_detect_read(const void *detect, const void *d_counters, uint64_t *out, void *stream);


/* De-novo adapter discovery (HeuristicDetector._get_contaminants, commands/detect/__init__.py:568-619; atropos detect
 * --detector heuristic) over the representatives the filter and the distinct pass of atr_detect_* leave.  A detector
 * made by atr_detect_create with nseq == 0 filters without the shortest-known-sequence test; atr_detect_batch refuses
 * such a detector (ATR_ERR_UNSUPPORTED).
 *
 * Every kept base of every representative is a slot; the slots of a read are consecutive (d_start[j]: the first slot
 * of representative j, the exclusive prefix sum of their kept lengths; total: their sum).  A k-mer is known by its
 * class, the dense rank of its text among the k-mers counted at that length (int32; KMER_NO_CLASS = -1 where the slot
 * has no room for k bytes).  Keys are 64-bit integers the caller sorts; nothing is hashed.
 *
 *   atr_detect_kmer_slots      d_reps[nrep]: the records of the representatives.  Writes the table of representatives
 *                              (nrep x 24 bytes), d_slot_rep[total] and d_level[nrep] = kmer_size.
 *   atr_detect_kmer_pair_keys  d_keys[p] = (class of the a-mer at p) << 32 | (class of the b-mer at p + a), or
 *                              INT64_MAX without room for a + b bytes.  A null class array (a or b == 1) is the bytes.
 *   atr_detect_kmer_rank       d_keys[n] sorted ascending, d_idx[n] the entry each came from, d_list (or null: the
 *                              entry is the slot) its slot.  d_cls[slot] = dense rank of the key; per class its run
 *                              d_begin / d_end in the sorted order (count = end - begin) and d_head, the smallest slot that
 *                              holds it; *d_nclasses.  d_work: atr_detect_kmer_rank_work_bytes(n) bytes.
 *   atr_detect_kmer_level      one level k over the n surviving slots (d_list or null: all slots): a class with
 *                              count > min_count is over-represented: level[read] = k + 1 for the reads that hold one,
 *                              a row (level, count, representative and offset of the first occurrence, quirk = 0) in d_cand (int32 x 5, at most
 *                              `capacity` rows are written; d_state[0] counts all), d_cand_of[class] = its row or -1,
 *                              d_state[8 + k] = over-represented classes.  With the classes of level k - 1 (d_cls_prev,
 *                              d_cand_of_prev) a read of exactly k bases whose text is over-represented sets the quirk
 *                              word of the rows of its two (k - 1)-mers.
 *   atr_detect_kmer_next       after it: the slots of reads with level == k + 1 and room for k + 1 bytes into
 *                              d_list_next with d_keys_next = class << 8 | next byte; d_state[1] = how many.
 *   atr_detect_kmer_gather     the texts of ncand rows, row c at d_text_off[c] .. d_text_off[c + 1] of d_out.
 *   atr_detect_kmer_support    npat patterns (npat x 320 bytes, d_pat_len): d_abundance[p] = representatives that hold
 *                              pattern p; d_longest[p] = min over the representatives with level >= len(p) that hold it
 *                              of (first index << 32 | record), all ones if none.
 * d_state: 330 int64 words, zeroed by the caller.  ATR_ERR_UNSUPPORTED, before anything is launched: kmer_size outside
 * 4 .. 32, 2^31 slots or more, a k-mer longer than 320, capacity above 2^20, more than 64 patterns. */
int atr_detect_kmer_slots(const atr_fastq_record *d_records, const int32_t *d_kept, const int64_t *d_reps,
                          const int64_t *d_start, int64_t nrep, int64_t total, int kmer_size, void *d_reptab,
                          int32_t *d_slot_rep, int32_t *d_level, void *stream);
int atr_detect_kmer_pair_keys(const void *d_reptab, const int32_t *d_slot_rep, int64_t total, const uint8_t *d_bytes,
                              const int32_t *d_id_a, int a, const int32_t *d_id_b, int b, int64_t *d_keys, void *stream);
size_t atr_detect_kmer_rank_work_bytes(int64_t n);
int atr_detect_kmer_rank(const int64_t *d_keys, const int64_t *d_idx, const int32_t *d_list, int64_t n, int32_t *d_cls,
                         int32_t *d_begin, int32_t *d_end, int32_t *d_head, int64_t *d_nclasses, void *d_work,
                         size_t work_bytes, void *stream);
int atr_detect_kmer_level(const void *d_reptab, const int32_t *d_slot_rep, const int32_t *d_list, int64_t n,
                          const int32_t *d_cls, const int32_t *d_cls_prev, const int32_t *d_begin, const int32_t *d_end,
                          const int32_t *d_head, int32_t *d_cand_of, const int32_t *d_cand_of_prev, int k, int64_t min_count,
                          int32_t *d_level, int32_t *d_cand, int64_t capacity, int64_t *d_state, void *stream);
int atr_detect_kmer_next(const void *d_reptab, const int32_t *d_slot_rep, const int32_t *d_list, int64_t n,
                         const int32_t *d_cls, const uint8_t *d_bytes, const int32_t *d_level, int k, int32_t *d_list_next,
                         int64_t *d_keys_next, int64_t *d_state, void *stream);
int atr_detect_kmer_gather(const void *d_reptab, int64_t nrep, const uint8_t *d_bytes, const int32_t *d_cand,
                           const int64_t *d_text_off, int64_t ncand, uint8_t *d_out, void *stream);
int atr_detect_kmer_support(const void *d_reptab, int64_t nrep, const uint8_t *d_bytes, const int32_t *d_level,
                            const uint8_t *d_patterns, const int32_t *d_pat_len, int npat, int64_t *d_abundance,
                            uint64_t *d_longest, void *stream);


/* The trim report: summary['trim'] of the reference (RecordHandler.summarize, commands/trim/__init__.py:129-137) and
 * the input totals, counted on the device while the trim pipeline runs.
 *
 * atr_report_create fixes the layout of the counter block of one read of the layout: n_adapters adapters, match
 * lengths 0 .. max_read_len, errors 0 .. max_errors.  ATR_ERR_UNSUPPORTED beyond the table bound (64 adapters,
 * 2^22 words).  The block itself is caller-allocated: atr_report_counters() int64 words, zeroed by the caller, resident
 * on the device for the whole run; every call below adds to it, none reads it back.  Words: [0] input records, [1]
 * input bases, [2] reads with an adapter, [3] matches outside the table (a caller that finds it non-zero must not
 * trust the block), [8 + d] records sent to destination d (ATR_DEST_*, 6 = merged), [16 + d] bases of their final
 * intervals, [24 + slot] bases trimmer `slot` counts as trimmed; from word 32 on per adapter: the base before a 3'
 * match (A, C, G, T, anything else or none; 3 words of padding), then [front | back][length][errors] matches.
 *
 *   atr_report_intervals  after a trimmer stage: (d_begin0, d_end0) the intervals before it, (d_begin1, d_end1) after.
 *                         mode ATR_REPORT_SUBSEQ counts what a read lost (Trimmer.subseq); ATR_REPORT_CLIP counts
 *                         front + back for every read that was not empty (Trimmer.clip counts what it was asked to
 *                         remove); ATR_REPORT_MINCUT counts what front / back still lacked at either end (MinCutter);
 *                         ATR_REPORT_NEND is SUBSEQ for NEndTrimmer, which counts a read of nothing but N twice.
 *   atr_report_adapters   once per adapter round, before the round's trim: d_took[i] != 0 where the round's match
 *                         d_best[i] (8 int16: astart, astop, rstart, rstop, matches, errors) of adapter d_which[i]
 *                         applies to the read [d_begin[i], d_end[i]); d_front / default_front as atr_match_trim_batch.
 *                         weight 1, or 2 for the 'mask' action (AdapterCutter calls Adapter.trimmed twice per match).
 *                         longest: upper bound of the interval lengths; ATR_ERR_UNSUPPORTED beyond max_read_len, before
 *                         anything is launched or counted.  variant: ATR_REPORT_LDS keeps the bins of a block in LDS
 *                         (ATR_ERR_UNSUPPORTED when the table for `longest` does not fit), ATR_REPORT_GLOBAL counts
 *                         with global atomics, ATR_REPORT_AUTO takes LDS when it fits.
 *   atr_report_outputs    after the filters: destinations, written bases, input totals, reads with an adapter.
 * atr_report_read copies the block to host memory and waits for the stream. */
#define ATR_REPORT_SUBSEQ 0
#define ATR_REPORT_CLIP 1
#define ATR_REPORT_MINCUT 2
#define ATR_REPORT_NEND 3
#define ATR_REPORT_AUTO 0
#define ATR_REPORT_LDS 1
#define ATR_REPORT_GLOBAL 2
int atr_report_create(int n_adapters, int max_read_len, int max_errors, void **out);
void atr_report_destroy(void *report);
int64_t atr_report_counters(const void *report);
int atr_report_intervals(const void *report, const atr_fastq_record *d_records, const int32_t *d_begin0,
                         const int32_t *d_end0, const int32_t *d_begin1, const int32_t *d_end1, int64_t n, int mode, int front,
                         int back, int slot, void *d_counters, void *stream);
int atr_report_adapters(const void *report, const uint8_t *d_bytes, const atr_fastq_record *d_records, const uint8_t *d_took,
                        const int16_t *d_best, const int64_t *d_which, const uint8_t *d_front, int default_front,
                        const int32_t *d_begin, const int32_t *d_end, int64_t n, int longest, int weight, int variant,
                        void *d_counters, void *stream);
int atr_report_outputs(const void *report, const atr_fastq_record *d_records, const int32_t *d_begin, const int32_t *d_end,
                       const uint8_t *d_matched, const uint8_t *d_dest, int64_t n, void *d_counters, void *stream);
int atr_report_read(const void *report, const void *d_counters, int64_t *out, void *stream);

/* ---- .gz output compressed on the device (gzip_kernels.hip, deflate_core.hpp) ----------------------------------------
 * atr_gzip_blocks turns n_bytes of text in device memory into one contiguous stream of BGZF members in input order:
 * a gzip member with the 6-byte 'BC' extra field (BSIZE = member size - 1) per ATR_GZIP_BLOCK bytes of text, the
 * last one possibly shorter, none for n_bytes == 0.  Each member holds one dynamic-Huffman deflate block over an
 * LZ77 parse (window 32 KiB), or a stored block where that would not be smaller: a member is at most its input plus
 * 31 bytes.  mtime 0, XFL 0, OS 255: the stream's bytes are a function of the text alone.  Concatenated members
 * are a valid gzip file; a BGZF file ends with the 28-byte member of atr_gzip_eof.
 *   atr_gzip_bound(n_bytes)       capacity the compacted output needs (ATR_ERR_INVALID for n_bytes < 0)
 *   atr_gzip_work_bytes(n_bytes)  bytes of d_work (0 for n_bytes < 0)
 *   d_total                       int64 on the device: the stream's length
 *   d_member_offsets              int64 [members + 1] on the device, or NULL: where every member starts, then the total
 * ATR_ERR_INVALID: a negative size, or out_capacity < atr_gzip_bound(n_bytes); ATR_ERR_UNSUPPORTED: n_bytes >= 4 GiB
 * (the limit of the text tensors) -- both before any pointer is looked at. */
#define ATR_GZIP_BLOCK 65280
int64_t atr_gzip_bound(int64_t n_bytes);
size_t atr_gzip_work_bytes(int64_t n_bytes);
int atr_gzip_eof(uint8_t *buf28);                 /* fills the 28 bytes; returns 28 */
int atr_gzip_blocks(const uint8_t *d_text, int64_t n_bytes, uint8_t *d_out, int64_t out_capacity, int64_t *d_total,
                    int64_t *d_member_offsets, void *d_work, void *stream);

/* ---- BGZF .gz input inflated on the device (gunzip_kernels.hip, inflate_core.hpp) ------------------------------------
 * A BGZF member is a gzip member of at most 64 KiB, compressed and as text, that carries its size in the 'BC' extra
 * subfield (BSIZE = size - 1) and its text size in the trailer (ISIZE), and whose window never reaches into the member
 * before it: the members of a stream are inflated independently, each straight to its place in the text.
 *   atr_bgzf_scan       HOST bytes: walks the whole members at the front of buf[0 .. n_bytes), at most max_members, and
 *                       fills member_at[0 .. k] (byte offsets) and text_at[0 .. k] (running sum of ISIZE), each of
 *                       max_members + 1 entries; *n_members = k, *covered = member_at[k].  It stops at the first member
 *                       that is not whole.  ATR_ERR_INVALID at a header that is no BGZF member -- magic, CM, FEXTRA,
 *                       no 'BC' subfield, SLEN other than 2, ISIZE above 65 536 --, with *n_members / *covered at it.
 *   atr_gunzip_members  DEVICE: member m = d_stream[d_member_at[m] .. d_member_at[m + 1]) is checked (header, BSIZE,
 *                       RFC 1951 in full, ISIZE, CRC-32) and its text written to d_text[d_text_at[m] .. d_text_at[m + 1]).
 *                       d_stream is readable up to the next multiple of 16 beyond n_stream.  d_status[m]: 0, or which
 *                       rule the member broke (inflate_core.hpp INF_E_*; the code is informational); d_bad: their
 *                       number.  A member with a nonzero status leaves its own text range unspecified and touches
 *                       nothing else; ranges that are none (decreasing, beyond n_stream or text_capacity, above
 *                       64 KiB) are such a status.
 * ATR_ERR_INVALID: a negative size, more members than n_stream can hold, a missing pointer; ATR_ERR_UNSUPPORTED:
 * n_stream or text_capacity >= 4 GiB, n_members > 2^22 (ATR_GUNZIP_MAX_MEMBERS) -- all before any pointer is looked at.
 * A capacity below d_text_at[n_members] cannot be seen from the host (the offsets are device memory): the members whose
 * text would not fit get the range status, and nothing of them is stored. */
#define ATR_GUNZIP_MAX_MEMBERS (1 << 22)
int atr_bgzf_scan(const uint8_t *buf, int64_t n_bytes, int64_t max_members, int64_t *member_at, int64_t *text_at,
                  int64_t *n_members, int64_t *covered);
int atr_gunzip_members(const uint8_t *d_stream, int64_t n_stream, const int64_t *d_member_at, const int64_t *d_text_at,
                       int64_t n_members, uint8_t *d_text, int64_t text_capacity, int32_t *d_status, int32_t *d_bad, void *stream);

/* ---- an ordinary .gz member inflated on the device (gunzip_stream_kernels.hip, inflate_stream_core.hpp) ---------------
 * A deflate stream without a member table, split speculatively: block starts are guessed per chunk of chunk_bytes,
 * every chunk is decoded with an unknown window, and only what a chain of confirmed block boundaries reaches is kept.
 *   atr_gunzip_stream_workspace   bytes of d_workspace for a call with these sizes (ATR_ERR_INVALID: no such call)
 *   atr_gunzip_stream   d_stream[0 .. n_stream) is a slab of ONE member's deflate data (n_stream < 2^28); a block starts at
 *                       bit start_bit (any bit, <= 8 n_stream); d_window[0 .. window_len) is the text before it (at most
 *                       32 768 bytes; 0 at a member's start) and crc_in the CRC-32 of the member's text so far.  The
 *                       text of the blocks in [start_bit, end_bit) is written to d_text[0 .. text_len), exactly what zlib
 *                       gives; end_bit is a block boundary: the bit behind the final block (final_seen), else the last
 *                       boundary up to which the text fits text_capacity (< 2^31) and the blocks end inside the slab.  A
 *                       caller goes on from end_bit with the last 32 KiB of text as the window and crc_out as crc_in.
 *                       chunk_bytes (64 .. 2^24) is the spacing of the speculative starts.
 *                       d_result: 8 int64 DEVICE words -- status, end_bit, text_len, final_seen, crc_out, chunks,
 *                       confirmed (chunks whose start the chain reached, chunk 0 among them), redecoded (stretches
 *                       decoded again from confirmed state).  status: 0; ATR_GUNZIP_NEED_INPUT / ATR_GUNZIP_NEED_ROOM
 *                       when not one block ends inside the slab / fits the capacity (end_bit = start_bit); or the rule
 *                       that corrupt data breaks (inflate_core.hpp INF_E_*), the text then being unspecified.
 * Every store lies in d_text[0 .. text_capacity), the workspace or d_result.  Nothing here waits for the kernels. */
#define ATR_GUNZIP_NEED_INPUT 101
#define ATR_GUNZIP_NEED_ROOM 102
int64_t atr_gunzip_stream_workspace(int64_t n_stream, int64_t chunk_bytes, int64_t text_capacity);
int atr_gunzip_stream(const uint8_t *d_stream, int64_t n_stream, int64_t start_bit, const uint8_t *d_window, int32_t window_len,
                      uint32_t crc_in, uint8_t *d_text, int64_t text_capacity, int64_t chunk_bytes, void *d_workspace,
                      int64_t workspace_bytes, int64_t *d_result, void *stream);

/* ---- device-resident FASTA batch -------------------------------------------------------------
 * The reference's FastaReader (io/seqio.py:233-280) over a chunk of text in device memory, under the
 * conditions of atr_fastq_index: below 4 GiB, 16-byte aligned, readable up to the next multiple of 16
 * plus one byte, ending in a line end, starting at a header or at the top of the file.  Every line is
 * stripped of the ASCII whitespace " \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f" (bytes >= 0x80 never count),
 * blank lines and lines that start with '#' are skipped, a line that starts with '>' opens a record.
 * Line ends are Python's universal newlines, as in atr_fastq_index, and the lines are counted by the same call:
 *
 *   atr_fastq_count_lines  nlines, as for FASTQ.
 *   atr_fasta_scan         d_line_ends[nlines]; d_info[0] = records (header lines), d_info[1] = bytes that
 *                          need unwrapping (the sequence lengths of all records with more than one sequence
 *                          line), d_info[2] = line_number * 8 + ATR_FASTA_ERR_HEADER of the first line that
 *                          is neither skipped nor a header in front of the first header (line_number from
 *                          1, skipped lines count), INT64_MAX if there is none.  d_work: scratch of
 *                          atr_fasta_work_bytes(nbytes, nlines) bytes (not the count's), handed unchanged to
 *                          atr_fasta_index.
 *   atr_fasta_index        one atr_fastq_record per record: name = the stripped header after '>';
 *                          the sequence is the single stripped sequence line in place if there is at most
 *                          one, else the record's lines gathered at d_bytes[tail_off ...] (tail_off: a
 *                          multiple of 16 at or beyond nbytes; tail_bytes: the room there, at least
 *                          d_info[1]; tail_off + tail_bytes below 4 GiB); qual_off = qual_len = flags = 0.
 *                          d_record_ends[r]: the last byte of the line end of the record's last line.
 *
 * No global atomics take part in the sums: equal input gives equal descriptors and an equal tail. */
#define ATR_FASTA_ERR_HEADER 1
size_t atr_fasta_work_bytes(int64_t nbytes, int64_t nlines);
int atr_fasta_scan(const uint8_t *d_bytes, int64_t nbytes, uint32_t *d_line_ends, int64_t nlines, void *d_work,
                   int64_t *d_info, void *stream);
int atr_fasta_index(uint8_t *d_bytes, int64_t nbytes, const uint32_t *d_line_ends, int64_t nlines, const void *d_work,
                    int64_t nrec, int64_t tail_off, int64_t tail_bytes, atr_fastq_record *d_records,
                    uint32_t *d_record_ends, void *stream);

/* FastaFormat (io/seqio.py:1008-1067, never wrapped): '>' name '\n' sequence[begin:end] '\n' of every
 * record with d_dest[r] == dest, in input order.  Arguments and the two-call protocol of atr_fastq_emit;
 * bases outside the unmasked interval read 'N'.  Only name_off / name_len / seq_off are read, so a
 * FASTQ batch (and a record whose name was re-pointed) is formatted as well. */
size_t atr_fasta_emit_work_bytes(int64_t n);
int atr_fasta_emit(const uint8_t *d_bytes, const atr_fastq_record *d_records, const int32_t *d_begin,
                   const int32_t *d_end, const int32_t *d_unmasked_begin, const int32_t *d_unmasked_end,
                   const uint8_t *d_dest, int dest, int64_t n, int record_bytes_hint, int64_t *d_offsets, void *d_work,
                   uint8_t *d_out, void *stream);

/* ---- unaligned BAM input (bam_kernels.hip, bam_core.hpp) ---------------------------------------------------------------
 * The inflated bytes of a BAM stream (the BGZF members go through atr_gunzip_members): a header, then records of
 * `block_size` (int32) + block_size bytes each (SAM/BAM specification, section 4.2).
 *   atr_bam_header    HOST bytes: "BAM\1", l_text, the text, n_ref and the reference entries at the front of
 *                     buf[0 .. n_bytes).  ATR_OK with *header_bytes and *n_ref; ATR_BAM_NEED_MORE when the buffer ends
 *                     inside the header; ATR_ERR_INVALID for another magic or a negative length.
 *   atr_bam_walk      DEVICE: d_bam[0 .. n_bytes) (16-byte aligned, readable up to the next multiple of 16 beyond
 *                     n_bytes; no byte at or beyond n_bytes is read), `entry` the offset of a true record start (the
 *                     header's end, 0 for a chunk that begins with a carried-over tail).  d_starts[0 .. count): the
 *                     ascending starts of every WHOLE record, exactly what the serial walk  at += 4 + block_size  from
 *                     entry gives for any byte content (slots at or beyond starts_capacity are not stored: (n_bytes -
 *                     entry) / 36 + 1 holds every table).  The walk stops at the first record that is not whole or
 *                     that is none.  d_result: 4 int64 DEVICE words -- count; consumed (the end of the last whole
 *                     record); the error word offset * 8 + ATR_BAM_ERR_* of the record the walk stopped at, INT64_MAX
 *                     if it merely ran out of bytes (with `final` set, bytes left over are ATR_BAM_ERR_TRUNCATED);
 *                     the tiles whose speculative result had to be repaired.  The bytes are cut into tiles of
 *                     tile_bytes (ATR_BAM_MIN_TILE .. ATR_BAM_MAX_TILE), each walked speculatively from the first
 *                     offset at which a plausible record chain begins (n_ref bounds the reference ids of one); one
 *                     serial pass over the TILES confirms or repairs them.  max_block: the largest block_size that is
 *                     no error (32 .. INT32_MAX).  d_workspace: atr_bam_walk_workspace(n_bytes, tile_bytes) bytes.
 *   atr_bam_to_fastq  DEVICE: '@' name '\n' SEQ '\n' '+' '\n' QUAL '\n' of records d_starts[0 .. n): the name without its
 *                     NUL, the bases from the nibbles through "=ACMGRSVTWYHKDBN", every quality byte + 33 (SAMReader.
 *                     _as_sequence then FastqFormat, io/seqio.py:580-585; no strand flip, no filtering by flag).
 *                     paired: records 2i and 2i + 1 are a pair (PairedEndSAMReader, :618-640) -- equal names; the first
 *                     has flag 0x40 and the second 0x80, or the second has 0x40 and the two are written in swapped
 *                     order; a last record without partner is left out (d_result[2]: records written).  Two calls,
 *                     as atr_fasta_emit: d_out NULL fills d_offsets[0 .. used] (exclusive prefix sum of the texts'
 *                     sizes, by output slot) and d_result[0] = d_offsets[used]; the second call writes d_out.
 *                     d_result[1]: the smallest ordinal * 8 + ATR_BAM_REC_* among the records that the reference
 *                     fails on, INT64_MAX if none; the first call sees l_seq == 0, l_read_name == 0 and the pairs'
 *                     names and flags, the second call '\n' / '\r' in a name and quality bytes above 93 (0xFF, "no
 *                     qualities", among them) and leaves the word of the first call in place.  d_work:
 *                     atr_bam_to_fastq_work_bytes(n) bytes.
 * ATR_ERR_UNSUPPORTED before any pointer is looked at: n_bytes >= 2^32 - 16 (walk); n_bytes >= 2^31 - 16 (decode: a
 * record's text is at most twice its bytes, and text tensors stay below 4 GiB).  Equal input gives equal results. */
#define ATR_BAM_NEED_MORE 1
#define ATR_BAM_MIN_TILE 64
#define ATR_BAM_MAX_TILE (1 << 24)
#define ATR_BAM_ERR_SMALL 1        /* block_size below 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq */
#define ATR_BAM_ERR_BIG 2          /* block_size above max_block */
#define ATR_BAM_ERR_LSEQ 3         /* negative l_seq */
#define ATR_BAM_ERR_TRUNCATED 4    /* final: bytes behind the last whole record */
#define ATR_BAM_REC_LSEQ0 1        /* no sequence (the reference has None) */
#define ATR_BAM_REC_QUAL 2         /* a quality byte above 93 */
#define ATR_BAM_REC_NAME 3         /* a line end in the name, or no name field at all */
#define ATR_BAM_REC_PAIR_NAME 4    /* the two records of a pair are named differently */
#define ATR_BAM_REC_PAIR_FLAGS 5   /* read 1 / read 2 flags of a pair */
int atr_bam_header(const uint8_t *buf, int64_t n_bytes, int64_t *header_bytes, int32_t *n_ref);
int64_t atr_bam_walk_workspace(int64_t n_bytes, int64_t tile_bytes);
int atr_bam_walk(const uint8_t *d_bam, int64_t n_bytes, int64_t entry, int32_t n_ref, int final, int64_t tile_bytes,
                 int64_t max_block, uint32_t *d_starts, int64_t starts_capacity, int64_t *d_result, void *d_workspace,
                 int64_t workspace_bytes, void *stream);
size_t atr_bam_to_fastq_work_bytes(int64_t n);
int atr_bam_to_fastq(const uint8_t *d_bam, int64_t n_bytes, const uint32_t *d_starts, int64_t n, int paired, int64_t *d_offsets,
                     int64_t *d_result, void *d_work, uint8_t *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif

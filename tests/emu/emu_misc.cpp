// emu_misc.cpp -- TEST INFRASTRUCTURE.  CPU run of the per-thread code of
// atropos_amd/csrc/misc_kernels.hip (misc_core.hpp, -DATR_HOST_EMU).
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <vector>

#include "aligner_host.hpp"
#include "misc_core.hpp"
#include "pairs_core.hpp"
#include "pairs_fast_core.hpp"
#include "pairs_long_core.hpp"
#include "wave_core.hpp"
#include "emu_abi.hpp"

using namespace atr;

extern "C" {

size_t emu_multi_locate_work_bytes(int64_t npairs, int max_ref_len) {
    return (size_t)npairs * 3 * ((size_t)max_ref_len + 1) * sizeof(int32_t);
}
EMU_TWIN(multi_locate_work_bytes);

int emu_multi_locate_batch(const uint8_t *refs, int64_t ref_stride, const int32_t *ref_lens, const uint8_t *queries,
                           int64_t q_stride, const int32_t *q_lens, int64_t npairs, double e, int flags,
                           int min_overlap, int max_matches, int max_ref_len, void *work, atr_result *records,
                           int32_t *counts, int out_stride, void *) {
    int16_t *out = (int16_t *)records;
    if (npairs < 0 || flags < 0 || flags > 15 || max_matches < 1 || out_stride < 1) return ATR_ERR_INVALID;
    (void)max_ref_len;
    std::vector<int16_t> dp((size_t)out_stride * 8);
    for (int64_t p = 0; p < npairs; ++p) {
        int16_t *rec = out + (size_t)p * out_stride * 8;
        // what multi_wave_kernel computes (one Hamming distance per candidate) ...
        counts[p] = multi_locate_diag(refs + p * ref_stride, ref_lens[p], queries + p * q_stride, q_lens[p], e, flags,
                                      min_overlap, max_matches, rec, out_stride);
        // ... against the reference's own column-by-column DP, kept as the cross-check
        const int c2 = multi_locate_one(refs + p * ref_stride, ref_lens[p], queries + p * q_stride, q_lens[p], e, flags,
                                        min_overlap, max_matches, (int *)work + p, npairs, dp.data(), out_stride);
        const int stored = std::min((int)counts[p], out_stride);
        if (c2 != counts[p] || memcmp(dp.data(), rec, (size_t)stored * 16) != 0) {
            fprintf(stderr, "emu_multi_locate_batch: the diagonal form disagrees with the DP (pair %lld: %d vs %d hits)\n",
                    (long long)p, (int)counts[p], c2);
            abort();
        }
    }
    return ATR_OK;
}

int emu_compare_batch(const char *ref, int m, const uint8_t *queries, int64_t q_stride, const int32_t *lens,
                      int64_t n, int max_len, int wildcard_ref, int wildcard_query, int suffix, atr_result *records, void *) {
    int16_t *out = (int16_t *)records;
    if (!ref || m < 0 || n < 0) return ATR_ERR_INVALID;
    if (m > 1024) return ATR_ERR_UNSUPPORTED;
    const Tables &T = tables();
    const bool use = wildcard_ref || wildcard_query;
    const uint8_t *tr = use ? (wildcard_ref ? T.iupac : T.acgt) : nullptr;
    const uint8_t *tq = use ? (wildcard_query ? T.iupac : T.acgt) : nullptr;
    for (int64_t p = 0; p < n; ++p)
        compare_one((const uint8_t *)ref, m, queries + p * q_stride, lens ? lens[p] : max_len, tr, tq, suffix != 0,
                    out + p * 8);
    return ATR_OK;
}

// atr_locate_debug: the scratch is the matrix alone
size_t emu_locate_debug_bytes(const atr_aligner *a, int n) { return a && n >= 0 ? 4 * ((size_t)a->p.m + 1) * ((size_t)n + 1) : 0; }
EMU_TWIN(locate_debug_bytes);

int emu_locate_debug(const atr_aligner *a, const uint8_t *d_packed, int n, void *d_matrix, atr_result *d_out, void *) {
    const uint32_t *packed = (const uint32_t *)d_packed;
    int32_t *matrix = (int32_t *)d_matrix;
    int16_t *rec = (int16_t *)d_out;
    if (!a || n < 0) return ATR_ERR_INVALID;
    const LocateParams &lp = a->p;
    const int p0 = round_up_rows(lp.m) - lp.m;
    std::vector<DebugCell> col((size_t)lp.m + 1);
    locate_debug_one(lp.m, n, a->max_error_rate, a->flags, a->min_overlap, a->indel_cost,
                     [&lp, p0](int i, uint32_t qc) { const int b = p0 + i - 1; return ((lp.nmask[qc][b >> 5] >> (b & 31)) & 1u) != 0u; },
                     [packed](int j) { return (packed[(size_t)((j - 1) >> 5) * 256 + (((j - 1) >> 3) & 3)] >> (4 * ((j - 1) & 7))) & 15u; },
                     col.data(), matrix, rec);
    return ATR_OK;
}
EMU_TWIN(locate_debug);

// atr_compare_packed
int emu_compare_packed(const atr_aligner *a, const uint8_t *d_packed, const int32_t *lens, int64_t n, int max_len, int suffix,
                       atr_result *records, void *) {
    const uint32_t *packed = (const uint32_t *)d_packed;
    int16_t *out = (int16_t *)records;
    if (!a || n < 0 || max_len < 0) return ATR_ERR_INVALID;
    if (max_len > ATR_MAX_READ_LEN) return ATR_ERR_UNSUPPORTED;
    const int nchunks = (max_len + 31) / 32;
    for (int64_t p = 0; p < n; ++p) {
        const uint32_t *mine = packed + ((size_t)(p / 64) * nchunks * 64 + (p % 64)) * 4;
        const int len = std::max(0, std::min(lens ? lens[p] : max_len, max_len));
        compare_packed_one(a->p.nmask, a->p.m, [mine](int w) { return mine[(size_t)(w >> 2) * 256 + (w & 3)]; }, len,
                           suffix != 0, out + p * 8);
    }
    return ATR_OK;
}

int emu_adapter_postfilter(atr_result *records, int64_t n, int m, int min_overlap, double max_error_rate,
                           const double *rmp, int rmp_ld, double max_rmp, int accept_full, void *) {
    int16_t *rec = (int16_t *)records;
    for (int64_t p = 0; p < n; ++p)
        adapter_postfilter_one(rec + 8 * p, m, min_overlap, max_error_rate, rmp, rmp_ld, max_rmp, accept_full != 0);
    return ATR_OK;
}
EMU_TWIN(adapter_postfilter);

// atr_insert_correct_batch: gated on the insert-match records; with the plane buffers the
// plane-guided walk of correct_planes_kernel, else the byte walk
int emu_insert_correct_batch(const atr_result *insert_records, const uint8_t *d_planes1, const uint8_t *d_planes2, int planes_max_len,
                             uint8_t *s1, uint8_t *q1, const int32_t *l1, uint8_t *s2, uint8_t *q2, const int32_t *l2,
                             int64_t stride, int64_t n, int max_len, int action, int min_qual_diff, const uint8_t *comp,
                             int32_t *changed, int32_t *newlen, void *) {
    const int16_t *records = (const int16_t *)insert_records;
    const uint32_t *planes1 = (const uint32_t *)d_planes1, *planes2 = (const uint32_t *)d_planes2;
    const int nchunks = (planes_max_len + 31) / 32;
    for (int64_t p = 0; p < n; ++p) {
        const int len1 = l1 ? l1[p] : max_len, len2 = l2 ? l2[p] : max_len;
        const int16_t *rec = records + 24 * p;
        if (rec[1] < 0 || rec[5] <= 0) {
            changed[2 * p] = changed[2 * p + 1] = 0;
            newlen[2 * p] = len1; newlen[2 * p + 1] = len2;
            continue;
        }
        if (!planes1) {
            correct_errors_one(s1 + p * stride, q1 ? q1 + p * stride : nullptr, len1, s2 + p * stride,
                               q2 ? q2 + p * stride : nullptr, len2, rec, action, min_qual_diff, true, comp, changed + 2 * p,
                               newlen + 2 * p);
            continue;
        }
        const int64_t tile = p >> 6;
        const int lane = (int)(p & 63), j = rec[3];
        auto word = [&](const uint32_t *planes, int plane, int idx) {
            return planes[(((size_t)tile * nchunks + idx) * 64 + lane) * 4 + plane];
        };
        uint32_t mism[10] = {0};                                     // ATR_INSERT_MAX_READ / 32 words
        for (int w = 0; w < nchunks; ++w) {
            const uint32_t a[4] = {word(planes1, 0, w), word(planes1, 1, w), word(planes1, 2, w), word(planes1, 3, w)};
            mism[w] = facing_mismatches(a, [&](int plane, int idx) { return word(planes2, plane, idx); }, nchunks, j, w);
        }
        auto code_at = [&](const uint32_t *planes, int pos) {
            uint32_t c = 0;
            for (int pl = 0; pl < 4; ++pl) c |= ((word(planes, pl, pos >> 5) >> (pos & 31)) & 1u) << pl;
            return c;
        };
        correct_errors_planes_one<10>(s1 + p * stride, q1 ? q1 + p * stride : nullptr, len1, s2 + p * stride,
                                     q2 ? q2 + p * stride : nullptr, len2, j, mism, nchunks, action, min_qual_diff, comp,
                                     changed + 2 * p, newlen + 2 * p, [&](int w, int b) { return code_at(planes1, 32 * w + b); },
                                     [&](int pos) { return code_at(planes2, pos); });
    }
    return 0;
}

int emu_correct_errors_batch(uint8_t *s1, uint8_t *q1, const int32_t *l1, uint8_t *s2, uint8_t *q2,
                             const int32_t *l2, int64_t stride, const int16_t *im, const uint8_t *mask, int64_t n,
                             int max_len, int action, int min_qual_diff, int truncate, const uint8_t comp[256],
                             int32_t *changed, int32_t *newlen, void *) {
    if (n < 0 || action < 0 || action > 2 || !comp) return ATR_ERR_INVALID;
    if ((q1 == nullptr) != (q2 == nullptr)) return ATR_ERR_INVALID;
    if (action != 0 && !q1) return ATR_ERR_INVALID;
    for (int64_t p = 0; p < n; ++p) {
        const int len1 = l1 ? l1[p] : max_len, len2 = l2 ? l2[p] : max_len;
        if (mask && !mask[p]) {
            changed[2 * p] = changed[2 * p + 1] = 0;
            newlen[2 * p] = len1; newlen[2 * p + 1] = len2;
            continue;
        }
        correct_errors_one(s1 + p * stride, q1 ? q1 + p * stride : nullptr, len1, s2 + p * stride,
                           q2 ? q2 + p * stride : nullptr, len2, im + 4 * p, action, min_qual_diff, truncate != 0,
                           comp, changed + 2 * p, newlen + 2 * p);
    }
    return ATR_OK;
}
EMU_TWIN(multi_locate_batch);
EMU_TWIN(compare_batch);
EMU_TWIN(compare_packed);
EMU_TWIN(insert_correct_batch);
EMU_TWIN(correct_errors_batch);

// atr_locate_pairs_batch: one pair after the other, column and staged reference in plain arrays
// test hook: also exercise the LDS-column variant (the library's fallback when stream-ordered allocation is missing)
int emu_pairs_use_lds_column = 0;

// test hooks of the fast pipeline (pairs_fast_core.hpp): 0 = off (every pair takes the full sweep), 1 = on;
// widen: run the banded pass with the widest class / extra rows, as a lane does whose wave mates need more
int emu_pairs_fast = 1, emu_pairs_fast_widen = 0, emu_pairs_fast_debug = 0;
long long emu_pairs_fast_stats[4];                                 // none / band ok / full sweep / certificate failed

}  // extern "C"

// One pair through the fast pipeline; returns false when the pair needs the full sweep.
template <int NW>
static bool emu_pair_fast_one(const atr::PairFastParams &fp, const uint32_t *rp, int rndw, int m, bool revcomp,
                              const uint32_t *qp, int qndw, int n, int need, uint32_t pair, uint32_t *rec) {
    using namespace atr;
    const PairParams &p = fp.pp;
    const bool sr = (p.flags & ATR_START_WITHIN_SEQ1) != 0, sq = (p.flags & ATR_START_WITHIN_SEQ2) != 0;
    if (m < 1 || n < 1 || (int)p.thr[m] > PF_MAX_K) { ++emu_pairs_fast_stats[2]; return false; }
    uint32_t tab[PF_TAB_ROWS * NW];
    bool known = pf_build_masks<NW>(tab, 1, rp, rndw, m, revcomp, sq);
    const int k = (int)p.thr[m];
    const int n_sweep = sq ? n : std::min(n, m + k);                   // _align.pyx:314-321
    const bool scan_last = n_sweep == n;
    PfScan T;
    pf_stream_init(T, need);
    std::vector<int> rowm_cost((size_t)n_sweep + 1, 0);
    PfMyers<NW> S;
    pf_myers_init<NW>(S, m, sr);
    for (int j = 1; j <= n_sweep; ++j) {
        const uint32_t code = packed_code(qp, j - 1);
        known = known && pf_codes_known(code);
        const int row = std::min(pf_code_row(code), PF_TAB_ROWS - 1);      // (an unknown code: the pair falls back anyway)
        uint32_t eq[NW];
        for (int w = 0; w < NW; ++w) eq[w] = tab[row * NW + w];
        pf_myers_step<NW>(S, eq, sq ? 0u : 1u);
        rowm_cost[(size_t)j] = S.score;
        pf_rowm_pass1(T, m, j, S.score, k, (int)fp.g_ap[j], (int)fp.g_as[j], p.min_overlap);
    }
    for (int j = n_sweep + 1; j <= n; ++j) known = known && pf_codes_known(packed_code(qp, j - 1));
    const bool er = (p.flags & ATR_STOP_WITHIN_SEQ1) != 0;
    if (scan_last)
        pf_stream_lastcol<NW>(T, S.pv, S.mv, m, n, sq, er, p.thr, (int)fp.g_ap[n], (int)fp.g_as[n], p.min_overlap, need, false);
    {
        const int mlb = pf_mlb_eff(T, need);
        for (int j = 1; j <= n_sweep; ++j) pf_rowm_pass2(T, m, j, rowm_cost[(size_t)j], k, (int)fp.g_ap[j], p.min_overlap, mlb);
    }
    if (scan_last)
        pf_stream_lastcol<NW>(T, S.pv, S.mv, m, n, sq, er, p.thr, (int)fp.g_ap[n], (int)fp.g_as[n], p.min_overlap, need, true);
    if (!known) { ++emu_pairs_fast_stats[2]; return false; }
    PfDecision D;
    pf_decide(T, m, n, need, pair, D);
    if (emu_pairs_fast_debug && D.kind == 2) fprintf(stderr, "pair %u wide: lo %d hi %d mlb %d rl %d\n", pair, D.task.d_lo, D.task.row_first, D.task.mlb, D.task.row_last);
    if (emu_pairs_fast_debug)
        fprintf(stderr, "pair %u m %d n %d kind %d cls %d d_lo %d rf %d rl %d mlb %d cand_first %d\n", pair, m, n,
                D.kind, D.cls, D.kind == 1 ? D.task.d_lo : 0, D.kind == 1 ? D.task.row_first : 0, D.kind == 1 ? D.task.row_last : 0,
                D.kind == 1 ? D.task.mlb : 0, D.kind == 1 ? D.task.cand_first : 0);
    if (D.kind == 0) {
        rec[0] = 0xFFFF0000u; rec[1] = rec[2] = rec[3] = 0u;
        ++emu_pairs_fast_stats[0];
        return true;
    }
    if (D.kind == 2) { ++emu_pairs_fast_stats[2]; return false; }
    PfBandLane L;
    L.d_lo = D.task.d_lo; L.row_first = D.task.row_first; L.row_last = D.task.row_last; L.m = m; L.n = n; L.n_sweep = n_sweep;
    L.cand_first = D.task.cand_first; L.mlb = D.task.mlb;
    L.scan_last = scan_last; L.live = true;
    const int cls = emu_pairs_fast_widen ? PF_CLASSES - 1 : D.cls;
    const int wb = pf_class_width(cls);
    int nrows = std::max(0, (int)L.row_last - (int)L.row_first + 1);
    if (emu_pairs_fast_widen) nrows += 9;
    PfRefStream rs;
    PfQueryStream qs;
    rs.init(rp, rndw, m, revcomp, L.row_first);
    qs.init(qp, qndw, L.row_first + L.d_lo - 1);
    switch (cls) {
        case 0: pf_band_sweep<16>(L, nrows, rs, qs, p, p.thr, fp.g_ap, rec); break;
        case 1: pf_band_sweep<32>(L, nrows, rs, qs, p, p.thr, fp.g_ap, rec); break;
        case 2: pf_band_sweep<48>(L, nrows, rs, qs, p, p.thr, fp.g_ap, rec); break;
        case 3: pf_band_sweep<64>(L, nrows, rs, qs, p, p.thr, fp.g_ap, rec); break;
        case 4: pf_band_sweep<80>(L, nrows, rs, qs, p, p.thr, fp.g_ap, rec); break;
        case 5: pf_band_sweep<96>(L, nrows, rs, qs, p, p.thr, fp.g_ap, rec); break;
        case 6: pf_band_sweep<112>(L, nrows, rs, qs, p, p.thr, fp.g_ap, rec); break;
        default: pf_band_sweep<128>(L, nrows, rs, qs, p, p.thr, fp.g_ap, rec); break;
    }
    ++emu_pairs_fast_stats[1];
    return true;
}

// pairs_wave_kernel (pairs_wave.hip) for one pair: the 64 lanes in lock step, the cross-lane move spelled out
template <bool XREP, bool SQ, int R, bool AND_MODE>
static void emu_pair_wave_one(const atr::PairParams &p, const uint32_t *rp, int m, bool revcomp, const uint32_t *qp, int n,
                              uint32_t *rec) {
    using namespace atr;
    constexpr int PAD = 64;
    constexpr uint32_t CAPW = (uint32_t)PAIRS_ORG_BIAS | ((uint32_t)INIT_COST_CAP << CSH);
    const bool sr = (p.flags & ATR_START_WITHIN_SEQ1) != 0, er = (p.flags & ATR_STOP_WITHIN_SEQ1) != 0;
    int k = (int)(p.e * m);
    if (k < 0) k = -1;
    int indel = p.indel_cost > k ? k + 1 : p.indel_cost;
    if (indel < 1) indel = 1;
    const uint32_t insw = (uint32_t)indel * COST1 + PRIO_INS, delw = (uint32_t)indel * COST1 + PRIO_DEL;
    const uint32_t klimit = (uint32_t)(k + 1) << CSH;
    const int max_n = SQ ? n : std::min(n, m + k), min_n = XREP ? 0 : std::max(0, n - m - k);
    const int span = std::max(0, max_n - min_n);
    const bool scan = max_n == n;
    std::vector<uint32_t> s_code(PAD + (PAIRS_MAX_LEN + 31) / 32 * 32 + 2 * PAD, 0xEEEEEEEEu), s_ref(PAIRS_MAX_LEN + 64, 0u);
    for (int j = 0; j < n; ++j) s_code[PAD + j] = packed_code(qp, j);
    for (int i = 0; i < m; ++i) {
        const uint32_t c = packed_code(rp, i);
        if (revcomp) s_ref[m - 1 - i] = bitrev4(c); else s_ref[i] = c;
    }
    const WaveGeom g = wave_geom(m, R);
    WaveRows<R> W[64];
    uint32_t upa[64], upb[64];
    int a[64];
    Best best[64];
    for (int l = 0; l < 64; ++l) {
        for (int rr = 0; rr < R; ++rr) {
            const int row = wave_slot_row(g, R, l, rr);
            uint32_t mask = 0u;
            if (row >= 1 && row <= m) {
                const uint32_t c = s_ref[row - 1];
                if (AND_MODE) { for (uint32_t q = 0; q < 16; ++q) mask |= ((c & q) == 0u ? 1u : 0u) << q; }
                else mask = ~(1u << c) & 0xFFFFu;
            }
            W[l].rowmask[rr] = mask;
            W[l].lstep[rr] = row < 0 ? 0u : row == 0 ? (SQ ? 1u : (uint32_t)indel << CSH) : delw;
            W[l].col[rr] = row < 0 ? WAVE_HUGE : init_word(row, min_n, sr, SQ, indel) + (uint32_t)(PAIRS_ORG_BIAS - (int)ORG_BIAS);
        }
        a[l] = min_n - l - 1;
        best[l].key = COST_FIELD_MAX - (m + n); best[l].word = (uint32_t)(m + n) << CSH;
        best[l].ref_stop = m; best[l].query_stop = n; best[l].matches = 0;
        upa[l] = upb[l] = WAVE_HUGE;
    }
    auto shr1 = [&](uint32_t *keep) {                               // keep[l] = bottom cell of lane l - 1; lane 0 untouched
        uint32_t tmp[64];
        for (int l = 1; l < 64; ++l) tmp[l] = W[l - 1].col[R - 1];
        for (int l = 1; l < 64; ++l) keep[l] = tmp[l];
    };
    shr1(upa);
    const uint32_t *code = s_code.data() + PAD;
    const int steps = span > 0 ? span + g.lanes - 1 : 0;
    auto trip = [&](bool guarded) {
        uint32_t bottom[4][64];
        bool hit[4][64];
        int a0[64];
        for (int l = 0; l < 64; ++l) a0[l] = a[l];
        for (int s = 0; s < 4; ++s) {
            uint32_t *up = (s & 1) ? upa : upb, *diag = (s & 1) ? upb : upa;
            shr1(up);
            for (int l = 0; l < 64; ++l) {
                uint32_t nw[R];
                wave_rows_step<XREP, SQ, R, CAPW>(W[l], diag[l], up[l], code[a0[l] + 1 + s], insw, nw);
                bottom[s][l] = nw[R - 1];
                if (guarded) {
                    ++a[l];
                    const bool active = (unsigned)(a[l] - min_n) < (unsigned)span;
                    hit[s][l] = XREP && l == g.lanes - 1 && active && nw[R - 1] < klimit;
                    if (active) for (int rr = 0; rr < R; ++rr) W[l].col[rr] = nw[rr];
                } else {
                    for (int rr = 0; rr < R; ++rr) W[l].col[rr] = nw[rr];
                }
            }
        }
        for (int l = 0; l < 64; ++l) {
            if (!guarded) {
                a[l] += 4;
                for (int s = 0; s < 4; ++s) hit[s][l] = XREP && l == g.lanes - 1 && bottom[s][l] < klimit;
            }
            for (int s = 0; s < 4; ++s)
                if (hit[s][l]) consider<XREP, PAIRS_ORG_BIAS>(best[l], bottom[s][l], m, a0[l] + 2 + s, p.min_overlap, p.thr, indel);
        }
    };
    int t = 1;
    for (; t <= steps && t <= g.lanes - 1; t += 4) trip(true);
    for (; t + 3 <= span; t += 4) trip(false);
    for (; t <= steps; t += 4) trip(true);
    Best fin = best[g.lanes - 1];
    if (scan) {
        const int first_row = er ? 0 : m;
        Best mine[64];
        int top = -1;
        for (int l = 0; l < 64; ++l) {
            mine[l].key = -1; mine[l].word = 0; mine[l].ref_stop = 0; mine[l].query_stop = n; mine[l].matches = 0;
            for (int rr = 0; rr < R; ++rr) {
                const int row = wave_slot_row(g, R, l, rr);
                if (row >= first_row && row <= m) consider<XREP, PAIRS_ORG_BIAS>(mine[l], W[l].col[rr], row, n, p.min_overlap, p.thr, indel);
            }
            top = std::max(top, mine[l].key < 0 ? -1 : (mine[l].key << 6) | (63 - l));
        }
        if (top >= 0 && (top >> 6) > fin.key) {
            const int src = 63 - (top & 63);
            fin.key = top >> 6; fin.word = mine[src].word; fin.ref_stop = mine[src].ref_stop; fin.query_stop = n;
            fin.matches = mine[src].matches;
        }
    }
    const int cost = (int)(fin.word >> CSH);
    int refstart = 0, querystart = 0, refstop = -1, querystop = 0, matches = 0, errors = 0;
    if (cost != m + n) {
        const int origin = (int)(fin.word & ORG_MASK) - PAIRS_ORG_BIAS;
        if (origin >= 0) querystart = origin; else refstart = -origin;
        refstop = fin.ref_stop; querystop = fin.query_stop; matches = fin.matches; errors = cost;
    }
    rec[0] = (uint32_t)(refstart & 0xFFFF) | ((uint32_t)(refstop & 0xFFFF) << 16);
    rec[1] = (uint32_t)(querystart & 0xFFFF) | ((uint32_t)(querystop & 0xFFFF) << 16);
    rec[2] = (uint32_t)(matches & 0xFFFF) | ((uint32_t)(errors & 0xFFFF) << 16);
    rec[3] = 0;
}

template <int R>
static void emu_pair_wave_r(const atr::PairParams &p, const uint32_t *rp, int m, bool revcomp, const uint32_t *qp, int n, uint32_t *rec) {
    const bool xrep = (p.flags & ATR_STOP_WITHIN_SEQ2) != 0, sq = (p.flags & ATR_START_WITHIN_SEQ2) != 0, am = p.and_mode != 0;
#define ATR_EMU_PW(X, S, A) emu_pair_wave_one<X, S, R, A>(p, rp, m, revcomp, qp, n, rec)
    if (xrep && sq) { if (am) ATR_EMU_PW(true, true, true); else ATR_EMU_PW(true, true, false); }
    else if (xrep) { if (am) ATR_EMU_PW(true, false, true); else ATR_EMU_PW(true, false, false); }
    else if (sq) { if (am) ATR_EMU_PW(false, true, true); else ATR_EMU_PW(false, true, false); }
    else { if (am) ATR_EMU_PW(false, false, true); else ATR_EMU_PW(false, false, false); }
#undef ATR_EMU_PW
}

extern "C" {

size_t emu_locate_pairs_long_work_bytes(int64_t, int) { return 16; }
EMU_TWIN(locate_pairs_long_work_bytes);

// atr_locate_pairs_long_batch: pairs_long_core.hpp, one pair after the other
int emu_locate_pairs_long_batch(const uint8_t *d_ref_packed, const int32_t *ref_lens, int ref_max_len, int revcomp,
                                const uint8_t *d_qry_packed, const int32_t *qry_lens, int qry_max_len, int64_t npairs,
                                double e, int flags, int wildcard_ref, int wildcard_query, int min_overlap, int indel_cost,
                                atr_result *records, void *, void *) {
    const uint32_t *ref_packed = (const uint32_t *)d_ref_packed, *qry_packed = (const uint32_t *)d_qry_packed;
    uint32_t *out = (uint32_t *)records;
    if (npairs < 0 || flags < 0 || flags > 15 || min_overlap < 1 || indel_cost < 1) return ATR_ERR_INVALID;
    if (ref_max_len > ATR_MAX_LONG_READ_LEN || qry_max_len > ATR_MAX_LONG_READ_LEN) return ATR_ERR_UNSUPPORTED;
    if (!(e >= 0.0) || e * (double)ref_max_len > (double)atr::PAIRS_LONG_MAX_K) return ATR_ERR_UNSUPPORTED;
    atr::PairLongParams p;
    p.e = e; p.flags = flags; p.min_overlap = min_overlap; p.indel_cost = indel_cost;
    p.and_mode = (wildcard_ref || wildcard_query) ? 1 : 0;
    const int rch = (ref_max_len + 31) / 32, qch = (qry_max_len + 31) / 32;
    std::vector<uint64_t> col((size_t)ref_max_len + 1);
    std::vector<uint8_t> refc((size_t)ref_max_len + 1);
    for (int64_t r = 0; r < npairs; ++r) {
        const int m = ref_lens ? ref_lens[r] : ref_max_len, n = qry_lens ? qry_lens[r] : qry_max_len;
        const uint32_t *rp = ref_packed + ((size_t)(r >> 6) * rch * 64 + (r & 63)) * 4;
        const uint32_t *qp = qry_packed + ((size_t)(r >> 6) * qch * 64 + (r & 63)) * 4;
        if (p.and_mode) atr::locate_pair_long<true>(col.data(), 1, refc.data(), 1, rp, m, revcomp != 0, qp, n, p, out + 4 * r);
        else atr::locate_pair_long<false>(col.data(), 1, refc.data(), 1, rp, m, revcomp != 0, qp, n, p, out + 4 * r);
    }
    return ATR_OK;
}
EMU_TWIN(locate_pairs_long_batch);

// atr_locate_pairs_*_batch: one body, the kernel family named by ``path`` (ATR_PAIRS_*)
static int pairs_batch(const uint32_t *ref_packed, const int32_t *ref_lens, int ref_max_len, int revcomp,
                       const uint32_t *qry_packed, const int32_t *qry_lens, int qry_max_len, int64_t npairs,
                       double e, int flags, int wildcard_ref, int wildcard_query, int min_overlap, int indel_cost,
                       const int32_t *need, int path, uint32_t *out) {
    if (npairs < 0) return ATR_ERR_INVALID;
    atr::PairParams p;
    const int rc = atr::pairs_params(e, flags, wildcard_ref, wildcard_query, min_overlap, indel_cost, ref_max_len,
                                     qry_max_len, p);
    if (rc != ATR_OK) return rc;
    const int rch = (ref_max_len + 31) / 32, qch = (qry_max_len + 31) / 32;
    std::vector<uint32_t> col((size_t)ref_max_len + 1), refw((size_t)(ref_max_len + 7) / 8 + 1);
    if (path < ATR_PAIRS_AUTO || path > ATR_PAIRS_WAVE) return ATR_ERR_INVALID;
    if (path == ATR_PAIRS_WAVE && !atr::wave_pairs_applies(ref_max_len, 0)) return ATR_ERR_UNSUPPORTED;
    const bool wave = path == ATR_PAIRS_WAVE || (path == ATR_PAIRS_AUTO && atr::wave_pairs_applies(ref_max_len, npairs));
    const long long fast_min = (ref_max_len <= 160 || need != nullptr) ? atr::PAIRS_FAST_MIN_PAIRS : 3 * atr::PAIRS_FAST_MIN_PAIRS / 2;
    const bool worth = path == ATR_PAIRS_FAST || npairs >= fast_min;                           // as the library
    const bool fast = !wave && path != ATR_PAIRS_FULL && (path == ATR_PAIRS_FAST || emu_pairs_fast) && worth &&
                      atr::pairs_fast_applies(e, flags, wildcard_ref, wildcard_query, indel_cost, ref_max_len, qry_max_len);
    static atr::PairFastParams fp;
    if (fast) { fp.pp = p; atr::pairs_fast_tables(e, fp); }
    for (int64_t r = 0; r < npairs; ++r) {
        const int64_t tile = r >> 6;
        const int lane = (int)(r & 63);
        int m = ref_lens ? ref_lens[r] : ref_max_len, n = qry_lens ? qry_lens[r] : qry_max_len;
        if (m > ref_max_len) m = ref_max_len;
        if (n > qry_max_len) n = qry_max_len;
        const uint32_t *rp = ref_packed + ((size_t)tile * rch * 64 + lane) * 4;
        const uint32_t *qp = qry_packed + ((size_t)tile * qch * 64 + lane) * 4;
        if (wave) {                                                  // as the library: a wavefront per pair
            switch (atr::wave_pair_rows(ref_max_len)) {
                case 1: emu_pair_wave_r<1>(p, rp, m, revcomp != 0, qp, n, out + 4 * r); break;
                case 2: emu_pair_wave_r<2>(p, rp, m, revcomp != 0, qp, n, out + 4 * r); break;
                case 3: emu_pair_wave_r<3>(p, rp, m, revcomp != 0, qp, n, out + 4 * r); break;
                case 4: emu_pair_wave_r<4>(p, rp, m, revcomp != 0, qp, n, out + 4 * r); break;
                default: emu_pair_wave_r<5>(p, rp, m, revcomp != 0, qp, n, out + 4 * r); break;
            }
            continue;
        }
        if (fast) {                                                  // as the library: costs, threats, banded payload
            const int nd = need ? need[r] : 1;
            bool done;
            if (ref_max_len <= 160) done = emu_pair_fast_one<5>(fp, rp, rch * 4, m, revcomp != 0, qp, qch * 4, n, nd, (uint32_t)r, out + 4 * r);
            else if (ref_max_len <= 256) done = emu_pair_fast_one<8>(fp, rp, rch * 4, m, revcomp != 0, qp, qch * 4, n, nd, (uint32_t)r, out + 4 * r);
            else done = emu_pair_fast_one<10>(fp, rp, rch * 4, m, revcomp != 0, qp, qch * 4, n, nd, (uint32_t)r, out + 4 * r);
            if (done) continue;
        }
        if (ref_max_len <= atr::PAIRS_REG_MAX) {                     // as the library: register-column variant
            // the wave's smallest m (select range of the row-m pick-up)
            int mlo = 0x7fffffff, mhi = 0;
            for (int64_t t = tile * 64; t < std::min<int64_t>(npairs, tile * 64 + 64); ++t) {
                mlo = std::min(mlo, std::min(ref_lens ? ref_lens[t] : ref_max_len, ref_max_len));
                mhi = std::max(mhi, std::min(ref_lens ? ref_lens[t] : ref_max_len, ref_max_len));
            }
            uint32_t tab[16 * 5];
#define ATR_EMU_REG(MT)                                                                                            \
            do {                                                                                                       \
                const bool xrep = (p.flags & ATR_STOP_WITHIN_SEQ2) != 0;                                               \
                if (p.and_mode) { atr::build_match_masks<MT, true>(tab, 1, rp, m, revcomp != 0);                       \
                                  if (xrep) atr::locate_pair_reg<MT, true, true>(tab, 1, m, mlo, mhi, qp, n, p, p.thr, out + 4 * r); \
                                  else atr::locate_pair_reg<MT, true, false>(tab, 1, m, mlo, mhi, qp, n, p, p.thr, out + 4 * r); } \
                else { atr::build_match_masks<MT, false>(tab, 1, rp, m, revcomp != 0);                                 \
                       if (xrep) atr::locate_pair_reg<MT, false, true>(tab, 1, m, mlo, mhi, qp, n, p, p.thr, out + 4 * r); \
                       else atr::locate_pair_reg<MT, false, false>(tab, 1, m, mlo, mhi, qp, n, p, p.thr, out + 4 * r); } \
            } while (0)
            if (ref_max_len <= 64) ATR_EMU_REG(64);
            else if (ref_max_len <= 104) ATR_EMU_REG(104);
            else ATR_EMU_REG(152);
#undef ATR_EMU_REG
            continue;
        }
        {   // as the library: register strips (the LDS-column kernel is only its fallback)
            int mtop = 0, mlo_s[atr::PAIRS_MAX_STRIPS], mhi_s[atr::PAIRS_MAX_STRIPS];
            for (int s = 0; s < atr::PAIRS_MAX_STRIPS; ++s) { mlo_s[s] = 0x7fffffff; mhi_s[s] = 0; }
            for (int64_t t = tile * 64; t < std::min<int64_t>(npairs, tile * 64 + 64); ++t) {
                const int mt = std::min(ref_lens ? ref_lens[t] : ref_max_len, ref_max_len);
                mtop = std::max(mtop, mt);
                for (int s = 0; s < atr::PAIRS_MAX_STRIPS; ++s) {
                    const int loc = mt - s * atr::PAIRS_STRIP_ROWS;
                    if (loc >= 1 && loc <= atr::PAIRS_STRIP_ROWS) { mlo_s[s] = std::min(mlo_s[s], loc); mhi_s[s] = std::max(mhi_s[s], loc); }
                }
            }
            uint32_t tabs[16 * (atr::PAIRS_STRIP_ROWS / 32)];
            std::vector<uint32_t> bnd((size_t)qry_max_len + 1);
            const bool xs = (flags & ATR_STOP_WITHIN_SEQ2) != 0;
            if (p.and_mode) { if (xs) atr::locate_pair_strips<true, true>(tabs, 1, bnd.data(), 1, rp, revcomp != 0, m, mlo_s, mhi_s, mtop, qp, n, p, p.thr, out + 4 * r);
                              else atr::locate_pair_strips<true, false>(tabs, 1, bnd.data(), 1, rp, revcomp != 0, m, mlo_s, mhi_s, mtop, qp, n, p, p.thr, out + 4 * r); }
            else { if (xs) atr::locate_pair_strips<false, true>(tabs, 1, bnd.data(), 1, rp, revcomp != 0, m, mlo_s, mhi_s, mtop, qp, n, p, p.thr, out + 4 * r);
                   else atr::locate_pair_strips<false, false>(tabs, 1, bnd.data(), 1, rp, revcomp != 0, m, mlo_s, mhi_s, mtop, qp, n, p, p.thr, out + 4 * r); }
            if (!emu_pairs_use_lds_column) continue;
        }
        atr::stage_reference(refw.data(), 1, rp, m, revcomp != 0);
        const bool xr = (flags & ATR_STOP_WITHIN_SEQ2) != 0;
        if (p.and_mode) { if (xr) atr::locate_pair_one<true, true>(col.data(), 1, refw.data(), 1, m, qp, n, p, p.thr, out + 4 * r);
                          else atr::locate_pair_one<true, false>(col.data(), 1, refw.data(), 1, m, qp, n, p, p.thr, out + 4 * r); }
        else { if (xr) atr::locate_pair_one<false, true>(col.data(), 1, refw.data(), 1, m, qp, n, p, p.thr, out + 4 * r);
               else atr::locate_pair_one<false, false>(col.data(), 1, refw.data(), 1, m, qp, n, p, p.thr, out + 4 * r); }
    }
    return ATR_OK;
}

int emu_locate_pairs_path_batch(const uint8_t *ref_packed, const int32_t *ref_lens, int ref_max_len, int revcomp,
    const uint8_t *qry_packed, const int32_t *qry_lens, int qry_max_len, int64_t npairs, double e, int flags,
    int wildcard_ref, int wildcard_query, int min_overlap, int indel_cost, const int32_t *need, int path, atr_result *out, void *) {
    return pairs_batch((const uint32_t *)ref_packed, ref_lens, ref_max_len, revcomp, (const uint32_t *)qry_packed, qry_lens, qry_max_len,
                     npairs, e, flags, wildcard_ref, wildcard_query, min_overlap, indel_cost, need, path, (uint32_t *)out);
}
EMU_TWIN(locate_pairs_path_batch);

int emu_locate_pairs_need_batch(const uint8_t *ref_packed, const int32_t *ref_lens, int ref_max_len, int revcomp,
    const uint8_t *qry_packed, const int32_t *qry_lens, int qry_max_len, int64_t npairs, double e, int flags,
    int wildcard_ref, int wildcard_query, int min_overlap, int indel_cost, const int32_t *need, atr_result *out, void *) {
    return pairs_batch((const uint32_t *)ref_packed, ref_lens, ref_max_len, revcomp, (const uint32_t *)qry_packed, qry_lens, qry_max_len,
                     npairs, e, flags, wildcard_ref, wildcard_query, min_overlap, indel_cost, need, ATR_PAIRS_AUTO, (uint32_t *)out);
}
EMU_TWIN(locate_pairs_need_batch);

int emu_locate_pairs_batch(const uint8_t *ref_packed, const int32_t *ref_lens, int ref_max_len, int revcomp,
    const uint8_t *qry_packed, const int32_t *qry_lens, int qry_max_len, int64_t npairs, double e, int flags,
    int wildcard_ref, int wildcard_query, int min_overlap, int indel_cost, atr_result *out, void *) {
    return pairs_batch((const uint32_t *)ref_packed, ref_lens, ref_max_len, revcomp, (const uint32_t *)qry_packed, qry_lens, qry_max_len,
                     npairs, e, flags, wildcard_ref, wildcard_query, min_overlap, indel_cost, nullptr, ATR_PAIRS_AUTO, (uint32_t *)out);
}
EMU_TWIN(locate_pairs_batch);

int emu_locate_pairs_full_batch(const uint8_t *ref_packed, const int32_t *ref_lens, int ref_max_len, int revcomp,
    const uint8_t *qry_packed, const int32_t *qry_lens, int qry_max_len, int64_t npairs, double e, int flags,
    int wildcard_ref, int wildcard_query, int min_overlap, int indel_cost, atr_result *out, void *) {
    return pairs_batch((const uint32_t *)ref_packed, ref_lens, ref_max_len, revcomp, (const uint32_t *)qry_packed, qry_lens, qry_max_len,
                     npairs, e, flags, wildcard_ref, wildcard_query, min_overlap, indel_cost, nullptr, ATR_PAIRS_FULL, (uint32_t *)out);
}
EMU_TWIN(locate_pairs_full_batch);

}  // extern "C"

// emu_overlap_a.cpp -- TEST INFRASTRUCTURE.  What pass A of the two-pass pre-pass decides by itself about a clean
// read-end overlap (piece_core.hpp: piece_overlap_word, piece_scan), per read, from the product's own per-lane source
// compiled with -DATR_HOST_EMU and the same host parameter derivation the library uses (filter_params with the
// certificates, piece_params with them handed over).  The reads arrive as ASCII rows; the bit planes are built here
// (plane p, bit b of word w = bit p of the code of base 32 w + b), a ragged read is moved to the end of its words as the
// kernel moves it.  Never loaded by the product package.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "aligner_host.hpp"
#include "filter_core.hpp"
#include "piece_core.hpp"

using namespace atr;

namespace {

template <int NW>
int scan_read(const atr_aligner *a, const FilterParams &fp, const PieceParams &pp, const uint8_t *row, int nr, int n, bool ragged, int32_t *state) {
    uint32_t pl[NW][4], twp[4];
    memset(pl, 0, sizeof(pl));
    const int back = ragged ? 32 * NW - nr : 0;                    // positions the read is moved up by
    for (int j = 0; j < nr; ++j) {
        const uint32_t code = a->qtable[row[j]] & 15u;
        const int pos = j + back;
        for (int q = 0; q < 4; ++q) if ((code >> q) & 1u) pl[pos >> 5][q] |= 1u << (pos & 31);
    }
    for (int q = 0; q < 4; ++q) {
        const int sh = n & 31;
        twp[q] = sh == 0 ? pl[NW - 1][q] : piece_funnel(pl[NW - 1][q], NW >= 2 ? pl[NW >= 2 ? NW - 2 : 0][q] : 0u, sh);
    }
    const int mf = fp.rows, T = a->p.m - mf;
    const PieceScan S = piece_scan<NW>(pp, pl, twp, n, mf, T, a->p.k);   // (no read-start view: the word is 0 with START_WITHIN_SEQ1)
    // what the tile loop makes of it (piece_filter.hpp): bit 0 a read-end condition, 1 flagged, 2 the adapter verbatim,
    // 3 queued for pass B (flagged, not verbatim, a window of at most `narrow` columns)
    const PieceTask pt = piece_task(S, back, nr, false, a->p.m, a->p.k, pp.head_cols);
    const bool exact = S.j_exact != 0 && a->p.m >= a->p.min_overlap, flagged = pt.flagged && !exact;
    if (state) *state = (S.tail ? 1 : 0) | (S.flagged ? 2 : 0) | (S.j_exact != 0 ? 4 : 0) | (flagged && !pt.full && pt.need <= pp.narrow ? 8 : 0);
    if (S.ovl != 0 && (S.flagged || S.j_exact != 0)) return -1;   // (a resolved read is neither flagged nor the adapter verbatim)
    return S.ovl;
}

}  // namespace

extern "C" {

// ovl[r]: the overlap pass A resolves read r with (0: it does not), -1: an inconsistent scan.  word: PieceParams::ovl_a.
// lens == nullptr: an equal-length batch of max_len bases; otherwise a ragged one (pass A sees 32 ceil(max_len / 32)).
// state (may be null): per read, the bits scan_read describes.  force_off: scan with the word set to 0 -- pass A as it is
// without the rule (the exact-overlap chain then runs over its own rows only).
// Returns 0, or 1 when the two-pass pre-pass does not take the aligner at this length (nothing written but *word = 0).
int emu_overlap_a_scan(const char *ref, int m, double e, int flags, int wr, int wq, int min_overlap, int indel_cost,
                       const uint8_t *ascii, int64_t stride, const int32_t *lens, int64_t nreads, int max_len,
                       int32_t *ovl, uint32_t *word, int32_t *state, int force_off) {
    atr_aligner *a = nullptr;
    *word = 0u;
    if (aligner_create(ref, m, e, flags, wr, wq, min_overlap, indel_cost, &a) != ATR_OK) return -1;
    const bool and_mode = a->wildcard_ref || a->wildcard_query;
    const FilterParams fp = filter_params(a->peq, a->codes, a->p.m, a->flags, and_mode, a->p.thr, a->p.min_overlap, true);
    const int nw = (max_len + 31) / 32, n = lens ? 32 * nw : max_len;
    PieceParams pp;
    if (nw < 1 || nw > PIECE_MAX_WORDS ||
        !piece_params(a->codes, a->p.m, fp.rows, a->p.k, a->flags, and_mode, a->table_kind == ATR_TABLE_CUSTOM, fp.thr_row, n, pp,
                      a->p.thr, a->p.min_overlap, fp.cert, a->p.indel)) {
        delete a;
        return 1;
    }
    *word = pp.ovl_a;
    if (force_off) pp.ovl_a = 0u;
    for (int64_t r = 0; r < nreads; ++r) {
        const int nr = lens ? std::min(std::max(lens[r], 0), max_len) : max_len;
        const uint8_t *row = ascii + r * stride;
        int v = 0;
        switch (nw) {
            case 1: v = scan_read<1>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            case 2: v = scan_read<2>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            case 3: v = scan_read<3>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            case 4: v = scan_read<4>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            case 5: v = scan_read<5>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            case 6: v = scan_read<6>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            case 7: v = scan_read<7>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            case 8: v = scan_read<8>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            case 9: v = scan_read<9>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
            default: v = scan_read<10>(a, fp, pp, row, nr, n, lens != nullptr, state ? state + r : nullptr); break;
        }
        ovl[r] = v;
    }
    delete a;
    return 0;
}

}  // extern "C"

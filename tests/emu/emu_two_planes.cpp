// emu_two_planes.cpp -- TEST INFRASTRUCTURE.  Pass A of the run-time compiled pre-pass (piece_core.hpp: piece_scan_spec,
// two code planes and one base mask) against the generic pass A (piece_scan, four base masks), per read, from the
// product's own per-lane source compiled with -DATR_HOST_EMU.  One source, three builds (tests/test_two_planes_host.py):
//   -DEMU_TWO_GEN   a program that writes the piece_spec_config.h the library would generate for an aligner and a read
//                   length (jit_config.hpp, the very generator of jit.hpp);
//   -DATR_SPEC=1 -I<dir of that header>           the twin as a shared object: emu_two_planes_scan();
//   ... -DEMU_TWO_MAIN                            the twin as a stand-alone program that makes its own reads (the
//                                                 sanitizer build).
// Never loaded by the product package.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aligner_host.hpp"
#include "filter_core.hpp"
#include "piece_core.hpp"

using namespace atr;

#ifdef EMU_TWO_GEN
#include "jit_config.hpp"
// emu_two_gen <adapter> <e> <flags> <min_overlap> <n> <out_dir>; exit 3: outside the two-pass envelope
int main(int argc, char **argv) {
    if (argc < 7) return 2;
    atr_aligner *a = nullptr;
    if (aligner_create(argv[1], (int)strlen(argv[1]), atof(argv[2]), atoi(argv[3]), 0, 0, atoi(argv[4]), 1, &a) != ATR_OK) return 1;
    const int n = atoi(argv[5]);
    const FilterParams fp = filter_params(a->peq, a->codes, a->p.m, a->flags, false, a->p.thr, a->p.min_overlap, true);
    PieceParams pp;
    if (!piece_params(a->codes, a->p.m, fp.rows, a->p.k, a->flags, false, a->table_kind == ATR_TABLE_CUSTOM, fp.thr_row, n, pp, a->p.thr,
                      a->p.min_overlap, fp.cert, a->p.indel)) { delete a; return 3; }
    const std::string cfg = jit::spec_config(a, fp, pp, n);
    FILE *f = fopen((std::string(argv[6]) + "/piece_spec_config.h").c_str(), "w");
    if (!f) return 1;
    fwrite(cfg.data(), 1, cfg.size(), f);
    fclose(f);
    delete a;
    return 0;
}
#else

namespace {

constexpr int NW = (spec::N + 31) / 32;

struct Twin {
    atr_aligner *a = nullptr;
    FilterParams fp;
    PieceParams pp;
};

// the aligner the config header was generated for, with the generic pass A's parameter block
bool make_twin(const char *ref, int m, double e, int flags, int min_overlap, Twin &t) {
    if (aligner_create(ref, m, e, flags, 0, 0, min_overlap, 1, &t.a) != ATR_OK) return false;
    t.fp = filter_params(t.a->peq, t.a->codes, t.a->p.m, t.a->flags, false, t.a->p.thr, t.a->p.min_overlap, true);
    if (!piece_params(t.a->codes, t.a->p.m, t.fp.rows, t.a->p.k, t.a->flags, false, t.a->table_kind == ATR_TABLE_CUSTOM, t.fp.thr_row,
                      spec::N, t.pp, t.a->p.thr, t.a->p.min_overlap, t.fp.cert, t.a->p.indel)) return false;
    return t.a->p.m == spec::P.m && t.a->p.k == spec::P.k && t.pp.steps == spec::PP.steps && t.pp.ovl_a == spec::PP.ovl_a;
}

// both scans of one read (ASCII row of spec::N bytes); seven words each: j_exact, j_s, j_e, flagged, tail, head, ovl
void scan_read(const Twin &t, const uint8_t *row, int32_t *gen, int32_t *spc) {
    constexpr int n = spec::N;
    uint32_t pl[NW][4], twp[4];
    memset(pl, 0, sizeof(pl));
    for (int j = 0; j < n; ++j) {
        const uint32_t code = t.a->qtable[row[j]] & 15u;
        for (int q = 0; q < 4; ++q) if ((code >> q) & 1u) pl[j >> 5][q] |= 1u << (j & 31);
    }
    for (int q = 0; q < 4; ++q) {
        const int sh = n & 31;
        twp[q] = sh == 0 ? pl[NW - 1][q] : piece_funnel(pl[NW - 1][q], NW >= 2 ? pl[NW >= 2 ? NW - 2 : 0][q] : 0u, sh);
    }
    constexpr int HWN = NW < PIECE_HEAD_WORDS ? NW : PIECE_HEAD_WORDS;
    uint32_t hpl[HWN][4];
    for (int w = 0; w < HWN; ++w)
        for (int q = 0; q < 4; ++q) hpl[w][q] = pl[w][q];
    const int mf = t.fp.rows, T = t.a->p.m - mf, k = t.a->p.k;
    const PieceScan G = piece_scan<NW>(t.pp, pl, twp, n, mf, T, k, hpl);
    const PieceScan S = piece_scan_spec<NW>(pl, twp, mf, T, k, hpl);
    const PieceScan *both[2] = {&G, &S};
    int32_t *out[2] = {gen, spc};
    for (int i = 0; i < 2; ++i) {
        const PieceScan &X = *both[i];
        out[i][0] = X.j_exact; out[i][1] = X.j_s; out[i][2] = X.j_e; out[i][3] = X.flagged; out[i][4] = X.tail; out[i][5] = X.head;
        out[i][6] = X.ovl;
    }
}

}  // namespace

extern "C" {

int emu_two_planes_n(void) { return spec::N; }
int emu_two_planes_on(void) { return ATR_PIECE_TWO_PLANES != 0 && spec::PP.and_mode == 0 && ATR_SPEC_RAGGED == 0; }

// gen / spc: seven words per read (scan_read).  Returns the number of reads on which the two scans differ in any word,
// -1 when the aligner is not the one this twin was built for.
long long emu_two_planes_scan(const char *ref, int m, double e, int flags, int min_overlap, const uint8_t *ascii, int64_t stride,
                              int64_t nreads, int32_t *gen, int32_t *spc) {
    Twin t;
    if (!make_twin(ref, m, e, flags, min_overlap, t)) { delete t.a; return -1; }
    long long bad = 0;
    for (int64_t r = 0; r < nreads; ++r) {
        scan_read(t, ascii + r * stride, gen + 7 * r, spc + 7 * r);
        if (memcmp(gen + 7 * r, spc + 7 * r, 28) != 0) ++bad;
    }
    delete t.a;
    return bad;
}

}  // extern "C"

#ifdef EMU_TWO_MAIN
// emu_two_planes <adapter> <e> <flags> <min_overlap> <reads>: random reads with the (edited) adapter, N and IUPAC codes and
// runs of A at the read start; exit 0 when the scans agree on every read and some read holds the adapter verbatim
int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const char *ref = argv[1];
    const int m = (int)strlen(ref), flags = atoi(argv[3]), mo = atoi(argv[4]), n = spec::N;
    const double e = atof(argv[2]);
    const long long reads = atoll(argv[5]);
    uint64_t st = 88172645463325252ull;
    const auto rnd = [&](int k) { st = st * 6364136223846793005ull + 1442695040888963407ull; return k > 0 ? (int)((st >> 33) % (uint64_t)k) : 0; };
    const char B[4] = {'A', 'C', 'G', 'T'}, X[6] = {'N', 'R', 'Y', 'K', 'n', '.'};
    std::vector<uint8_t> buf((size_t)reads * n);
    for (long long r = 0; r < reads; ++r) {
        uint8_t *row = buf.data() + r * n;
        for (int j = 0; j < n; ++j) row[j] = (uint8_t)B[rnd(4)];
        if (rnd(4) != 0) {                                        // the adapter somewhere, cut at the read end
            const int at = rnd(n - 3);
            for (int i = 0; i < m && at + i < n; ++i) row[at + i] = (uint8_t)ref[i];
            if (rnd(3) == 0) row[at + rnd(std::min(m, n - at))] = (uint8_t)B[rnd(4)];
        }
        if (rnd(3) == 0) for (int j = 0, run = rnd(10); j <= run; ++j) row[j] = 'A';
        if (rnd(2) == 0) row[rnd(n)] = (uint8_t)X[rnd(6)];
    }
    std::vector<int32_t> gen((size_t)reads * 7), spc((size_t)reads * 7);
    const long long bad = emu_two_planes_scan(ref, m, e, flags, mo, buf.data(), n, reads, gen.data(), spc.data());
    long long exact = 0;
    for (long long r = 0; r < reads; ++r) exact += gen[7 * r] != 0;
    printf("emu_two_planes: n = %d, %lld reads, %lld differ, %lld with the adapter verbatim, two planes %s\n", n, reads, bad, exact,
           emu_two_planes_on() ? "on" : "off");
    return bad == 0 && exact > 0 ? 0 : 1;
}
#endif
#endif

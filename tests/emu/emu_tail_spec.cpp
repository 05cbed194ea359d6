// emu_tail_spec.cpp -- TEST INFRASTRUCTURE.  The band sweeps of the run-time compiled DP tail (csrc/tail_filter.hpp:
// tail_band_locate / tail_band_locate_last, rows issued TAIL_ROWS_UNROLL to a body) against the generic ones they replace
// (filter_core.hpp: band_locate / band_locate_last), per lane, from the product's own source compiled with
// -DATR_HOST_EMU: random aligners, reads and window words, the four record words compared.  The window blocks of the tail
// run the unchanged lane_step / lane_result of locate_core.hpp and have no twin of their own; there are no wave-level
// shuffles in either sweep (the wave reductions only pick the ND variant, which is an argument here).
// With -DEMU_TAIL_MAIN: a stand-alone driver (the sanitizer build of tests/test_tail_spec_host.py).  Never loaded by
// the product package.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "aligner_host.hpp"
#include "filter_core.hpp"
#include "tail_filter.hpp"

using namespace atr;

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return n > 0 ? (int)(next() % (uint32_t)n) : 0; }
    int range(int lo, int hi) { return lo + below(hi - lo + 1); }
};

const char BASES[4] = {'A', 'C', 'G', 'T'};

// the adapter with up to `edits` edit operations
std::vector<char> edited(Rng &g, const std::vector<char> &ref, int edits) {
    std::vector<char> s = ref;
    for (int e = 0; e < edits && s.size() > 2; ++e) {
        const int at = g.below((int)s.size()), what = g.below(4);
        if (what < 2) s[at] = BASES[g.below(4)];
        else if (what == 2) s.insert(s.begin() + at, BASES[g.below(4)]);
        else s.erase(s.begin() + at);
    }
    return s;
}

// band_stage's result for one lane (stride 1): bases dlo + 1 .. as dwords of eight codes, 0 beyond the read
void stage(const atr_aligner *a, const std::vector<char> &read, int dlo, uint32_t (&ns)[BAND_STREAM]) {
    for (int k = 0; k < BAND_STREAM; ++k) {
        uint32_t w = 0;
        for (int t = 0; t < 8; ++t) {
            const int j0 = dlo + 8 * k + t;                         // 0-based index of base dlo + 1 + 8k + t
            const uint32_t code = j0 >= 0 && j0 < (int)read.size() ? (a->qtable[(uint8_t)read[j0]] & 15u) : 0u;
            w |= code << (4 * t);
        }
        ns[k] = w;
    }
}

template <bool AND_MODE>
long long run_cases(const atr_aligner *a, Rng &g, long long cases, long long *accepted) {
    const int m = a->p.m, k = a->p.k;
    const Uniform u = make_uniform(a->p, round_up_rows(m));
    uint32_t rreps[FILTER_MAX_M];
    for (int i = 0; i < FILTER_MAX_M; ++i) rreps[i] = i < m ? (uint32_t)(a->codes[i] & 15u) * 0x11111111u : 0u;
    const bool noindel = a->indel_cost > k;
    const std::vector<char> ref(a->ref.begin(), a->ref.end());
    long long bad = 0;
    for (long long t = 0; t < cases; ++t) {
        const int n = g.range(m + 2, 200);
        std::vector<char> read(n);
        for (char &c : read) c = g.below(50) == 0 ? 'N' : BASES[g.below(4)];
        uint32_t ns[BAND_STREAM], ra[4], rb[4];
        if (g.below(2) == 0) {
            // row-m band read: the (edited) adapter ends at column dlo + m + c0; the wave's widest read decides smax
            const std::vector<char> ad = edited(g, ref, g.range(0, k + 1));
            const int s = g.range(0, BAND_W - 1), smax = g.range(s, BAND_W - 1);
            const int dlo = g.range(0, std::max(0, n - m)), c0 = g.range(0, s);
            const int end = std::min(n, dlo + m + c0), start = end - (int)ad.size();
            for (int i = 0; i < (int)ad.size(); ++i) if (start + i >= 0 && start + i < n) read[start + i] = ad[i];
            const uint32_t ww = window_word(dlo, std::min(1023, dlo + m - k + s), false, m, true);
            stage(a, read, dlo, ns);
            band_locate<AND_MODE>(u, rreps, noindel, ns, 1, n, ww, smax, a->p.thr, ra);
            tail_band_locate<AND_MODE, FILTER_MAX_M>(u, rreps, noindel, ns, 1, n, ww, smax, a->p.thr, rb);
        } else {
            // last-column band read: a prefix of the (edited) adapter at the read end, rows top - span .. top looked at;
            // the wave's highest row, widest band and first row of interest are arguments
            const int top = g.range(1, m), span = g.range(0, std::min(top - 1, 8)), width = g.range(3, BAND_W - 1);
            const bool rowm = g.below(4) == 0;
            const std::vector<char> ad = edited(g, std::vector<char>(ref.begin(), ref.begin() + top), g.range(0, 2));
            for (int i = 0; i < (int)ad.size() && i < n; ++i) read[n - std::min(n, (int)ad.size()) + i] = ad[i + std::max(0, (int)ad.size() - n)];
            const int dlo = std::max(0, n - top - g.range(0, width));
            const uint32_t ww = last_band_word(dlo, top, span, width, rowm);
            const int smax = g.range(width, BAND_W - 1), rows_max = rowm || g.below(3) == 0 ? m : g.range(top, m);
            const int cap_lo = g.range(std::max(0, top - span - 3), top - span);
            const bool active = g.below(8) != 0;
            stage(a, read, dlo, ns);
            band_locate_last<AND_MODE>(u, rreps, noindel, ns, 1, n, ww, active, smax, rows_max, cap_lo, a->p.thr, ra);
            tail_band_locate_last<AND_MODE, FILTER_MAX_M>(u, rreps, noindel, ns, 1, n, ww, active, smax, rows_max, cap_lo, a->p.thr, rb);
        }
        if (memcmp(ra, rb, sizeof(ra)) != 0) ++bad;
        if ((ra[0] >> 16) != 0xFFFFu) ++*accepted;
    }
    return bad;
}

}  // namespace

extern "C" {

// `aligners` random aligners (the first is C2's), `per` cases each.  Returns the number of cases whose records differ
// (-1: an aligner could not be made); *accepted: cases in which the generic sweep found a match.
long long emu_tail_spec_run(uint64_t seed, int aligners, long long per, long long *accepted) {
    Rng g{seed * 2654435761ull + 12345u};
    long long bad = 0, acc = 0;
    for (int t = 0; t < aligners; ++t) {
        std::vector<char> ref;
        double e = 0.1;
        int wild = 0, indel = 1;
        if (t == 0) {
            const char *truseq = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC";
            ref.assign(truseq, truseq + strlen(truseq));
        } else {
            const int m = g.range(8, FILTER_MAX_M);
            const int period = g.below(3) == 0 ? g.range(1, 5) : m;
            for (int i = 0; i < m; ++i) ref.push_back(i >= period ? ref[i - period] : BASES[g.below(4)]);
            const double es[4] = {0.05, 0.1, 0.12, 0.2};
            e = es[g.below(4)];
            wild = g.below(4) == 0;
            if (wild) ref[g.below(m)] = 'N';
            indel = g.below(5) == 0 ? 2 + g.below(3) : 1;
        }
        const int m = (int)ref.size();
        if ((int)(e * m) > 7) e = 7.0 / m;                         // (2k + 1 diagonals inside the band)
        atr_aligner *a = nullptr;
        if (aligner_create(ref.data(), m, e, 14, wild, wild, g.range(1, 5), indel, &a) != ATR_OK) return -1;
        bad += wild ? run_cases<true>(a, g, per, &acc) : run_cases<false>(a, g, per, &acc);
        delete a;
    }
    if (accepted) *accepted = acc;
    return bad;
}

}  // extern "C"

#ifdef EMU_TAIL_MAIN
int main(int argc, char **argv) {
    const int aligners = argc > 1 ? atoi(argv[1]) : 8;
    const long long per = argc > 2 ? atoll(argv[2]) : 2000;
    long long acc = 0;
    const long long bad = emu_tail_spec_run(7, aligners, per, &acc);
    printf("emu_tail_spec: %d aligners x %lld cases, %lld differ, %lld with a match\n", aligners, per, bad, acc);
    return bad == 0 && acc > 0 ? 0 : 1;
}
#endif

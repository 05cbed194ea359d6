// TEST INFRASTRUCTURE: a stand-alone program over detect_kmer_core.hpp and the CPU twin of the k-mer kernels
// (emu_kmer.cpp), for AddressSanitizer / UBSan builds: random reads go through the slots, the ranks by doubling, the
// level loop, the gather and the support call with exactly sized buffers, and every level's over-represented k-mers
// (text, count, first occurrence), level[] and the support words are compared with a model on std::map and std::string.
//   g++ -std=c++17 -DATR_HOST_EMU -fsanitize=address,undefined -I include -I atropos_amd/csrc \
//       tests/emu/kmer_fuzz_main.cpp tests/emu/emu_kmer.cpp -o kmer_fuzz && ./kmer_fuzz 40
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <set>
#include <string>
#include <vector>

#include "atropos_hip.h"
#include "detect_kmer_core.hpp"
#include "fastq_core.hpp"

using namespace atr;

extern "C" {
decltype(atr_detect_kmer_slots) emu_detect_kmer_slots;
decltype(atr_detect_kmer_pair_keys) emu_detect_kmer_pair_keys;
decltype(atr_detect_kmer_rank_work_bytes) emu_detect_kmer_rank_work_bytes;
decltype(atr_detect_kmer_rank) emu_detect_kmer_rank;
decltype(atr_detect_kmer_level) emu_detect_kmer_level;
decltype(atr_detect_kmer_next) emu_detect_kmer_next;
decltype(atr_detect_kmer_gather) emu_detect_kmer_gather;
decltype(atr_detect_kmer_support) emu_detect_kmer_support;
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

#define FAIL(...) do { fprintf(stderr, "round %d: ", round); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

struct Classes {
    std::vector<int32_t> begin, end, head;
};

// sort + rank of `keys` (entry i belongs to slot list[i], or i): classes into cls
static int rank_keys(const std::vector<int64_t> &keys, const int32_t *list, std::vector<int32_t> &cls, Classes &c) {
    const int64_t n = (int64_t)keys.size();
    std::vector<int64_t> idx((size_t)n), sorted((size_t)n);
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return keys[(size_t)a] < keys[(size_t)b] || (keys[(size_t)a] == keys[(size_t)b] && a > b); });
    for (int64_t i = 0; i < n; ++i) sorted[(size_t)i] = keys[(size_t)idx[(size_t)i]];
    c.begin.assign((size_t)n, -7); c.end.assign((size_t)n, -7); c.head.assign((size_t)n, -7);
    std::vector<uint8_t> work(emu_detect_kmer_rank_work_bytes(n));
    int64_t nclasses = -1;
    const int rc = emu_detect_kmer_rank(sorted.data(), idx.data(), list, n, cls.data(), c.begin.data(), c.end.data(), c.head.data(),
                                        &nclasses, work.data(), work.size(), nullptr);
    return rc ? -1 : (int)nclasses;
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 20;
    for (int round = 0; round < rounds; ++round) {
        const int k0 = KMER_MIN_K + (int)(rnd() % (round % 5 == 0 ? 29 : 9));
        const int nreads = 1 + (int)(rnd() % 60);
        const std::string motif = [&] { std::string m; for (int i = 0; i < 40; ++i) m += "ACGT"[rnd() % 4]; return m; }();
        std::vector<std::string> reads;
        std::set<std::string> seen;
        while ((int)reads.size() < nreads) {
            std::string s;
            const int len = k0 + (int)(rnd() % (round % 7 == 0 ? 321 - k0 : 60));
            while ((int)s.size() < len) {
                if (rnd() % 3 == 0) s += motif.substr(rnd() % 20, 1 + rnd() % 20);
                else s += "ACGTN"[rnd() % 5];
            }
            s.resize((size_t)len);
            if (seen.insert(s).second) reads.push_back(s);
        }
        // the chunk: the sequences back to back with a gap, records in a shuffled order behind unused ones
        std::vector<uint8_t> bytes;
        std::vector<FastqRecord> recs((size_t)nreads + 3);
        std::vector<int32_t> kept((size_t)nreads + 3, 0);
        std::vector<int64_t> reps, start;
        int64_t total = 0;
        for (int j = 0; j < nreads; ++j) {
            const size_t r = (size_t)j + (j > nreads / 2 ? 3 : 0);
            recs[r].seq_off = (uint32_t)bytes.size();
            recs[r].seq_len = (uint32_t)reads[(size_t)j].size() + 2;
            kept[r] = (int32_t)reads[(size_t)j].size();
            bytes.insert(bytes.end(), reads[(size_t)j].begin(), reads[(size_t)j].end());
            bytes.push_back('A'); bytes.push_back('A');
            reps.push_back((int64_t)r); start.push_back(total);
            total += kept[r];
        }
        std::vector<KmerRep> tab((size_t)nreads);
        std::vector<int32_t> slot_rep((size_t)total), level((size_t)nreads, -1);
        if (emu_detect_kmer_slots((const atr_fastq_record *)recs.data(), kept.data(), reps.data(), start.data(), nreads, total, k0,
                                  tab.data(), slot_rep.data(), level.data(), nullptr))
            FAIL("slots");
        // classes at k0 by doubling
        std::map<int, std::vector<int32_t>> ids;
        Classes classes;
        auto combine = [&](int a, int b) {
            std::vector<int64_t> keys((size_t)total);
            if (emu_detect_kmer_pair_keys(tab.data(), slot_rep.data(), total, bytes.data(), a == 1 ? nullptr : ids[a].data(), a,
                                          b == 1 ? nullptr : ids[b].data(), b, keys.data(), nullptr))
                return -1;
            ids[a + b].assign((size_t)total, -9);
            return rank_keys(keys, nullptr, ids[a + b], classes);
        };
        int top = 1;
        while (2 * top <= k0) { if (combine(top, top) < 0) FAIL("doubling %d", top); top *= 2; }
        int have = top;
        for (int bit = top / 2; bit; bit /= 2)
            if (k0 & bit) { if (combine(have, bit) < 0) FAIL("combine %d + %d", have, bit); have += bit; }
        std::vector<int32_t> cls = ids[k0], cls_prev, cand_of_prev, spare((size_t)total, -9);
        // the level loop against the model
        const int64_t min_count = 1 + (int64_t)(rnd() % 3), capacity = 1 << 16;
        std::vector<int64_t> state(KMER_S_WORDS, 0);
        std::vector<int32_t> cand((size_t)capacity * KMER_C_WORDS, -1), list;
        std::vector<int> member((size_t)nreads, 1);
        std::map<std::string, long long> over_all;
        std::map<int, std::vector<int>> members_at;                       // level -> the reads counted there
        int64_t n = total;
        int k = k0;
        bool have_list = false;
        for (;; ++k) {
            std::map<std::string, long long> counts;
            members_at[k] = member;
            for (int j = 0; j < nreads; ++j)
                if (member[(size_t)j])
                    for (size_t o = 0; o + (size_t)k <= reads[(size_t)j].size(); ++o) ++counts[reads[(size_t)j].substr(o, (size_t)k)];
            std::vector<int> next_member((size_t)nreads, 0);
            long long n_over = 0;
            for (const auto &kv : counts)
                if (kv.second > min_count) { ++n_over; over_all[kv.first] = kv.second; }
            for (int j = 0; j < nreads; ++j)
                if (member[(size_t)j])
                    for (size_t o = 0; o + (size_t)k <= reads[(size_t)j].size(); ++o)
                        if (counts[reads[(size_t)j].substr(o, (size_t)k)] > min_count) next_member[(size_t)j] = 1;
            std::vector<int32_t> cand_of((size_t)std::max<int64_t>(n, 1), -9);
            if (emu_detect_kmer_level(tab.data(), slot_rep.data(), have_list ? list.data() : nullptr, n, cls.data(),
                                      cls_prev.empty() ? nullptr : cls_prev.data(), classes.begin.data(), classes.end.data(),
                                      classes.head.data(), cand_of.data(), cls_prev.empty() ? nullptr : cand_of_prev.data(), k,
                                      min_count, level.data(), cand.data(), capacity, state.data(), nullptr))
                FAIL("level %d", k);
            std::vector<int32_t> list_next((size_t)std::max<int64_t>(n, 1));
            std::vector<int64_t> keys_next((size_t)std::max<int64_t>(n, 1));
            if (emu_detect_kmer_next(tab.data(), slot_rep.data(), have_list ? list.data() : nullptr, n, cls.data(), bytes.data(),
                                     level.data(), k, list_next.data(), keys_next.data(), state.data(), nullptr))
                FAIL("next %d", k);
            if (state[KMER_S_OVER + k] != n_over) FAIL("level %d: %lld over-represented classes, the model has %lld", k,
                                                       (long long)state[KMER_S_OVER + k], n_over);
            for (int j = 0; j < nreads; ++j)
                if ((level[(size_t)j] == k + 1) != (next_member[(size_t)j] == 1)) FAIL("level[%d] after level %d", j, k);
            const int64_t n_next = state[KMER_S_SURVIVORS];
            long long expect_next = 0;
            for (int j = 0; j < nreads; ++j)
                if (next_member[(size_t)j] && (int)reads[(size_t)j].size() >= k + 1) expect_next += (long long)reads[(size_t)j].size() - k;
            if (n_next != expect_next) FAIL("level %d: %lld survivors, the model has %lld", k, (long long)n_next, expect_next);
            if (n_over == 0 || n_next == 0) break;
            list_next.resize((size_t)n_next); keys_next.resize((size_t)n_next);
            std::vector<int32_t> cls_new = spare;
            if (rank_keys(keys_next, list_next.data(), cls_new, classes) < 0) FAIL("rank at level %d", k + 1);
            spare = cls_prev.empty() ? std::vector<int32_t>((size_t)total, -9) : cls_prev;
            cls_prev = cls; cls = cls_new; cand_of_prev = cand_of; list = list_next; have_list = true;
            member = next_member; n = n_next;
        }
        // the candidate table: texts and counts
        const int64_t ncand = state[KMER_S_CANDIDATES];
        if (ncand != (int64_t)over_all.size() || ncand > capacity) FAIL("%lld rows, the model has %zu", (long long)ncand, over_all.size());
        std::vector<int64_t> text_off((size_t)ncand + 1, 0);
        for (int64_t c = 0; c < ncand; ++c) text_off[(size_t)c + 1] = text_off[(size_t)c] + cand[(size_t)c * KMER_C_WORDS + KMER_C_LEVEL];
        std::vector<uint8_t> out((size_t)text_off[(size_t)ncand]);
        if (emu_detect_kmer_gather(tab.data(), nreads, bytes.data(), cand.data(), text_off.data(), ncand, out.data(), nullptr)) FAIL("gather");
        for (int64_t c = 0; c < ncand; ++c) {
            const std::string text(out.begin() + text_off[(size_t)c], out.begin() + text_off[(size_t)c + 1]);
            const auto it = over_all.find(text);
            if (it == over_all.end() || it->second != cand[(size_t)c * KMER_C_WORDS + KMER_C_COUNT]) FAIL("row %lld: %s", (long long)c, text.c_str());
            over_all.erase(it);
            // the row names the first occurrence among the reads counted at its level, in record order
            const int32_t *w = cand.data() + (size_t)c * KMER_C_WORDS;
            const std::vector<int> &mem = members_at[w[KMER_C_LEVEL]];
            int fj = -1;
            size_t fo = 0;
            for (int j = 0; j < nreads && fj < 0; ++j)
                if (mem[(size_t)j] && (fo = reads[(size_t)j].find(text)) != std::string::npos) fj = j;
            if (w[KMER_C_REP] != fj || w[KMER_C_OFFSET] != (int32_t)fo) FAIL("row %lld: not the first occurrence", (long long)c);
        }
        // support
        std::vector<std::string> pats = {motif.substr(0, 12), motif.substr(5, 8), reads[0], reads[0].substr(reads[0].size() / 2), "ACGTACGTAC"};
        std::vector<uint8_t> pat_bytes(pats.size() * KMER_MAX_READ, 0);
        std::vector<int32_t> pat_len;
        for (size_t p = 0; p < pats.size(); ++p) {
            std::copy(pats[p].begin(), pats[p].end(), pat_bytes.begin() + (long)(p * KMER_MAX_READ));
            pat_len.push_back((int32_t)pats[p].size());
        }
        std::vector<int64_t> abundance(pats.size(), -1);
        std::vector<uint64_t> longest(pats.size(), 5);
        if (emu_detect_kmer_support(tab.data(), nreads, bytes.data(), level.data(), pat_bytes.data(), pat_len.data(), (int)pats.size(),
                                    abundance.data(), longest.data(), nullptr))
            FAIL("support");
        for (size_t p = 0; p < pats.size(); ++p) {
            int64_t ab = 0;
            uint64_t best = ~0ull;
            for (int j = 0; j < nreads; ++j) {
                const size_t at = reads[(size_t)j].find(pats[p]);
                if (at == std::string::npos) continue;
                ++ab;
                if (level[(size_t)j] >= (int)pats[p].size()) best = std::min<uint64_t>(best, ((uint64_t)at << 32) | (uint64_t)reps[(size_t)j]);
            }
            if (abundance[p] != ab || longest[p] != best) FAIL("support of pattern %zu", p);
        }
    }
    printf("ok: %d rounds\n", rounds);
    return 0;
}

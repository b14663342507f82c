// tools/ix_select_check.cpp -- the host steps of the trace-id index (zipkin_amd/csrc/zk_ix_select.h) without a
// device: the plan of a service's slices, the select's rounds as zk_ix_trace_ids runs them (differing bits,
// 12-bit digit, histogram, bin choice, certain / candidate lists, the equal-keys end, final sort) over entry
// sets aimed at each of them, compared with a full sort, and the bitmap's name ids. Not product code and not
// part of the suite; meant to be built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Izipkin_amd/csrc tools/ix_select_check.cpp -o /tmp/ix_select_check && /tmp/ix_select_check
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "zk_ix_select.h"

using namespace zk;

static int run_case(const std::vector<IxEntry>& all, uint32_t limit, const char* name) {
    const uint64_t cap = 4096;
    std::vector<IxEntry> ref = all;
    std::vector<uint64_t> rid(limit), gid(limit);
    std::vector<int64_t> rts(limit), gts(limit);
    const uint32_t rn = ix_emit(ref.data(), ref.size(), IxEntry{0, 0}, 0, limit, rid.data(), rts.data());
    std::vector<IxEntry> certain, cand = all;
    uint64_t want = limit, copies = 0;
    IxEntry same{0, 0};
    int rounds = 0;
    while (certain.size() + cand.size() > cap) {
        uint64_t oh = 0, nh = 0, ol = 0, nl = 0;
        for (auto& e : cand) { oh |= ~e.tkey; nh |= e.tkey; ol |= e.id; nl |= ~e.id; }
        if (!((oh & nh) | (ol & nl))) {  // all one pair: the end
            same = IxEntry{~oh, ol};
            copies = want;
            cand.clear();
            break;
        }
        const uint32_t shift = td_shift_of(oh & nh, ol & nl);
        std::vector<uint32_t> hist(kTdBins, 0);
        for (auto& e : cand) hist[td_digit(~e.tkey, e.id, shift)]++;
        uint64_t below = 0;
        const uint32_t bin = td_pick_bin(hist.data(), want, &below);
        if (bin >= kTdBins || hist[bin] >= cand.size() || below >= want) { printf("%s: no split\n", name); return 1; }
        std::vector<IxEntry> next;
        for (auto& e : cand) {
            const uint32_t d = td_digit(~e.tkey, e.id, shift);
            if (d < bin) certain.push_back(e);
            else if (d == bin) next.push_back(e);
        }
        if (next.size() != hist[bin] || next.size() >= cand.size()) { printf("%s: the list did not shrink\n", name); return 1; }
        want -= below;
        cand.swap(next);
        if (++rounds > 11) { printf("%s: more than 11 rounds\n", name); return 1; }
    }
    certain.insert(certain.end(), cand.begin(), cand.end());
    if (certain.size() + copies > cap) { printf("%s: %zu entries reach the host\n", name, certain.size() + (size_t)copies); return 1; }
    const uint32_t gn = ix_emit(certain.data(), certain.size(), same, copies, limit, gid.data(), gts.data());
    if (gn != rn) { printf("%s: n %u != %u\n", name, gn, rn); return 1; }
    for (uint32_t i = 0; i < gn; ++i)
        if (gid[i] != rid[i] || gts[i] != rts[i]) { printf("%s: limit %u entry %u differs\n", name, limit, i); return 1; }
    printf("%s limit %u: ok, %d rounds, %u out%s\n", name, limit, rounds, gn, copies ? " (equal-keys end)" : "");
    return 0;
}

int main() {
    std::mt19937_64 r(11);
    int bad = 0;
    auto mk = [&](size_t n, auto ts, auto id) {
        std::vector<IxEntry> t(n);
        for (size_t i = 0; i < n; ++i) t[i] = IxEntry{(uint64_t)ts(i) ^ kTdSign, (uint64_t)id(i)};
        return t;
    };
    auto rnd = [&](size_t) { return r(); };
    for (uint32_t limit : {1u, 100u, 4095u, 4096u}) {
        bad += run_case(mk(20000, [&](size_t) { return 1400000000000000ull + (r() % 8 << 20); }, rnd), limit, "eight-timestamps");
        bad += run_case(mk(20000, [&](size_t) { return 1400000000000000ull + r() % 1024; }, rnd), limit, "low-ten-bits");
        bad += run_case(mk(9000, [&](size_t) { return 5; }, [&](size_t) { return 0xABCDEFull; }), limit, "all-equal");
        bad += run_case(mk(11000, [&](size_t i) { return i < 3000 ? 2000 + r() % 1000 : i < 8000 ? 1000 : r() % 1000; },
                           [&](size_t i) { return i >= 3000 && i < 8000 ? 1ull << 63 : r(); }), limit, "equal-block-straddles");
        bad += run_case(mk(10000, [&](size_t i) { return i % 2 ? INT64_MIN : INT64_MAX; }, [&](size_t i) { return i % 4 < 2 ? 0ull : ~0ull; }),
                        limit, "four-pairs-at-the-extremes");
        bad += run_case(mk(30000, rnd, rnd), limit, "random");
        bad += run_case(mk(100, [&](size_t) { return r() % 3; }, [&](size_t) { return r() % 3; }), limit, "small");
        bad += run_case(mk(9000, [&](size_t) { return 7; }, [&](size_t i) { return 0xABCD000000000000ull + i / 2; }), limit, "sequential-ids-twice");
    }
    // the plan of a service's slices
    {
        const uint64_t o0[] = {0, 0, 5, 5, 9}, o1[] = {0, 3, 3, 3, 3}, o2[] = {0, 1, 2, 2, 40};
        const uint64_t* offs[] = {o0, o1, o2};
        std::vector<IxSpan> sp;
        const uint64_t want[4] = {4, 6, 0, 42};
        for (uint32_t s = 0; s < 4; ++s) {
            const uint64_t total = ix_plan(offs, 3, s, &sp);
            uint64_t sum = 0;
            for (auto& x : sp) { sum += x.count; if (!x.count || x.start != offs[x.segment][s]) { printf("plan: slice\n"); ++bad; } }
            if (total != want[s] || sum != total) { printf("plan: service %u holds %llu\n", s, (unsigned long long)total); ++bad; }
        }
        if (ix_plan(offs, 3, 2, &sp) != 0 || !sp.empty()) { printf("plan: an empty service has slices\n"); ++bad; }
    }
    // the bitmap's ids: bit 0 is not a name
    {
        std::vector<uint32_t> bm(kIxNameWords, 0);
        for (uint32_t id : {0u, 1u, 31u, 32u, 4097u, 65535u}) bm[id >> 5] |= 1u << (id & 31);
        uint16_t out[8] = {};
        const uint32_t n = ix_names_of(bm.data(), out, 8);
        const uint16_t want[5] = {1, 31, 32, 4097, 65535};
        if (n != 5 || ix_names_of(bm.data(), nullptr, 0) != 5) { printf("names: count %u\n", n); ++bad; }
        for (int i = 0; i < 5; ++i) if (out[i] != want[i]) { printf("names: id %d\n", i); ++bad; }
        uint16_t two[2] = {};
        if (ix_names_of(bm.data(), two, 2) != 5 || two[0] != 1 || two[1] != 31) { printf("names: a short array\n"); ++bad; }
    }
    printf(bad ? "FAILED\n" : "ALL OK\n");
    return bad != 0;
}

// tools/td_select_check.cpp -- the host steps of zk_td_top (zipkin_amd/csrc/zk_td_select.h) without a device:
// the select's rounds (differing bits, 12-bit digit, histogram, bin choice, certain / candidate lists, final
// sort) run on the host over tables aimed at each of them and are compared with a full sort. Not product
// code and not part of the suite; meant to be built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Izipkin_amd/csrc tools/td_select_check.cpp -o /tmp/td_select_check && /tmp/td_select_check
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "zk_td_select.h"

using namespace zk;

static int run_case(std::vector<TdEntry> tab, uint32_t order, uint32_t k, const char* name) {
    const uint64_t cap = ZK_TD_MAX_TOP;
    std::vector<TdEntry> ref = tab;
    std::vector<uint64_t> rid(k), gid(k);
    std::vector<int64_t> rs(k), rd(k), gs(k), gd(k);
    const uint32_t rn = td_emit(ref.data(), ref.size(), order, k, rid.data(), rs.data(), rd.data());
    std::vector<TdEntry> certain, cand = tab;
    uint64_t want = k;
    int rounds = 0;
    while (certain.size() + cand.size() > cap) {
        uint64_t oh = 0, nh = 0, ol = 0, nl = 0;
        for (auto& e : cand) {
            const uint64_t hi = td_order_key(order, e.skey, e.ekey);
            oh |= hi; nh |= ~hi; ol |= e.id; nl |= ~e.id;
        }
        if (!((oh & nh) | (ol & nl))) { printf("%s: no differing bit\n", name); return 1; }
        const uint32_t shift = td_shift_of(oh & nh, ol & nl);
        std::vector<uint32_t> hist(kTdBins, 0);
        for (auto& e : cand) hist[td_digit(td_order_key(order, e.skey, e.ekey), e.id, shift)]++;
        uint64_t below = 0;
        const uint32_t bin = td_pick_bin(hist.data(), want, &below);
        if (bin >= kTdBins || hist[bin] >= cand.size() || below >= want) { printf("%s: no split\n", name); return 1; }
        std::vector<TdEntry> next;
        for (auto& e : cand) {
            const uint32_t d = td_digit(td_order_key(order, e.skey, e.ekey), e.id, shift);
            if (d < bin) certain.push_back(e);
            else if (d == bin) next.push_back(e);
        }
        if (next.size() != hist[bin]) { printf("%s: count\n", name); return 1; }
        want -= below;
        cand.swap(next);
        ++rounds;
    }
    certain.insert(certain.end(), cand.begin(), cand.end());
    const uint32_t gn = td_emit(certain.data(), certain.size(), order, k, gid.data(), gs.data(), gd.data());
    if (gn != rn) { printf("%s: n %u != %u\n", name, gn, rn); return 1; }
    for (uint32_t i = 0; i < gn; ++i)
        if (gid[i] != rid[i] || gs[i] != rs[i] || gd[i] != rd[i]) { printf("%s: order %u k %u entry %u differs\n", name, order, k, i); return 1; }
    printf("%s order %u k %u: ok, %d rounds, %u out\n", name, order, k, rounds, gn);
    return 0;
}

int main() {
    std::mt19937_64 r(7);
    int bad = 0;
    auto mk = [&](size_t n, auto dur, auto st) {
        std::vector<TdEntry> t(n);
        for (size_t i = 0; i < n; ++i) {
            const uint64_t s = (uint64_t)st(i), d = (uint64_t)dur(i);
            t[i] = TdEntry{r() | 1, s ^ kTdSign, (s + d) ^ kTdSign};
        }
        t[0].id = 0;
        t[1].id = ~0ull;
        return t;
    };
    for (uint32_t order = 0; order < 4; ++order)
        for (uint32_t k : {1u, 64u, 4096u}) {
            bad += run_case(mk(20000, [&](size_t) { return r() % 40 * 10; }, [&](size_t) { return 1400000000000000ull + r() % 300 * 1000; }), order, k, "collide");
            bad += run_case(mk(5000, [&](size_t) { return 777; }, [&](size_t) { return 5; }), order, k, "one-duration");
            bad += run_case(mk(5000, [&](size_t i) { return (1u << 20) + i; }, [&](size_t i) { return i; }), order, k, "low-bits");
            bad += run_case(mk(10000, [&](size_t i) { return i % 2 ? 12345ull : 12345ull + (1ull << 63); }, [&](size_t) { return (uint64_t)-1; }), order, k, "sign-bit");
            bad += run_case(mk(20000, [&](size_t i) { return (uint64_t)(i % 2) << 40 | (uint64_t)(i / 2 % 2) << 20; }, [&](size_t i) { return i % 7; }), order, k, "three-rounds");
            bad += run_case(mk(30000, [&](size_t) { return r(); }, [&](size_t) { return r(); }), order, k, "random");
            bad += run_case(mk(100, [&](size_t) { return r() % 3; }, [&](size_t) { return r() % 3; }), order, k, "small");
        }
    // ids that differ in their lowest bits only
    {
        std::vector<TdEntry> t(9000);
        for (size_t i = 0; i < t.size(); ++i) t[i] = TdEntry{0xABCD000000000000ull + i, 5 ^ kTdSign, 9 ^ kTdSign};
        for (uint32_t order = 0; order < 4; ++order) bad += run_case(t, order, 4096, "sequential-ids");
    }
    printf(bad ? "FAILED\n" : "ALL OK\n");
    return bad != 0;
}

// sanitize_phase.cpp -- stand-alone driver of the host code of the triples and of read-backed phasing (bgreat_amd/csrc/phase_host.h: the order of
// the triples, the join of neighbouring bubbles with the triple counts, the lines of the two files), built with -fsanitize=address,undefined by
// tests/test_phase_sanitizers.py.  No device, no library: the header alone.  The inputs are heap blocks of exactly their size, so a search or a
// join that reads beyond a list is caught.
//   sanitize_phase  ->  prints "phase ok"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "phase_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bgr_bubble bubble(int32_t s, int32_t t, int32_t b, int32_t c) { return bgr_bubble{s, t, {b, c}, {1, 1, 1, 1}}; }
static bgr_triple triple(int32_t a, int32_t b, int32_t c, uint64_t n) {
    int32_t t[3];
    bgr::phase_canonical(a, b, c, t);
    return bgr_triple{t[0], t[1], t[2], 0, n};
}
static std::vector<bgr_triple> sorted(std::vector<bgr_triple> v) {
    std::sort(v.begin(), v.end(), [](const bgr_triple& x, const bgr_triple& y) { return bgr::phase_key(x.from, x.via, x.to) < bgr::phase_key(y.from, y.via, y.to); });
    return v;
}
static bool same(const bgr_phase& p, int32_t via, int32_t s, int32_t i0, int32_t i1, int32_t o0, int32_t o1, int32_t t, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    return p.via == via && p.source == s && p.in[0] == i0 && p.in[1] == i1 && p.out[0] == o0 && p.out[1] == o1 && p.sink == t && p.reserved == 0 && p.count[0] == a && p.count[1] == b &&
           p.count[2] == c && p.count[3] == d;
}

int main() {
    const int32_t top = 0x3FFFFFFF;
    // the key and the canonical form, at both ends of the id range
    CHECK(bgr::phase_key(1, 1, 1) < bgr::phase_key(1, 1, -1) && bgr::phase_key(1, 1, -1) < bgr::phase_key(1, -1, 1) && bgr::phase_key(1, -top, -top) < bgr::phase_key(-1, 1, 1));
    CHECK(bgr::phase_key(top, top, top) < bgr::phase_key(-top, 1, 1) && bgr::phase_key(-top, -top, top) < bgr::phase_key(-top, -top, -top));
    CHECK(bgr::phase_id_ok(1) && bgr::phase_id_ok(-top) && !bgr::phase_id_ok(0) && !bgr::phase_id_ok(INT32_MIN) && !bgr::phase_id_ok(top + 1) && !bgr::phase_id_ok(-top - 1));
    int32_t t[3];
    bgr::phase_canonical(3, -2, 1, t); CHECK(t[0] == -1 && t[1] == 2 && t[2] == -3);
    bgr::phase_canonical(-1, 1, -1, t); CHECK(t[0] == 1 && t[1] == -1 && t[2] == 1);
    bgr::phase_canonical(top, -top, top, t); CHECK(t[0] == top && t[1] == -top && t[2] == top);
    bgr::phase_canonical(-top, top, -top, t); CHECK(t[0] == top && t[1] == -top && t[2] == top);

    {   // the search: every member found with its count, both spellings; misses before, between and behind; an empty list
        const std::vector<bgr_triple> v = sorted({triple(2, 4, 5, 4), triple(3, 4, 6, 5), triple(2, 4, 6, 1), triple(top, top, top, ~0ull), triple(1, 1, 1, 9)});
        uint64_t bad = 0;
        CHECK(bgr::phase_check(nullptr, 0, v.data(), v.size(), &bad) == 0);
        CHECK(bgr::phase_count_of(v.data(), v.size(), 2, 4, 5) == 4 && bgr::phase_count_of(v.data(), v.size(), -5, -4, -2) == 4 && bgr::phase_count_of(v.data(), v.size(), 3, 4, 6) == 5);
        CHECK(bgr::phase_count_of(v.data(), v.size(), top, top, top) == ~0ull && bgr::phase_count_of(v.data(), v.size(), -top, -top, -top) == ~0ull && bgr::phase_count_of(v.data(), v.size(), 1, 1, 1) == 9);
        CHECK(bgr::phase_count_of(v.data(), v.size(), 3, 4, 5) == 0 && bgr::phase_count_of(v.data(), v.size(), 1, 1, -1) == 0 && bgr::phase_count_of(v.data(), v.size(), -top, top, top) == 0);
        CHECK(bgr::phase_count_of(nullptr, 0, 1, 2, 3) == 0);
    }
    {   // the checks: an id that is none, a triple that is not canonical, a list that is not ascending
        uint64_t bad = 99;
        std::vector<bgr_bubble> b = {bubble(1, 4, 2, 3), bubble(4, 7, 5, 0)};
        CHECK(bgr::phase_check(b.data(), b.size(), nullptr, 0, &bad) == 1 && bad == 1);
        b[1].branch[1] = INT32_MIN; CHECK(bgr::phase_check(b.data(), b.size(), nullptr, 0, &bad) == 1);
        std::vector<bgr_triple> v = {triple(1, 2, 3, 1), bgr_triple{0, 1, 1, 0, 1}};
        CHECK(bgr::phase_check(nullptr, 0, v.data(), v.size(), &bad) == 2 && bad == 1);
        v[1] = bgr_triple{3, 2, -1, 0, 1}; CHECK(bgr::phase_check(nullptr, 0, v.data(), v.size(), &bad) == 3 && bad == 1);   // ((1, -2, -3) stands for it)
        v[1] = triple(1, 2, 3, 1); CHECK(bgr::phase_check(nullptr, 0, v.data(), v.size(), &bad) == 4 && bad == 1);
        v[1] = triple(1, 1, 3, 1); CHECK(bgr::phase_check(nullptr, 0, v.data(), v.size(), &bad) == 4);
    }
    {   // 1 -> {2, 3} -> 4 -> {5, 6} -> 7: one record, whatever the order of the bubbles; no triples: the record with four zeroes
        const std::vector<bgr_triple> v = sorted({triple(2, 4, 5, 4), triple(3, 4, 6, 5), triple(2, 4, 6, 1)});
        for (const std::vector<bgr_bubble>& b : {std::vector<bgr_bubble>{bubble(1, 4, 2, 3), bubble(4, 7, 5, 6)}, std::vector<bgr_bubble>{bubble(4, 7, 6, 5), bubble(1, 4, 3, 2)}}) {
            const std::vector<bgr_phase> r = bgr::phase_of(b.data(), b.size(), v.data(), v.size());
            CHECK(r.size() == 1 && same(r[0], 4, 1, 2, 3, 5, 6, 7, 4, 1, 0, 5));
            const std::vector<bgr_phase> z = bgr::phase_of(b.data(), b.size(), nullptr, 0);
            CHECK(z.size() == 1 && same(z[0], 4, 1, 2, 3, 5, 6, 7, 0, 0, 0, 0));
        }
    }
    {   // the shared unitig walked backwards in both records: reported in the reading with via > 0, the branches as that reading orients them
        const std::vector<bgr_bubble> b = {bubble(1, -4, 2, 3), bubble(-7, 4, 5, 6)};   // X = (1, -4): its mate (4, -1, -2, -3) has source 4; Y = (-7, 4) has sink 4
        const std::vector<bgr_triple> v = sorted({triple(5, 4, -2, 3), triple(6, 4, -3, 2)});
        const std::vector<bgr_phase> r = bgr::phase_of(b.data(), b.size(), v.data(), v.size());
        CHECK(r.size() == 1 && same(r[0], 4, -7, 5, 6, -2, -3, -1, 3, 0, 0, 2));
    }
    {   // a chain of three and a bubble on its own: two records, ordered by via; a single bubble, no bubble: none
        const std::vector<bgr_bubble> b = {bubble(1, 9, 2, 3), bubble(9, 5, 7, 8), bubble(5, 12, 10, 11), bubble(20, 23, 21, 22)};
        const std::vector<bgr_phase> r = bgr::phase_of(b.data(), b.size(), nullptr, 0);
        CHECK(r.size() == 2 && r[0].via == 5 && r[1].via == 9 && r[0].source == 9 && r[0].sink == 12 && r[1].source == 1 && r[1].sink == 5);
        CHECK(bgr::phase_of(b.data() + 3, 1, nullptr, 0).empty() && bgr::phase_of(nullptr, 0, nullptr, 0).empty());
    }
    {   // ids at the top of the range
        const std::vector<bgr_bubble> b = {bubble(top - 6, top - 3, top - 5, top - 4), bubble(top - 3, top, top - 2, top - 1)};
        const std::vector<bgr_triple> v = sorted({triple(top - 4, top - 3, top - 1, 7)});
        const std::vector<bgr_phase> r = bgr::phase_of(b.data(), b.size(), v.data(), v.size());
        CHECK(r.size() == 1 && same(r[0], top - 3, top - 6, top - 5, top - 4, top - 2, top - 1, top, 0, 0, 0, 7));
    }

    // the calls and the lines
    const uint64_t big = ~0ull;
    const uint64_t c1[4] = {4, 1, 0, 5}, c2[4] = {1, 5, 5, 0}, c3[4] = {0, 0, 0, 0}, c4[4] = {big, big, big, big - 1}, c5[4] = {big, 1, 0, big}, c6[4] = {2, 1, 3, 2};
    CHECK(!strcmp(bgr::phase_call(c1), "cis") && !strcmp(bgr::phase_call(c2), "trans") && !strcmp(bgr::phase_call(c3), ".") && !strcmp(bgr::phase_call(c4), "trans"));
    CHECK(!strcmp(bgr::phase_call(c5), "cis") && !strcmp(bgr::phase_call(c6), "."));
    std::string buf = bgr::triples_header();
    bgr::triples_line(bgr_triple{-top, top, -1, 0, big}, &buf);
    CHECK(buf == "#from\tvia\tto\tcount\n-1073741823\t1073741823\t-1\t18446744073709551615\n");
    buf = bgr::phase_header();
    bgr_phase p = {4, -1, {2, -3}, {-5, 6}, 7, 0, {big, 0, 1, 2}};
    bgr::phase_line(p, &buf);
    CHECK(buf == "#via\tsource\tin1\tin2\tout1\tout2\tsink\tn11\tn12\tn21\tn22\tphase\n4\t-1\t2\t-3\t-5\t6\t7\t18446744073709551615\t0\t1\t2\tcis\n");

    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("phase ok\n");
    return 0;
}

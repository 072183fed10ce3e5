// sanitize_bubbles.cpp -- stand-alone driver of the host code of bubble calling (bgreat_amd/csrc/bubbles_host.h: the rule an oriented id passes,
// the writer's comparison of the two branches), built with -fsanitize=address,undefined by tests/test_bubbles_sanitizers.py.  No device, no
// library: the header alone.  The adjacency arrays are heap blocks of exactly their size, so a rule that reads a slot it may not read is caught.
//   sanitize_bubbles  ->  prints "bubbles ok"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bubbles_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Adj {   // what pass 1 leaves for n unitigs, built edge by edge in the order given
    uint64_t n;
    std::vector<uint32_t> deg;
    std::vector<int32_t> to;
    std::vector<uint64_t> cnt;
    explicit Adj(uint64_t n_) : n(n_), deg(2 * n_, 0), to(4 * n_, 0x5A5A5A5A), cnt(4 * n_, 0xA5A5A5A5A5A5A5A5ull) {}
    void link(int32_t a, int32_t b, uint64_t c) {   // a canonical link: the edge and, unless it is its own, the strand mate
        bgr::bubbles_add_edge(deg.data(), to.data(), cnt.data(), a, b, c);
        if (b != -a) bgr::bubbles_add_edge(deg.data(), to.data(), cnt.data(), -b, -a, c);
    }
    std::vector<bgr_bubble> all() const {
        std::vector<bgr_bubble> out;
        for (uint64_t o = 0; o < 2 * n; ++o) {
            bgr_bubble r;
            if (bgr::bubble_at(deg.data(), to.data(), cnt.data(), n, bgr::bubbles_id_of(o), &r)) out.push_back(r);
        }
        return out;
    }
};

static bool same(const bgr_bubble& r, int32_t s, int32_t t, int32_t b, int32_t c, uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3) {
    return r.source == s && r.sink == t && r.branch[0] == b && r.branch[1] == c && r.count[0] == c0 && r.count[1] == c1 && r.count[2] == c2 && r.count[3] == c3;
}

int main() {
    // the oriented index and back, at both ends of the id range
    for (int32_t x : {1, -1, 2, -2, 0x3FFFFFFF, -0x3FFFFFFF}) CHECK(bgr::bubbles_id_of(bgr::bubbles_o(x)) == x);
    CHECK(bgr::bubbles_o(1) == 0 && bgr::bubbles_o(-1) == 1 && bgr::bubbles_o(-0x3FFFFFFF) == 2ull * 0x3FFFFFFE + 1);
    CHECK(bgr::bubbles_id_less(2, -2) && bgr::bubbles_id_less(-2, 3) && !bgr::bubbles_id_less(-2, 2));

    {   // one bubble 1 -> {2, 3} -> 4, its edges in both orders of arrival: the same single record, counts beyond 2^32 kept
        const uint64_t big = (1ull << 40) + 7;
        Adj x(4), y(4);
        x.link(1, 2, big); x.link(1, 3, 5); x.link(2, 4, 6); x.link(3, 4, 9);
        y.link(3, 4, 9); y.link(1, 3, 5); y.link(2, 4, 6); y.link(1, 2, big);
        for (const Adj* a : {&x, &y}) {
            const std::vector<bgr_bubble> r = a->all();
            CHECK(r.size() == 1 && same(r[0], 1, 4, 2, 3, big, 6, 5, 9));
        }
    }
    {   // the same bubble with every id negated and reversed: reported under the smaller (s, t) -- here -4's mate, source 1 again -- branches 2 before 3
        Adj a(4);
        a.link(-4, -3, 9); a.link(-4, -2, 6); a.link(-3, -1, 5); a.link(-2, -1, 1);
        const std::vector<bgr_bubble> r = a.all();
        CHECK(r.size() == 1 && same(r[0], 1, 4, 2, 3, 1, 6, 5, 9));
    }
    {   // a bubble walked against its unitigs: source -3, branches -2 and 1 (|1| before |-2|), sink 4
        Adj a(4);
        a.link(-3, -2, 2); a.link(-3, 1, 3); a.link(-2, 4, 4); a.link(1, 4, 5);
        const std::vector<bgr_bubble> r = a.all();
        CHECK(r.size() == 1 && same(r[0], -3, 4, 1, -2, 3, 5, 2, 4));
    }
    {   // a third successor only counts (its slot does not exist: the arrays would be overrun), and opens nothing
        Adj a(5);
        a.link(1, 2, 1); a.link(1, 3, 1); a.link(1, 5, 1); a.link(2, 4, 1); a.link(3, 4, 1);
        CHECK(a.deg[bgr::bubbles_o(1)] == 3 && a.all().empty());
    }
    {   // an extra way into a branch, into the sink; branches to different sinks; the sink reached in the other orientation
        Adj a(5), b(5), c(5), d(4);
        a.link(1, 2, 1); a.link(1, 3, 1); a.link(2, 4, 1); a.link(3, 4, 1); a.link(-5, 2, 1);
        b.link(1, 2, 1); b.link(1, 3, 1); b.link(2, 4, 1); b.link(3, 4, 1); b.link(-5, 4, 1);
        c.link(1, 2, 1); c.link(1, 3, 1); c.link(2, 4, 1); c.link(3, 5, 1);
        d.link(1, 2, 1); d.link(1, 3, 1); d.link(2, 4, 1); d.link(3, -4, 1);
        CHECK(a.all().empty() && b.all().empty() && c.all().empty() && d.all().empty());
    }
    {   // fewer than four unitigs: the sink is the source, the branches are one unitig on its two strands, a link onto itself, one that is its own mate
        Adj a(3), b(3), c(4), d(4);
        a.link(1, 2, 1); a.link(1, 3, 1); a.link(2, 1, 1); a.link(3, 1, 1);
        b.link(1, 2, 1); b.link(1, -2, 1); b.link(2, 3, 1); b.link(-2, 3, 1);
        c.link(1, 1, 1); c.link(1, 2, 1); c.link(2, 4, 1); c.link(1, 3, 1);
        d.link(1, -1, 1); d.link(1, 2, 1); d.link(2, 4, 1); d.link(-1, 3, 1);
        CHECK(a.all().empty() && b.all().empty() && c.all().empty() && d.all().empty());
        CHECK(d.deg[bgr::bubbles_o(1)] == 2 && d.deg[bgr::bubbles_o(-1)] == 1);   // (1 -> -1 is one edge)
    }
    {   // a successor outside 1 .. n opens nothing and is not followed
        Adj a(4);
        a.link(1, 2, 1); a.link(1, 3, 1); a.link(2, 4, 1); a.link(3, 4, 1);
        a.to[2 * bgr::bubbles_o(1)] = 9;
        CHECK(a.all().empty());
    }

    // the writer's comparison
    const std::string u = "ACGTTGCAAC";
    CHECK(bgr::bubbles_oriented(u.data(), u.size(), false) == u);
    CHECK(bgr::bubbles_oriented(u.data(), u.size(), true) == "GTTGCAACGT");
    CHECK(bgr::bubbles_oriented(u.data(), 0, true).empty() && bgr::bubbles_oriented(u.data(), 1, true) == "T" && bgr::bubbles_oriented("acgtN", 5, true) == "Nacgt");
    std::string kind, diff;
    bgr::bubbles_compare("ACGTA", "ACCTA", &kind, &diff); CHECK(kind == "snv" && diff == "2:G>C");
    bgr::bubbles_compare("ACGTA", "TCGTA", &kind, &diff); CHECK(kind == "snv" && diff == "0:A>T");
    bgr::bubbles_compare("ACGTA", "ACGTC", &kind, &diff); CHECK(kind == "snv" && diff == "4:A>C");
    bgr::bubbles_compare("ACGTA", "TCGTC", &kind, &diff); CHECK(kind == "mnv" && diff == ".");
    bgr::bubbles_compare("ACGTA", "ACGTA", &kind, &diff); CHECK(kind == "mnv" && diff == ".");
    bgr::bubbles_compare("ACGTA", "ACGT", &kind, &diff); CHECK(kind == "indel" && diff == ".");
    bgr::bubbles_compare("", "A", &kind, &diff); CHECK(kind == "indel" && diff == ".");

    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("bubbles ok\n");
    return 0;
}

// sanitize_haplotypes.cpp -- stand-alone driver of the host code of the haplotypes' sequences (bgreat_amd/csrc/haplotypes_host.h: the oriented ids of
// an entry, the checks of the two lists before any device work, the walk strings, the header line, the check of the records the writer takes), built
// with -fsanitize=address,undefined by tests/test_haplotypes_sanitizers.py.  No device, no library: the header alone.  The inputs are heap blocks of
// exactly their size, so a check that reads beyond a list is caught.
//   sanitize_haplotypes  ->  prints "haplotypes ok"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "haplotypes_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bgr_bubble bubble(int32_t s, int32_t t, int32_t b, int32_t c) { return bgr_bubble{s, t, {b, c}, {1, 1, 1, 1}}; }
static bgr_block_entry entry(uint32_t block, uint32_t index, uint32_t size, uint32_t bub, uint32_t flags) { return bgr_block_entry{block, index, size, bub, flags, 0}; }

int main() {
    const int32_t top = 0x3FFFFFFF;
    const uint32_t R = BGR_BLOCK_REVERSED, H = BGR_BLOCK_HAP, C = BGR_BLOCK_CIRCULAR, X = BGR_BLOCK_CONFLICT;
    {   // the oriented ids, as bgr_write_blocks prints them
        const bgr_bubble b = bubble(1, -4, 2, 3);
        const bgr_block_entry e0 = entry(1, 0, 1, 0, 0), e1 = entry(1, 0, 1, 0, H), e2 = entry(1, 0, 1, 0, R), e3 = entry(1, 0, 1, 0, R | H | C);
        CHECK(bgr::hap_src(e0, b) == 1 && bgr::hap_snk(e0, b) == -4 && bgr::hap_branch(e0, b, 0) == 2 && bgr::hap_branch(e0, b, 1) == 3);
        CHECK(bgr::hap_branch(e1, b, 0) == 3 && bgr::hap_branch(e1, b, 1) == 2);
        CHECK(bgr::hap_src(e2, b) == 4 && bgr::hap_snk(e2, b) == -1 && bgr::hap_branch(e2, b, 0) == -2 && bgr::hap_branch(e2, b, 1) == -3);
        CHECK(bgr::hap_branch(e3, b, 0) == -3 && bgr::hap_branch(e3, b, 1) == -2 && bgr::hap_ring(e3) == C && bgr::hap_ring(e0) == 0);
    }
    // a chain of two, a block of one read reversed, a ring of two
    const std::vector<bgr_bubble> b = {bubble(1, 4, 2, 3), bubble(4, 7, 5, 6), bubble(-8, 11, 9, -10), bubble(12, 15, 13, 14), bubble(-12, -15, 16, 17)};
    const std::vector<bgr_block_entry> e = {entry(1, 0, 2, 0, 0), entry(1, 1, 2, 1, H), entry(2, 0, 1, 2, R), entry(3, 0, 2, 3, C), entry(3, 1, 2, 4, C | R)};
    {   // the checks, each refusal with its record
        uint64_t bad = 99;
        CHECK(bgr::haplotypes_check(b.data(), b.size(), e.data(), e.size(), 17, &bad) == 0);
        CHECK(bgr::haplotypes_check(nullptr, 0, nullptr, 0, 0, &bad) == 0);
        CHECK(bgr::haplotypes_check(b.data(), b.size(), nullptr, 0, 17, &bad) == 0);
        CHECK(bgr::haplotypes_check(b.data(), b.size(), e.data(), e.size(), 16, &bad) == 1 && bad == 4);   // an id beyond the graph
        std::vector<bgr_bubble> c = b;
        c[1].branch[1] = 0; CHECK(bgr::haplotypes_check(c.data(), c.size(), e.data(), e.size(), 17, &bad) == 1 && bad == 1);
        c[1].branch[1] = INT32_MIN; CHECK(bgr::haplotypes_check(c.data(), c.size(), e.data(), e.size(), ~0ull, &bad) == 1);
        c[1].branch[1] = top + 1; CHECK(bgr::haplotypes_check(c.data(), c.size(), e.data(), e.size(), ~0ull, &bad) == 1);
        std::vector<bgr_block_entry> f = e;
        f[2].bubble = 5; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 2 && bad == 2);
        f = e; f[4].flags = 16; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 2 && bad == 4);
        f = e; f[1].index = 0; f[1].size = 1; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 3 && bad == 1);   // a block that ends early
        f = e; f[1].size = 3; f[1].index = 1; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 3 && bad == 1);   // a size that changes
        f = e; f[1].block = 2; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 3 && bad == 1);
        f = e; f[2].block = 1; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 3 && bad == 2);   // numbers that do not ascend
        f = e; f[4].flags = R; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 3 && bad == 4);   // a ring flag that changes
        f = e; f.pop_back(); f.shrink_to_fit(); CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 3 && bad == 3);   // the last block ends late
        f = {entry(1, 1, 2, 1, H)}; f.shrink_to_fit(); CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 3 && bad == 0);   // a list that begins inside a block
        f = e; f[1].bubble = 3; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 4 && bad == 1);   // 4 is not 12: no link
        f = e; f[4].flags = C; CHECK(bgr::haplotypes_check(b.data(), b.size(), f.data(), f.size(), 17, &bad) == 4 && bad == 4);   // (-12 is not 15)
        CHECK(bgr::haplotypes_check(b.data(), b.size(), e.data(), 0x40000000ull, 17, &bad) == 5);   // (refused before a record is read)
    }
    {   // the walks and the header lines
        std::string w;
        bgr::hap_walk(e.data(), 2, b.data(), 0, &w); CHECK(w == ">1>2>4>6>7");
        w.clear(); bgr::hap_walk(e.data(), 2, b.data(), 1, &w); CHECK(w == ">1>3>4>5>7");
        w.clear(); bgr::hap_walk(e.data() + 2, 1, b.data(), 0, &w); CHECK(w == "<11<9>8");
        w.clear(); bgr::hap_walk(e.data() + 2, 1, b.data(), 1, &w); CHECK(w == "<11>10>8");
        w.clear(); bgr::hap_walk(e.data() + 3, 2, b.data(), 0, &w); CHECK(w == ">12>13>15<16>12");
        w.clear(); bgr::hap_walk_id(-top, &w); bgr::hap_walk_id(top, &w); CHECK(w == "<1073741823>1073741823");
        std::string buf;
        bgr::hap_header(bgr_haplotype{1, 0, 2, 0, 0, 26}, e.data(), b.data(), &buf);
        CHECK(buf == ">block1_A bubbles=2 length=26 ring=. walk=>1>2>4>6>7\n");
        buf.clear(); bgr::hap_header(bgr_haplotype{3, 1, 2, C, 0, ~0ull}, e.data() + 3, b.data(), &buf);
        CHECK(buf == ">block3_B bubbles=2 length=18446744073709551615 ring=circular walk=>12>14>15<17>12\n");
        buf.clear(); bgr::hap_header(bgr_haplotype{0xFFFFFFFFu, 0, 1, C | X, 0, 0}, e.data() + 2, b.data(), &buf);
        CHECK(buf == ">block4294967295_A bubbles=1 length=0 ring=conflict walk=<11<9>8\n");
    }
    {   // the records the writer takes: those of the kept blocks, back to back
        std::vector<bgr_haplotype> h = {{1, 0, 2, 0, 0, 10}, {1, 1, 2, 0, 10, 12}, {3, 0, 2, C, 22, 5}, {3, 1, 2, C, 27, 5}};
        std::vector<uint64_t> first(h.size());
        uint64_t bad = 99;
        CHECK(bgr::hap_records_ok(h.data(), h.size(), e.data(), e.size(), 32, first.data(), &bad) && first[0] == 0 && first[1] == 0 && first[2] == 3 && first[3] == 3);
        CHECK(bgr::hap_records_ok(nullptr, 0, e.data(), e.size(), 0, nullptr, &bad) && bgr::hap_records_ok(nullptr, 0, nullptr, 0, 0, nullptr, &bad));
        CHECK(!bgr::hap_records_ok(h.data(), h.size(), e.data(), e.size(), 33, first.data(), &bad) && bad == 4);   // bytes left over
        CHECK(!bgr::hap_records_ok(h.data(), h.size(), e.data(), e.size(), 31, first.data(), &bad) && bad == 3);   // a sequence beyond the bytes
        CHECK(!bgr::hap_records_ok(nullptr, 0, e.data(), e.size(), 1, nullptr, &bad));
        std::vector<bgr_haplotype> g = h;
        g[1].hap = 0; CHECK(!bgr::hap_records_ok(g.data(), g.size(), e.data(), e.size(), 32, first.data(), &bad) && bad == 1);
        g = h; g[1].block = 2; CHECK(!bgr::hap_records_ok(g.data(), g.size(), e.data(), e.size(), 32, first.data(), &bad) && bad == 1);
        g = h; g[2].block = 4; g[3].block = 4; CHECK(!bgr::hap_records_ok(g.data(), g.size(), e.data(), e.size(), 32, first.data(), &bad) && bad == 2);   // no such block
        g = h; g[2].flags = 0; CHECK(!bgr::hap_records_ok(g.data(), g.size(), e.data(), e.size(), 32, first.data(), &bad) && bad == 2);
        g = h; g[2].size = 1; CHECK(!bgr::hap_records_ok(g.data(), g.size(), e.data(), e.size(), 32, first.data(), &bad) && bad == 2);
        g = h; g[2].offset = 21; CHECK(!bgr::hap_records_ok(g.data(), g.size(), e.data(), e.size(), 32, first.data(), &bad) && bad == 2);
        g = h; g[3].length = ~0ull; CHECK(!bgr::hap_records_ok(g.data(), g.size(), e.data(), e.size(), 32, first.data(), &bad) && bad == 3);
        g = {h[2], h[3], h[0], h[1]}; g[0].offset = 0; g[1].offset = 5; g[2].offset = 10; g[3].offset = 20;
        CHECK(!bgr::hap_records_ok(g.data(), g.size(), e.data(), e.size(), 32, first.data(), &bad) && bad == 2);   // out of block order
    }

    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("haplotypes ok\n");
    return 0;
}

// sanitize_blocks.cpp -- stand-alone driver of the host code of haplotype blocks (bgreat_amd/csrc/blocks_host.h: how a bubble record reads as a
// node, when a phase record is a decided link, the checks of the two lists before any device work, the header and line of the file), built with
// -fsanitize=address,undefined by tests/test_blocks_sanitizers.py.  No device, no library: the header alone.  The inputs are heap blocks of exactly
// their size, so a check that reads beyond a list is caught.
//   sanitize_blocks  ->  prints "blocks ok"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "blocks_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bgr_bubble bubble(int32_t s, int32_t t, int32_t b, int32_t c) { return bgr_bubble{s, t, {b, c}, {1, 1, 1, 1}}; }
static bgr_phase phase(int32_t via, int32_t s, int32_t i0, int32_t i1, int32_t o0, int32_t o1, int32_t t) { return bgr_phase{via, s, {i0, i1}, {o0, o1}, t, 0, {1, 0, 0, 1}}; }

// the decision as phase_call's 128-bit sums make it
static bool decided128(const uint64_t c[4], uint64_t min_phase, uint32_t* parity) {
    const unsigned __int128 cis = (unsigned __int128)c[0] + c[3], trans = (unsigned __int128)c[1] + c[2];
    *parity = trans > cis ? 1u : 0u;
    return (trans > cis ? trans - cis : cis - trans) >= min_phase;
}

int main() {
    const int32_t top = 0x3FFFFFFF;
    const uint64_t big = ~0ull;
    {   // the decision against 128-bit sums: small counts, carries on either side, thresholds at, below and above the difference
        const uint64_t vals[] = {0, 1, 2, 3, 7, big - 2, big - 1, big, 1ull << 63, (1ull << 63) - 1};
        const uint64_t mins[] = {1, 2, 3, 4, big - 1, big, 1ull << 63};
        uint64_t checked = 0;
        for (uint64_t a : vals) for (uint64_t b : vals) for (uint64_t c : vals) for (uint64_t d : vals) for (uint64_t m : mins) {
            const uint64_t n[4] = {a, b, c, d};
            uint32_t p = 9, q = 9;
            const bool x = bgr::blocks_decided(n, m, &p), y = decided128(n, m, &q);
            if (x != y || (x && p != q)) { printf("FAIL decided {%llu %llu %llu %llu} min %llu\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)c, (unsigned long long)d, (unsigned long long)m); ++failures; }
            ++checked;
        }
        CHECK(checked == 70000);
        const uint64_t c1[4] = {6, 1, 2, 0}, c2[4] = {big, big, big - 1, big}, c3[4] = {1, 1, 1, 1}, c4[4] = {0, 0, 0, 0};
        uint32_t p = 0;
        CHECK(bgr::blocks_decided(c1, 3, &p) && p == 0 && !bgr::blocks_decided(c1, 4, &p) && bgr::blocks_decided(c2, 1, &p) && p == 0 && !bgr::blocks_decided(c2, 2, &p));
        CHECK(!bgr::blocks_decided(c3, 1, &p) && !bgr::blocks_decided(c4, 1, &p) && !strcmp(bgr::phase_call(c3), "."));
    }
    {   // a record as a node, both ways: the mate of the mate is the record
        const bgr_bubble b = bubble(1, -4, 2, 3);
        CHECK(bgr::blocks_source(b, 0) == 1 && bgr::blocks_sink(b, 0) == -4 && bgr::blocks_branch(b, 0, 0) == 2 && bgr::blocks_branch(b, 0, 1) == 3);
        CHECK(bgr::blocks_source(b, 1) == 4 && bgr::blocks_sink(b, 1) == -1 && bgr::blocks_branch(b, 1, 0) == -2 && bgr::blocks_branch(b, 1, 1) == -3);
        const bgr_bubble t = bubble(-top, top - 1, top - 3, -(top - 2));
        CHECK(bgr::blocks_source(t, 1) == -(top - 1) && bgr::blocks_sink(t, 1) == top && bgr::blocks_branch(t, 1, 1) == top - 2);
    }
    {   // the checks, each refusal with its record
        uint64_t bad = 99;
        std::vector<bgr_bubble> b = {bubble(1, 4, 2, 3), bubble(4, 7, 5, 6), bubble(-8, 11, 9, -10)};
        std::vector<bgr_phase> p = {phase(4, 1, 2, 3, 5, 6, 7)};
        CHECK(bgr::blocks_check(b.data(), b.size(), p.data(), p.size(), 11, &bad) == 0);
        CHECK(bgr::blocks_check(nullptr, 0, nullptr, 0, 0, &bad) == 0);
        CHECK(bgr::blocks_check(b.data(), b.size(), p.data(), p.size(), 10, &bad) == 1 && bad == 2);   // an id beyond n_unitigs
        std::vector<bgr_bubble> c = b;
        c[1].branch[0] = 0; CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 1 && bad == 1);
        c[1].branch[0] = INT32_MIN; CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 1);
        c[1].branch[0] = top + 1; CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, ~0ull, &bad) == 1);
        c = b; c[2].branch[0] = 10; c[2].branch[1] = -9; CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 2 && bad == 2);   // the branches' order
        c = b; c[0].branch[1] = -2; CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 2 && bad == 0);   // a branch and its own mate
        c = b; c[1].sink = 5; CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 2 && bad == 1);
        c = b; c[1] = bubble(7, 4, 5, 6); CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 3 && bad == 1);   // (-4, -7) is the canonical reading
        c = b; std::swap(c[0], c[1]); CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 4 && bad == 1);   // unsorted
        c = b; c[1] = bubble(1, 5, 6, 7); CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 4 && bad == 1);   // one source twice
        c = b; c[1] = bubble(-1, 5, 6, 7); CHECK(bgr::blocks_check(c.data(), c.size(), nullptr, 0, 11, &bad) == 0);              // (1 and -1 are two oriented ids)
        std::vector<bgr_phase> q = p;
        q[0].out[1] = 12; CHECK(bgr::blocks_check(b.data(), b.size(), q.data(), q.size(), 11, &bad) == 5 && bad == 0);
        q = p; q[0].via = -4; CHECK(bgr::blocks_check(b.data(), b.size(), q.data(), q.size(), 11, &bad) == 5);
        q = {phase(8, 4, 5, 6, 9, -10, 11), phase(4, 1, 2, 3, 5, 6, 7)}; CHECK(bgr::blocks_check(b.data(), b.size(), q.data(), q.size(), 11, &bad) == 6 && bad == 1);
        q = {p[0], p[0]}; CHECK(bgr::blocks_check(b.data(), b.size(), q.data(), q.size(), 11, &bad) == 6 && bad == 1);
        CHECK(bgr::blocks_check(b.data(), 0x40000000ull, nullptr, 0, 11, &bad) == 7);   // (refused before a record is read)
    }
    {   // the entries the writer takes, and the lines
        const std::vector<bgr_bubble> b = {bubble(1, -4, 2, 3), bubble(-7, 4, 5, 6)};
        std::vector<bgr_block_entry> e = {bgr_block_entry{1, 0, 2, 0, 0, 0}, bgr_block_entry{1, 1, 2, 1, BGR_BLOCK_REVERSED | BGR_BLOCK_HAP, 0}};
        uint64_t bad = 99;
        CHECK(bgr::blocks_entries_ok(e.data(), e.size(), b.size(), &bad) && bgr::blocks_entries_ok(nullptr, 0, 0, &bad));
        CHECK(!bgr::blocks_entries_ok(e.data(), e.size(), 1, &bad) && bad == 1);
        std::vector<bgr_block_entry> f = e;
        f[0].flags = 16; CHECK(!bgr::blocks_entries_ok(f.data(), f.size(), b.size(), &bad) && bad == 0);
        f = e; f[1].index = 2; CHECK(!bgr::blocks_entries_ok(f.data(), f.size(), b.size(), &bad) && bad == 1);
        f = e; f[1].block = 0; CHECK(!bgr::blocks_entries_ok(f.data(), f.size(), b.size(), &bad) && bad == 1);
        std::string buf = bgr::blocks_header();
        for (const bgr_block_entry& x : e) bgr::blocks_line(x, b[x.bubble], &buf);
        CHECK(buf == "#block\tindex\tsize\tbubble\tsource\tsink\thapA\thapB\tstrand\tring\n1\t0\t2\t1\t1\t-4\t2\t3\t+\t.\n1\t1\t2\t2\t-4\t7\t-6\t-5\t-\t.\n");
        buf.clear();
        bgr::blocks_line(bgr_block_entry{0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0, BGR_BLOCK_CIRCULAR | BGR_BLOCK_CONFLICT | BGR_BLOCK_HAP, 0}, bubble(-top, top, top - 1, -(top - 2)), &buf);
        CHECK(buf == "4294967295\t4294967294\t4294967295\t1\t-1073741823\t1073741823\t-1073741821\t1073741822\t+\tconflict\n");
        buf.clear();
        bgr::blocks_line(bgr_block_entry{2, 0, 1, 0, BGR_BLOCK_CIRCULAR | BGR_BLOCK_REVERSED, 0}, bubble(1, 4, 2, 3), &buf);
        CHECK(buf == "2\t0\t1\t1\t-4\t-1\t-2\t-3\t-\tcircular\n");
    }

    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("blocks ok\n");
    return 0;
}

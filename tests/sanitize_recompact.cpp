// sanitize_recompact.cpp -- stand-alone driver of the host code of the re-compaction (bgreat_amd/csrc/recompact_host.h: the keep bytes, --min-reads,
// the check of a result, the header line and with them the writer's bytes) and of the run's flag rules for its switch (run_stages.h), meant to be
// built with -fsanitize=address,undefined and run as a plain program.  No device, no library.
//   sanitize_recompact                     ->  prints "recompact ok"
//   sanitize_recompact write IN OUT        ->  IN: "n walk_n seq_bytes n_unitigs k", then per record "seq_off seq_len walk_off n_unitigs flags", the walk ids, the characters;
//                                              OUT: the file as bgr_write_recompact writes it (the same two functions, the same order); status 3 when the check refuses
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "recompact_host.h"
#include "run_stages.h"

namespace bgr { RunCounts g_run_counts; }

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static std::string file_of(const std::vector<bgr_chain>& c, const std::vector<int32_t>& walk, const std::string& seq) {
    std::string out;
    for (size_t i = 0; i < c.size(); ++i) {
        bgr::recompact_header(i + 1, c[i], walk.data() + c[i].walk_off, &out);
        out.append(seq.data() + c[i].seq_off, c[i].seq_len);
        out += '\n';
    }
    return out;
}

static int write_mode(const char* in, const char* outp) {
    std::ifstream f(in);
    uint64_t n, wn, sb, nu;
    uint32_t k;
    f >> n >> wn >> sb >> nu >> k;
    std::vector<bgr_chain> c(n);
    for (auto& r : c) f >> r.seq_off >> r.seq_len >> r.walk_off >> r.n_unitigs >> r.flags;
    std::vector<int32_t> walk(wn);
    for (auto& w : walk) f >> w;
    std::string seq;
    f >> seq;
    if (!f && sb) return 4;
    if (seq.size() != sb) return 4;
    uint64_t bad = 0;
    if (!bgr::recompact_records_ok(c.data(), n, walk.data(), wn, sb, nu, k, &bad)) return 3;
    std::ofstream o(outp, std::ios::binary);
    o << file_of(c, walk, seq);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "write")) return write_mode(argv[2], argv[3]);
    using namespace bgr;
    // the flag rules: the switch implies abundance and nothing else, and nothing implies it
    {
        RunSwitches s = {};
        CHECK(counts_wanted(s) == 0);
        s.recompact = true;
        CHECK(counts_wanted(s) == (kCountRecompact | kCountAbundance));
        s.haplotypes = true;
        const uint32_t chain = kCountLinks | kCountBubbles | kCountTriples | kCountPhase | kCountBlocks | kCountHaplotypes | kCountAbundance;
        CHECK(counts_wanted(s) == (chain | kCountRecompact));
        s.recompact = false;
        CHECK(counts_wanted(s) == chain);
        RunSwitches all = {true, true, true, true, true, true, true, true, true, true, false};
        CHECK(!(counts_wanted(all) & kCountRecompact));
        CHECK(kCountRecompact == 1024);
    }
    // keep = reads >= min_reads; 0 keeps everything
    {
        const bgr_unitig_abundance rows[4] = {{0, 0, 0}, {1, 9, 9}, {2, 0, 0}, {~0ull, 1, 1}};
        uint8_t keep[5] = {7, 7, 7, 7, 7};
        recompact_keep(rows, 4, 0, keep);
        CHECK(keep[0] == 1 && keep[1] == 1 && keep[2] == 1 && keep[3] == 1 && keep[4] == 7);
        recompact_keep(rows, 4, 1, keep);
        CHECK(keep[0] == 0 && keep[1] == 1 && keep[2] == 1 && keep[3] == 1);
        recompact_keep(rows, 4, 2, keep);
        CHECK(keep[0] == 0 && keep[1] == 0 && keep[2] == 1 && keep[3] == 1);
        recompact_keep(rows, 4, 999999999, keep);
        CHECK(keep[2] == 0 && keep[3] == 1);
        recompact_keep(rows, 0, 1, keep);
    }
    // --min-reads: one to nine digits
    {
        uint64_t v = 77;
        CHECK(recompact_parse_min_reads("0", &v) && v == 0);
        CHECK(recompact_parse_min_reads("1", &v) && v == 1);
        CHECK(recompact_parse_min_reads("007", &v) && v == 7);
        CHECK(recompact_parse_min_reads("999999999", &v) && v == 999999999ull);
        v = 5;
        CHECK(!recompact_parse_min_reads("1000000000", &v) && v == 5);
        CHECK(!recompact_parse_min_reads("", &v) && !recompact_parse_min_reads(nullptr, &v) && !recompact_parse_min_reads("-1", &v) && !recompact_parse_min_reads("+1", &v));
        CHECK(!recompact_parse_min_reads("1 ", &v) && !recompact_parse_min_reads(" 1", &v) && !recompact_parse_min_reads("1e3", &v) && !recompact_parse_min_reads("0x1", &v) && v == 5);
    }
    // the check of a result and the bytes of the file
    {
        std::vector<bgr_chain> c = {{0, 7, 0, 2, 0}, {7, 5, 2, 1, BGR_CHAIN_CIRCULAR}};
        std::vector<int32_t> walk = {3, -1, 2};
        const std::string seq = "ACGTACGGGGGG";
        uint64_t bad = 99;
        CHECK(recompact_records_ok(c.data(), 2, walk.data(), 3, 12, 3, 5, &bad) && bad == 2);
        CHECK(file_of(c, walk, seq) == ">1 LN:i:7 unitigs=2 ring=. walk=>3<1\nACGTACG\n>2 LN:i:5 unitigs=1 ring=circular walk=>2\nGGGGG\n");
        CHECK(recompact_records_ok(nullptr, 0, nullptr, 0, 0, 3, 5, &bad) && bad == 0);
        CHECK(!recompact_records_ok(nullptr, 0, nullptr, 1, 0, 3, 5, &bad));
        CHECK(!recompact_records_ok(c.data(), 2, walk.data(), 3, 13, 3, 5, &bad) && bad == 2);    // a byte too many
        CHECK(!recompact_records_ok(c.data(), 2, walk.data(), 3, 11, 3, 5, &bad) && bad == 1);    // the last chain runs over the end
        CHECK(!recompact_records_ok(c.data(), 2, walk.data(), 2, 12, 3, 5, &bad) && bad == 1);    // ... of the walk
        CHECK(!recompact_records_ok(c.data(), 2, walk.data(), 3, 12, 2, 5, &bad) && bad == 0);    // id 3 in a graph of two
        CHECK(!recompact_records_ok(c.data(), 2, walk.data(), 3, 12, 3, 6, &bad) && bad == 1);    // five characters at k = 6
        auto broken = [&](auto change) { auto d = c; auto w = walk; change(d, w); uint64_t b; return !recompact_records_ok(d.data(), d.size(), w.data(), w.size(), 12, 3, 5, &b); };
        CHECK(broken([](auto& d, auto&) { d[1].seq_off = 6; }));
        CHECK(broken([](auto& d, auto&) { d[1].walk_off = 1; }));
        CHECK(broken([](auto& d, auto&) { d[0].n_unitigs = 0; }));
        CHECK(broken([](auto& d, auto&) { d[0].n_unitigs = 0xFFFFFFFFu; }));
        CHECK(broken([](auto& d, auto&) { d[0].seq_len = ~0ull; }));
        CHECK(broken([](auto& d, auto&) { d[1].flags = 2; }));
        CHECK(broken([](auto&, auto& w) { w[1] = 0; }));
        CHECK(broken([](auto&, auto& w) { w[2] = INT32_MIN; }));
        CHECK(broken([](auto&, auto& w) { w[0] = 4; }));
        CHECK(!broken([](auto&, auto& w) { w[0] = -3; }));
        std::string h;
        const int32_t big[2] = {INT32_MIN + 1, INT32_MAX};
        recompact_header(18446744073709551615ull, bgr_chain{0, ~0ull, 0, 2, 0}, big, &h);
        CHECK(h == ">18446744073709551615 LN:i:18446744073709551615 unitigs=2 ring=. walk=<2147483647>2147483647\n");
    }
    if (fails) { printf("%d checks FAILed\n", fails); return 1; }
    printf("recompact ok\n");
    return 0;
}

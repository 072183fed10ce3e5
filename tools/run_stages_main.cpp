// tools/run_stages_main.cpp -- the rules of bgreat_amd/csrc/run_stages.h driven by stages that only record, as a program of its own (no GPU, no
// HIP, no Python; tests/test_run_stages_host.py builds it under AddressSanitizer + UBSan):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/run_stages tools/run_stages_main.cpp
//   /tmp/run_stages end <what> <ok> [<name> <code>]...   the stages of `what` end; the named ones return `code` when they are ended with true.
//                                                        Prints "end <name> <0|1>" per call, then "rc <code>"
//   /tmp/run_stages wanted                               "<switches> <mask>" for every combination of the ten switches (bit i of `switches` = the
//                                                        i-th member of RunSwitches)
// The table has the bits, the order and the tiers of the real one (capi_abundance.hip).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bgreat_amd/csrc/run_stages.h"

using namespace bgr;

static const char* const kNames[8] = {"links", "bubbles", "triples", "phase", "blocks", "haplotypes", "pileup", "abundance"};
struct bgr_graph {   // (the handle is opaque to the rule: here it is the log and the failures to play)
    std::vector<std::string> log;
    int fail[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
template <int I>
static int end_stage(bgr_graph* g, bool ok) {
    g->log.push_back(std::string("end ") + kNames[I] + (ok ? " 1" : " 0"));
    return ok ? g->fail[I] : BGR_OK;
}
static const RunStage kStages[8] = {
    {kCountLinks, nullptr, nullptr, nullptr, end_stage<0>, kTierTables},      {kCountBubbles, nullptr, nullptr, nullptr, end_stage<1>, kTierDerived},
    {kCountTriples, nullptr, nullptr, nullptr, end_stage<2>, kTierTables},    {kCountPhase, nullptr, nullptr, nullptr, end_stage<3>, kTierDerived},
    {kCountBlocks, nullptr, nullptr, nullptr, end_stage<4>, kTierDerived},    {kCountHaplotypes, nullptr, nullptr, nullptr, end_stage<5>, kTierDerived},
    {kCountPileup, nullptr, nullptr, nullptr, end_stage<6>, kTierPileup},     {kCountAbundance, nullptr, nullptr, nullptr, end_stage<7>, kTierAbundance},
};

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "wanted")) {
        for (uint32_t m = 0; m < 1024; ++m) {
            auto b = [&](int i) { return ((m >> i) & 1u) != 0; };
            printf("%u %u\n", m, counts_wanted(RunSwitches{b(0), b(1), b(2), b(3), b(4), b(5), b(6), b(7), b(8), b(9)}));
        }
        return 0;
    }
    if (argc < 4 || strcmp(argv[1], "end") || argc % 2) { fprintf(stderr, "usage: run_stages end <what> <ok> [<name> <code>]... | run_stages wanted\n"); return 2; }
    bgr_graph g;
    for (int i = 4; i < argc; i += 2) {
        int at = -1;
        for (int j = 0; j < 8; ++j) if (!strcmp(argv[i], kNames[j])) at = j;
        if (at < 0) { fprintf(stderr, "no stage %s\n", argv[i]); return 2; }
        g.fail[at] = atoi(argv[i + 1]);
    }
    const int rc = end_stages(kStages, 8, &g, (uint32_t)strtoul(argv[2], nullptr, 0), atoi(argv[3]) != 0);
    for (const std::string& l : g.log) puts(l.c_str());
    printf("rc %d\n", rc);
    return 0;
}

// Harness of tests/test_inside_sanitizers.py: the host builder and lookup of the inside index (inside_index.cpp) over the cases of a text file,
// compiled with -fsanitize=address,undefined.  A case: "case <name> <k> <n unitigs> <n entries> <n absent>", the unitigs one per line, the
// definition's entries "<canonical> <id> <j> <forward window is canonical>" one per line (inside_ref.py wrote them), then k-mer words the graph
// does not hold.  Built with 1, 3 and 8 threads, each table must hold exactly the definition's entries: every one found on both strands with its
// value, as many entries as the definition has, every k-mer of every unitig that is no entry not found, the absent words not found.  A case with
// n entries = -1 must be refused (k > 32, a character outside ACGT) and leave nothing allocated.
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "graph_build.h"
#include "inside_index.h"

using namespace bgr;

static uint64_t word_of(const std::string& s) {
    uint64_t x = 0;
    for (char c : s) x = (x << 2) | (c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u);
    return x;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: sanitize_inside CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string tag, name;
    int fails = 0, cases = 0;
    uint32_t k;
    long n_u, n_e, n_a;
    while (in >> tag >> name >> k >> n_u >> n_e >> n_a) {
        if (tag != "case") { printf("FAIL: not a case line\n"); return 1; }
        std::vector<std::string> us(n_u);
        for (auto& u : us) in >> u;
        std::map<uint64_t, uint64_t> want;
        for (long i = 0; i < n_e; ++i) {
            uint64_t c, id, j, fc;
            in >> c >> id >> j >> fc;
            want[c] = bgr_inside_val((uint32_t)id, (uint32_t)j, fc != 0);
        }
        std::vector<uint64_t> absent(n_a);
        for (auto& x : absent) in >> x;
        std::vector<char> seqs;
        std::vector<uint64_t> offs(1, 0);
        for (const auto& u : us) { seqs.insert(seqs.end(), u.begin(), u.end()); offs.push_back(seqs.size()); }
        for (unsigned T : {1u, 3u, 8u}) {
            set_build_threads(T);
            HostGraph g;
            std::string err;
            if (!build_graph(k, us.size(), seqs.data(), offs.data(), 0.0, 0, g, err)) { printf("FAIL %s: graph: %s\n", name.c_str(), err.c_str()); return 1; }
            InsideIndex ix;
            const int rc = build_inside_index(g.header(), g.base(), T, ix, err);
            if (n_e < 0) {
                if (rc != 1 || ix.tab || ix.slots || err.empty()) { printf("FAIL %s: not refused (rc %d)\n", name.c_str(), rc); ++fails; }
                continue;
            }
            if (rc != 0) { printf("FAIL %s: build: %s\n", name.c_str(), err.c_str()); return 1; }
            if (ix.entries != want.size() || ix.slots < 2 * ix.entries || ix.bytes() != 16 * ix.slots) { printf("FAIL %s T=%u: %llu entries in %llu slots, the definition has %zu\n", name.c_str(), T, (unsigned long long)ix.entries, (unsigned long long)ix.slots, want.size()); ++fails; }
            uint64_t used = 0;
            for (uint64_t s = 0; s < ix.slots; ++s) used += ix.tab[s].key != BGR_EMPTY_KEY;
            if (used != ix.entries) { printf("FAIL %s T=%u: %llu slots in use\n", name.c_str(), T, (unsigned long long)used); ++fails; }
            for (const auto& kv : want) {
                uint64_t v = 0, v2 = 0;
                if (!inside_lookup(ix, k, kv.first, &v) || v != kv.second || !inside_lookup(ix, k, bgr_rcb(kv.first, k), &v2) || v2 != kv.second) { printf("FAIL %s T=%u: entry %llu\n", name.c_str(), T, (unsigned long long)kv.first); ++fails; }
            }
            for (const auto& u : us)
                for (size_t j = 0; j + k <= u.size(); ++j) {
                    const uint64_t x = word_of(u.substr(j, k)), r = bgr_rcb(x, k), c = x < r ? x : r;
                    uint64_t v = 0;
                    if (inside_lookup(ix, k, x, &v) != (want.count(c) != 0)) { printf("FAIL %s T=%u: k-mer at %zu\n", name.c_str(), T, j); ++fails; }
                }
            for (uint64_t x : absent) {
                uint64_t v = 0;
                if (inside_lookup(ix, k, x, &v)) { printf("FAIL %s T=%u: absent word %llu found\n", name.c_str(), T, (unsigned long long)x); ++fails; }
            }
        }
        ++cases;
    }
    if (fails || !cases) { printf("FAIL: %d failures in %d cases\n", fails, cases); return 1; }
    printf("%d cases\ninside ok\n", cases);
    return 0;
}

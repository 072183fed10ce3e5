// sanitize_gaf_cs.cpp -- stand-alone driver of the host formatter's GAF lines with the cs:Z: field (bgreat_amd/csrc/record_format.h: gaf_line,
// append_cs_ops, format_range_ext), built with -fsanitize=address,undefined by tests/test_gaf_cs_sanitizers.py.  No device, no library: the
// headers alone.  Every read, header, unitig and row is a heap block of exactly its size, so a formatter that reads beyond one is caught.
//   sanitize_gaf_cs CASES  ->  prints, per case of the file, "== <name> <variant> ok=<0|1>" and the lines format_range_ext wrote (variants: plain,
//                              cs, tagged, tagged+cs), then "gaf cs ok"; the Python side compares them with gaf_ref.py + gaf_cs_ref.py
// CASES, line by line: "case <name> <k> <n_unitigs> <n_reads>", the unitigs, the tag table (n_unitigs + 1 numbers), then per read its header,
// its characters ("-" for none) and "<status> <n_ints> <ints ...>".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "record_format.h"

static std::unique_ptr<char[]> exact(const std::string& s) {
    std::unique_ptr<char[]> p(new char[s.size() ? s.size() : 1]);
    memcpy(p.get(), s.data(), s.size());
    return p;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: sanitize_gaf_cs CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    size_t n_cases = 0;
    while (std::getline(in, line)) {
        std::istringstream head(line);
        std::string word, name;
        uint32_t k = 0;
        uint64_t n_unitigs = 0, n_reads = 0;
        if (!(head >> word >> name >> k >> n_unitigs >> n_reads) || word != "case") { printf("FAIL: bad case line '%s'\n", line.c_str()); return 1; }
        std::string all;
        std::vector<uint64_t> uoffs(1, 0);
        for (uint64_t i = 0; i < n_unitigs; ++i) { std::getline(in, line); all += line; uoffs.push_back(all.size()); }
        const std::unique_ptr<char[]> seqs = exact(all);
        const std::unique_ptr<uint64_t[]> offs(new uint64_t[n_unitigs + 1]);
        for (uint64_t i = 0; i <= n_unitigs; ++i) offs[i] = uoffs[i];
        Unitigs u;
        u.seqs = seqs.get(); u.offs = offs.get(); u.n = n_unitigs; u.k = k;
        std::getline(in, line);
        const std::unique_ptr<uint32_t[]> table(new uint32_t[n_unitigs + 1]);
        { std::istringstream t(line); for (uint64_t i = 0; i <= n_unitigs; ++i) t >> table[i]; }
        std::vector<std::unique_ptr<char[]>> keep;
        std::vector<RecSlice> recs;
        std::vector<int32_t> ints;
        std::vector<uint64_t> poffs(1, 0);
        std::vector<uint8_t> status;
        for (uint64_t r = 0; r < n_reads; ++r) {
            std::string h, s;
            std::getline(in, h);
            std::getline(in, s);
            if (s == "-") s.clear();
            std::getline(in, line);
            std::istringstream row(line);
            uint32_t st = 0;
            uint64_t np = 0;
            row >> st >> np;
            for (uint64_t i = 0; i < np; ++i) { int64_t v; row >> v; ints.push_back((int32_t)v); }
            poffs.push_back(ints.size());
            status.push_back((uint8_t)st);
            keep.push_back(exact(h));
            const char* hp = keep.back().get();
            keep.push_back(exact(s));
            recs.push_back(RecSlice{hp, keep.back().get(), (uint32_t)h.size(), (uint32_t)s.size()});
        }
        const std::unique_ptr<int32_t[]> paths(new int32_t[ints.size() ? ints.size() : 1]);
        for (size_t i = 0; i < ints.size(); ++i) paths[i] = ints[i];
        const std::unique_ptr<uint64_t[]> po(new uint64_t[poffs.size()]);
        for (size_t i = 0; i < poffs.size(); ++i) po[i] = poffs[i];
        const std::unique_ptr<uint8_t[]> stp(new uint8_t[status.size() ? status.size() : 1]);
        for (size_t i = 0; i < status.size(); ++i) stp[i] = status[i];
        const struct { const char* what; bool tagged, cs; } variants[] = {{"plain", false, false}, {"cs", false, true}, {"tagged", true, false}, {"tagged+cs", true, true}};
        for (const auto& v : variants) {
            std::string pbuf, nbuf, obuf, bug;
            const bool ok = format_range_ext(recs.data(), paths.get(), po.get(), stp.get(), 0, n_reads, &u, true, false, pbuf, nbuf, obuf, bug, v.tagged ? table.get() : nullptr,
                                             v.tagged ? n_unitigs + 1 : 0, v.cs);
            printf("== %s %s ok=%d\n", name.c_str(), v.what, ok ? 1 : 0);
            fwrite(pbuf.data(), 1, pbuf.size(), stdout);
        }
        ++n_cases;
    }
    if (!n_cases) { printf("FAIL: no case\n"); return 1; }
    printf("gaf cs ok\n");
    return 0;
}

// sanitize_variants.cpp -- stand-alone driver of the host code of SNV calling (bgreat_amd/csrc/variants_host.h: the --min-af parser, the test an
// allele passes, the VCF writer), built with -fsanitize=address,undefined by tests/test_variants_sanitizers.py.  No device, no library: the header alone.
//   sanitize_variants OUT.vcf  ->  writes the VCF of a hand-made table of sites and prints "variants ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "variants_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the text in a heap block of exactly its size: a parser that reads past the terminator is caught
static bool parse(const char* text, uint32_t* ppm) {
    const size_t n = strlen(text) + 1;
    std::unique_ptr<char[]> p(new char[n]);
    memcpy(p.get(), text, n);
    return bgr::parse_af_ppm(p.get(), ppm);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: sanitize_variants OUT.vcf\n"); return 2; }
    uint32_t ppm = 77;
    const struct { const char* text; uint32_t ppm; } good[] = {{"0", 0}, {"1", 1000000}, {"0.2", 200000}, {"0.000001", 1}, {"1.000000", 1000000}, {"00.5", 500000}, {"0.999999", 999999}};
    for (const auto& g : good) { CHECK(parse(g.text, &ppm)); CHECK(ppm == g.ppm); }
    const char* bad[] = {"", ".", ".5", "0.", "1.1", "2", "1.000001", "0.0000001", "0.2x", " 0.2", "-0.2", "1e-3", "99999999999999999999", "0.99999999999999999999", "nan"};
    for (const char* b : bad) { ppm = 77; CHECK(!parse(b, &ppm)); CHECK(ppm == 77); }
    CHECK(!bgr::parse_af_ppm(nullptr, &ppm));

    // the 64-bit comparison at its edges
    const uint32_t w[4] = {0xFFFFFFFFu, 3000000u, 0, 1};
    CHECK(bgr::variants_passing(0xFFFFFFFFu, w, 2, 1, 1, 1000000) == 1u);          // A: every read
    CHECK(bgr::variants_passing(4000000000u, w, 2, 1, 1, 750) == 3u);              // C at the exact tie
    CHECK(bgr::variants_passing(4000000000u, w, 2, 1, 1, 751) == 1u);
    CHECK(bgr::variants_passing(4000000000u, w, 0, 1, 1, 0) == 10u);               // the unitig's own letter is no allele
    CHECK(bgr::variants_passing(5, w, 2, 6, 1, 0) == 0u);

    // two unitigs in the 2-bit store (forward strand at F, first base in the most significant bits): "ACGTACGTAC" at 0, "GGGTTT" at 40
    const std::string u1 = "ACGTACGTAC", u2 = "GGGTTT";
    std::vector<uint64_t> seq(3, 0);
    auto put = [&](uint64_t F, const std::string& s) { for (size_t i = 0; i < s.size(); ++i) { const uint64_t p = F + i; seq[p >> 5] |= (uint64_t)(strchr("ACGT", s[i]) - "ACGT") << (62 - 2 * (p & 31)); } };
    put(0, u1); put(40, u2);
    std::vector<BgrUnitigMeta> meta(3);
    memset(meta.data(), 0, meta.size() * sizeof(BgrUnitigMeta));
    meta[1].len = 10; meta[1].F = 0; meta[2].len = 6; meta[2].F = 40;
    const bgr_variant_params prm = {1, 1, 0};
    const std::vector<bgr_variant_site> sites = {{1, 0, 10, 0, 2, 0, 0, 0}, {1, 3, 20, 4, 5, 4, 0, 2}, {1, 9, 4000000000u, 3000000000u, 0, 0, 0, 7}, {2, 1, 9, 3, 3, 0, 3, 0}, {2, 5, 2, 0, 2, 0, 0, 0}};
    std::string err;
    FILE* f = fopen(argv[1], "wb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    CHECK(bgr::vcf_write(f, meta.data(), seq.data(), 2, prm, sites.data(), sites.size(), &err));
    fclose(f);
    std::string got;
    f = fopen(argv[1], "rb");
    char buf[4096];
    for (size_t n; f && (n = fread(buf, 1, sizeof buf, f)) > 0;) got.append(buf, n);
    if (f) fclose(f);
    CHECK(got.find("##contig=<ID=1,length=10>\n##contig=<ID=2,length=6>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n") != std::string::npos);
    CHECK(got.find("\n1\t1\t.\tA\tC\t.\tPASS\tDP=10;AD=8,2;NN=0\n") != std::string::npos);
    CHECK(got.find("\n1\t4\t.\tT\tC,A,G\t.\tPASS\tDP=20;AD=5,5,4,4;NN=2\n") != std::string::npos);
    CHECK(got.find("\n1\t10\t.\tC\tA\t.\tPASS\tDP=4000000000;AD=999999993,3000000000;NN=7\n") != std::string::npos);
    CHECK(got.find("\n2\t2\t.\tG\tA,C,T\t.\tPASS\tDP=9;AD=0,3,3,3;NN=0\n") != std::string::npos);
    CHECK(got.size() > 0 && got.back() == '\n' && got.find("\n2\t6\t.\tT\tC\t.\tPASS\tDP=2;AD=0,2;NN=0\n") == got.size() - strlen("\n2\t6\t.\tT\tC\t.\tPASS\tDP=2;AD=0,2;NN=0\n"));
    // what is no site is refused before anything is written (f null: the checks alone)
    std::vector<bgr_variant_site> bad_sites = sites;
    std::swap(bad_sites[0], bad_sites[1]);
    CHECK(!bgr::vcf_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), bad_sites.size(), &err) && err.find("order") != std::string::npos);
    bad_sites = {{3, 0, 5, 1, 0, 0, 0, 0}};
    CHECK(!bgr::vcf_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), 1, &err) && err.find("outside") != std::string::npos);
    bad_sites = {{2, 6, 5, 1, 0, 0, 0, 0}};
    CHECK(!bgr::vcf_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), 1, &err) && err.find("outside") != std::string::npos);
    bad_sites = {{1, 0, 5, 9, 0, 0, 0, 5}};   // only the unitig's own letter and Ns
    CHECK(!bgr::vcf_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), 1, &err) && err.find("no passing allele") != std::string::npos);
    const bgr_variant_params bad_prm = {0, 1, 0};
    CHECK(!bgr::vcf_write(nullptr, meta.data(), seq.data(), 2, bad_prm, sites.data(), sites.size(), &err));
    CHECK(bgr::vcf_write(nullptr, meta.data(), seq.data(), 2, prm, nullptr, 0, &err));
    if (failures) return 1;
    printf("variants ok\n");
    return 0;
}

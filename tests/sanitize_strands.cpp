// sanitize_strands.cpp -- stand-alone driver of the host code of the per-strand SNV calling (bgreat_amd/csrc/variants_host.h: the --min-alt-strand
// parser, the strand filter, the VCF writer with ADF / ADR), built with -fsanitize=address,undefined by tests/test_strands_sanitizers.py.  No device,
// no library: the header alone.
//   sanitize_strands OUT.vcf  ->  writes the VCF of a hand-made table of sites and prints "strands ok"
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
static bool parse(const char* text, uint32_t* out) {
    const size_t n = strlen(text) + 1;
    std::unique_ptr<char[]> p(new char[n]);
    memcpy(p.get(), text, n);
    return bgr::parse_min_alt_strand(p.get(), out);
}

static std::string slurp(const char* path) {
    std::string got;
    FILE* f = fopen(path, "rb");
    char buf[4096];
    for (size_t n; f && (n = fread(buf, 1, sizeof buf, f)) > 0;) got.append(buf, n);
    if (f) fclose(f);
    return got;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: sanitize_strands OUT.vcf\n"); return 2; }
    uint32_t v = 77;
    const struct { const char* text; uint32_t v; } good[] = {{"0", 0}, {"1", 1}, {"007", 7}, {"999999999", 999999999u}, {"000000000", 0}};
    for (const auto& g : good) { CHECK(parse(g.text, &v)); CHECK(v == g.v); }
    const char* bad[] = {"", "-1", "+1", "1.0", "1x", " 1", "1 ", "0x1", "1000000000", "99999999999999999999", "1e3"};
    for (const char* b : bad) { v = 77; CHECK(!parse(b, &v)); CHECK(v == 77); }
    CHECK(!bgr::parse_min_alt_strand(nullptr, &v));

    // the strand filter at its edges: the candidates 0b1011 with totals w and forward counts f
    const uint32_t w[4] = {0xFFFFFFFFu, 4, 9, 2}, f[4] = {0xFFFFFFFEu, 2, 9, 0};
    CHECK(bgr::variants_strand_passing(11u, w, f, 0) == 11u);    // 0 keeps every candidate
    CHECK(bgr::variants_strand_passing(11u, w, f, 1) == 3u);     // T is never read forward
    CHECK(bgr::variants_strand_passing(11u, w, f, 2) == 2u);     // A is read once on the other strand
    CHECK(bgr::variants_strand_passing(15u, w, f, 1) == 3u);     // G is never read on the other strand
    CHECK(bgr::variants_strand_passing(11u, w, f, 3) == 0u);
    CHECK(bgr::variants_strand_passing(0u, w, f, 0) == 0u);

    // two unitigs in the 2-bit store (forward strand at F, first base in the most significant bits): "ACGTACGTAC" at 0, "GGGTTT" at 40
    const std::string u1 = "ACGTACGTAC", u2 = "GGGTTT";
    std::vector<uint64_t> seq(3, 0);
    auto put = [&](uint64_t F, const std::string& s) { for (size_t i = 0; i < s.size(); ++i) { const uint64_t p = F + i; seq[p >> 5] |= (uint64_t)(strchr("ACGT", s[i]) - "ACGT") << (62 - 2 * (p & 31)); } };
    put(0, u1); put(40, u2);
    std::vector<BgrUnitigMeta> meta(3);
    memset(meta.data(), 0, meta.size() * sizeof(BgrUnitigMeta));
    meta[1].len = 10; meta[1].F = 0; meta[2].len = 6; meta[2].F = 40;
    bgr_variant_strand_params prm = {1, 1, 0, 0};
    //                                             unitig pos depth        a  c  g  t  n  fdepth      fa fc fg ft fn
    const std::vector<bgr_variant_strand_site> sites = {{1, 0, 10,          0, 2, 0, 0, 0, 4,          0, 1, 0, 0, 0, {0, 0}},
                                                        {1, 3, 20,          4, 5, 4, 0, 2, 9,          4, 2, 0, 0, 1, {0, 0}},
                                                        {1, 9, 4000000000u, 3000000000u, 0, 0, 0, 7, 3999999999u, 2999999999u, 0, 0, 0, 7, {0, 0}},
                                                        {2, 1, 9,           3, 3, 0, 3, 0, 4,          3, 0, 0, 1, 0, {0, 0}},
                                                        {2, 5, 2,           0, 2, 0, 0, 0, 0,          0, 0, 0, 0, 0, {0, 0}}};
    std::string err;
    FILE* fo = fopen(argv[1], "wb");
    if (!fo) { printf("cannot open %s\n", argv[1]); return 2; }
    CHECK(bgr::vcf_strands_write(fo, meta.data(), seq.data(), 2, prm, sites.data(), sites.size(), &err));
    fclose(fo);
    std::string got = slurp(argv[1]);
    CHECK(got.find("##bgreat_thresholds=<min_depth=1,min_alt=1,min_af_ppm=0,min_alt_strand=0>\n") != std::string::npos);
    CHECK(got.find("##INFO=<ID=AD,") < got.find("##INFO=<ID=ADF,") && got.find("##INFO=<ID=ADF,") < got.find("##INFO=<ID=ADR,") && got.find("##INFO=<ID=ADR,") < got.find("##INFO=<ID=NN,"));
    CHECK(got.find("##contig=<ID=1,length=10>\n##contig=<ID=2,length=6>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n") != std::string::npos);
    CHECK(got.find("\n1\t1\t.\tA\tC\t.\tPASS\tDP=10;AD=8,2;ADF=3,1;ADR=5,1;NN=0\n") != std::string::npos);
    CHECK(got.find("\n1\t4\t.\tT\tC,A,G\t.\tPASS\tDP=20;AD=5,5,4,4;ADF=2,2,4,0;ADR=3,3,0,4;NN=2\n") != std::string::npos);   // several ALTs, fn > 0
    CHECK(got.find("\n1\t10\t.\tC\tA\t.\tPASS\tDP=4000000000;AD=999999993,3000000000;ADF=999999993,2999999999;ADR=0,1;NN=7\n") != std::string::npos);
    CHECK(got.find("\n2\t2\t.\tG\tA,C,T\t.\tPASS\tDP=9;AD=0,3,3,3;ADF=0,3,0,1;ADR=0,0,3,2;NN=0\n") != std::string::npos);
    const std::string tail = "\n2\t6\t.\tT\tC\t.\tPASS\tDP=2;AD=0,2;ADF=0,0;ADR=0,2;NN=0\n";
    CHECK(got.size() > tail.size() && got.compare(got.size() - tail.size(), tail.size(), tail) == 0);
    // min_alt_strand 1: the one-strand alleles leave the lines; a record whose alleles all leave is no site
    prm.min_alt_strand = 1;
    CHECK(!bgr::vcf_strands_write(nullptr, meta.data(), seq.data(), 2, prm, sites.data(), sites.size(), &err) && err.find("no passing allele") != std::string::npos);
    const std::vector<bgr_variant_strand_site> fewer(sites.begin(), sites.begin() + 4);
    fo = fopen(argv[1], "wb");
    CHECK(fo && bgr::vcf_strands_write(fo, meta.data(), seq.data(), 2, prm, fewer.data(), fewer.size(), &err));
    if (fo) fclose(fo);
    got = slurp(argv[1]);
    CHECK(got.find("min_alt_strand=1>\n") != std::string::npos);
    CHECK(got.find("\n1\t4\t.\tT\tC\t.\tPASS\tDP=20;AD=5,5;ADF=2,2;ADR=3,3;NN=2\n") != std::string::npos);
    CHECK(got.find("\n2\t2\t.\tG\tT\t.\tPASS\tDP=9;AD=0,3;ADF=0,1;ADR=0,2;NN=0\n") != std::string::npos);
    prm.min_alt_strand = 0;
    // what is no site is refused before anything is written (f null: the checks alone)
    std::vector<bgr_variant_strand_site> bad_sites = sites;
    std::swap(bad_sites[0], bad_sites[1]);
    CHECK(!bgr::vcf_strands_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), bad_sites.size(), &err) && err.find("order") != std::string::npos);
    bad_sites = {{3, 0, 5, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0}}};
    CHECK(!bgr::vcf_strands_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), 1, &err) && err.find("outside") != std::string::npos);
    bad_sites = {{1, 0, 5, 0, 1, 0, 0, 0, 6, 0, 0, 0, 0, 0, {0, 0}}};   // more forward reads than reads
    CHECK(!bgr::vcf_strands_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), 1, &err) && err.find("do not fit") != std::string::npos);
    bad_sites = {{1, 0, 5, 0, 1, 0, 0, 0, 5, 0, 2, 0, 0, 0, {0, 0}}};   // an allele read forward more often than read
    CHECK(!bgr::vcf_strands_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), 1, &err) && err.find("do not fit") != std::string::npos);
    bad_sites = {{1, 0, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0, {0, 0}}};   // counts that sum beyond 32 bits
    CHECK(!bgr::vcf_strands_write(nullptr, meta.data(), seq.data(), 2, prm, bad_sites.data(), 1, &err) && err.find("do not fit") != std::string::npos);
    const bgr_variant_strand_params bad_prm = {0, 1, 0, 0};
    CHECK(!bgr::vcf_strands_write(nullptr, meta.data(), seq.data(), 2, bad_prm, sites.data(), sites.size(), &err));
    CHECK(bgr::vcf_strands_write(nullptr, meta.data(), seq.data(), 2, prm, nullptr, 0, &err));
    if (failures) return 1;
    printf("strands ok\n");
    return 0;
}

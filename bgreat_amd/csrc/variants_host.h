// variants_host.h -- the part of SNV calling that is plain C++ (bgr_variant_site in include/bgreat_gpu.h has the definition): the test an allele
// passes, shared by the kernel and the writer, the --min-af parser and the VCF writer.  No HIP in here: the host sanitizer program compiles it alone.
#ifndef BGREAT_AMD_VARIANTS_HOST_H
#define BGREAT_AMD_VARIANTS_HOST_H

#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/bgreat_gpu.h"
#include "graph_layout.h"

namespace bgr {

// bit X (A C G T = 0 .. 3) set: allele X passes at a base with this depth, the four alt words `w` and the unitig's own code `ref` (whose word counts
// the Ns and is no allele).  64-bit integers only: c * 1 000 000 < 2^52.
BGR_HD uint32_t variants_passing(uint32_t depth, const uint32_t w[4], uint32_t ref, uint32_t min_depth, uint32_t min_alt, uint32_t min_af_ppm) {
    if (depth < min_depth) return 0;
    uint32_t m = 0;
    for (uint32_t x = 0; x < 4; ++x)
        if (x != ref && w[x] >= min_alt && (uint64_t)w[x] * 1000000ull >= (uint64_t)min_af_ppm * depth) m |= 1u << x;
    return m;
}
inline bool variants_params_ok(const bgr_variant_params& p) { return p.min_depth >= 1 && p.min_alt >= 1 && p.min_af_ppm <= 1000000u; }


// "0", "1", "0.2", "0.000001": digits, an optional point with one to six digits behind it, a value of at most 1 -> parts per million, exactly
inline bool parse_af_ppm(const char* s, uint32_t* ppm) {
    if (!s || !ppm || *s < '0' || *s > '9') return false;
    uint64_t whole = 0, frac = 0;
    uint32_t nd = 0;
    for (; *s >= '0' && *s <= '9'; ++s) { whole = whole * 10 + (uint64_t)(*s - '0'); if (whole > 1) return false; }
    if (*s == '.') {
        ++s;
        for (; *s >= '0' && *s <= '9'; ++s) { if (++nd > 6) return false; frac = frac * 10 + (uint64_t)(*s - '0'); }
        if (nd == 0) return false;
        for (uint32_t i = nd; i < 6; ++i) frac *= 10;
    }
    if (*s != 0) return false;
    const uint64_t v = whole * 1000000ull + frac;
    if (v > 1000000ull) return false;
    *ppm = (uint32_t)v;
    return true;
}

// the VCF of `sites` (in (unitig, pos) order) into f; meta / seq: the graph's sections on the host.  false with *err set: a site that is none, or a
// failed write.  f null: the checks alone.
inline bool vcf_write(FILE* f, const BgrUnitigMeta* meta, const uint64_t* seq, uint64_t n_unitigs, const bgr_variant_params& prm, const bgr_variant_site* sites,
                      uint64_t n, std::string* err) {
    auto ref_of = [&](const bgr_variant_site& s) -> uint32_t { const uint64_t p = meta[s.unitig].F + s.pos; return (uint32_t)(seq[p >> 5] >> (62 - 2 * (p & 31))) & 3u; };
    if (!variants_params_ok(prm)) { *err = "thresholds out of range (min_depth >= 1, min_alt >= 1, min_af_ppm <= 1000000)"; return false; }
    for (uint64_t i = 0; i < n; ++i) {
        const bgr_variant_site& s = sites[i];
        if (s.unitig == 0 || s.unitig > n_unitigs || s.pos >= meta[s.unitig].len) { *err = "site " + std::to_string(i) + " lies outside the graph"; return false; }
        if (i && (sites[i - 1].unitig > s.unitig || (sites[i - 1].unitig == s.unitig && sites[i - 1].pos >= s.pos))) { *err = "site " + std::to_string(i) + " is out of (unitig, pos) order"; return false; }
        const uint32_t w[4] = {s.a, s.c, s.g, s.t};
        if (!variants_passing(s.depth, w, ref_of(s), prm.min_depth, prm.min_alt, prm.min_af_ppm)) { *err = "site " + std::to_string(i) + " has no passing allele under these thresholds"; return false; }
    }
    if (!f) return true;   // (the checks alone)
    std::string buf = "##fileformat=VCFv4.2\n##source=bgreat-mi355x\n";
    buf += "##bgreat_thresholds=<min_depth=" + std::to_string(prm.min_depth) + ",min_alt=" + std::to_string(prm.min_alt) + ",min_af_ppm=" + std::to_string(prm.min_af_ppm) + ">\n";
    buf += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads covering the base\">\n";
    buf += "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Reads per allele: those that agree with the unitig, then each ALT\">\n";
    buf += "##INFO=<ID=NN,Number=1,Type=Integer,Description=\"Reads with a character outside ACGT at the base\">\n";
    bool ok = true;
    auto flush = [&](bool all) { if (ok && !buf.empty() && (all || buf.size() > (1u << 20))) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); } };
    for (uint64_t i = 0; i < n; ++i)
        if (i == 0 || sites[i - 1].unitig != sites[i].unitig) {
            buf += "##contig=<ID=" + std::to_string(sites[i].unitig) + ",length=" + std::to_string(meta[sites[i].unitig].len) + ">\n";
            flush(false);
        }
    buf += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    for (uint64_t i = 0; i < n && ok; ++i) {
        const bgr_variant_site& s = sites[i];
        const uint32_t ref = ref_of(s), w[4] = {s.a, s.c, s.g, s.t};
        uint32_t m = variants_passing(s.depth, w, ref, prm.min_depth, prm.min_alt, prm.min_af_ppm), order[4], na = 0;
        while (m) {   // by count descending, ties A < C < G < T
            uint32_t best = 4;
            for (uint32_t x = 0; x < 4; ++x) if (((m >> x) & 1u) && (best == 4 || w[x] > w[best])) best = x;
            order[na++] = best;
            m &= ~(1u << best);
        }
        buf += std::to_string(s.unitig); buf += '\t'; buf += std::to_string((uint64_t)s.pos + 1); buf += "\t.\t"; buf += "ACGT"[ref]; buf += '\t';
        for (uint32_t x = 0; x < na; ++x) { if (x) buf += ','; buf += "ACGT"[order[x]]; }
        buf += "\t.\tPASS\tDP="; buf += std::to_string(s.depth);
        buf += ";AD="; buf += std::to_string((uint32_t)(s.depth - (s.a + s.c + s.g + s.t + s.n)));
        for (uint32_t x = 0; x < na; ++x) { buf += ','; buf += std::to_string(w[order[x]]); }
        buf += ";NN="; buf += std::to_string(s.n); buf += '\n';
        flush(false);
    }
    flush(true);
    if (!ok) *err = "write failed";
    return ok;
}

}  // namespace bgr

#endif

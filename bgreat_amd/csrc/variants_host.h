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
// the strand filter on top: of the alleles in `m` those seen at least min_alt_strand times on each strand -- f[x] of the w[x] observations forward,
// the others reverse.  min_alt_strand = 0 keeps m.
BGR_HD uint32_t variants_strand_passing(uint32_t m, const uint32_t w[4], const uint32_t f[4], uint32_t min_alt_strand) {
    uint32_t out = 0;
    for (uint32_t x = 0; x < 4; ++x)
        if (((m >> x) & 1u) && (min_alt_strand == 0 || (f[x] >= min_alt_strand && f[x] <= w[x] && w[x] - f[x] >= min_alt_strand))) out |= 1u << x;
    return out;
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

// --min-alt-strand: a non-negative integer, digits only, at most nine of them
inline bool parse_min_alt_strand(const char* s, uint32_t* out) {
    if (!s || !out || !*s) return false;
    uint32_t v = 0, nd = 0;
    for (; *s >= '0' && *s <= '9'; ++s) { if (++nd > 9) return false; v = v * 10 + (uint32_t)(*s - '0'); }
    if (*s != 0) return false;
    *out = v;
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

// the same for records with the forward numbers (bgr_variant_strand_site) under the strand filter: the thresholds line ends in min_alt_strand, the
// INFO lines of ADF and ADR follow AD's, and a site's INFO is DP, AD, ADF (forward: those that agree with the unitig, then each ALT), ADR = AD - ADF, NN.
// A record whose forward numbers exceed its totals is refused as well.
inline bool vcf_strands_write(FILE* f, const BgrUnitigMeta* meta, const uint64_t* seq, uint64_t n_unitigs, const bgr_variant_strand_params& prm,
                              const bgr_variant_strand_site* sites, uint64_t n, std::string* err) {
    auto ref_of = [&](const bgr_variant_strand_site& s) -> uint32_t { const uint64_t p = meta[s.unitig].F + s.pos; return (uint32_t)(seq[p >> 5] >> (62 - 2 * (p & 31))) & 3u; };
    auto passing = [&](const bgr_variant_strand_site& s, uint32_t ref) -> uint32_t {
        const uint32_t w[4] = {s.a, s.c, s.g, s.t}, fw[4] = {s.fa, s.fc, s.fg, s.ft};
        return variants_strand_passing(variants_passing(s.depth, w, ref, prm.min_depth, prm.min_alt, prm.min_af_ppm), w, fw, prm.min_alt_strand);
    };
    if (!variants_params_ok(bgr_variant_params{prm.min_depth, prm.min_alt, prm.min_af_ppm})) { *err = "thresholds out of range (min_depth >= 1, min_alt >= 1, min_af_ppm <= 1000000)"; return false; }
    for (uint64_t i = 0; i < n; ++i) {
        const bgr_variant_strand_site& s = sites[i];
        if (s.unitig == 0 || s.unitig > n_unitigs || s.pos >= meta[s.unitig].len) { *err = "site " + std::to_string(i) + " lies outside the graph"; return false; }
        if (i && (sites[i - 1].unitig > s.unitig || (sites[i - 1].unitig == s.unitig && sites[i - 1].pos >= s.pos))) { *err = "site " + std::to_string(i) + " is out of (unitig, pos) order"; return false; }
        const uint64_t alts = (uint64_t)s.a + s.c + s.g + s.t + s.n, falts = (uint64_t)s.fa + s.fc + s.fg + s.ft + s.fn;
        if (s.fdepth > s.depth || s.fa > s.a || s.fc > s.c || s.fg > s.g || s.ft > s.t || s.fn > s.n || alts > s.depth || falts > s.fdepth || alts - falts > (uint64_t)(s.depth - s.fdepth)) {
            *err = "site " + std::to_string(i) + " has forward numbers that do not fit its totals"; return false;
        }
        if (!passing(s, ref_of(s))) { *err = "site " + std::to_string(i) + " has no passing allele under these thresholds"; return false; }
    }
    if (!f) return true;   // (the checks alone)
    std::string buf = "##fileformat=VCFv4.2\n##source=bgreat-mi355x\n";
    buf += "##bgreat_thresholds=<min_depth=" + std::to_string(prm.min_depth) + ",min_alt=" + std::to_string(prm.min_alt) + ",min_af_ppm=" + std::to_string(prm.min_af_ppm) +
           ",min_alt_strand=" + std::to_string(prm.min_alt_strand) + ">\n";
    buf += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads covering the base\">\n";
    buf += "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Reads per allele: those that agree with the unitig, then each ALT\">\n";
    buf += "##INFO=<ID=ADF,Number=R,Type=Integer,Description=\"Reads per allele that run along the unitig's strand as given\">\n";
    buf += "##INFO=<ID=ADR,Number=R,Type=Integer,Description=\"Reads per allele that run along the unitig's other strand as given\">\n";
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
        const bgr_variant_strand_site& s = sites[i];
        const uint32_t ref = ref_of(s), w[4] = {s.a, s.c, s.g, s.t}, fw[4] = {s.fa, s.fc, s.fg, s.ft};
        uint32_t m = passing(s, ref), order[4], na = 0;
        while (m) {   // by count descending, ties A < C < G < T
            uint32_t best = 4;
            for (uint32_t x = 0; x < 4; ++x) if (((m >> x) & 1u) && (best == 4 || w[x] > w[best])) best = x;
            order[na++] = best;
            m &= ~(1u << best);
        }
        const uint32_t ad0 = s.depth - (s.a + s.c + s.g + s.t + s.n), adf0 = s.fdepth - (s.fa + s.fc + s.fg + s.ft + s.fn);
        buf += std::to_string(s.unitig); buf += '\t'; buf += std::to_string((uint64_t)s.pos + 1); buf += "\t.\t"; buf += "ACGT"[ref]; buf += '\t';
        for (uint32_t x = 0; x < na; ++x) { if (x) buf += ','; buf += "ACGT"[order[x]]; }
        buf += "\t.\tPASS\tDP="; buf += std::to_string(s.depth);
        buf += ";AD="; buf += std::to_string(ad0);
        for (uint32_t x = 0; x < na; ++x) { buf += ','; buf += std::to_string(w[order[x]]); }
        buf += ";ADF="; buf += std::to_string(adf0);
        for (uint32_t x = 0; x < na; ++x) { buf += ','; buf += std::to_string(fw[order[x]]); }
        buf += ";ADR="; buf += std::to_string(ad0 - adf0);
        for (uint32_t x = 0; x < na; ++x) { buf += ','; buf += std::to_string(w[order[x]] - fw[order[x]]); }
        buf += ";NN="; buf += std::to_string(s.n); buf += '\n';
        flush(false);
    }
    flush(true);
    if (!ok) *err = "write failed";
    return ok;
}

}  // namespace bgr

#endif

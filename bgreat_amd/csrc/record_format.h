// record_format.h -- part of the translation unit pipeline.cpp (included by it alone): the bytes of the output files.  Records as the
// reference writes them, correction mode's spelled reads, GAF lines; works on plain arrays and knows nothing of the pipeline.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bgreat_gpu.h"
#include "fastx.h"
#include "haplotag_host.h"

namespace {

using bgr::RecSlice;

// to_string(v) + '.'  (aligner.cpp:600-609).  Two digits per step from a table, written back to front into their final place
// (the per-digit divide loop this replaces was the largest single cost of the host pipeline: ~50 ns per read).
static const char kDigitPairs[] =
    "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263"
    "646566676869707172737475767778798081828384858687888990919293949596979899";
inline char* put_int(char* o, int32_t v) {
    uint32_t u = (uint32_t)v;
    if (v < 0) { *o++ = '-'; u = 0u - u; }
    const unsigned len = u < 10 ? 1 : u < 100 ? 2 : u < 1000 ? 3 : u < 10000 ? 4 : u < 100000 ? 5 : u < 1000000 ? 6 : u < 10000000 ? 7 :
                         u < 100000000 ? 8 : u < 1000000000 ? 9 : 10;
    char* e = o + len;
    char* w = e;
    while (u >= 100) {
        const uint32_t q = u / 100, r = u - q * 100;
        w -= 2;
        memcpy(w, kDigitPairs + 2 * r, 2);
        u = q;
    }
    if (u >= 10) memcpy(w - 2, kDigitPairs + 2 * u, 2);
    else w[-1] = (char)('0' + u);
    *e++ = '.';
    return e;
}

// ---- correction mode (-c): recoverPath / getUnitig / compactionEnd (aligner.cpp:270-302, utils.cpp:171-179) ------
struct Unitigs {
    const char* seqs = nullptr;
    const uint64_t* offs = nullptr;
    uint64_t n = 0;
    uint32_t k = 0;
};
inline char rc_char(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }  // utils.cpp:52-59
inline void oriented_unitig(const Unitigs& u, int32_t id, std::string& out) {  // getUnitig: forward, or reverse complement for id < 0
    out.clear();
    const uint64_t i = (uint64_t)(id < 0 ? -(int64_t)id : id);
    if (i == 0 || i > u.n) return;  // unitigs[0] is "" (aligner.cpp:408)
    const char* s = u.seqs + u.offs[i - 1];
    const uint64_t len = u.offs[i] - u.offs[i - 1];
    if (id > 0) { out.assign(s, len); return; }
    out.resize(len);
    for (uint64_t j = 0; j < len; ++j) out[j] = rc_char(s[len - 1 - j]);
}
// The read as spelled by its path: unitigs glued on their k-1 overlaps, then substr(offset, read length).
// false = the reference's "bug compaction" exit (no orientation of the next unitig continues the walk).
bool recover_path(const Unitigs& u, const int32_t* path, uint64_t n, uint32_t read_len, std::string& walk, std::string& tmp, std::string& rc) {
    const uint32_t K1 = u.k - 1;
    oriented_unitig(u, path[1], walk);
    for (uint64_t i = 2; i < n; ++i) {
        oriented_unitig(u, path[i], tmp);
        if (walk.empty() || tmp.empty() || walk.size() < K1 || tmp.size() < K1) return false;
        if (walk.compare(walk.size() - K1, K1, tmp, 0, K1) == 0) { walk.append(tmp, K1, std::string::npos); continue; }
        rc.resize(tmp.size());
        for (size_t j = 0; j < tmp.size(); ++j) rc[j] = rc_char(tmp[tmp.size() - 1 - j]);
        if (walk.compare(walk.size() - K1, K1, rc, 0, K1) == 0) { walk.append(rc, K1, std::string::npos); continue; }
        return false;
    }
    const int32_t off = path[0];
    if (off < 0 || (uint64_t)off > walk.size()) return false;  // std::out_of_range in the reference
    walk.erase(0, (size_t)off);
    if (walk.size() > read_len) walk.resize(read_len);
    return true;
}

// ---- GAF output (--gaf, bgr_run_options.gaf): one line per mapped read; the definition is in include/bgreat_gpu.h ------
inline void put_u64(std::string& o, uint64_t v) {
    char b[24];
    char* e = b + sizeof(b);
    char* w = e;
    do { *--w = (char)('0' + v % 10); v /= 10; } while (v);
    o.append(w, (size_t)(e - w));
}
// The value of the cs:Z: field (minimap2's short form, substitutions only: include/bgreat_gpu.h): walk[off ...] under the read's first cl characters,
// or -- on_rc -- its reverse complement under the read's last cl.  ":<n>" per maximal run of equal characters, "*<path><read>" in lower case per
// difference, 'n' for a read character outside ACGT.
inline void append_cs_ops(const std::string& walk, uint64_t off, uint32_t cl, const char* read, uint32_t L, bool on_rc, std::string& out) {
    uint32_t run = 0;
    for (uint32_t j = 0; j < cl; ++j) {
        const char p = on_rc ? rc_char(walk[off + cl - 1 - j]) : walk[off + j], r = on_rc ? read[L - cl + j] : read[j];
        if (p == r) { ++run; continue; }
        if (run) { out.push_back(':'); put_u64(out, run); run = 0; }
        out.push_back('*');
        out.push_back((char)(p | 0x20));
        out.push_back(r == 'A' || r == 'C' || r == 'G' || r == 'T' ? (char)(r | 0x20) : 'n');
    }
    if (run) { out.push_back(':'); put_u64(out, run); }
}
// Appends the line of one mapped read (path of n >= 2 ints) to `out`.  The walk is recover_path's, with the orientation each unitig was glued
// on in kept in `fwd`; false = the path spells no walk (walk / tmp then hold what the reference prints behind "bug compaction").
// tail (or null): what goes between NM:i: and the newline, made from the walk while it is at hand -- the cs:Z: field.
bool gaf_line(const Unitigs& u, const int32_t* path, uint64_t n, const char* h, uint32_t hl, const char* read, uint32_t L, bool on_rc, std::string& out,
              std::string& walk, std::string& tmp, std::string& rc, std::vector<uint8_t>& fwd, std::string* tail = nullptr) {
    const uint32_t K1 = u.k - 1;
    oriented_unitig(u, path[1], walk);
    tmp.clear();
    if (walk.empty()) return false;
    fwd.assign(1, path[1] > 0 ? 1 : 0);
    for (uint64_t i = 2; i < n; ++i) {
        oriented_unitig(u, path[i], tmp);
        if (tmp.empty() || walk.size() < K1 || tmp.size() < K1) return false;
        if (walk.compare(walk.size() - K1, K1, tmp, 0, K1) == 0) { walk.append(tmp, K1, std::string::npos); fwd.push_back(path[i] > 0 ? 1 : 0); continue; }
        rc.resize(tmp.size());
        for (size_t j = 0; j < tmp.size(); ++j) rc[j] = rc_char(tmp[tmp.size() - 1 - j]);
        if (walk.compare(walk.size() - K1, K1, rc, 0, K1) == 0) { walk.append(rc, K1, std::string::npos); fwd.push_back(path[i] > 0 ? 0 : 1); continue; }
        return false;
    }
    if (path[0] < 0 || (uint64_t)path[0] > walk.size()) return false;
    const uint64_t off = (uint64_t)path[0], plen = walk.size();
    const uint32_t cl = (uint32_t)std::min<uint64_t>(L, plen - off);
    uint32_t nm = 0;   // characters of the read that differ from what the path spells under them
    if (!on_rc) { for (uint32_t j = 0; j < cl; ++j) nm += walk[off + j] != read[j]; }
    else for (uint32_t j = 0; j < cl; ++j) nm += rc_char(walk[off + j]) != read[L - 1 - j];
    const uint32_t qs = on_rc ? L - cl : 0u, qe = on_rc ? L : cl;
    const uint64_t pstart = on_rc ? plen - (off + cl) : off;
    size_t nl = 0;   // the name: behind the header's first character up to the first space or tab
    while (1 + nl < hl && h[1 + nl] != ' ' && h[1 + nl] != '\t') ++nl;
    if (nl) out.append(h + 1, nl); else out.push_back('*');
    out.push_back('\t'); put_u64(out, L);
    out.push_back('\t'); put_u64(out, qs);
    out.push_back('\t'); put_u64(out, qe);
    out.append("\t+\t");
    for (uint64_t s = 0; s + 1 < n; ++s) {   // a read mapped on its reverse complement: the path from its end, every orientation flipped
        const uint64_t i = on_rc ? n - 1 - s : 1 + s;
        const int64_t id = path[i] < 0 ? -(int64_t)path[i] : (int64_t)path[i];
        out.push_back((fwd[i - 1] != 0) != on_rc ? '>' : '<');
        put_u64(out, (uint64_t)id);
    }
    out.push_back('\t'); put_u64(out, plen);
    out.push_back('\t'); put_u64(out, pstart);
    out.push_back('\t'); put_u64(out, pstart + cl);
    out.push_back('\t'); put_u64(out, cl - nm);
    out.push_back('\t'); put_u64(out, cl);
    out.append("\t255\tNM:i:"); put_u64(out, nm);
    out.push_back('\n');
    if (tail) { tail->assign("\tcs:Z:"); append_cs_ops(walk, off, cl, read, L, on_rc, *tail); }
    return true;
}

// Records lo..hi of a batch (`recs`; `paths` / `poffs`: what the device found for them) as the reference writes them: mapped -> "header\n" +
// "int." * n + "\n" into pbuf (alignerGreedy.cpp:406-411), the others -> "header\nread\n" into nbuf (alignerGreedy.cpp:421-427).
void format_range(const RecSlice* recs, const int32_t* paths, const uint64_t* poffs, uint64_t lo, uint64_t hi, std::string& pbuf, std::string& nbuf) {
    uint64_t pmax = 0, nmax = 0;  // exact upper bounds, so the loop below writes through raw pointers
    for (uint64_t i = lo; i < hi; ++i) {
        const RecSlice& r = recs[i];
        const uint64_t np = poffs[i + 1] - poffs[i];
        if (np) pmax += r.hl + 2 + 12 * np; else nmax += (uint64_t)r.hl + r.sl + 2;
    }
    pbuf.resize(pmax);
    nbuf.resize(nmax);
    char* po = pmax ? &pbuf[0] : nullptr;
    char* no = nmax ? &nbuf[0] : nullptr;
    char* const p0 = po;
    for (uint64_t i = lo; i < hi; ++i) {
        const RecSlice& r = recs[i];
        if (poffs[i + 1] > poffs[i]) {
            memcpy(po, r.h, r.hl); po += r.hl;
            *po++ = '\n';
            for (uint64_t j = poffs[i]; j < poffs[i + 1]; ++j) po = put_int(po, paths[j]);
            *po++ = '\n';
        } else {
            memcpy(no, r.h, r.hl); no += r.hl;
            *no++ = '\n';
            memcpy(no, r.s, r.sl); no += r.sl;
            *no++ = '\n';
        }
    }
    pbuf.resize(pmax ? (size_t)(po - p0) : 0);
}

// The host twin of the view of an exhaustive row (exhaustive_rows_kernels.h; a fetched row has left the arena, so that condition has gone): the ints of
// the row as a reader of greedy rows takes it -- without its end offset, or none where the row is not a whole [begin, ids .., end] row of a mapped read.
inline uint64_t exhaustive_view_ints(uint64_t np, uint8_t status) { return ((status & BGR_ST_MASK) == BGR_ST_ALIGNED && np >= 3) ? np - 1 : 0; }

// The same with the opt-in output variants (`status`: the device's byte per read): GAF lines in the place of the path records (`gaf`; needs `correct`,
// the unitigs), correction mode (mapped reads are written as header + corrected read, alignerGreedy.cpp:394-404) and the no-overlap split (reads
// without any anchor go to a third buffer).
// Returns false on the reference's "bug compaction" condition (aligner.cpp:280-283: it prints "bug compaction", the walk
// so far and the unitig that does not continue it, and exits); the buffers then hold the records BEFORE that read and
// `bug` the two strings the reference prints.
// tag_table (n_unitigs + 1 words, or null): a GAF line gains the fields of its read's haplotag (haplotag_host.h), computed from the path ints held here.
// gaf_cs: a GAF line ends in the cs:Z: field, behind the tags.
// exhaustive_rows: the rows are those of exhaustive mode (bgr_graph_exhaustive_paths_enable) and are read through exhaustive_view_ints.
bool format_range_ext(const RecSlice* recs, const int32_t* paths, const uint64_t* poffs, const uint8_t* status, uint64_t lo, uint64_t hi, const Unitigs* correct, bool gaf,
                      bool split_no_overlap, std::string& pbuf, std::string& nbuf, std::string& obuf, std::string& bug, const uint32_t* tag_table = nullptr, uint64_t tag_rows = 0,
                      bool gaf_cs = false, bool exhaustive_rows = false) {
    pbuf.clear(); nbuf.clear(); obuf.clear();
    std::string walk, tmp, rc, cs;
    std::vector<uint8_t> fwd;
    for (uint64_t i = lo; i < hi; ++i) {
        const RecSlice& r = recs[i];
        const uint64_t np = exhaustive_rows ? exhaustive_view_ints(poffs[i + 1] - poffs[i], status[i]) : poffs[i + 1] - poffs[i];
        if (np && gaf) {
            if (np < 2) { walk.clear(); tmp.clear(); }
            if (np < 2 || !gaf_line(*correct, paths + poffs[i], np, r.h, r.hl, r.s, r.sl, (status[i] & BGR_ST_RC) != 0, pbuf, walk, tmp, rc, fwd, gaf_cs ? &cs : nullptr)) {
                bug = walk + " " + tmp;
                return false;
            }
            if (tag_table) {
                const bgr_read_tag tag = bgr::haplotag_row(tag_table, tag_rows - 1, paths + poffs[i] + 1, np - 1);
                if (tag.block) { pbuf.pop_back(); bgr::haplotag_suffix(tag, &pbuf); pbuf.push_back('\n'); }
            }
            if (gaf_cs) { pbuf.pop_back(); pbuf.append(cs); pbuf.push_back('\n'); }
        } else if (np) {
            if (correct && (np < 2 || !recover_path(*correct, paths + poffs[i], np, r.sl, walk, tmp, rc))) {
                bug = walk + " " + tmp;
                return false;
            }
            pbuf.append(r.h, r.hl);
            pbuf.push_back('\n');
            if (correct) {
                if (status[i] & BGR_ST_RC) {  // the path was found on the reverse complement: turn the spelled read back
                    rc.resize(walk.size());
                    for (size_t j = 0; j < walk.size(); ++j) rc[j] = rc_char(walk[walk.size() - 1 - j]);
                    pbuf.append(rc);
                } else {
                    pbuf.append(walk);
                }
            } else {
                char num[16];
                for (uint64_t j = poffs[i]; j < poffs[i + 1]; ++j) { char* e = put_int(num, paths[j]); pbuf.append(num, (size_t)(e - num)); }
            }
            pbuf.push_back('\n');
        } else {
            std::string& o = (split_no_overlap && (status[i] & BGR_ST_MASK) == BGR_ST_NOANCHOR) ? obuf : nbuf;
            o.append(r.h, r.hl);
            o.push_back('\n');
            o.append(r.s, r.sl);
            o.push_back('\n');
        }
    }
    return true;
}

}  // namespace

// bubbles_host.h -- the part of bubble calling that is plain C++ (bgr_bubble in include/bgreat_gpu.h has the definition): the rule an oriented id
// passes to open a bubble, shared by the kernels' two passes, and the comparison of the two branches that the writer prints.  No HIP in here: the
// host sanitizer program compiles it alone.
#ifndef BGREAT_AMD_BUBBLES_HOST_H
#define BGREAT_AMD_BUBBLES_HOST_H

#include <stdint.h>

#include <string>

#include "../../include/bgreat_gpu.h"
#include "graph_layout.h"

namespace bgr {

// the oriented id's index: x -> 2 (|x| - 1) + (x < 0), the order the records come out in; the strand mate -x is the index with its low bit flipped
BGR_HD uint64_t bubbles_o(int32_t x) { return x < 0 ? 2 * (uint64_t)(-(int64_t)x - 1) + 1 : 2 * (uint64_t)((int64_t)x - 1); }
BGR_HD int32_t bubbles_id_of(uint64_t o) { const int32_t v = (int32_t)(o >> 1) + 1; return o & 1 ? -v : v; }
BGR_HD uint32_t bubbles_abs(int32_t x) { return x < 0 ? (uint32_t)(-(int64_t)x) : (uint32_t)x; }
// (|x|, x < 0) < (|y|, y < 0)
BGR_HD bool bubbles_id_less(int32_t x, int32_t y) { return bubbles_o(x) < bubbles_o(y); }

// The adjacency as pass 1 leaves it: deg[o(x)] = |out(x)| (every supported successor counted), to[2 o(x) + i] / cnt[2 o(x) + i] for i < min(deg, 2)
// the first two of them in the order their atomics arrived, which must not show in any result.  in(x) is not kept: it has as many members as
// out(-x), deg[o(x) ^ 1].  n: the number of unitigs; a successor outside 1 .. n opens nothing (none is ever stored).
// -> true when the oriented `s` opens a bubble AND stands for it (of (s, t) and (-t, -s) the pair with the smaller key, links_pack's order:
// (|s|, s < 0, |t|, t < 0)); *out is then the record, its branches in (|id|, id < 0) order.  A slot beyond min(deg, 2) is never read.
BGR_HD bool bubble_at(const uint32_t* deg, const int32_t* to, const uint64_t* cnt, uint64_t n, int32_t s, bgr_bubble* out) {
    const uint64_t os = bubbles_o(s);
    if (deg[os] != 2) return false;
    int32_t b = to[2 * os], c = to[2 * os + 1];
    uint64_t sb = cnt[2 * os], sc = cnt[2 * os + 1];
    if (b == 0 || c == 0 || bubbles_abs(b) > n || bubbles_abs(c) > n) return false;
    const uint64_t ob = bubbles_o(b), oc = bubbles_o(c);
    if (deg[ob ^ 1] != 1 || deg[oc ^ 1] != 1) return false;   // |in(b)| == |in(c)| == 1
    if (deg[ob] != 1 || deg[oc] != 1) return false;           // |out(b)| == |out(c)| == 1
    const int32_t t = to[2 * ob];
    if (to[2 * oc] != t || t == 0 || bubbles_abs(t) > n) return false;
    if (deg[bubbles_o(t) ^ 1] != 2) return false;             // |in(t)| == 2
    const uint32_t as = bubbles_abs(s), ab = bubbles_abs(b), ac = bubbles_abs(c), at = bubbles_abs(t);
    if (as == ab || as == ac || as == at || ab == ac || ab == at || ac == at) return false;
    // the strand mate (-t, -s, -b, -c) is the same bubble: (|s|, s < 0, |t|, t < 0) against (|t|, t > 0, |s|, s > 0); |s| != |t| decides
    if (at < as) return false;
    uint64_t bt = cnt[2 * ob], ct = cnt[2 * oc];
    if (bubbles_id_less(c, b)) { const int32_t x = b; b = c; c = x; uint64_t y = sb; sb = sc; sc = y; y = bt; bt = ct; ct = y; }
    out->source = s; out->sink = t; out->branch[0] = b; out->branch[1] = c;
    out->count[0] = sb; out->count[1] = bt; out->count[2] = sc; out->count[3] = ct;
    return true;
}

// one oriented edge from -> to of a supported link joins the adjacency; *slot = the successor slot it took, 2 when it only counts.  The serial
// form of what pass 1 does with an atomic add (the host program and the tests' hand-made adjacency go through it).
inline void bubbles_add_edge(uint32_t* deg, int32_t* to, uint64_t* cnt, int32_t from, int32_t dest, uint64_t count) {
    const uint64_t o = bubbles_o(from);
    const uint32_t r = deg[o]++;
    if (r < 2) { to[2 * o + r] = dest; cnt[2 * o + r] = count; }
}

// ---- the writer's comparison --------------------------------------------------------------------------------------------------------------
inline char bubbles_complement(char c) {
    switch (c) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
        case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
        default: return c;
    }
}
// the unitig's characters as the oriented id walks them: reversed and complemented for a negative id
inline std::string bubbles_oriented(const char* seq, uint64_t len, bool reverse) {
    std::string s(seq, len);
    if (reverse) {
        for (uint64_t i = 0, j = len; i < j--; ++i) { const char x = bubbles_complement(s[i]), y = bubbles_complement(s[j]); s[i] = y; s[j] = x; }
    }
    return s;
}
// kind and diff of two oriented branches: "snv" with "pos:X>Y" (equal length, exactly one position differs; pos 0-based on the first branch),
// "mnv" (equal length, more than one -- or none, which a compacted graph does not hold) and "indel" (lengths differ), both with "."
inline void bubbles_compare(const std::string& x, const std::string& y, std::string* kind, std::string* diff) {
    *diff = ".";
    if (x.size() != y.size()) { *kind = "indel"; return; }
    uint64_t nd = 0, at = 0;
    for (uint64_t i = 0; i < x.size(); ++i) if (x[i] != y[i]) { if (!nd) at = i; ++nd; }
    if (nd == 1) { *kind = "snv"; *diff = std::to_string(at) + ":" + x[at] + ">" + y[at]; }
    else *kind = "mnv";
}

}  // namespace bgr

#endif

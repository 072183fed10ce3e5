// phase_host.h -- the part of the triples and of read-backed phasing that is plain C++ (bgr_triple and bgr_phase in include/bgreat_gpu.h have
// the definitions): the order of the triples, the join of neighbouring bubbles with the triple counts, and the lines of the two files.  No HIP in
// here: the host sanitizer program compiles it alone.
#ifndef BGREAT_AMD_PHASE_HOST_H
#define BGREAT_AMD_PHASE_HOST_H

#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bgreat_gpu.h"
#include "bubbles_host.h"

namespace bgr {

// the two words a triple sorts by (the packing of triples_kernels.h, which the kernel's table holds): (|a|, a < 0, |b|, b < 0) and (|c|, c < 0)
inline uint64_t phase_word(int32_t x) { return ((uint64_t)bubbles_abs(x) << 1) | (uint64_t)(x < 0); }
inline std::pair<uint64_t, uint64_t> phase_key(int32_t a, int32_t b, int32_t c) { return {(phase_word(a) << 32) | phase_word(b), phase_word(c)}; }
inline bool phase_id_ok(int32_t x) { return x != 0 && x != INT32_MIN && bubbles_abs(x) < 0x40000000u; }
// (a, b, c) and (-c, -b, -a) are one triple: -> the one with the smaller key (ids that phase_id_ok passes)
inline void phase_canonical(int32_t a, int32_t b, int32_t c, int32_t out[3]) {
    const bool keep = phase_key(a, b, c) < phase_key(-c, -b, -a);
    out[0] = keep ? a : -c; out[1] = keep ? b : -b; out[2] = keep ? c : -a;
}

// count of the canonical form of (a, b, c) in `triples` (canonical, strictly ascending by key); 0 when it is not there
inline uint64_t phase_count_of(const bgr_triple* triples, uint64_t n, int32_t a, int32_t b, int32_t c) {
    int32_t t[3];
    phase_canonical(a, b, c, t);
    const std::pair<uint64_t, uint64_t> want = phase_key(t[0], t[1], t[2]);
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (phase_key(triples[mid].from, triples[mid].via, triples[mid].to) < want) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && phase_key(triples[lo].from, triples[lo].via, triples[lo].to) == want ? triples[lo].count : 0;
}

// -> 0, or what is wrong with the input: 1 = a bubble names an id that is none, 2 = a triple does, 3 = a triple is not canonical, 4 = the triples
// are not strictly ascending; *bad = the record
inline int phase_check(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_triple* triples, uint64_t n_triples, uint64_t* bad) {
    for (uint64_t i = 0; i < n_bubbles; ++i) {
        *bad = i;
        if (!phase_id_ok(bubbles[i].source) || !phase_id_ok(bubbles[i].sink) || !phase_id_ok(bubbles[i].branch[0]) || !phase_id_ok(bubbles[i].branch[1])) return 1;
    }
    for (uint64_t i = 0; i < n_triples; ++i) {
        const bgr_triple& t = triples[i];
        *bad = i;
        if (!phase_id_ok(t.from) || !phase_id_ok(t.via) || !phase_id_ok(t.to)) return 2;
        if (!(phase_key(t.from, t.via, t.to) < phase_key(-t.to, -t.via, -t.from))) return 3;
        if (i && !(phase_key(triples[i - 1].from, triples[i - 1].via, triples[i - 1].to) < phase_key(t.from, t.via, t.to))) return 4;
    }
    return 0;
}

// The neighbour pairs of `bubbles` (records as bgr_graph_bubbles delivers them; input that phase_check passes) with the counts of the triples that
// thread them: every bubble is read in both orientations, (s, t, b, c) and (-t, -s, -b, -c); X and Y are neighbours through m when X's sink and
// Y's source are m, reported in the reading with m > 0 and ordered by it.  An oriented id is the source of at most one bubble and the sink of at
// most one; of a list that breaks this the first record of an id counts.
inline std::vector<bgr_phase> phase_of(const bgr_bubble* bubbles, uint64_t n_bubbles, const bgr_triple* triples, uint64_t n_triples) {
    struct Oriented { int32_t s, t, b[2]; };
    std::vector<Oriented> all(2 * n_bubbles);
    std::vector<std::pair<uint64_t, uint64_t>> by_source(2 * n_bubbles);   // {o(source), index into `all`}
    for (uint64_t i = 0; i < n_bubbles; ++i) {
        const bgr_bubble& r = bubbles[i];
        int32_t b0 = r.branch[0], b1 = r.branch[1];
        if (bubbles_id_less(b1, b0)) std::swap(b0, b1);
        all[2 * i] = Oriented{r.source, r.sink, {b0, b1}};
        all[2 * i + 1] = Oriented{-r.sink, -r.source, {-b0, -b1}};   // ((|id|, id < 0): negating both keeps the order unless |b0| == |b1|, which no bubble has)
        if (bubbles_id_less(all[2 * i + 1].b[1], all[2 * i + 1].b[0])) std::swap(all[2 * i + 1].b[0], all[2 * i + 1].b[1]);
        by_source[2 * i] = {bubbles_o(all[2 * i].s), 2 * i};
        by_source[2 * i + 1] = {bubbles_o(all[2 * i + 1].s), 2 * i + 1};
    }
    std::sort(by_source.begin(), by_source.end());
    std::vector<bgr_phase> out;
    std::vector<std::pair<uint64_t, uint64_t>> by_via;   // {m, index into `all` of X}: at most one X per m is kept
    for (uint64_t x = 0; x < all.size(); ++x)
        if (all[x].t > 0) by_via.push_back({(uint64_t)all[x].t, x});
    std::sort(by_via.begin(), by_via.end());
    for (size_t i = 0; i < by_via.size(); ++i) {
        if (i && by_via[i - 1].first == by_via[i].first) continue;
        const Oriented& X = all[by_via[i].second];
        const int32_t m = X.t;
        const auto it = std::lower_bound(by_source.begin(), by_source.end(), std::make_pair(bubbles_o(m), (uint64_t)0));
        if (it == by_source.end() || it->first != bubbles_o(m)) continue;
        const Oriented& Y = all[it->second];
        bgr_phase p;
        p.via = m; p.source = X.s; p.in[0] = X.b[0]; p.in[1] = X.b[1]; p.out[0] = Y.b[0]; p.out[1] = Y.b[1]; p.sink = Y.t; p.reserved = 0;
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) p.count[2 * a + b] = phase_count_of(triples, n_triples, p.in[a], m, p.out[b]);
        out.push_back(p);
    }
    return out;
}

// "cis" when n11 + n22 > n12 + n21, "trans" when it is smaller, "." when they are equal (128-bit sums: four full 64-bit counts do not wrap)
inline const char* phase_call(const uint64_t count[4]) {
    const unsigned __int128 cis = (unsigned __int128)count[0] + count[3], trans = (unsigned __int128)count[1] + count[2];
    return cis > trans ? "cis" : (cis < trans ? "trans" : ".");
}

// ---- the lines of the two files ---------------------------------------------------------------------------------------------------------------
inline const char* triples_header() { return "#from\tvia\tto\tcount\n"; }
inline void triples_line(const bgr_triple& t, std::string* buf) {
    *buf += std::to_string(t.from); *buf += '\t'; *buf += std::to_string(t.via); *buf += '\t'; *buf += std::to_string(t.to); *buf += '\t';
    *buf += std::to_string(t.count); *buf += '\n';
}
inline const char* phase_header() { return "#via\tsource\tin1\tin2\tout1\tout2\tsink\tn11\tn12\tn21\tn22\tphase\n"; }
inline void phase_line(const bgr_phase& p, std::string* buf) {
    const int32_t ids[7] = {p.via, p.source, p.in[0], p.in[1], p.out[0], p.out[1], p.sink};
    for (int32_t x : ids) { *buf += std::to_string(x); *buf += '\t'; }
    for (int i = 0; i < 4; ++i) { *buf += std::to_string(p.count[i]); *buf += '\t'; }
    *buf += phase_call(p.count); *buf += '\n';
}

}  // namespace bgr

#endif

// inside_index.cpp -- see inside_index.h.  The unitigs are read from the blob's 2-bit store (meta + seq), so any graph with a host blob can
// have the index.  Two parallel passes over contiguous ranges of unitigs (host_parallel.h): count the selected windows, then insert them --
// a slot's key is claimed with a compare-and-swap, its value lowered to the smallest (id, j) with another: the table's CONTENT does not
// depend on the threads or their timing (which slot of a probe sequence a key lives in may).
#include "inside_index.h"

#include <chrono>
#include <cstdlib>
#include <vector>

#include "host_parallel.h"

namespace bgr {

void InsideIndex::release() {
    free(tab);
    tab = nullptr;
    slots = entries = 0;
}

namespace {

// fn(canonical, id, j, forward window is canonical) for every selected window of the unitigs [ub, ue) (ids from 1)
template <class Fn>
void selected_windows(const BgrBlobHeader* h, const uint8_t* base, uint64_t ub, uint64_t ue, Fn fn) {
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(base + h->off_meta);
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(base + h->off_seq);
    const uint32_t k = h->k;
    const uint64_t mask = k == 32 ? ~0ULL : (1ULL << (2 * k)) - 1;
    for (uint64_t id = ub; id < ue; ++id) {
        const uint64_t F = meta[id].F, len = meta[id].len;
        if (len < k) continue;
        uint64_t x = 0;
        for (uint64_t p = 0; p < len; ++p) {
            const uint64_t b = F + p;
            x = ((x << 2) | ((seq[b >> 5] >> (62 - 2 * (b & 31))) & 3)) & mask;
            if (p + 1 < k) continue;
            const uint64_t r = bgr_rcb(x, k);
            if (x == r) continue;
            const uint64_t c = x < r ? x : r;
            if (bgr_jump_selects(bgr_mix64(c))) fn(c, (uint32_t)id, (uint32_t)(p + 1 - k), x < r);
        }
    }
}

}  // namespace

int build_inside_index(const BgrBlobHeader* h, const uint8_t* base, unsigned T, InsideIndex& out, std::string& err) {
    out.release();
    if (h->k > BGR_NARROW_MAX_K) { err = "the inside index holds one-word k-mers: k <= 32"; return 1; }
    if (h->has_exc) { err = "the inside index needs a graph of ACGT-only unitigs (it is read from the 2-bit store)"; return 1; }
    const auto t0 = std::chrono::steady_clock::now();
    if (T < 1) T = 1;
    const uint64_t n = h->n_unitigs;
    std::vector<uint64_t> counts(T, 0);
    parallel_ranges(T, n, [&](uint64_t b, uint64_t e, unsigned t) {
        uint64_t c = 0;
        selected_windows(h, base, b + 1, e + 1, [&c](uint64_t, uint32_t, uint32_t, bool) { ++c; });
        counts[t] = c;
    });
    uint64_t windows = 0;
    for (uint64_t c : counts) windows += c;
    const uint64_t slots = windows < 8 ? 16 : 2 * windows;
    BgrInsideEntry* tab = static_cast<BgrInsideEntry*>(malloc(slots * sizeof(BgrInsideEntry)));
    if (!tab) { err = "no memory for the inside index (" + std::to_string(slots * sizeof(BgrInsideEntry)) + " bytes)"; return 2; }
    parallel_ranges(T, slots, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t s = b; s < e; ++s) { tab[s].key = BGR_EMPTY_KEY; tab[s].val = ~0ULL; }
    });
    std::vector<uint64_t> placed(T, 0);
    parallel_ranges(T, n, [&](uint64_t b, uint64_t e, unsigned t) {
        uint64_t mine = 0;
        selected_windows(h, base, b + 1, e + 1, [&](uint64_t c, uint32_t id, uint32_t j, bool fc) {
            const uint64_t v = bgr_inside_val(id, j, fc);
            uint64_t s = bgr_inside_slot(bgr_mix64(c), slots);
            for (;;) {   // (ends: fewer keys than half the slots)
                uint64_t seen = __atomic_load_n(&tab[s].key, __ATOMIC_RELAXED);
                if (seen == BGR_EMPTY_KEY) {
                    if (__atomic_compare_exchange_n(&tab[s].key, &seen, c, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { ++mine; seen = c; }
                }
                if (seen == c) {
                    uint64_t cur = __atomic_load_n(&tab[s].val, __ATOMIC_RELAXED);
                    while (v < cur && !__atomic_compare_exchange_n(&tab[s].val, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
                    return;
                }
                if (++s == slots) s = 0;
            }
        });
        placed[t] = mine;
    });
    out.tab = tab;
    out.slots = slots;
    for (uint64_t c : placed) out.entries += c;
    out.build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

bool inside_lookup(const InsideIndex& ix, uint32_t k, uint64_t kmer, uint64_t* val) {
    if (!ix.tab || k > BGR_NARROW_MAX_K) return false;
    if (k < 32) kmer &= (1ULL << (2 * k)) - 1;
    const uint64_t r = bgr_rcb(kmer, k);
    if (kmer == r) return false;
    const uint64_t c = kmer < r ? kmer : r;
    for (uint64_t s = bgr_inside_slot(bgr_mix64(c), ix.slots);; s = s + 1 == ix.slots ? 0 : s + 1) {
        if (ix.tab[s].key == c) { *val = ix.tab[s].val; return true; }
        if (ix.tab[s].key == BGR_EMPTY_KEY) return false;
    }
}

}  // namespace bgr

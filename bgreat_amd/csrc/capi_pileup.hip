// capi_pileup.hip -- the C-ABI's pileup (bgr_pileup_base in include/bgreat_gpu.h has the definition): the aligners' tables (the total one
// and, with strands, the forward one), the run's totals in the graph object, the three writers.
#include <cstdio>
#include <cstring>

#include "capi_internal.h"
#include "pileup_kernels.h"

// ---- pileup (bgr_pileup_base in include/bgreat_gpu.h has the definition) -------------------------------------------------------------------
int graph_base_offs(bgr_graph* g, const char* who) {   // prefix sums of the unitig lengths, once per graph
    if (g->host.blob.empty()) return fail(BGR_E_ARG, std::string(who) + ": the graph has no host blob (the unitig lengths and characters are read from it)");
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (g->base_offs.empty()) {
        const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
        std::vector<uint64_t> o(g->header.n_unitigs + 2, 0);
        for (uint64_t i = 1; i <= g->header.n_unitigs; ++i) o[i + 1] = o[i] + meta[i].len;
        g->base_offs.swap(o);
    }
    return BGR_OK;
}
int pileup_refusal(const bgr_graph* g, const char* who) {
    if (g->header.has_exc)
        return fail(BGR_E_ARG, std::string(who) + ": the pileup (--pileup, --depth) needs a graph of ACGT-only unitigs: on one with other characters the 2-bit store does not spell them and a path read backwards does not spell the reverse complement");
    return BGR_OK;
}
// A table of the pileup's layout in `tab` -- and, with `offs`, the graph's base_offs next to it -- on the first enable: allocated (a failure leaves
// neither and reports `what`), zeroed / uploaded on the aligner's own stream (as bgr_aligner_reset_counters), waited for.
static int pileup_table_alloc(bgr_aligner* a, DevBuf& tab, DevBuf* offs, const char* who, const char* what) {
    const uint64_t n = a->graph->header.n_unitigs, bytes = bgr::pileup_table_bytes(a->graph->header.total_bases / 2, n);
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = tab.ensure(bytes);
    if (e == hipSuccess && offs) e = offs->ensure((n + 2) * 8);
    if (e != hipSuccess) {
        tab.release();
        if (offs) offs->release();
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": " + std::to_string(bytes) + " bytes for the " + what + ": " + hipGetErrorString(e));
    }
    HIP_TRY(hipMemsetAsync(tab.p, 0, bytes, a->stream));
    if (offs) HIP_TRY(hipMemcpyAsync(offs->p, a->graph->base_offs.data(), (n + 2) * 8, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return BGR_OK;
}

int bgr_aligner_pileup_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_pileup_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_enable: an internal stream of another aligner");
    if (on) {
        int rc = pileup_refusal(a->graph, "bgr_aligner_pileup_enable");
        if (rc == BGR_OK) rc = graph_base_offs(a->graph, "bgr_aligner_pileup_enable");
        if (rc == BGR_OK) rc = bgr_aligner_abundance_enable(a, 1);   // (its reads column bounds every depth: bgr_aligner_pileup checks it)
        if (rc != BGR_OK) return rc;
    }
    PileupTables& t = a->sh->pileup;
    if (on && !t.tab) {
        const int rc = pileup_table_alloc(a, t.table, &t.offs, "bgr_aligner_pileup_enable", "pileup table (20 per base of the graph)");
        if (rc != BGR_OK) return rc;
        t.tab = t.table.as<uint32_t>();
        t.base_offs = t.offs.as<const uint64_t>();
    }
    t.on = on != 0;
    return BGR_OK;
}

int bgr_aligner_pileup_strands_enable(bgr_aligner* a, uint32_t on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_pileup_strands_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_strands_enable: an internal stream of another aligner");
    PileupTables& t = a->sh->pileup;
    const bool fresh = on && !t.fwd_tab;
    if (fresh) {   // the second table first: a refusal leaves the aligner as it was
        int rc = pileup_refusal(a->graph, "bgr_aligner_pileup_strands_enable");
        if (rc == BGR_OK) rc = pileup_table_alloc(a, t.fwd, nullptr, "bgr_aligner_pileup_strands_enable", "forward pileup table (20 more per base of the graph)");
        if (rc != BGR_OK) return rc;
        t.fwd_tab = t.fwd.as<uint32_t>();
    }
    if (on) {
        const int rc = bgr_aligner_pileup_enable(a, 1);   // (as the pileup enables abundance)
        if (rc != BGR_OK) {
            if (fresh) { t.fwd.release(); t.fwd_tab = nullptr; }   // (nothing stays allocated behind a refusal)
            return rc;
        }
    }
    t.strands_on = on != 0;
    return BGR_OK;
}

// alt / delta words -> rows: the depth is the running sum of a unitig's delta words, N lies in the alt word of the unitig's own base
static void pileup_unitig_rows(const bgr_graph* g, const uint32_t* words, uint64_t id, bgr_pileup_base* out) {   // the len rows of one unitig
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_seq);
    const uint32_t* alt = words;
    const uint32_t* delta = words + bgr::pileup_alt_words(g->header.total_bases / 2);
    const uint64_t b0 = g->base_offs[id], d0 = b0 + id - 1, F = meta[id].F;
    uint32_t depth = 0;
    for (uint64_t pos = 0; pos < meta[id].len; ++pos) {
        depth += delta[d0 + pos];   // (mod 2^32)
        const uint64_t p = F + pos;
        const uint32_t ref = (uint32_t)(seq[p >> 5] >> (62 - 2 * (p & 31))) & 3u;
        const uint32_t* w = alt + 4 * (b0 + pos);
        uint32_t c[4] = {w[0], w[1], w[2], w[3]};
        c[ref] = 0;   // (nothing that differs from the base has the base's code: that word counted the Ns)
        out[pos] = bgr_pileup_base{depth, c[0], c[1], c[2], c[3], w[ref]};
    }
}
static void pileup_rows(const bgr_graph* g, const uint32_t* words, bgr_pileup_base* out) {
    for (uint64_t id = 1; id <= g->header.n_unitigs; ++id) pileup_unitig_rows(g, words, id, out + g->base_offs[id]);
}
// this aligner's reads column may not have reached 2^32 anywhere: it bounds every depth on the unitig, and a depth is kept mod 2^32
int pileup_guard(const bgr_unitig_abundance* rows, uint64_t n, const char* who) {
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i].reads >> 32)
            return fail(BGR_E_CAPACITY, std::string(who) + ": unitig " + std::to_string(i + 1) + " lies on " + std::to_string(rows[i].reads) + " reads' paths: a per-base depth (32 bits) may have wrapped; no pileup is delivered");
    return BGR_OK;
}
// the guard over this aligner's abundance as it stands, then every stream that adds to its tables waited for
int guarded_sync(bgr_aligner* a, const char* who) {
    const uint64_t n = a->graph->header.n_unitigs;
    std::vector<bgr_unitig_abundance> ab(n);
    int rc = bgr_aligner_abundance(a, ab.data(), n);   // (synchronises the aligner's stream and its twins')
    if (rc == BGR_OK) rc = pileup_guard(ab.data(), n, who);
    return rc == BGR_OK ? sync_all(a) : rc;
}
// the aligner's table on the host (every stream that adds to it waited for), behind the guard
static int pileup_snapshot(bgr_aligner* a, const char* who, std::vector<uint32_t>& words, uint64_t* skipped, bool fwd = false) {
    if (fwd && !a->sh->pileup.fwd_tab) return fail(BGR_E_ARG, std::string(who) + ": strands were never counted on this aligner (bgr_aligner_pileup_strands_enable)");
    if (!a->sh->pileup.tab) return fail(BGR_E_ARG, std::string(who) + ": the pileup was never enabled on this aligner (bgr_aligner_pileup_enable)");
    const uint64_t n = a->graph->header.n_unitigs, T = a->graph->header.total_bases / 2;
    if (const int rc = guarded_sync(a, who); rc != BGR_OK) return rc;
    words.resize(bgr::pileup_alt_words(T) + bgr::pileup_delta_words(T, n));
    const uint32_t* tab = fwd ? a->sh->pileup.fwd_tab : a->sh->pileup.tab;
    if (!words.empty()) HIP_TRY(hipMemcpy(words.data(), tab, words.size() * 4, hipMemcpyDeviceToHost));
    unsigned long long sk = 0;
    HIP_TRY(hipMemcpy(&sk, reinterpret_cast<const char*>(tab) + bgr::pileup_tail_byte(T, n), 8, hipMemcpyDeviceToHost));
    *skipped = sk;
    return BGR_OK;
}

static int aligner_pileup(bgr_aligner* a, bgr_pileup_base* out, uint64_t n_bases, uint64_t* skipped, bool fwd, const char* who) {
    static_assert(sizeof(bgr_pileup_base) == 24, "six u32 per base");
    if (!a || (n_bases && !out)) return fail(BGR_E_ARG, std::string(who) + ": null argument");
    if (a->is_twin) return fail(BGR_E_ARG, std::string(who) + ": an internal stream of another aligner");
    if (n_bases != a->graph->header.total_bases / 2) return fail(BGR_E_ARG, std::string(who) + ": n_bases is not the sum of the graph's unitig lengths");
    std::vector<uint32_t> words;
    uint64_t sk = 0;
    const int rc = pileup_snapshot(a, who, words, &sk, fwd);
    if (rc != BGR_OK) return rc;
    pileup_rows(a->graph, words.data(), out);
    if (skipped) *skipped = sk;
    return BGR_OK;
}
int bgr_aligner_pileup(bgr_aligner* a, bgr_pileup_base* out, uint64_t n_bases, uint64_t* skipped) { return aligner_pileup(a, out, n_bases, skipped, false, "bgr_aligner_pileup"); }
int bgr_aligner_pileup_forward(bgr_aligner* a, bgr_pileup_base* out, uint64_t n_bases) { return aligner_pileup(a, out, n_bases, nullptr, true, "bgr_aligner_pileup_forward"); }

int bgr_aligner_reset_pileup(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_pileup: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_reset_pileup: an internal stream of another aligner");
    if (!a->sh->pileup.table.p) return BGR_OK;
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;
    HIP_TRY(hipMemsetAsync(a->sh->pileup.table.p, 0, bgr::pileup_table_bytes(a->graph->header.total_bases / 2, a->graph->header.n_unitigs), a->stream));
    if (a->sh->pileup.fwd.p) HIP_TRY(hipMemsetAsync(a->sh->pileup.fwd.p, 0, bgr::pileup_table_bytes(a->graph->header.total_bases / 2, a->graph->header.n_unitigs), a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return BGR_OK;   // (the abundance table stays: the guard's column then counts more launches than the pileup holds, which errs on the safe side)
}

// what a whole run calls (run_counts.h, through capi_abundance.hip): the graph's pileup switch gathers the tables on the host, its variants switch
// (capi_variants.hip) on a device
void run_pileup_begin(bgr_graph* g) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    if (g->pileup_on) {
        g->pileup_words.clear();
        g->pileup_skipped = 0;
        g->pileup_valid = false;
        g->pileup_fwd_words.clear();
        g->pileup_fwd_valid = false;
    }
    if (g->variants_on) {
        variants_run_free(g);
        g->variants_sites.clear();
        g->variants_valid = false;
        g->variants_strand_sites.clear();
        g->variants_strands_valid = false;
    }
}
static int run_pileup_sum(bgr_graph* g, bgr_aligner* a, bool fwd) {   // one of the aligner's tables joins the run's sum of it (the forward table's tail is 0)
    std::vector<uint32_t> words;
    uint64_t sk = 0;
    const int rc = pileup_snapshot(a, "bgr_align_all", words, &sk, fwd);
    if (rc != BGR_OK) return rc;
    std::lock_guard<std::mutex> l(g->abundance_m);
    std::vector<uint32_t>& sum = fwd ? g->pileup_fwd_words : g->pileup_words;
    if (sum.empty()) sum.swap(words);
    else for (size_t i = 0; i < words.size(); ++i) sum[i] += words[i];   // (mod 2^32: the delta sums commute)
    if (!fwd) g->pileup_skipped += sk;
    return BGR_OK;
}
int run_pileup_collect(bgr_graph* g, bgr_aligner* a) {
    int rc = g->pileup_on ? run_pileup_sum(g, a, false) : BGR_OK;
    if (rc == BGR_OK && g->pileup_on && g->pileup_strands_on) rc = run_pileup_sum(g, a, true);
    if (rc != BGR_OK) return rc;
    return g->variants_on ? variants_collect(g, a) : BGR_OK;   // (behind the snapshot: the first aligner's table leaves it here)
}
int run_pileup_end(bgr_graph* g, bool ok) {   // behind the abundance's end: the summed reads column guards the summed table
    int rc = BGR_OK;
    if (g->pileup_on) {
        std::lock_guard<std::mutex> l(g->abundance_m);
        if (ok) {
            const uint64_t T = g->header.total_bases / 2, n = g->header.n_unitigs;
            if (g->pileup_words.empty()) g->pileup_words.assign(bgr::pileup_alt_words(T) + bgr::pileup_delta_words(T, n), 0u);   // (a run without aligners' tables: nothing mapped)
            rc = g->abundance_valid ? pileup_guard(g->abundance.data(), g->abundance.size(), "bgr_align_all") : fail(BGR_E_INTERNAL, "bgr_align_all: a pileup without the abundance totals that guard it");
        }
        if (!ok || rc != BGR_OK) { g->pileup_words.clear(); g->pileup_words.shrink_to_fit(); }
        g->pileup_valid = ok && rc == BGR_OK;
        if (g->pileup_strands_on && g->pileup_valid && g->pileup_fwd_words.empty()) g->pileup_fwd_words.assign(g->pileup_words.size(), 0u);
        if (!g->pileup_strands_on || !g->pileup_valid) { g->pileup_fwd_words.clear(); g->pileup_fwd_words.shrink_to_fit(); }
        g->pileup_fwd_valid = g->pileup_strands_on && g->pileup_valid;
    }
    if (g->variants_on) {
        const int vrc = variants_end(g, ok && rc == BGR_OK);
        if (rc == BGR_OK) rc = vrc;
    }
    return rc;
}

int bgr_graph_pileup_enable(bgr_graph* g, uint32_t on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_pileup_enable: null graph");
    if (on) {
        int rc = pileup_refusal(g, "bgr_graph_pileup_enable");
        if (rc == BGR_OK) rc = graph_base_offs(g, "bgr_graph_pileup_enable");
        if (rc != BGR_OK) return rc;
    }
    g->pileup_on = on != 0;
    return BGR_OK;
}

int bgr_graph_pileup_enabled(const bgr_graph* g) { return g && g->pileup_on ? 1 : 0; }

int bgr_graph_pileup_strands_enable(bgr_graph* g, uint32_t on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_pileup_strands_enable: null graph");
    if (on) {
        const int rc = bgr_graph_pileup_enable(g, 1);   // (as the aligner's switch enables the aligner's pileup)
        if (rc != BGR_OK) return rc;
    }
    g->pileup_strands_on = on != 0;
    return BGR_OK;
}

int bgr_graph_pileup_strands_enabled(const bgr_graph* g) { return g && g->pileup_strands_on ? 1 : 0; }

// the totals of the last successful run (fwd: the forward ones) are there
static int graph_pileup_check(const bgr_graph* g, const char* who, bool fwd = false) {
    if (g->pileup_valid && (!fwd || g->pileup_fwd_valid)) return BGR_OK;
    return fail(BGR_E_ARG, std::string(who) + ": no " + (fwd ? "forward " : "") + "totals -- they are those of the last successful bgr_align_all with " + (fwd ? "bgr_graph_pileup_strands_enable" : "bgr_graph_pileup_enable") + " on");
}
static int graph_pileup(const bgr_graph* g, bgr_pileup_base* out, uint64_t n_bases, uint64_t* skipped, bool fwd, const char* who) {
    if (!g || (n_bases && !out)) return fail(BGR_E_ARG, std::string(who) + ": null argument");
    const int rc = graph_pileup_check(g, who, fwd);
    if (rc != BGR_OK) return rc;
    if (n_bases != g->header.total_bases / 2) return fail(BGR_E_ARG, std::string(who) + ": n_bases is not the sum of the graph's unitig lengths");
    pileup_rows(g, (fwd ? g->pileup_fwd_words : g->pileup_words).data(), out);
    if (skipped) *skipped = g->pileup_skipped;
    return BGR_OK;
}
int bgr_graph_pileup(const bgr_graph* g, bgr_pileup_base* out, uint64_t n_bases, uint64_t* skipped) { return graph_pileup(g, out, n_bases, skipped, false, "bgr_graph_pileup"); }
int bgr_graph_pileup_forward(const bgr_graph* g, bgr_pileup_base* out, uint64_t n_bases) { return graph_pileup(g, out, n_bases, nullptr, true, "bgr_graph_pileup_forward"); }

// the writers: host code, deterministic bytes, straight from the graph's totals
static int pileup_write(const char* path, const bgr_graph* g, bool sites, const char* who, bool strands = false) {
    if (!path || !g) return fail(BGR_E_ARG, std::string(who) + ": null argument");
    const int rc = graph_pileup_check(g, who, strands);
    if (rc != BGR_OK) return rc;
    std::vector<bgr_pileup_base> frows(strands ? g->header.max_unitig_len + 1 : 0);
    const uint64_t n = g->header.n_unitigs;
    std::vector<bgr_pileup_base> rows(g->header.max_unitig_len + 1);   // (converted unitig by unitig: no second table on the host)
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_seq);
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, std::string(who) + ": cannot open " + path);
    std::string buf = strands ? "#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tdepth+\tA+\tC+\tG+\tT+\tN+\n" : sites ? "#unitig\tpos\tref\tdepth\tA\tC\tG\tT\tN\n" : "";
    bool ok = true;
    auto flush = [&](bool all) { if (ok && !buf.empty() && (all || buf.size() > (1u << 20))) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); } };
    for (uint64_t id = 1; id <= n && ok; ++id) {
        const uint64_t len = meta[id].len;
        if (len > rows.size()) rows.resize(len);
        pileup_unitig_rows(g, g->pileup_words.data(), id, rows.data());
        if (strands) {
            if (len > frows.size()) frows.resize(len);
            pileup_unitig_rows(g, g->pileup_fwd_words.data(), id, frows.data());
        }
        const bgr_pileup_base* r = rows.data();
        if (sites) {
            for (uint64_t pos = 0; pos < len; ++pos) {
                const bgr_pileup_base& b = r[pos];
                if (!(b.depth | b.a | b.c | b.g | b.t | b.n)) continue;
                const uint64_t p = meta[id].F + pos;
                buf += std::to_string(id); buf += '\t'; buf += std::to_string(pos); buf += '\t';
                buf += "ACGT"[(seq[p >> 5] >> (62 - 2 * (p & 31))) & 3u];
                for (const uint32_t v : {b.depth, b.a, b.c, b.g, b.t, b.n}) { buf += '\t'; buf += std::to_string(v); }
                if (strands) { const bgr_pileup_base& fb = frows[pos]; for (const uint32_t v : {fb.depth, fb.a, fb.c, fb.g, fb.t, fb.n}) { buf += '\t'; buf += std::to_string(v); } }
                buf += '\n';
            }
        } else {
            for (uint64_t pos = 0; pos < len;) {   // maximal runs of equal non-zero depth
                uint64_t e = pos + 1;
                while (e < len && r[e].depth == r[pos].depth) ++e;
                if (r[pos].depth) { buf += std::to_string(id); buf += '\t'; buf += std::to_string(pos); buf += '\t'; buf += std::to_string(e); buf += '\t'; buf += std::to_string(r[pos].depth); buf += '\n'; }
                pos = e;
            }
        }
        flush(false);
    }
    flush(true);
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, std::string(who) + ": write to " + path + " failed");
    return BGR_OK;
}
int bgr_write_pileup(const char* path, const bgr_graph* g) { return pileup_write(path, g, true, "bgr_write_pileup"); }
int bgr_write_depth(const char* path, const bgr_graph* g) { return pileup_write(path, g, false, "bgr_write_depth"); }
int bgr_write_pileup_strands(const char* path, const bgr_graph* g) { return pileup_write(path, g, true, "bgr_write_pileup_strands", true); }


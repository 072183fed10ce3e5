// capi_variants.hip -- the C-ABI's SNV sites (bgr_variant_site in include/bgreat_gpu.h has the definition; variants_kernels.h the passes): the
// calls on an aligner's pileup tables, the run's table on a device while its aligners are collected, the sites in the graph object, the
// parsers' wrappers and the VCF writers.  Records are 32 bytes, or 64 with the forward numbers (strands): one code path for both.
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "capi_internal.h"
#include "variants_kernels.h"

// ---- SNV sites (bgr_variant_site in include/bgreat_gpu.h has the definition; variants_kernels.h the passes) -------------------------------------
// the five launches over one table (with strands: and its forward table; Site says which) on `stream` of the current device, then the records' way to
// the host: into `vec` (as many as there are), or into `out` when they are at most `cap`.  *n = their number in any case.  ms: null, or the five
// launches' milliseconds.  prm.min_alt_strand counts only with strands
template <class Site>
static int variants_call(const BgrDeviceGraph& dg, const bgr_graph* g, const uint32_t* table, const uint32_t* table_fwd, const uint64_t* base_offs, const bgr_variant_strand_params& prm,
                         DevBuf& scratch, DevBuf& outbuf, hipStream_t stream, const char* who, std::vector<Site>* vec, Site* out, uint64_t cap, uint64_t* n, double* ms) {
    static_assert(sizeof(bgr_variant_site) == 32, "eight u32 per site");
    static_assert(sizeof(bgr_variant_strand_site) == 64, "sixteen u32 per site");
    const bool strands = std::is_same<Site, bgr_variant_strand_site>::value;
    const std::string tag = strands ? ", strands" : "";
    if (!strands) table_fwd = nullptr;
    const uint64_t nu = g->header.n_unitigs, T = g->header.total_bases / 2, tiles = bgr::variants_tiles(T, nu);
    *n = 0;
    if (ms) for (int i = 0; i < 5; ++i) ms[i] = 0;
    if (vec) vec->clear();
    if (tiles == 0 || nu == 0) return BGR_OK;
    hipError_t e = scratch.ensure(bgr::variants_scratch_bytes(tiles, strands));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": the passes' tile arrays: " + hipGetErrorString(e)); }
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 6; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } guard{ev};
    if (ms) {
        for (int i = 0; i < 6; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        HIP_TRY(hipEventRecord(ev[0], stream));
    }
    e = bgr::launch_variants_count(dg, nu, T, table, table_fwd, base_offs, prm, scratch.p, stream, ms ? ev + 1 : nullptr);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_variants_*_kernel" + tag + "): " + hipGetErrorString(e));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, bgr::variants_total_word(scratch.p, tiles), 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *n = total;
    if (total > T) return fail(BGR_E_INTERNAL, std::string(who) + ": more sites than bases");
    if (!vec && total > cap) return fail(BGR_E_CAPACITY, std::string(who) + ": " + std::to_string(total) + " sites, room for " + std::to_string(cap));
    if (total) {
        e = outbuf.ensure(total * sizeof(Site));
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": " + std::to_string(total) + " site records on the device: " + hipGetErrorString(e)); }
        e = bgr::launch_variants_emit(dg, nu, T, table, table_fwd, base_offs, prm, scratch.p, outbuf.p, stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_variants_classify_kernel" + tag + ", emit): " + hipGetErrorString(e));
        if (ms) HIP_TRY(hipEventRecord(ev[5], stream));
        if (vec) { vec->resize(total); out = vec->data(); }
        HIP_TRY(hipMemcpyAsync(out, outbuf.p, total * sizeof(Site), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    if (ms)
        for (int i = 0; i < (total ? 5 : 4); ++i) { float f = 0; HIP_TRY(hipEventElapsedTime(&f, ev[i], ev[i + 1])); ms[i] = f; }
    return BGR_OK;
}

// the run's table (VariantsRun, capi_internal.h) and its stream, released
void variants_run_free(bgr_graph* g) {
    if (!g->variants_run) return;
    if (hipSetDevice(g->variants_run->device) == hipSuccess) {
        if (g->variants_run->stream) (void)hipStreamDestroy(g->variants_run->stream);
        g->variants_run->table.release(); g->variants_run->offs.release(); g->variants_run->stage.release(); g->variants_run->table_fwd.release();
    }
    delete g->variants_run;
    g->variants_run = nullptr;
}

// dst += src, two whole pileup tables of `bytes` bytes; the current device is dst's, `stream` one of its streams, waited for before the return.
// On one device one kernel; across devices -- or whenever the test hook names a piece size -- through `stage`, a piece of at most 64 MiB at a time
static int variants_table_add(uint32_t* dst, int dst_device, const uint32_t* src, int src_device, uint64_t bytes, DevBuf& stage, uint32_t num_cus, hipStream_t stream, const char* who) {
    const int64_t hook = bgr::opt("test.variants_stage_bytes");
    hipError_t e;
    if (dst_device == src_device && hook == 0) {
        e = bgr::launch_pileup_add(dst, src, bytes / 4, true, num_cus, stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_pileup_add_kernel): " + hipGetErrorString(e));
    } else {
        uint64_t piece = hook > 0 ? ((uint64_t)hook + 15) / 16 * 16 : (64ull << 20);
        if (piece > (64ull << 20)) piece = 64ull << 20;
        if (piece > bytes) piece = (bytes + 15) / 16 * 16;
        e = stage.ensure(piece);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorOutOfMemory ? BGR_E_NOMEM : BGR_E_HIP, std::string(who) + ": the staging piece of a table from another device: " + hipGetErrorString(e)); }
        for (uint64_t off = 0; off < bytes; off += piece) {   // (the pieces follow each other on one stream: the copy of the next waits for the add of this one)
            const uint64_t len = bytes - off < piece ? bytes - off : piece;
            if (dst_device == src_device) HIP_TRY(hipMemcpyAsync(stage.p, reinterpret_cast<const char*>(src) + off, len, hipMemcpyDeviceToDevice, stream));
            else HIP_TRY(hipMemcpyPeerAsync(stage.p, dst_device, reinterpret_cast<const char*>(src) + off, src_device, len, stream));
            e = bgr::launch_pileup_add(dst + off / 4, static_cast<const uint32_t*>(stage.p), len / 4, off + len == bytes, num_cus, stream);
            if (e != hipSuccess) return fail(BGR_E_HIP, std::string(who) + ": kernel launch (bgr_pileup_add_kernel): " + hipGetErrorString(e));
        }
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return BGR_OK;
}

template <class Site>
static int aligner_sites(bgr_aligner* a, const bgr_variant_strand_params* params, Site* out, uint64_t cap, uint64_t* n, const std::string& who) {
    const bool strands = std::is_same<Site, bgr_variant_strand_site>::value;
    if (n) *n = 0;
    if (!a || !params || !n || (cap && !out)) return fail(BGR_E_ARG, who + ": null argument");
    if (a->is_twin) return fail(BGR_E_ARG, who + ": an internal stream of another aligner");
    if (!bgr::variants_params_ok(bgr_variant_params{params->min_depth, params->min_alt, params->min_af_ppm}))
        return fail(BGR_E_ARG, who + ": thresholds out of range (min_depth >= 1, min_alt >= 1, min_af_ppm <= 1000000)");
    if (strands && (!a->sh->pileup.tab || !a->sh->pileup.fwd_tab)) return fail(BGR_E_ARG, who + ": strands were never counted on this aligner (bgr_aligner_pileup_strands_enable)");
    if (!a->sh->pileup.tab) return fail(BGR_E_ARG, who + ": the pileup was never enabled on this aligner (bgr_aligner_pileup_enable)");
    if (const int rc = guarded_sync(a, who.c_str()); rc != BGR_OK) return rc;
    return variants_call<Site>(a->dg, a->graph, a->sh->pileup.tab, a->sh->pileup.fwd_tab, a->sh->pileup.base_offs, *params, a->var.scratch, a->var.out, a->stream, who.c_str(), nullptr, out, cap, n,
                               a->sh->knob_no_events ? nullptr : a->var_ms);
}
int bgr_aligner_pileup_sites(bgr_aligner* a, const bgr_variant_params* params, bgr_variant_site* out, uint64_t cap, uint64_t* n) {
    const bgr_variant_strand_params sp = {params ? params->min_depth : 0, params ? params->min_alt : 0, params ? params->min_af_ppm : 0, 0};
    return aligner_sites(a, params ? &sp : nullptr, out, cap, n, "bgr_aligner_pileup_sites");
}
int bgr_aligner_pileup_strand_sites(bgr_aligner* a, const bgr_variant_strand_params* params, bgr_variant_strand_site* out, uint64_t cap, uint64_t* n) {
    return aligner_sites(a, params, out, cap, n, "bgr_aligner_pileup_strand_sites");
}

int bgr_aligner_pileup_sites_times(bgr_aligner* a, double ms[5]) {
    if (!a || !ms) return fail(BGR_E_ARG, "bgr_aligner_pileup_sites_times: null argument");
    for (int i = 0; i < 5; ++i) ms[i] = a->var_ms[i];
    return BGR_OK;
}

int bgr_aligner_pileup_add(bgr_aligner* dst, bgr_aligner* src) {
    if (!dst || !src) return fail(BGR_E_ARG, "bgr_aligner_pileup_add: null aligner");
    if (dst->is_twin || src->is_twin) return fail(BGR_E_ARG, "bgr_aligner_pileup_add: an internal stream of another aligner");
    if (dst == src || dst->graph != src->graph) return fail(BGR_E_ARG, "bgr_aligner_pileup_add: two different aligners of one graph are needed");
    if (!dst->sh->pileup.tab || !src->sh->pileup.tab) return fail(BGR_E_ARG, "bgr_aligner_pileup_add: the pileup was never enabled on one of the aligners (bgr_aligner_pileup_enable)");
    if (!dst->sh->pileup.fwd_tab != !src->sh->pileup.fwd_tab)
        return fail(BGR_E_ARG, "bgr_aligner_pileup_add: one of the aligners has a forward table (bgr_aligner_pileup_strands_enable) and the other has none");
    if (const int rc = sync_all(src); rc != BGR_OK) return rc;
    if (const int rc = sync_all(dst); rc != BGR_OK) return rc;   // (the current device is dst's from here on)
    const uint64_t bytes = bgr::pileup_table_bytes(dst->graph->header.total_bases / 2, dst->graph->header.n_unitigs);
    const int rc = variants_table_add(dst->sh->pileup.tab, dst->device, src->sh->pileup.tab, src->device, bytes, dst->var.stage, (uint32_t)dst->num_cus, dst->stream, "bgr_aligner_pileup_add");
    if (rc != BGR_OK || !dst->sh->pileup.fwd_tab) return rc;
    return variants_table_add(dst->sh->pileup.fwd_tab, dst->device, src->sh->pileup.fwd_tab, src->device, bytes, dst->var.stage, (uint32_t)dst->num_cus, dst->stream, "bgr_aligner_pileup_add");
}

// a run's aligner, its streams idle from here on: the first one's table becomes the run's (the buffers move: nothing is allocated), the others' are added
int variants_collect(bgr_graph* g, bgr_aligner* a) {
    if (!a->sh->pileup.tab) return fail(BGR_E_ARG, "bgr_align_all: the pileup was never enabled on an aligner of the run");
    const bool strands = g->variants_strands_on;   // the forward table travels with the total one
    if (strands && !a->sh->pileup.fwd_tab) return fail(BGR_E_ARG, "bgr_align_all: strands were never counted on an aligner of the run");
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;
    std::lock_guard<std::mutex> l(g->abundance_m);   // (the lanes of a split run end side by side: one at a time here)
    if (!g->variants_run) {
        VariantsRun* r = new VariantsRun();
        r->device = a->device; r->num_cus = a->num_cus; r->dg = a->dg;
        if (hipStreamCreate(&r->stream) != hipSuccess) { delete r; (void)hipGetLastError(); return fail(BGR_E_HIP, "bgr_align_all: a stream for the run's pileup table"); }
        PileupTables& t = a->sh->pileup;   // (the aligner's twins read the same block: the tables are gone for them too)
        std::swap(r->table, t.table);
        std::swap(r->offs, t.offs);
        if (strands) { std::swap(r->table_fwd, t.fwd); t.fwd_tab = nullptr; t.strands_on = false; }
        t.tab = nullptr; t.base_offs = nullptr; t.on = false;
            g->variants_run = r;
        return BGR_OK;
    }
    VariantsRun* r = g->variants_run;
    HIP_TRY(hipSetDevice(r->device));
    const uint64_t bytes = bgr::pileup_table_bytes(g->header.total_bases / 2, g->header.n_unitigs);
    const int rc = variants_table_add(static_cast<uint32_t*>(r->table.p), r->device, a->sh->pileup.tab, a->device, bytes, r->stage, (uint32_t)r->num_cus, r->stream, "bgr_align_all");
    if (rc != BGR_OK || !strands) return rc;
    if (!r->table_fwd.p) return fail(BGR_E_INTERNAL, "bgr_align_all: the run's pileup table has no forward table");
    return variants_table_add(static_cast<uint32_t*>(r->table_fwd.p), r->device, a->sh->pileup.fwd_tab, a->device, bytes, r->stage, (uint32_t)r->num_cus, r->stream, "bgr_align_all");
}
// the run's end: behind the guard of the summed abundance the passes run once on the run's table; the table is freed whatever happens
int variants_end(bgr_graph* g, bool ok) {
    std::lock_guard<std::mutex> l(g->abundance_m);
    int rc = BGR_OK;
    if (ok) {
        rc = g->abundance_valid ? pileup_guard(g->abundance.data(), g->abundance.size(), "bgr_align_all") : fail(BGR_E_INTERNAL, "bgr_align_all: sites without the abundance totals that guard them");
        if (rc == BGR_OK && g->variants_run) {
            VariantsRun* r = g->variants_run;
            DevBuf scratch, outbuf;
            uint64_t n = 0;
            const bgr_variant_strand_params sp = {g->variants_prm.min_depth, g->variants_prm.min_alt, g->variants_prm.min_af_ppm, g->variants_min_alt_strand};
            if (hipSetDevice(r->device) != hipSuccess) rc = fail(BGR_E_HIP, "bgr_align_all: hipSetDevice for the run's pileup table");
            else if (!g->variants_strands_on)
                rc = variants_call<bgr_variant_site>(r->dg, g, static_cast<const uint32_t*>(r->table.p), nullptr, static_cast<const uint64_t*>(r->offs.p), sp, scratch, outbuf, r->stream,
                                                     "bgr_align_all", &g->variants_sites, nullptr, 0, &n, nullptr);
            else if (!r->table_fwd.p) rc = fail(BGR_E_INTERNAL, "bgr_align_all: the run's pileup table has no forward table");
            else {
                rc = variants_call<bgr_variant_strand_site>(r->dg, g, static_cast<const uint32_t*>(r->table.p), static_cast<const uint32_t*>(r->table_fwd.p), static_cast<const uint64_t*>(r->offs.p), sp,
                                                            scratch, outbuf, r->stream, "bgr_align_all", &g->variants_strand_sites, nullptr, 0, &n, nullptr);
                if (rc == BGR_OK) {   // (bgr_graph_variants then delivers the same sites without the forward numbers)
                    g->variants_sites.resize(g->variants_strand_sites.size());
                    for (size_t i = 0; i < g->variants_sites.size(); ++i) memcpy(&g->variants_sites[i], &g->variants_strand_sites[i], sizeof(bgr_variant_site));
                }
            }
            scratch.release(); outbuf.release();
        }
    }
    variants_run_free(g);
    if (!ok || rc != BGR_OK) { g->variants_sites.clear(); g->variants_sites.shrink_to_fit(); g->variants_strand_sites.clear(); g->variants_strand_sites.shrink_to_fit(); }
    g->variants_called = g->variants_prm;
    g->variants_called_strand = g->variants_min_alt_strand;
    g->variants_valid = ok && rc == BGR_OK;
    g->variants_strands_valid = g->variants_valid && g->variants_strands_on;
    return rc;
}

int bgr_graph_variants_enable(bgr_graph* g, const bgr_variant_params* params) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_variants_enable: null graph");
    if (params) {
        if (!bgr::variants_params_ok(*params)) return fail(BGR_E_ARG, "bgr_graph_variants_enable: thresholds out of range (min_depth >= 1, min_alt >= 1, min_af_ppm <= 1000000)");
        int rc = pileup_refusal(g, "bgr_graph_variants_enable");
        if (rc == BGR_OK) rc = graph_base_offs(g, "bgr_graph_variants_enable");
        if (rc != BGR_OK) return rc;
        g->variants_prm = *params;
    }
    g->variants_on = params != nullptr;
    g->variants_strands_on = false;   // (the plain switch: 32-byte records, no forward table)
    return BGR_OK;
}

int bgr_graph_variants_strands_enable(bgr_graph* g, const bgr_variant_strand_params* params) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_variants_strands_enable: null graph");
    if (!params) return bgr_graph_variants_enable(g, nullptr);
    const bgr_variant_params prm = {params->min_depth, params->min_alt, params->min_af_ppm};
    const int rc = bgr_graph_variants_enable(g, &prm);
    if (rc != BGR_OK) return rc;
    g->variants_strands_on = true;
    g->variants_min_alt_strand = params->min_alt_strand;
    return BGR_OK;
}

int bgr_graph_variants_enabled(const bgr_graph* g) { return g && g->variants_on ? 1 : 0; }

// the sites of the last successful run (sites: null for a null graph); sw: the switch that makes a run call them
template <class Site>
static int graph_sites(const std::vector<Site>* sites, bool valid, Site* out, uint64_t cap, uint64_t* n, const std::string& who, const char* sw) {
    if (n) *n = 0;
    if (!sites || !n || (cap && !out)) return fail(BGR_E_ARG, who + ": null argument");
    if (!valid) return fail(BGR_E_ARG, who + ": no totals -- they are those of the last successful bgr_align_all with " + sw + " on");
    *n = sites->size();
    if (sites->size() > cap) return fail(BGR_E_CAPACITY, who + ": " + std::to_string(sites->size()) + " sites, room for " + std::to_string(cap));
    if (!sites->empty()) memcpy(out, sites->data(), sites->size() * sizeof(Site));
    return BGR_OK;
}
int bgr_graph_variants(const bgr_graph* g, bgr_variant_site* out, uint64_t cap, uint64_t* n) {
    return graph_sites(g ? &g->variants_sites : nullptr, g && g->variants_valid, out, cap, n, "bgr_graph_variants", "bgr_graph_variants_enable");
}
int bgr_graph_variant_strand_sites(const bgr_graph* g, bgr_variant_strand_site* out, uint64_t cap, uint64_t* n) {
    return graph_sites(g ? &g->variants_strand_sites : nullptr, g && g->variants_strands_valid, out, cap, n, "bgr_graph_variant_strand_sites", "bgr_graph_variants_strands_enable");
}

int bgr_graph_variants_params(const bgr_graph* g, bgr_variant_params* out) {
    if (!g || !out) return fail(BGR_E_ARG, "bgr_graph_variants_params: null argument");
    if (!g->variants_valid) return fail(BGR_E_ARG, "bgr_graph_variants_params: no totals -- they are those of the last successful bgr_align_all with bgr_graph_variants_enable on");
    *out = g->variants_called;
    return BGR_OK;
}

template <class Params, class Site>
static int vcf_file(const char* path, const bgr_graph* g, const Params* params, const Site* sites, uint64_t n, const std::string& who,
                    bool (*write)(FILE*, const BgrUnitigMeta*, const uint64_t*, uint64_t, const Params&, const Site*, uint64_t, std::string*)) {
    if (!path || !g || !params || (n && !sites)) return fail(BGR_E_ARG, who + ": null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, who + ": the graph has no host blob (the reference letters are read from it)");
    if (g->header.has_exc) return fail(BGR_E_ARG, who + ": a graph of ACGT-only unitigs is needed (--vcf): the 2-bit store does not spell other characters");
    const BgrUnitigMeta* meta = reinterpret_cast<const BgrUnitigMeta*>(g->host.base() + g->header.off_meta);
    const uint64_t* seq = reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_seq);
    std::string err;
    if (!write(nullptr, meta, seq, g->header.n_unitigs, *params, sites, n, &err)) return fail(BGR_E_ARG, who + ": " + err);   // (the checks alone: no file for sites that are none)
    FILE* f = fopen(path, "wb");
    if (!f) return fail(BGR_E_IO, who + ": cannot open " + path);
    bool ok = write(f, meta, seq, g->header.n_unitigs, *params, sites, n, &err);
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(BGR_E_IO, who + ": write to " + path + " failed");
    return BGR_OK;
}
int bgr_write_vcf(const char* path, const bgr_graph* g, const bgr_variant_params* params, const bgr_variant_site* sites, uint64_t n) {
    return vcf_file(path, g, params, sites, n, "bgr_write_vcf", bgr::vcf_write);
}
int bgr_write_vcf_strands(const char* path, const bgr_graph* g, const bgr_variant_strand_params* params, const bgr_variant_strand_site* sites, uint64_t n) {
    return vcf_file(path, g, params, sites, n, "bgr_write_vcf_strands", bgr::vcf_strands_write);
}

int bgr_parse_min_alt_strand(const char* text, uint32_t* out) {
    if (!text || !out) return fail(BGR_E_ARG, "bgr_parse_min_alt_strand: null argument");
    if (!bgr::parse_min_alt_strand(text, out)) return fail(BGR_E_ARG, std::string("bgr_parse_min_alt_strand: '") + text + "' is no non-negative integer of at most nine digits");
    return BGR_OK;
}

int bgr_parse_af_ppm(const char* text, uint32_t* ppm) {
    if (!text || !ppm) return fail(BGR_E_ARG, "bgr_parse_af_ppm: null argument");
    if (!bgr::parse_af_ppm(text, ppm)) return fail(BGR_E_ARG, std::string("bgr_parse_af_ppm: '") + text + "' is no fraction between 0 and 1 with at most six decimals");
    return BGR_OK;
}

// capi.hip -- implementation of the C-ABI declared in include/bgreat_gpu.h: index, distribution, mapping, batches, the
// asynchronous form, host buffers and readsets (the text route and the counting features have their own units: capi_text.hip, capi_abundance.hip, capi_links.hip, capi_triples.hip,
// capi_pileup.hip, capi_variants.hip; capi_internal.h has what they share).  Thin: argument checks, HIP memory
// and stream management, launch geometry; the algorithm lives in graph_build.cpp (index) and
// the *_kernels.hip files (mapping; launch interface align_kernels.h).  There is no CPU mapping path in this library.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <dlfcn.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bgreat_gpu.h"
#include "abundance_kernels.h"
#include "align_kernels.h"
#include "fanout.h"
#include "fastx.h"
#include "anchor_index.h"
#include "graph_build.h"
#include "launch_plan.h"
#include "launch_taker.h"
#include "links_kernels.h"
#include "triples_kernels.h"
#include "pileup_kernels.h"
#include "read_pack.h"
#include "text_kernels.h"
#include "options.h"
#include "capi_internal.h"
#include "inside_kernels.h"
#include "exhaustive_rows_kernels.h"

namespace bgr {
static thread_local std::string tl_err;
int set_error(int code, const std::string& msg) { tl_err = msg; return code; }  // (`fail` in every unit of the C-ABI, and pipeline.cpp)
}

namespace {

int drain_timers(bgr_aligner* a) {
    if (a->ev_used == 0) return BGR_OK;
    HIP_TRY(hipStreamSynchronize(a->stream));
    for (int i = 0; i < a->ev_used; ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, a->ev[i][0], a->ev[i][a->ev_marks[i]]));
        a->t_ms += ms;
        for (int j = 0; j < a->ev_marks[i]; ++j) {
            HIP_TRY(hipEventElapsedTime(&ms, a->ev[i][j], a->ev[i][j + 1]));
            a->t_slot_ms[j] += ms;
        }
        ++a->t_launches;
    }
    a->ev_used = 0;
    return BGR_OK;
}

}  // namespace

// No single launch whose results could be read again (a batch mapped in pieces, a text piece, a batch in flight): bgr_aligner_fetch finds n = 0, on the aligner itself
void forget_launch(bgr_aligner* a) { a->last_n = 0; a->holder = nullptr; }

extern "C" {

const char* bgr_last_error(void) { return bgr::tl_err.c_str(); }

int bgr_set_option(const char* name, int64_t value) {
    bgr::Option* o = name ? bgr::find_option(name) : nullptr;
    if (!o) return fail(BGR_E_ARG, std::string("bgr_set_option: unknown option '") + (name ? name : "") + "'");
    if (value < o->lo || value > o->hi) return fail(BGR_E_ARG, std::string("bgr_set_option: value out of range for '") + name + "'");
    o->value.store(value, std::memory_order_relaxed);
    return BGR_OK;
}
int bgr_get_option(const char* name, int64_t* value) {
    bgr::Option* o = name ? bgr::find_option(name) : nullptr;
    if (!o || !value) return fail(BGR_E_ARG, std::string("bgr_get_option: unknown option '") + (name ? name : "") + "'");
    *value = o->value.load(std::memory_order_relaxed);
    return BGR_OK;
}
const char* bgr_option_name(uint32_t index, const char** what) {
    size_t n;
    bgr::Option* t = bgr::option_table(&n);
    if (index >= n) return nullptr;
    if (what) *what = t[index].what;
    return t[index].name;
}
void bgr_set_build_threads(uint32_t threads) { bgr::set_build_threads(threads); }

int bgr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- index ------------------------------------------------------------------------------------------
int bgr_graph_build(uint32_t k, uint64_t n_unitigs, const char* seqs, const uint64_t* offsets, double gamma, bgr_graph** out) {
    return bgr_graph_build_ex(k, n_unitigs, seqs, offsets, gamma, 0, out);
}

int bgr_graph_build_ex(uint32_t k, uint64_t n_unitigs, const char* seqs, const uint64_t* offsets, double gamma, uint32_t flags, bgr_graph** out) {
    if (!out || (n_unitigs && (!seqs || !offsets))) return fail(BGR_E_ARG, "bgr_graph_build: null argument");
    if (flags & ~(uint32_t)(BGR_BUILD_ANCHORS | BGR_BUILD_NO_EVICTIONS)) return fail(BGR_E_ARG, "bgr_graph_build: unknown flag");
    bgr_graph* g = new bgr_graph();
    std::string err;
    uint64_t zero[1] = {0};
    if (!bgr::build_graph(k, n_unitigs, seqs, n_unitigs ? offsets : zero, gamma > 0 ? gamma : 0.0, flags, g->host, err)) {
        delete g;
        return fail(BGR_E_ARG, err);
    }
    g->header = *g->host.header();
    if (g->host.jump_buckets) {  // (the graph object's header copy describes the device image: the blob's own header stays as it was)
        g->header.off_jump = g->host.jump_off; g->header.jump_entries = g->host.jump_entries; g->header.jump_buckets = g->host.jump_buckets;
        g->header.jump_stride = g->host.jump_stride; g->header.jump_dropped_x1000 = g->host.jump_dropped_x1000;
    }
    const uint64_t nu = g->header.n_unitigs;  // loading stopped at the first short sequence
    g->ascii.assign(seqs + (nu ? offsets[0] : 0), seqs + (nu ? offsets[nu] : 0));
    g->ascii_offs.resize(nu + 1);
    for (uint64_t i = 0; i <= nu; ++i) g->ascii_offs[i] = nu ? offsets[i] - offsets[0] : 0;
    *out = g;
    return BGR_OK;
}

int bgr_graph_unitigs(const bgr_graph* g, const char** seqs, const uint64_t** offsets, uint64_t* n) {
    if (!g || !seqs || !offsets || !n) return fail(BGR_E_ARG, "bgr_graph_unitigs: null argument");
    if (g->ascii_offs.empty()) return fail(BGR_E_ARG, "bgr_graph_unitigs: this graph was created from a blob and carries no unitig characters");
    *seqs = g->ascii.data();
    *offsets = g->ascii_offs.data();
    *n = g->ascii_offs.size() - 1;
    return BGR_OK;
}

int bgr_graph_build_from_fasta(const char* path, uint32_t k, double gamma, bgr_graph** out) {
    return bgr_graph_build_from_fasta_ex(path, k, gamma, 0, out);
}

int bgr_graph_build_from_fasta_ex(const char* path, uint32_t k, double gamma, uint32_t flags, bgr_graph** out) {
    if (!path || !out) return fail(BGR_E_ARG, "bgr_graph_build_from_fasta: null argument");
    std::vector<char> seqs;
    std::vector<uint64_t> offs;
    std::string err;
    if (!bgr::read_unitig_fasta(path, k, seqs, offs, err)) return fail(BGR_E_IO, err);
    return bgr_graph_build_ex(k, offs.size() - 1, seqs.data(), offs.data(), gamma, flags, out);
}

int bgr_graph_anchor_lookup(const bgr_graph* g, uint64_t kmer, uint64_t* index_out, uint64_t* position_out) {
    if (!g || !index_out) return fail(BGR_E_ARG, "bgr_graph_anchor_lookup: null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_anchor_lookup: graph has no host blob");
    if (!g->header.anc_n) return fail(BGR_E_ARG, "bgr_graph_anchor_lookup: the graph was built without BGR_BUILD_ANCHORS");
    const uint64_t idx = bgr::anchor_lookup(g->host.header(), g->host.base(), kmer);
    *index_out = idx;
    if (position_out) *position_out = idx == ~0ULL ? 0 : reinterpret_cast<const uint64_t*>(g->host.base() + g->header.off_anc_pos)[idx];
    return BGR_OK;
}

int bgr_graph_key_lookup(const bgr_graph* g, uint64_t key, uint32_t* slot_out) {
    if (!g || !slot_out) return fail(BGR_E_ARG, "bgr_graph_key_lookup: null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_key_lookup: graph has no host blob");
    if (g->header.wide_keys) return fail(BGR_E_ARG, "bgr_graph_key_lookup: the graph has two-word keys (k > 32): use bgr_graph_key_lookup_wide");
    *slot_out = bgr::host_lookup(g->host.header(), g->host.base(), key);
    return BGR_OK;
}

int bgr_graph_key_lookup_wide(const bgr_graph* g, uint64_t key_hi, uint64_t key_lo, uint32_t* slot_out) {
    if (!g || !slot_out) return fail(BGR_E_ARG, "bgr_graph_key_lookup_wide: null argument");
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_key_lookup_wide: graph has no host blob");
    *slot_out = bgr::host_lookup_wide(g->host.header(), g->host.base(), key_hi, key_lo);
    return BGR_OK;
}

const void* bgr_graph_blob(const bgr_graph* g, uint64_t* bytes) {
    if (!g || g->host.blob.empty()) { if (bytes) *bytes = 0; return nullptr; }
    if (bytes) *bytes = g->header.blob_bytes;
    return g->host.blob.data();
}

int bgr_graph_from_blob(const void* blob, uint64_t bytes, bgr_graph** out) {
    if (!blob || !out) return fail(BGR_E_ARG, "bgr_graph_from_blob: null argument");
    std::string err;
    if (!bgr::validate_blob(blob, bytes, err)) return fail(BGR_E_ARG, err);
    bgr_graph* g = new bgr_graph();
    if (!g->host.blob.reset((bytes + 7) / 8)) { delete g; return fail(BGR_E_ARG, "bgr_graph_from_blob: out of memory"); }
    memcpy(g->host.blob.data(), blob, bytes);
    g->header = *g->host.header();
    *out = g;
    return BGR_OK;
}

int bgr_graph_info(const bgr_graph* g, bgr_graph_info_t* o) {
    if (!g || !o) return fail(BGR_E_ARG, "bgr_graph_info: null argument");
    const BgrBlobHeader& h = g->header;
    memset(o, 0, sizeof(*o));
    o->k = h.k; o->n_levels = 2; o->n_unitigs = h.n_unitigs; o->n_keys = h.n_placed + h.n_fallback;
    o->n_left_keys = h.n_left_keys; o->n_right_keys = h.n_right_keys; o->n_fallback = h.n_fallback;
    o->total_bases = h.total_bases; o->blob_bytes = h.blob_bytes; o->mphf_bytes = h.n_buckets * 4;
    o->max_unitig_len = h.max_unitig_len; o->has_exceptions = h.has_exc; o->has_anchors = h.anc_n ? 1 : 0; o->gamma = h.gamma;
    o->jump_entries = h.jump_entries; o->jump_bytes = h.jump_buckets * 2 * sizeof(BgrJumpEntry); o->jump_stride = h.jump_stride;
    o->jump_absent = bgr::jump_absent_reason(&h);
    o->jump_dropped_x1000 = h.jump_dropped_x1000;
    return BGR_OK;
}

const void* bgr_graph_jump_index(const bgr_graph* g, uint64_t* bytes) {
    const bool have = g && !g->host.blob.empty() && g->host.jump_buckets;
    if (bytes) *bytes = have ? g->host.jump_buckets * 2 * sizeof(BgrJumpEntry) : 0;
    return have ? g->host.base() + g->host.jump_off : nullptr;
}

void bgr_graph_destroy(bgr_graph* g) {
    if (!g) return;
    for (auto& kv : g->dev) {
        if (kv.second.owned && kv.second.ptr) {
            if (hipSetDevice(kv.first) == hipSuccess) (void)hipFree(kv.second.ptr);
        }
    }
    variants_run_free(g);
    inside_free_devices(g);
    delete g;
}

int bgr_graph_upload(bgr_graph* g, int device) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_upload: null graph");
    if (g->dev.count(device)) return BGR_OK;
    if (g->host.blob.empty()) return fail(BGR_E_ARG, "bgr_graph_upload: graph has no host blob (adopted graphs live on one device)");
    HIP_TRY(hipSetDevice(device));
    void* p = nullptr;
    // (a graph with a jump index: the section behind the blob goes along, and the device copy's header gets its four fields)
    const uint64_t image = g->host.image_bytes();
    HIP_TRY(hipMalloc(&p, image));
    hipError_t e = hipMemcpy(p, g->host.blob.data(), image, hipMemcpyHostToDevice);
    if (e == hipSuccess && g->host.jump_buckets)
        e = hipMemcpy(static_cast<char*>(p) + offsetof(BgrBlobHeader, off_jump), &g->header.off_jump, sizeof(BgrBlobHeader) - offsetof(BgrBlobHeader, off_jump), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (from pageable memory on the null stream; the aligners' streams are non-blocking: the blob is there before any of them starts)
    if (e != hipSuccess) { (void)hipFree(p); return fail(BGR_E_HIP, std::string("blob H2D: ") + hipGetErrorString(e)); }
    g->dev[device] = {p, true};
    return BGR_OK;
}

// ---- one-off distribution of the graph over the GPUs of one process -------------------------------------------------------
// The blob goes from the host to the first device once and from there device to device over xGMI: as ONE RCCL broadcast
// (a communicator per device from ncclCommInitAll; librccl is looked up at run time, so the library has no link-time
// dependency on it), or, when RCCL is not available or refuses, as peer copies in a doubling schedule (1 -> 2 -> 4 -> 8
// holders: every round uses disjoint point-to-point links).
namespace {

struct Rccl {
    typedef int (*CommInitAll_t)(void** comms, int n, const int* devs);
    typedef int (*Group_t)(void);
    typedef int (*Broadcast_t)(const void* send, void* recv, size_t count, int dtype, int root, void* comm, hipStream_t stream);
    typedef int (*CommDestroy_t)(void* comm);
    void* lib = nullptr;
    CommInitAll_t CommInitAll = nullptr;
    Group_t GroupStart = nullptr, GroupEnd = nullptr;
    Broadcast_t Broadcast = nullptr;
    CommDestroy_t CommDestroy = nullptr;
    bool load() {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) return false;
        CommInitAll = reinterpret_cast<CommInitAll_t>(dlsym(lib, "ncclCommInitAll"));
        GroupStart = reinterpret_cast<Group_t>(dlsym(lib, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<Group_t>(dlsym(lib, "ncclGroupEnd"));
        Broadcast = reinterpret_cast<Broadcast_t>(dlsym(lib, "ncclBroadcast"));
        CommDestroy = reinterpret_cast<CommDestroy_t>(dlsym(lib, "ncclCommDestroy"));
        return CommInitAll && GroupStart && GroupEnd && Broadcast && CommDestroy;
    }
};

// ptr[i] on device devs[i]; ptr[0] holds the blob.  false = RCCL not usable here (nothing has been copied, or partly:
// the caller then overwrites with peer copies).
bool fanout_rccl(const std::vector<int>& devs, const std::vector<void*>& ptr, uint64_t bytes, std::string& why) {
    Rccl r;
    if (!r.load()) { why = "librccl not loadable"; return false; }
    const int n = (int)devs.size();
    std::vector<void*> comms(n, nullptr);
    if (r.CommInitAll(comms.data(), n, devs.data()) != 0) { why = "ncclCommInitAll failed"; return false; }
    std::vector<hipStream_t> streams(n, nullptr);
    bool ok = true;
    for (int i = 0; i < n && ok; ++i) ok = hipSetDevice(devs[i]) == hipSuccess && hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking) == hipSuccess;
    if (ok) {
        ok = r.GroupStart() == 0;
        for (int i = 0; i < n && ok; ++i) {
            ok = hipSetDevice(devs[i]) == hipSuccess &&
                 r.Broadcast(ptr[i], ptr[i], (size_t)bytes, /*ncclChar*/ 0, /*root rank*/ 0, comms[i], streams[i]) == 0;
        }
        ok = r.GroupEnd() == 0 && ok;
    }
    for (int i = 0; i < n; ++i) {
        if (streams[i]) { if (hipSetDevice(devs[i]) == hipSuccess) { ok = hipStreamSynchronize(streams[i]) == hipSuccess && ok; (void)hipStreamDestroy(streams[i]); } }
    }
    for (void* c : comms) if (c) (void)r.CommDestroy(c);
    if (!ok) why = "RCCL broadcast failed";
    return ok;
}

// one round of the doubling schedule: concurrent peer copies over disjoint links, complete on return
bool peer_round(const std::vector<bgr::FanoutCopy>& round, uint64_t bytes, std::string& why) {
    std::vector<hipStream_t> streams;
    std::vector<int> sdev;
    bool ok = true;
    for (const bgr::FanoutCopy& c : round) {
        if (hipSetDevice(c.src_dev) != hipSuccess) { ok = false; why = "hipSetDevice failed"; break; }
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, c.src_dev, c.dst_dev) == hipSuccess && can) {
            hipError_t pe = hipDeviceEnablePeerAccess(c.dst_dev, 0);  // direct xGMI path; without it the runtime stages through the host
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { ok = false; why = "hipStreamCreate failed"; break; }
        streams.push_back(st);
        sdev.push_back(c.src_dev);
        hipError_t e = hipMemcpyPeerAsync(c.dst, c.dst_dev, c.src, c.src_dev, bytes, st);
        if (e != hipSuccess) { ok = false; why = std::string("hipMemcpyPeerAsync: ") + hipGetErrorString(e); break; }
    }
    for (size_t j = 0; j < streams.size(); ++j) {  // (also after a failure: nothing may still be writing when the buffers are released)
        if (hipSetDevice(sdev[j]) == hipSuccess) {
            hipError_t e = hipStreamSynchronize(streams[j]);
            if (e != hipSuccess && ok) { ok = false; why = std::string("peer copy: ") + hipGetErrorString(e); }
            (void)hipStreamDestroy(streams[j]);
        }
    }
    return ok;
}

}  // namespace

int bgr_devices_init(bgr_graph* g, int first_device, uint32_t n_devices, uint32_t how) {
    if (!g) return fail(BGR_E_ARG, "bgr_devices_init: null graph");
    if (n_devices == 0) n_devices = 1;
    if (how > BGR_FANOUT_PEER) return fail(BGR_E_ARG, "bgr_devices_init: unknown distribution method");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return fail(BGR_E_HIP, "no HIP device available");
    if (first_device < 0 || (uint64_t)first_device + n_devices > (uint64_t)nd) return fail(BGR_E_ARG, "bgr_devices_init: device range outside the visible devices");
    int rc = bgr_graph_upload(g, first_device);  // host -> first device (idempotent)
    if (rc != BGR_OK) return rc;
    const uint64_t bytes = g->host.image_bytes();  // (the device image: the blob and, behind it, the jump index)
    bgr::FanoutOps ops;
    ops.alloc = [bytes](int dev, void** out) { return hipSetDevice(dev) == hipSuccess && hipMalloc(out, bytes) == hipSuccess; };
    ops.release = [](int dev, void* p) { if (p && hipSetDevice(dev) == hipSuccess) (void)hipFree(p); };
    ops.broadcast = [bytes](const std::vector<int>& devs, const std::vector<void*>& ptr, std::string& why) { return fanout_rccl(devs, ptr, bytes, why); };
    ops.peer_round = [bytes](const std::vector<bgr::FanoutCopy>& round, std::string& why) { return peer_round(round, bytes, why); };
    // (bookkeeping in fanout.h: new buffers are registered only once they hold the blob; after a failure they are released and
    // g->dev is unchanged, so bgr_graph_upload / bgr_aligner_create can still bring the blob to a device on their own)
    std::map<int, void*> resident;
    for (auto& kv : g->dev) resident[kv.first] = kv.second.ptr;
    g->fanout_method = 0;
    const bgr::FanoutResult r = bgr::fanout_blob(first_device, n_devices, how, resident, ops);
    if (!r.error.empty()) return fail(r.hip_error ? BGR_E_HIP : BGR_E_ARG, "bgr_devices_init: " + r.error);
    for (auto& kv : resident) if (!g->dev.count(kv.first)) g->dev[kv.first] = {kv.second, true};
    g->fanout_method = (uint32_t)r.method;
    return BGR_OK;
}

uint32_t bgr_devices_method(const bgr_graph* g) { return g ? g->fanout_method : 0; }

const void* bgr_graph_device_blob(const bgr_graph* g, int device) {
    if (!g) return nullptr;
    auto it = g->dev.find(device);
    return it == g->dev.end() ? nullptr : it->second.ptr;
}

int bgr_graph_adopt_device_blob(int device, const void* dev_blob, uint64_t bytes, bgr_graph** out) {
    if (!dev_blob || !out || bytes < sizeof(BgrBlobHeader)) return fail(BGR_E_ARG, "bgr_graph_adopt_device_blob: bad argument");
    HIP_TRY(hipSetDevice(device));
    bgr_graph* g = new bgr_graph();
    hipError_t e = hipMemcpy(&g->header, dev_blob, sizeof(BgrBlobHeader), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { delete g; return fail(BGR_E_HIP, std::string("header D2H: ") + hipGetErrorString(e)); }
    std::string verr;  // the same checks as for a host blob: the kernels index HBM with these numbers
    if (!bgr::validate_blob_header(&g->header, bytes, verr)) {
        delete g;
        return fail(BGR_E_ARG, "bgr_graph_adopt_device_blob: " + verr);
    }
    g->dev[device] = {const_cast<void*>(dev_blob), false};
    *out = g;
    return BGR_OK;
}

// ---- mapping ----------------------------------------------------------------------------------------
int bgr_aligner_create(bgr_graph* g, int device, bgr_aligner** out) {
    if (!g || !out) return fail(BGR_E_ARG, "bgr_aligner_create: null argument");
    int nd = 0;
    hipError_t e0 = hipGetDeviceCount(&nd);
    if (e0 != hipSuccess || nd == 0) return fail(BGR_E_HIP, "no HIP device available (this library has no CPU mapping path)");
    if (device < 0 || device >= nd) return fail(BGR_E_ARG, "bgr_aligner_create: device index out of range");
    int rc = bgr_graph_upload(g, device);
    if (rc != BGR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    bgr_aligner* a = new bgr_aligner();
    a->graph = g;
    a->device = device;
    a->sh = new AlignerShared();   // (a twin gives its own up for its owner's: twins_setup)
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) { delete a; return fail(BGR_E_HIP, hipGetErrorString(e)); }
    a->num_cus = prop.multiProcessorCount;
    a->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 65536;
    e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete a; return fail(BGR_E_HIP, hipGetErrorString(e)); }
    for (auto& launch : a->ev)
        for (hipEvent_t& ev : launch)
            if (hipEventCreate(&ev) != hipSuccess) { delete a; return fail(BGR_E_HIP, "hipEventCreate failed"); }
    if (a->blocking_sync && hipEventCreateWithFlags(&a->ev_wait, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) a->blocking_sync = false;
    bgr::resolve_device_graph(&g->header, g->dev[device].ptr, a->dg);
    e = a->launch.small.ensure(bgr::kSmallBytes);
    if (e == hipSuccess) e = hipMemset(a->launch.small.p, 0, a->launch.small.cap);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the fill runs on the null stream, which the aligner's non-blocking stream does not wait for)
    if (e != hipSuccess) { delete a; return fail(BGR_E_HIP, hipGetErrorString(e)); }
    *out = a;
    return BGR_OK;
}

void bgr_aligner_destroy(bgr_aligner* a) {
    if (!a) return;
    if (a->text.phase_s[4] > 0 && bgr::opt("timing"))
        fprintf(stderr, "bgreat: text calls %.0f on device %d: to record count %.3f s, records %.3f s, mapping + sizes %.3f s, streams out %.3f s\n", a->text.phase_s[4], a->device,
                a->text.phase_s[0], a->text.phase_s[1], a->text.phase_s[2], a->text.phase_s[3]);
    if (a->twin) { bgr_aligner_destroy(a->twin); a->twin = nullptr; }
    if (hipSetDevice(a->device) == hipSuccess) {
        if (a->stream) (void)hipStreamSynchronize(a->stream);
        a->launch.release(); a->fetch.release(); a->text.release(); a->tag.release(); a->var.release(); a->abundance.release();
        if (!a->is_twin) a->sh->release();   // (the tables every stream added to: the twins' streams are gone)
        for (int i = 0; i < kTimerRing; ++i) for (int j = 0; j <= kTimerSlots; ++j) (void)hipEventDestroy(a->ev[i][j]);
        if (a->ev_wait) (void)hipEventDestroy(a->ev_wait);
        if (a->stream) (void)hipStreamDestroy(a->stream);
    }
    delete a;
}

int bgr_aligner_configure(bgr_aligner* a, uint32_t waves_per_block, uint32_t blocks_per_cu, uint32_t lds_mphf) {
    if (!a || waves_per_block > 16 || lds_mphf > 2) return fail(BGR_E_ARG, "bgr_aligner_configure: bad argument");
    a->sh->cfg_waves = waves_per_block;
    a->sh->cfg_blocks_per_cu = blocks_per_cu;
    a->sh->cfg_lds_mphf = lds_mphf;
    return BGR_OK;
}

// The knobs: where each is kept and what becomes of a value beyond its limit -- refused, the limit instead, or its bits under the limit (the knobs
// without a limit of their own keep 32 bits); `inverted`: kept as "off"
enum class Over { kReject, kClamp, kMask };
struct KnobRule { uint32_t id; uint64_t limit; Over over; uint64_t AlignerShared::*dst; bool inverted; };
static const KnobRule kKnobs[] = {
    {BGR_KNOB_EXH_FRAME_CAP, 1u << 20, Over::kClamp, &AlignerShared::knob_frame_cap, false},
    {BGR_KNOB_EXH_SEARCH, 2, Over::kReject, &AlignerShared::knob_search, false},
    {BGR_KNOB_BATCH_SPLIT_LIMIT, ~0ull, Over::kMask, &AlignerShared::knob_split_limit, false},
    {BGR_KNOB_DEBUG_STOP, 0xFFFFFFFFull, Over::kMask, &AlignerShared::knob_debug_stop, false},
    {BGR_KNOB_BATCH_OVERLAP, 0xFFFFFFFFull, Over::kMask, &AlignerShared::knob_overlap, false},
    {BGR_KNOB_DEVICE_OVERLAP, 0xFFFFFFFFull, Over::kMask, &AlignerShared::knob_device_overlap, false},
    {BGR_KNOB_GREEDY_FAST, 1, Over::kReject, &AlignerShared::knob_greedy_fast, false},
    {BGR_KNOB_EXH_FAST, 1, Over::kReject, &AlignerShared::knob_exh_fast, false},
    {BGR_KNOB_ANCHORS_FAST, 1, Over::kReject, &AlignerShared::knob_anc_fast, false},
    {BGR_KNOB_GREEDY_PREPASS, 1, Over::kReject, &AlignerShared::knob_prepass, false},
    {BGR_KNOB_GREEDY_JUMP, 1, Over::kReject, &AlignerShared::knob_no_jump, false},
    {BGR_KNOB_KERNEL_EVENTS, 1, Over::kReject, &AlignerShared::knob_no_events, true},
    {BGR_KNOB_ABUNDANCE_FORM, 2, Over::kReject, &AlignerShared::knob_abundance_form, false},
    {BGR_KNOB_LINKS_FORM, 2, Over::kReject, &AlignerShared::knob_links_form, false},
    {BGR_KNOB_EXH_MEMO_CAP, 1u << 24, Over::kClamp, &AlignerShared::knob_memo_cap, false},
};

int bgr_aligner_set_knob(bgr_aligner* a, uint32_t knob, uint64_t value) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_set_knob: null aligner");
    for (const KnobRule& r : kKnobs) {
        if (r.id != knob) continue;
        if (value > r.limit) {
            if (r.over == Over::kReject) break;
            value = r.over == Over::kClamp ? r.limit : value & r.limit;
        }
        a->sh->*r.dst = r.inverted ? (value ? 0u : 1u) : value;
        return BGR_OK;
    }
    return fail(BGR_E_ARG, "bgr_aligner_set_knob: unknown knob or value out of range");
}

// What the planner needs of the graph / device / caller's tuning (launch_plan.h)
static bgr::PlanGraph plan_graph_of(const BgrBlobHeader& h) {
    bgr::PlanGraph g;
    g.k = h.k; g.slot_fill_x100 = h.slot_fill_x100; g.table_bytes = (uint32_t)std::min<uint64_t>((uint64_t)h.n_buckets * 4, 0xFFFFFFFFull);
    g.total_bases = h.total_bases; g.n_unitigs = h.n_unitigs; g.n_buckets = h.n_buckets; g.max_unitig_len = h.max_unitig_len;
    g.anc_n = h.anc_n; g.anc_active_levels = h.anc_active_levels; g.has_exc = h.has_exc != 0; g.wide_keys = h.wide_keys != 0;
    return g;
}
static bgr::PlanTuning plan_tuning_of(const bgr_aligner* a) {
    bgr::PlanTuning t;
    t.cfg_waves = a->sh->cfg_waves; t.cfg_blocks_per_cu = a->sh->cfg_blocks_per_cu; t.cfg_lds_mphf = a->sh->cfg_lds_mphf;
    t.frame_cap = a->sh->knob_frame_cap; t.search = a->sh->knob_search; t.memo_cap = a->sh->knob_memo_cap;
    t.no_greedy_fast = a->sh->knob_greedy_fast != 0; t.no_exh_fast = a->sh->knob_exh_fast != 0; t.no_anc_fast = a->sh->knob_anc_fast != 0;
    return t;
}

// The planner by itself, on numbers (no device, no graph object): what tests/test_launch_plan.py sweeps on the CPU.
extern "C" int bgr_plan_launch(const bgr_plan_input* in, bgr_plan_output* out) {
    if (!in || !out) return fail(BGR_E_ARG, "bgr_plan_launch: null argument");
    bgr::PlanGraph g;
    g.k = in->k; g.slot_fill_x100 = in->slot_fill_x100; g.table_bytes = in->table_bytes; g.total_bases = in->graph_bases; g.n_unitigs = in->n_unitigs;
    g.n_buckets = in->table_bytes / 4; g.max_unitig_len = in->max_unitig_len; g.anc_n = in->anchors ? 1 : 0; g.anc_active_levels = in->anchor_levels; g.has_exc = in->has_exceptions != 0;
    g.wide_keys = in->wide_keys != 0;
    bgr::PlanDevice d;
    if (in->num_cus) d.num_cus = in->num_cus;
    if (in->lds_per_cu) d.lds_per_cu = in->lds_per_cu;
    for (uint32_t i = 0; i < bgr::kResidentKernels; ++i) if (in->resident_waves[i]) d.resident[i] = in->resident_waves[i];
    bgr::PlanTuning t;
    t.cfg_waves = in->cfg_waves; t.cfg_blocks_per_cu = in->cfg_blocks_per_cu; t.cfg_lds_mphf = in->cfg_lds_mphf;
    bgr::PlanBatch b;
    b.mode = in->mode; b.max_mismatch = in->max_mismatch; b.partial = in->partial; b.max_read_len = in->max_read_len; b.n_reads = in->n_reads; b.total_bases = in->total_bases;
    const bgr::LaunchPlan P = bgr::plan_launch(g, d, t, b);
    memset(out, 0, sizeof(*out));
    if (P.error) return fail(BGR_E_ARG, P.error);
    auto put = [out](int slot, const bgr::LaunchCfg& c) {
        out->pass[slot] = bgr_plan_pass{1, c.blocks, c.waves_per_block, c.lds_bytes, c.stage_mphf};
    };
    // slot 0: the mode's general kernel, the first pass that maps one read per wave (in a launch that sends every read to the last pass: that pass)
    const uint32_t general = bgr::many_reads_per_wave(P.pass[0].kernel) ? 1 : 0;
    for (uint32_t i = 0; i < P.n_passes; ++i) {
        const bgr::Pass& ps = P.pass[i];
        if (i == general) put(0, ps.cfg);
        switch (ps.kernel) {
            case bgr::KernelId::kGreedyMulti: put(1, ps.cfg); break;
            case bgr::KernelId::kExhaustive4: put(2, ps.cfg); break;
            case bgr::KernelId::kAnchors4: put(3, ps.cfg); break;
            case bgr::KernelId::kExhaustive: if (i != general) put(4, ps.cfg); break;  // (behind the level search)
            case bgr::KernelId::kExhaustiveLast: put(5, ps.cfg); break;
            default: break;
        }
    }
    out->level_search = P.level_search; out->deep_only = P.pass[0].kernel == bgr::KernelId::kExhaustiveLast; out->x4_levels = P.x4_levels; out->memo_cap = P.memo_cap;
    out->deep_scratch_bytes = P.deep_scratch_bytes;
    out->arena_ints = P.arena_cap;
    return BGR_OK;
}

// The buffer of each list of reads a pass leaves to a later one (bgr::List; greedy mode keeps the follow-up items' rings in `ovf`)
static DevBuf* list_buf(bgr_aligner* a, bgr::List l) {
    switch (l) {
        case bgr::List::kSearch: return &a->launch.ovf;
        case bgr::List::kDepthFirst: case bgr::List::kGeneral: return &a->launch.ovf2;
        case bgr::List::kFirst: return &a->launch.lst;
        case bgr::List::kRetry: return &a->launch.retry;
        default: return nullptr;
    }
}

// HIP events on the aligner's stream behind the kernels of a launch (bgr_aligner_kernel_times); timed = false: none
struct LaunchMarks {
    bgr_aligner* a;
    bool timed;
    int marks = 0;
    int launch = -1;   // the launch's place in the ring (-1: the one being queued, a->ev_used; else one whose kernels behind its settling join it)
    hipError_t operator()(const char* name) {
        if (!timed || marks >= kTimerSlots) return hipSuccess;
        a->t_slot_name[marks] = name;
        return hipEventRecord(a->ev[launch < 0 ? a->ev_used : launch][++marks], a->stream);
    }
};

// ---- the kernels behind the passes of a launch --------------------------------------------------------------------------------------------
// What each of them is handed (and queues on a->stream): the rows in a->launch.results / arena, the reads they were mapped from, and the launch's own arena and budget
struct BehindPasses {
    bgr_aligner* a;
    uint64_t arena_cap;
    const uint64_t* read_offs;
    uint64_t n_reads, total_bases;
    bgr::PileupReads reads;      // the read characters where this launch has them
    uint32_t arena_own = 0, max_read_len = 0, max_mismatch = 0;   // (the inside pass)
    const uint2* view = nullptr; // an exhaustive launch (bgr_aligner_exhaustive_paths_enable): its rows without their end offset, a->launch.rows_view
    const uint2* rows() const { return view ? view : a->launch.results.as<uint2>(); }
    const int32_t* arena() const { return a->launch.arena.as<int32_t>(); }
};
// The inside pass (bgr_aligner_inside_enable) over the reads the passes left without an anchor
static hipError_t inside_launch(const BehindPasses& c) {
    bgr_aligner* a = c.a;
    bgr::InsideLaunch il{a->launch.results.as<uint2>(), a->launch.arena.as<int32_t>(), a->launch.small.as<uint32_t>(), (uint32_t)c.arena_cap, c.arena_own, c.read_offs, (uint32_t)c.n_reads,
                         c.max_read_len, c.max_mismatch, c.reads};
    return bgr::launch_inside(a->dg, a->sh->inside_tab, a->sh->inside_slots, il, reinterpret_cast<unsigned long long*>(a->launch.small.as<char>() + bgr::kSmallInside), (uint32_t)a->num_cus, a->stream);
}
// Unitig abundance (bgr_aligner_abundance_enable): one kernel behind the last pass adds this launch's rows to the aligner's table.  Every route
// comes through here once per batch (a fetch into larger buffers after BGR_E_CAPACITY launches nothing), so nothing is counted twice.
// (The kernel is queued before anybody knows how the launch ends: one that fails later -- an arena overflow, found when its cursors are read -- has
// added the rows it did write.  include/bgreat_gpu.h says so: after a failed launch the table is undefined until bgr_aligner_reset_abundance.)
static hipError_t abundance_launch(const BehindPasses& c) {
    return bgr::launch_abundance(c.a->dg, c.a->graph->header.n_unitigs, c.rows(), c.arena(), c.arena_cap, c.read_offs, (uint32_t)c.n_reads, c.a->abundance.as<unsigned long long>(),
                                 abundance_plan_of(c.a, c.n_reads, c.total_bases), c.a->stream);
}
// Links (bgr_aligner_links_enable): likewise one kernel that adds the consecutive pairs of this launch's rows to the aligner's hash table.
static hipError_t links_launch(const BehindPasses& c) {
    const CountTable& t = c.a->sh->links;
    const bgr::LinksPlan lp = bgr::plan_links(t.bound, c.n_reads, (uint32_t)c.a->num_cus, (uint32_t)c.a->sh->knob_links_form);
    return bgr::launch_links(c.a->graph->header.n_unitigs, c.rows(), c.arena(), c.arena_cap, (uint32_t)c.n_reads, t.tab, t.cap, lp, c.a->stream);
}
// Triples (bgr_aligner_triples_enable): likewise one kernel that adds every three consecutive ids of this launch's rows to the aligner's hash table.
static hipError_t triples_launch(const BehindPasses& c) {
    const CountTable& t = c.a->sh->triples;
    return bgr::launch_triples(c.a->graph->header.n_unitigs, c.rows(), c.arena(), c.arena_cap, (uint32_t)c.n_reads, t.tab, t.cap, (uint32_t)c.a->num_cus, c.a->stream);
}
// Pileup (bgr_aligner_pileup_enable): likewise one kernel that adds per-base depth and mismatches, the read characters from `reads`.
static hipError_t pileup_launch(const BehindPasses& c) {
    const PileupTables& t = c.a->sh->pileup;
    const BgrBlobHeader& h = c.a->graph->header;
    return bgr::launch_pileup(c.a->dg, h.n_unitigs, h.total_bases / 2, c.rows(), c.arena(), c.arena_cap, c.read_offs, (uint32_t)c.n_reads, c.reads, t.base_offs, t.tab,
                              t.strands_on ? t.fwd_tab : nullptr, (uint32_t)c.a->num_cus, c.a->stream);
}
// One entry per feature, in stream order.  what: the words of its refusal of an exhaustive launch; kernel: its timer slot (bgr_aligner_kernel_times)
// and its name in the message of a failed launch; writes_rows: it is part of the mapping -- not run over rows that are kept
struct LaunchFeature {
    bool (*on)(const AlignerShared&);
    const char *what, *kernel;
    hipError_t (*launch)(const BehindPasses&);
    bool writes_rows;
};
static const LaunchFeature kBehindPasses[] = {
    {[](const AlignerShared& s) { return s.inside_tab != nullptr; }, "runs the inside pass (bgr_aligner_inside_enable), which writes rows", "bgr_align_inside_kernel", inside_launch, true},
    {[](const AlignerShared& s) { return s.abundance_on; }, "counts unitig abundance (bgr_aligner_abundance_enable), which is defined on the rows", "bgr_abundance_kernel", abundance_launch, false},
    {[](const AlignerShared& s) { return s.links.on; }, "counts links (bgr_aligner_links_enable), which are defined on the rows", "bgr_links_kernel", links_launch, false},
    {[](const AlignerShared& s) { return s.triples.on; }, "counts triples (bgr_aligner_triples_enable), which are defined on the rows", "bgr_triples_kernel", triples_launch, false},
    {[](const AlignerShared& s) { return s.pileup.on; }, "counts a pileup (bgr_aligner_pileup_enable), which is defined on the rows", "bgr_pileup_kernel", pileup_launch, false},
};
// The kernels of the enabled features, queued on the aligner's stream: behind the passes of a mapping launch, and -- option test.count_with_path_stats --
// behind bgr_aligner_path_stats' kernel over whatever rows the buffers hold then (rows_kept, as under option test.keep_rows: the counting kernels alone)
static int queue_behind_passes(const BehindPasses& c, bool rows_kept, LaunchMarks& mark) {
    for (const LaunchFeature& f : kBehindPasses) {
        if (!f.on(*c.a->sh) || (f.writes_rows && rows_kept)) continue;
        const hipError_t e = f.launch(c);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (") + f.kernel + "): " + hipGetErrorString(e));
        HIP_TRY(mark(f.kernel));
    }
    return BGR_OK;
}

// ---- the mapping launch of one batch, in stages ---------------------------------------------------------------------------------------------
// The passes come from plan_launch (launch_plan.h, a pure function of numbers); the stages check, size the buffers and enqueue.
struct LaunchJob {
    bgr_aligner* a;
    const bgr_params* p;
    const void *d_reads, *d_read_offsets;
    uint64_t n_reads, total_bases;
    uint32_t max_read_len;
    bool planes_ready;
    const void* d_src_off;
    uint64_t reads_bytes;
    // what launch_size adds: the plan, what every pass shares, the graph as the passes see it
    bgr::LaunchPlan P;
    bool keep_rows = false, inline_pack = false;
    bgr::BatchIO io{};
    bgr::KernelParams kp{};
    BgrDeviceGraph dg;
};

// What a launch is refused for before anything of the aligner changes
static int launch_refusal(const bgr_aligner* a, const bgr_params* p, uint64_t n_reads, uint32_t max_read_len) {
    if (!a || !p) return fail(BGR_E_ARG, "bgr_align_device: null argument");
    if (p->mode > BGR_MODE_ANCHORS) return fail(BGR_E_ARG, "bgr_align_device: unknown mode");
    if (p->mode == BGR_MODE_ANCHORS && !a->graph->header.anc_n)
        return fail(BGR_E_ARG, "bgr_align_device: BGR_MODE_ANCHORS needs a graph built with BGR_BUILD_ANCHORS");
    if (p->mode != BGR_MODE_GREEDY && a->graph->header.wide_keys)
        return fail(BGR_E_ARG, "bgr_align_device: a graph with k > 32 (two-word keys) maps in greedy mode only; exhaustive mode (-b) needs k <= 32");
    for (const bool writes_rows : {false, true})   // (the counting features first, then the pass that writes rows: the order the refusals have always had)
        for (const LaunchFeature& f : kBehindPasses)   // (bgr_aligner_exhaustive_paths_enable: the counting features read an exhaustive launch through its view; the inside pass writes greedy rows)
            if (f.writes_rows == writes_rows && p->mode == BGR_MODE_EXHAUSTIVE && f.on(*a->sh) && !(a->sh->exhaustive_paths && !f.writes_rows))
                return fail(BGR_E_ARG, std::string("bgr_align_device: this aligner ") + f.what + " of the greedy modes; exhaustive mode (-b) is refused");
    if (a->sh->inside_tab && n_reads && max_read_len > bgr::kInsideMaxReadLen)
        return fail(BGR_E_ARG, "bgr_align_device: this aligner runs the inside pass (bgr_aligner_inside_enable), which takes reads of at most 32 000 characters");
    return BGR_OK;
}

// The plan, the buffers it needs, and what every pass is handed (j.io, j.kp, j.dg)
static int launch_size(LaunchJob& j) {
    bgr_aligner* a = j.a;
    const bgr_params* p = j.p;
    const uint64_t n_reads = j.n_reads;
    HIP_TRY(a->launch.results.ensure(n_reads * 8));
    if (!a->plan_dev_known) {
        a->plan_dev.num_cus = (uint32_t)a->num_cus;
        a->plan_dev.lds_per_cu = a->lds_per_cu;
        for (uint32_t k = 0; k < bgr::kResidentKernels; ++k) a->plan_dev.resident[k] = bgr::resident_waves_per_cu(static_cast<bgr::KernelId>(k));
        a->plan_dev_known = true;
    }
    bgr::PlanBatch pb;
    pb.mode = p->mode; pb.max_mismatch = p->max_mismatch; pb.partial = p->partial; pb.max_read_len = j.max_read_len;
    pb.n_reads = n_reads; pb.total_bases = j.total_bases;
    pb.inside = a->sh->inside_tab != nullptr;   // (2 more arena ints per read: the rows of the inside pass)
    j.P = bgr::plan_launch(plan_graph_of(a->graph->header), a->plan_dev, plan_tuning_of(a), pb);
    const bgr::LaunchPlan& P = j.P;
    if (P.error) return fail(BGR_E_ARG, P.error);
    const bgr::Pass& first = P.pass[0];
    if (P.deep_scratch_bytes) HIP_TRY(a->launch.deepbuf.ensure(P.deep_scratch_bytes));
    // test hook (option test.keep_rows): everything of this launch but its mapping passes -- (a->launch.results, a->launch.arena) keep the rows a test wrote there behind
    // a first launch of the same reads, and the counting kernels and the text call's format launches read those.  Only over buffers that launch sized.
    j.keep_rows = bgr::opt("test.keep_rows") != 0;
    if (j.keep_rows && (a->sized_n != n_reads || a->last_arena_cap != P.arena_cap))
        return fail(BGR_E_ARG, "bgr_align_device: option test.keep_rows needs the launch before on this aligner to have had the same n_reads and the same arena");
    HIP_TRY(a->launch.arena.ensure(P.arena_cap * 4));
    a->last_arena_cap = P.arena_cap; a->last_total_bases = j.total_bases;
    a->sized_n = n_reads;
    for (uint32_t i = 0; i < P.n_passes; ++i) {  // the lists the passes leave each other, and the rings of follow-up items of the sixteen-reads-per-wave kernel
        const bgr::Pass& ps = P.pass[i];
        if (ps.appends != bgr::List::kNone) HIP_TRY(list_buf(a, ps.appends)->ensure(n_reads * 4));
        if (ps.kernel == bgr::KernelId::kGreedyMulti) HIP_TRY(a->launch.ovf.ensure((uint64_t)ps.cfg.blocks * ps.cfg.waves_per_block * P.q_cap * 8));
    }
    // (bgr_aligner_launch_info: the first pass; the level search ran unless every read went to the last pass)
    a->last_launch[0] = first.cfg.blocks; a->last_launch[1] = first.cfg.waves_per_block * 64; a->last_launch[2] = first.cfg.lds_bytes;
    a->last_launch[3] = first.cfg.stage_mphf | (P.level_search && first.kernel != bgr::KernelId::kExhaustiveLast ? 2u : 0u) | (bgr::many_reads_per_wave(first.kernel) ? 4u : 0u);

    // A launch handed ASCII reads maps them straight from the characters: the mapping kernels stage each read's 2-bit words themselves (round 5:
    // the pre-pass was 4-11 % of a launch and existed only to write 40 B per read that the next kernel read back).  BGR_KNOB_GREEDY_PREPASS 1 = the
    // pre-pass over the ASCII bytes and 2-bit planes as in rounds 2-4 (what bgr_align_batch_packed's host-packed planes still use)
    // (greedy and exhaustive mode: their several-reads-per-wave kernels stage their groups, the one-read-per-wave kernels go through load_packed.  Anchors
    // mode keeps the pre-pass: its four-reads-per-wave kernel -- BooPHF arithmetic at 96 VGPRs -- lost more inside than the pre-pass cost: 934 vs 965-1 000 Mreads/s)
    // ... and so do launches without a several-reads-per-wave pass (-i, budgets beyond 254, exception planes, the knobs): the one-read-per-wave kernels alone are
    // faster from planes (depth-first 11.8 vs 12.8 ms per 5 M reads, level search 14.0 vs 14.3 per 2 M)
    j.inline_pack = (first.kernel == bgr::KernelId::kGreedyMulti || first.kernel == bgr::KernelId::kExhaustive4) && !j.planes_ready && j.d_reads && !a->sh->knob_prepass;
    if (!j.reads_bytes) j.reads_bytes = j.total_bases;  // (reads end to end: the buffer holds exactly their bases)
    if (!j.inline_pack) {
        HIP_TRY(a->launch.pk_fw3.ensure(P.plane_words * 8));
        HIP_TRY(a->launch.pk_nm.ensure(P.plane_words * 8));
        HIP_TRY(a->launch.pk_hasn.ensure((n_reads + 31) / 32 * 4 + 4));
    }
    bgr::BatchIO& io = j.io;  // (the loop over the passes sets the rest)
    io.ascii = j.inline_pack ? static_cast<const uint8_t*>(j.d_reads) : nullptr;
    io.ascii_src = j.inline_pack ? static_cast<const uint32_t*>(j.d_src_off) : nullptr;
    io.ascii_bytes = j.reads_bytes;
    io.fw3 = a->launch.pk_fw3.as<uint64_t>(); io.nmw = a->launch.pk_nm.as<uint64_t>(); io.hasn = a->launch.pk_hasn.as<uint32_t>();
    io.read_offs = static_cast<const uint64_t*>(j.d_read_offsets);
    io.n_reads = (uint32_t)n_reads;
    io.results = a->launch.results.as<uint2>(); io.arena = a->launch.arena.as<int32_t>(); io.cursor = a->launch.small.as<uint32_t>();
    io.path_cap = P.path_cap; io.arena_cap = (uint32_t)P.arena_cap; io.arena_chunk = P.arena_chunk;
    io.arena_own = (uint32_t)P.arena_own;  // (< 2^32: plan_launch refuses a launch whose arena is larger)
    io.deep_stride = (uint32_t)P.deep_stride; io.deep_memo_cap = P.memo_cap;
    io.search_iters = P.search_iters; io.wide_scan = P.wide_scan ? 1u : 0u; io.task_ctr = bgr::kCurTasks;
    j.kp = {p->max_mismatch, p->effort, p->partial, p->mode, (uint32_t)a->sh->knob_debug_stop};
    // the filter in front of a large key table pays where many read positions are probed per anchor (greedy scans: chr1-scale graph
    // 1 020 -> 1 184 Mreads/s, L2 requests per read 135 -> 28).  The exhaustive scan meets its first hit within a few positions; with
    // fingerprints behind it the filter cost it more than it saved (4-allele graph: 697 without, 664 with), with the bucket's keys compared
    // directly behind it, it pays there too (4-allele graph 702 -> 720, chr1-scale graph 1 111 -> 1 231): on by default for the minimizer
    // kind (option exh_filter = 0: without); the one-hash kind of short k stays off in exhaustive mode
    j.dg = a->dg;
    if (p->mode == BGR_MODE_EXHAUSTIVE && !(j.dg.filter_kind == BGR_FILTER_MINIMIZER && a->sh->exh_filter)) j.dg.bloom = nullptr;
    return BGR_OK;
}

// The pre-pass, where the launch needs the 2-bit planes made, and the passes, back to back on the stream.  A pass behind a list maps what an earlier
// pass listed; with an empty list its waves exit at once (no host round trip in between).  The sixteen-reads-per-wave kernel works off the follow-up
// items of its reads (the next anchors of a read whose first ones failed, then its reverse complement: alignerGreedy.cpp:41-56) in its own per-wave
// queues, inside the launch.
static int launch_passes(const LaunchJob& j, LaunchMarks& mark) {
    bgr_aligner* a = j.a;
    const bgr::LaunchPlan& P = j.P;
    hipError_t e = hipSuccess;
    if (!j.planes_ready && !j.inline_pack) {
        HIP_TRY(hipMemsetAsync(a->launch.pk_hasn.p, 0, (j.n_reads + 31) / 32 * 4, a->stream));
        const uint8_t* reads = static_cast<const uint8_t*>(j.d_reads);
        uint64_t *fw3 = a->launch.pk_fw3.as<uint64_t>(), *nmw = a->launch.pk_nm.as<uint64_t>();
        uint32_t* hasn = a->launch.pk_hasn.as<uint32_t>();
        e = j.d_src_off ? bgr::launch_pack_reads_at(reads, static_cast<const uint32_t*>(j.d_src_off), j.io.read_offs, j.io.n_reads, j.reads_bytes, j.total_bases, fw3, nmw, hasn, a->stream)
                        : bgr::launch_pack_reads(reads, j.io.read_offs, j.io.n_reads, j.total_bases, fw3, nmw, hasn, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("pre-pass launch: ") + hipGetErrorString(e));
        HIP_TRY(mark("bgr_pack_reads_kernel"));
    }
    for (uint32_t i = 0; i < (j.keep_rows ? 0u : P.n_passes); ++i) {
        const bgr::Pass& ps = P.pass[i];
        bgr::BatchIO pio = j.io;
        pio.words_per_read = ps.words;
        pio.frames_per_wave = ps.frames;
        pio.subset = ps.maps == bgr::List::kNone ? nullptr : static_cast<const uint32_t*>(list_buf(a, ps.maps)->p);
        pio.subset_ctr = bgr::list_word(ps.maps);
        uint32_t* appends = ps.appends == bgr::List::kNone ? nullptr : static_cast<uint32_t*>(list_buf(a, ps.appends)->p);
        if (ps.kernel == bgr::KernelId::kGreedyMulti) {
            pio.queue = a->launch.ovf.as<uint2>();
            pio.q_cap = P.q_cap;
            pio.gen_list = appends;
            pio.gen_ctr = bgr::list_word(ps.appends);
        } else {
            pio.ovf_list = appends;
            pio.ovf_ctr = bgr::list_word(ps.appends);
        }
        if (ps.kernel == bgr::KernelId::kExhaustiveLast) pio.deep_scratch = a->launch.deepbuf.as<uint32_t>();
#ifdef BGR_PHASE_TIMING
        if (ps.kernel == bgr::KernelId::kGreedyMulti || ps.kernel == bgr::KernelId::kExhaustive4) {  // time stamps per wave (the greedy kernel: then its scan counts)
            const uint64_t waves = (uint64_t)ps.cfg.blocks * ps.cfg.waves_per_block, bytes = waves * (ps.kernel == bgr::KernelId::kGreedyMulti ? 64 : 32);
            HIP_TRY(a->launch.wave_times.ensure(bytes));
            if (ps.kernel == bgr::KernelId::kGreedyMulti) HIP_TRY(hipMemsetAsync(a->launch.wave_times.p, 0, bytes, a->stream));  // (waves with no reads write nothing)
            pio.wave_times = a->launch.wave_times.as<unsigned long long>();
            a->wave_times_n = waves;
        }
#endif
        // the staged sixteen-reads-per-wave greedy kernel jumps over verified unitig interiors when the graph has the index for it (graph_layout.h):
        // a flag says so, and the kernel finds the section through the blob's header (BgrDeviceGraph must not grow: the kernel is short of
        // SGPRs).  No other kernel is told.  BGR_KNOB_GREEDY_JUMP 1: not this one either.
        BgrDeviceGraph dgp = j.dg;
        if (ps.kernel == bgr::KernelId::kGreedyMulti && ps.cfg.stage_mphf && a->graph->header.jump_buckets && !a->sh->knob_no_jump) dgp.flags |= BGR_GF_JUMP;
        e = bgr::launch_align(ps.kernel, ps.variant, dgp, pio, j.kp, ps.cfg, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (") + ps.name + "): " + hipGetErrorString(e));
        HIP_TRY(mark(ps.name));
        if (ps.kernel == bgr::KernelId::kExhaustiveLast) {  // what settle_launch needs to run the last pass again for the reads it handed back
            a->deep.open = true;
            a->deep.pass = ps; a->deep.io = pio; a->deep.kp = j.kp; a->deep.dg = j.dg;
            a->deep.per_wave_lds = bgr::deep_lds_bytes_per_wave(j.max_read_len);
            a->deep.path_cap = P.path_cap; a->deep.memo_cap = P.memo_cap;
            a->deep.runs = 1;
        }
    }
    return BGR_OK;
}

// Behind the last pass: the inside pass, then the counting kernels (kBehindPasses) -- in stream order in front of everything that reads the rows -- with the
// read characters where this launch has them: the ASCII bytes when the mapping kernels packed them themselves, else the 2-bit planes (host-packed or pre-pass)
// An exhaustive launch (bgr_aligner_exhaustive_paths_enable; without the switch launch_refusal has left no feature on): its last pass writes no row for a read
// it hands back, and settle_launch maps those again -- the rows are final, and every read is counted exactly once, only behind that.  So nothing is queued
// here: what the counting kernels are handed is kept in a->deep_count, and settle_launch queues the view kernel and them (count_settled).
static int launch_behind_passes(const LaunchJob& j, LaunchMarks& mark) {
    BehindPasses c{j.a, j.P.arena_cap, j.io.read_offs, j.n_reads, j.total_bases, {}, j.io.arena_own, j.max_read_len, j.p->max_mismatch};
    if (j.inline_pack) { c.reads.ascii = static_cast<const uint8_t*>(j.d_reads); c.reads.src_off = static_cast<const uint32_t*>(j.d_src_off); c.reads.ascii_bytes = j.reads_bytes; }
    else { c.reads.fw3 = j.io.fw3; c.reads.nmw = j.io.nmw; c.reads.hasn = j.io.hasn; }
    if (j.p->mode != BGR_MODE_EXHAUSTIVE) return queue_behind_passes(c, j.keep_rows, mark);
    bool counting = false;
    for (const LaunchFeature& f : kBehindPasses) counting = counting || (!f.writes_rows && f.on(*j.a->sh));
    if (!counting) return BGR_OK;
    HIP_TRY(j.a->launch.rows_view.ensure(j.n_reads * 8));
    bgr_aligner::DeepCount& C = j.a->deep_count;
    C.open = true;
    C.arena_cap = c.arena_cap; C.n_reads = c.n_reads; C.total_bases = c.total_bases; C.read_offs = c.read_offs; C.reads = c.reads;
    C.ev_launch = -1; C.marks = 0;   // (align_device_impl sets them once the launch has its place in the ring)
    return BGR_OK;
}

// The mapping launch of one batch.  planes_ready: the aligner's 2-bit planes (pk_fw3 / pk_nm / pk_hasn) already hold the batch
// (bgr_align_batch_packed copied them in); else they are made from the ASCII reads at d_reads by the pre-pass.
// d_src_off (may be null): where each read's characters start in d_reads when they lie scattered in a text (text route); reads_bytes: bytes of d_reads.
int align_device_impl(bgr_aligner* a, const bgr_params* p, const void* d_reads, const void* d_read_offsets, uint64_t n_reads,
                             uint64_t total_bases, uint32_t max_read_len, bool planes_ready, const void* d_src_off = nullptr, uint64_t reads_bytes = 0,
                             bool cursor_is_zero = false) {
    if (const int rc = launch_refusal(a, p, n_reads, max_read_len); rc != BGR_OK) return rc;
    // an exhaustive launch whose counting is still to come (bgr_aligner_exhaustive_paths_enable) is settled and counted before its buffers are written again
    if (a->deep_count.open) { if (const int rc = settle_pending(a); rc != BGR_OK) return rc; }
    a->view_ready = false;
    a->holder = nullptr;   // (a launch on the aligner's own stream and buffers; bgr_align_device names the twin behind this call when that took it)
    a->last_n = n_reads; a->last_mode = p->mode;
    a->deep.open = false; a->deep.runs = 0; a->deep.memo_cap = 0;
    if (n_reads == 0) return BGR_OK;
    if ((!d_reads && !planes_ready) || !d_read_offsets) return fail(BGR_E_ARG, "bgr_align_device: null device buffer");
    if (n_reads >= 0xFFFFFFFFull) return fail(BGR_E_ARG, "bgr_align_device: more than 2^32-2 reads in one batch");
    HIP_TRY(hipSetDevice(a->device));
    if (a->ev_used == kTimerRing) { int rc = drain_timers(a); if (rc != BGR_OK) return rc; }
    LaunchJob j{a, p, d_reads, d_read_offsets, n_reads, total_bases, max_read_len, planes_ready, d_src_off, reads_bytes};
    if (const int rc = launch_size(j); rc != BGR_OK) return rc;
    // the cursor block: arena cursor, overflow flag, list counts (the text form: the parse launch cleared it)
    if (!cursor_is_zero) HIP_TRY(hipMemsetAsync(a->launch.small.p, 0, bgr::kCurWords * 4, a->stream));
    // HIP events on the aligner's stream: one in front of the launch, one behind every kernel of it (bgr_aligner_kernel_times)
    // (timing a kernel is not free: the events make the runtime dispatch with completion stamps and keep the kernels of a launch apart -- three events around two
    // kernels cost a 262 144-read launch 16 of its 167 us, 1 730 -> 1 560 Mreads/s, and stamps taken by the dispatch packets themselves (hipExtLaunchKernelGGL)
    // cost the same, profiles/r05_mode_by_batch_size.txt; BGR_KNOB_KERNEL_EVENTS 0: none -- bgr_align_all without its timing option)
    const bool timed = !a->sh->knob_no_events;
    LaunchMarks mark{a, timed};
    if (timed) HIP_TRY(hipEventRecord(a->ev[a->ev_used][0], a->stream));
    if (const int rc = launch_passes(j, mark); rc != BGR_OK) return rc;
    if (const int rc = launch_behind_passes(j, mark); rc != BGR_OK) return rc;
    if (timed) {
        if (a->deep_count.open) { a->deep_count.ev_launch = a->ev_used; a->deep_count.marks = mark.marks; }   // (count_settled times its kernels as this launch's)
        a->ev_marks[a->ev_used] = mark.marks;
        ++a->ev_used;
    }
    return BGR_OK;
}

// The view of the rows in a->launch.results (exhaustive_rows_kernels.h), queued on the aligner's stream
int view_launch(bgr_aligner* a, uint64_t n_reads, uint64_t arena_cap) {
    HIP_TRY(a->launch.rows_view.ensure(n_reads * 8));
    const hipError_t e = bgr::launch_exhaustive_rows(a->launch.results.as<uint2>(), (uint32_t)n_reads, arena_cap, a->launch.rows_view.as<uint2>(), a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (bgr_exhaustive_rows_kernel): ") + hipGetErrorString(e));
    return BGR_OK;
}

// Behind a settled exhaustive launch whose counting waited for that (a->deep_count): the view of its rows, now final, then the counting kernels over the view.
// Timed as kernels of that launch while it is the ring's newest entry: one slot for the host's wait in between, one for the view kernel, one per feature.
static int count_settled(bgr_aligner* a) {
    bgr_aligner::DeepCount& C = a->deep_count;
    if (!C.open) return BGR_OK;
    C.open = false;   // (whatever happens below: nothing is counted twice)
    const bool timed = C.ev_launch >= 0 && C.ev_launch == a->ev_used - 1;
    LaunchMarks mark{a, timed, C.marks, C.ev_launch};
    HIP_TRY(mark("settle_launch (host)"));
    if (const int rc = view_launch(a, C.n_reads, C.arena_cap); rc != BGR_OK) return rc;
    HIP_TRY(mark("bgr_exhaustive_rows_kernel"));
    a->view_ready = true;
    BehindPasses c{a, C.arena_cap, C.read_offs, C.n_reads, C.total_bases, C.reads};
    c.view = a->launch.rows_view.as<uint2>();
    const int rc = queue_behind_passes(c, true, mark);
    if (timed) a->ev_marks[C.ev_launch] = mark.marks;
    return rc;
}

// Behind a mapping launch, with its stream waited for and the cursor block on the host (`cur`): the arena must not have overflowed, and in
// exhaustive mode the last pass may have handed reads back whose table of remembered calls filled up (exh_memo, exhaustive_kernels.hip):
// those run again -- the last pass only, over that list -- with a table sixteen times as large and as few waves as the list has reads, until
// none is left.  A search visits at most positions x halves x 2 nodes, so this ends; what can end it early is the device's memory.
int settle_launch(bgr_aligner* a, uint32_t* cur) {
    if (cur[bgr::kCurOverflow]) return fail(BGR_E_INTERNAL, "path arena overflow (internal sizing error)");
    if (!a->deep.open) return count_settled(a);   // (a launch whose passes were not run: option test.keep_rows)
    const uint32_t kRetry = bgr::list_word(bgr::List::kRetry);
    while (cur[kRetry]) {
        const uint32_t n_retry = cur[kRetry];
        auto& D = a->deep;
        if (D.runs >= bgr::kDeepRuns || D.memo_cap >= (1u << 28))
            return fail(BGR_E_NOMEM, "exhaustive search: a read's table of remembered calls outgrew 2^28 entries per wave (8 GiB)");
        D.memo_cap *= 16;
        const uint64_t stride = bgr::deep_scratch_words(D.path_cap, D.pass.frames, D.memo_cap);
        if (stride > 0xFFFFFFFFull) return fail(BGR_E_NOMEM, "exhaustive search: a read's table of remembered calls outgrew the 16 GiB a wave can address");
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const uint64_t room = (uint64_t)free_b + a->launch.deepbuf.cap;
        uint64_t waves = std::min<uint64_t>(n_retry, (uint64_t)D.pass.cfg.blocks * D.pass.cfg.waves_per_block);
        waves = std::min<uint64_t>(waves, std::max<uint64_t>(1, room / 2 / (stride * 4)));
        if (stride * 4 > room - room / 8) return fail(BGR_E_NOMEM, "exhaustive search: not enough device memory for a read's table of remembered calls");
        HIP_TRY(a->launch.deepbuf.ensure(waves * stride * 4));
        // the list handed back becomes the list to map; the kernel appends to the other one
        DevBuf& other = a->launch.retry2;
        HIP_TRY(other.ensure((uint64_t)n_retry * 4));
        bgr::BatchIO io = D.io;
        io.subset = io.ovf_list;
        io.subset_ctr = bgr::kCurRetrySubset;
        io.ovf_list = static_cast<uint32_t*>(other.p);
        io.ovf_ctr = kRetry;
        io.deep_scratch = static_cast<uint32_t*>(a->launch.deepbuf.p);
        io.deep_stride = (uint32_t)stride;
        io.deep_memo_cap = D.memo_cap;
        uint32_t ctr[2] = {0, n_retry};  // the count of the list handed back = 0, the count of the list to map (kCurRetrySubset, the word behind it) = n
        HIP_TRY(hipMemcpyAsync(static_cast<uint32_t*>(a->launch.small.p) + kRetry, ctr, 8, hipMemcpyHostToDevice, a->stream));
        bgr::LaunchCfg cfg = D.pass.cfg;
        cfg.waves_per_block = (uint32_t)std::min<uint64_t>(cfg.waves_per_block, waves);
        cfg.blocks = (uint32_t)std::max<uint64_t>(1, waves / cfg.waves_per_block);
        cfg.lds_bytes = bgr::kLdsFixed + cfg.waves_per_block * D.per_wave_lds;
        hipError_t e = bgr::launch_align(D.pass.kernel, D.pass.variant, D.dg, io, D.kp, cfg, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("kernel launch (last pass, run again): ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(cur, a->launch.small.p, bgr::kCurWords * 4, hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(wait_stream(a));
        if (cur[bgr::kCurOverflow]) return fail(BGR_E_INTERNAL, "path arena overflow (internal sizing error)");
        std::swap(a->launch.retry, a->launch.retry2);  // (D.io.ovf_list names the list the next round maps)
        D.io.ovf_list = io.ovf_list;
        ++D.runs;
    }
    a->deep.open = false;
    return count_settled(a);   // (bgr_aligner_exhaustive_paths_enable: the rows are final -- the counting kernels that waited for this)
}
// ... for callers that have not looked at the cursor yet (exhaustive launches only: nothing to settle otherwise but the arena flag, which every fetch checks)
static int settle_launch_sync(bgr_aligner* a) {
    if (!a->deep.open && !a->deep_count.open) return BGR_OK;
    uint32_t cur[bgr::kCurWords];
    HIP_TRY(hipMemcpyAsync(cur, a->launch.small.p, sizeof(cur), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return settle_launch(a, cur);
}

int settle_pending(bgr_aligner* a) {
    if (!a->deep.open && !a->deep_count.open) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    return settle_launch_sync(a);
}

int last_rows(bgr_aligner* h, const std::string& who, const uint2** rows) {
    *rows = h->launch.results.as<uint2>();
    if (h->last_mode != BGR_MODE_EXHAUSTIVE) return BGR_OK;
    if (!h->sh->exhaustive_paths) return fail(BGR_E_ARG, who + ": the last launch was exhaustive; " + (who == "bgr_aligner_haplotags" ? "rows" : "paths") + " of the greedy modes only");
    if (const int rc = settle_pending(h); rc != BGR_OK) return rc;
    if (!h->view_ready && h->last_n) {
        HIP_TRY(hipSetDevice(h->device));
        if (const int rc = view_launch(h, h->last_n, h->last_arena_cap); rc != BGR_OK) return rc;
        h->view_ready = true;
    }
    *rows = h->launch.rows_view.as<uint2>();
    return BGR_OK;
}

// The aligner's first n_twins twins (a chain a -> twin -> twin's twin ...), created on first use.  A twin reads the aligner's shared block (its
// tuning, knobs, switches, the tables of links, triples and pileup); its abundance table is its own (bgr_aligner_abundance sums them).
static int twins_setup(bgr_aligner* a, unsigned n_twins) {
    bgr_aligner* prev = a;
    for (unsigned t = 0; t < n_twins; ++t, prev = prev->twin) {
        if (!prev->twin) {
            const int rc = bgr_aligner_create(a->graph, a->device, &prev->twin);
            if (rc != BGR_OK) return rc;
            delete prev->twin->sh;
            prev->twin->is_twin = true;
            prev->twin->sh = a->sh;
        }
        if (a->sh->abundance_on) { const int rc = abundance_table(prev->twin); if (rc != BGR_OK) return rc; }   // (one per stream; nothing to do once it exists)
    }
    return BGR_OK;
}

// true / false: nothing queued or running on the aligner's stream
static int stream_idle(bgr_aligner* a, bool* idle) {
    const hipError_t e = hipStreamQuery(a->stream);
    if (e != hipSuccess && e != hipErrorNotReady) return fail(BGR_E_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
    *idle = e == hipSuccess;
    return BGR_OK;
}

// The public form: a greedy / anchors launch that finds the aligner's stream busy -- the caller has not waited for the launch before -- may go to the
// twin (launch_taker.h), whose workgroups then start on the CU slots that the finished workgroups of the launch before free, instead of behind its last
// straggler.  Everything inside the library that copies on a->stream around its launch (batch pieces, begin / wait, the packed and the text form) calls
// align_device_impl and stays on its own stream.  An exhaustive launch stays too: what it has to settle lives in the aligner that launched it.
int bgr_align_device(bgr_aligner* a, const bgr_params* p, const void* d_reads, const void* d_read_offsets, uint64_t n_reads,
                     uint64_t total_bases, uint32_t max_read_len) {
    if (!a || !p) return fail(BGR_E_ARG, "bgr_align_device: null argument");
    bgr_aligner* taker = a;
    if (!a->is_twin && !a->sh->knob_device_overlap && p->mode != BGR_MODE_EXHAUSTIVE && n_reads) {
        HIP_TRY(hipSetDevice(a->device));
        bool primary_idle = true, twin_idle = true;
        int rc = stream_idle(a, &primary_idle);
        if (rc == BGR_OK && !primary_idle && a->twin) rc = stream_idle(a->twin, &twin_idle);
        if (rc != BGR_OK) return rc;
        if (bgr::launch_taker(primary_idle, twin_idle, a->holder != nullptr) == bgr::Taker::kTwin) {
            rc = twins_setup(a, 1);
            if (rc != BGR_OK) return rc;
            taker = a->twin;
        }
    }
    const int rc = align_device_impl(taker, p, d_reads, d_read_offsets, n_reads, total_bases, max_read_len, false);
    if (rc == BGR_OK) a->holder = taker == a ? nullptr : taker;
    return rc;
}

uint64_t bgr_packed_plane_words(uint64_t n_reads, uint64_t total_bases) { return bgr::packed_plane_words(n_reads, total_bases); }

int bgr_pack_reads(const char* reads, const uint64_t* read_offsets, uint64_t n, uint64_t* fw3, uint32_t* hasn, uint32_t* nm_index, uint64_t* nm_value,
                   uint64_t nm_cap, uint64_t* nm_count, uint32_t* max_read_len) {
    if (!read_offsets || !fw3 || !hasn || !nm_count || (n && !reads)) return fail(BGR_E_ARG, "bgr_pack_reads: null argument");
    const uint64_t base = read_offsets[0];
    memset(hasn, 0, ((n + 31) / 32) * 4);
    uint64_t cnt = 0;
    uint32_t longest = 0;
    std::vector<uint64_t> nm;
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t off = read_offsets[r] - base, len64 = read_offsets[r + 1] - read_offsets[r];
        if (len64 > 0x7FFFFFFFull) return fail(BGR_E_ARG, "bgr_pack_reads: read longer than 2^31 bases");
        const uint32_t len = (uint32_t)len64, words = (len + 31) >> 5;
        longest = std::max(longest, len);
        if (nm.size() < words) nm.resize(words);
        const uint64_t w0 = bgr::packed_word_offset(off, r);
        if (bgr::pack_read(reads + read_offsets[r], len, fw3 + w0, nm.data())) {
            hasn[r >> 5] |= 1u << (r & 31);
            if (cnt + words > nm_cap || !nm_index || !nm_value) return fail(BGR_E_CAPACITY, "bgr_pack_reads: N-mask list too small");
            for (uint32_t j = 0; j < words; ++j) { nm_index[cnt] = (uint32_t)(w0 + j); nm_value[cnt] = nm[j]; ++cnt; }
        }
    }
    *nm_count = cnt;
    if (max_read_len) *max_read_len = longest;
    return BGR_OK;
}

int bgr_align_batch_packed(bgr_aligner* a, const bgr_params* p, const bgr_packed_reads* pk, uint64_t n, int32_t* paths_out, uint64_t paths_cap,
                           uint64_t* path_offsets, uint8_t* status) {
    if (!a || !p || !pk || !path_offsets || (n && (!pk->read_offsets || !pk->fw3 || !pk->hasn || !status))) return fail(BGR_E_ARG, "bgr_align_batch_packed: null argument");
    if (pk->nm_count && (!pk->nm_index || !pk->nm_value)) return fail(BGR_E_ARG, "bgr_align_batch_packed: null N-mask list");
    path_offsets[0] = 0;
    forget_launch(a);
    if (n == 0) return BGR_OK;
    if (pk->read_offsets[0] != 0) return fail(BGR_E_ARG, "bgr_align_batch_packed: read_offsets must start at 0 (they address the planes)");
    const uint64_t total = pk->read_offsets[n];
    if (n >= 0x7FFFFFFFull || 2 * (total + 16 * n) >= 0xFFFFFFFFull - (256ull << 20))
        return fail(BGR_E_ARG, "bgr_align_batch_packed: batch too large for one launch (2*(bases + 16*reads) must stay below 2^32 - 2^28); pack it in pieces");
    HIP_TRY(hipSetDevice(a->device));
    const uint64_t plane_words = bgr::packed_plane_words(n, total);
    if (const int rc = settle_pending(a); rc != BGR_OK) return rc;   // (an exhaustive launch still to be counted reads the planes that are written next)
    HIP_TRY(a->launch.in_offs.ensure((n + 1) * 8));
    HIP_TRY(a->launch.pk_fw3.ensure(plane_words * 8));
    HIP_TRY(a->launch.pk_nm.ensure(plane_words * 8));
    HIP_TRY(a->launch.pk_hasn.ensure((n + 31) / 32 * 4 + 4));
    HIP_TRY(hipMemcpyAsync(a->launch.in_offs.p, pk->read_offsets, (n + 1) * 8, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(a->launch.pk_fw3.p, pk->fw3, ((total >> 5) + n + 1) * 8, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(a->launch.pk_hasn.p, pk->hasn, (n + 31) / 32 * 4, hipMemcpyHostToDevice, a->stream));
    if (pk->nm_count) {  // the N-mask words of the few reads that hold an N: a sparse list, scattered into the plane on the device
        const uint64_t voff = (pk->nm_count * 4 + 7) & ~7ull;  // indices, then the values 8-byte aligned, in the ASCII staging buffer (unused here)
        HIP_TRY(a->launch.in_reads.ensure(voff + pk->nm_count * 8));
        char* d = static_cast<char*>(a->launch.in_reads.p);
        HIP_TRY(hipMemcpyAsync(d, pk->nm_index, pk->nm_count * 4, hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipMemcpyAsync(d + voff, pk->nm_value, pk->nm_count * 8, hipMemcpyHostToDevice, a->stream));
        hipError_t e = bgr::launch_scatter_words(reinterpret_cast<const uint32_t*>(d), reinterpret_cast<const uint64_t*>(d + voff), pk->nm_count,
                                                 static_cast<uint64_t*>(a->launch.pk_nm.p), plane_words, a->stream);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("N-mask scatter launch: ") + hipGetErrorString(e));
    }
    uint32_t max_len = pk->max_read_len;
    if (!max_len) {
        for (uint64_t i = 0; i < n; ++i) max_len = std::max<uint32_t>(max_len, (uint32_t)std::min<uint64_t>(pk->read_offsets[i + 1] - pk->read_offsets[i], 0x7FFFFFFFull));
    }
    // (the host buffers may be reused once the copies are done: bgr_aligner_fetch below synchronises the stream)
    int rc = align_device_impl(a, p, nullptr, a->launch.in_offs.p, n, total, max_len, true);
    if (rc != BGR_OK) return rc;
    return bgr_aligner_fetch(a, n, paths_out, paths_cap, path_offsets, status);
}

int bgr_aligner_sync(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_sync: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    // its own stream and its twins': un-waited bgr_align_device launches may run on the first twin's, and every launch has completed when this returns
    for (bgr_aligner* x = a; x; x = x->twin) {
        HIP_TRY(hipStreamSynchronize(x->stream));
        const bool counts = x->deep_count.open;
        const int rc = settle_launch_sync(x);  // (exhaustive mode: reads the last pass handed back are mapped before the results count as final)
        if (rc != BGR_OK) return rc;
        if (counts) HIP_TRY(hipStreamSynchronize(x->stream));   // (... and the counting kernels that waited for that have run)
    }
    return BGR_OK;
}

int bgr_aligner_arena_ints(bgr_aligner* a, uint64_t* ints) {
    if (!a || !ints) return fail(BGR_E_ARG, "bgr_aligner_arena_ints: null argument");
    *ints = holder_of(a)->last_arena_cap;
    return BGR_OK;
}

int bgr_aligner_device_results(bgr_aligner* a, void** d_results, void** d_arena, void** d_cursor) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_device_results: null aligner");
    a = holder_of(a);   // (the buffers of the last launch)
    if (d_results) *d_results = a->launch.results.p;
    if (d_arena) *d_arena = a->launch.arena.p;
    if (d_cursor) *d_cursor = a->launch.small.p;
    return BGR_OK;
}

int bgr_aligner_exhaustive_paths_enable(bgr_aligner* a, int on) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_exhaustive_paths_enable: null aligner");
    if (a->is_twin) return fail(BGR_E_ARG, "bgr_aligner_exhaustive_paths_enable: an internal twin (the switch belongs to the aligner it was made for)");
    if (const int rc = sync_all(a); rc != BGR_OK) return rc;   // (a launch in flight ends under the switch it began under)
    a->sh->exhaustive_paths = on != 0;
    return BGR_OK;
}

int bgr_graph_exhaustive_paths_enable(bgr_graph* g, int on) {
    if (!g) return fail(BGR_E_ARG, "bgr_graph_exhaustive_paths_enable: null graph");
    std::lock_guard<std::mutex> l(g->abundance_m);
    g->exhaustive_paths_on = on != 0;
    return BGR_OK;
}

int bgr_graph_exhaustive_paths_enabled(const bgr_graph* g) { return g && g->exhaustive_paths_on ? 1 : 0; }

int bgr_aligner_device_rows_view(bgr_aligner* a, void** d_view) {
    if (!a || !d_view) return fail(BGR_E_ARG, "bgr_aligner_device_rows_view: null argument");
    *d_view = nullptr;
    a = holder_of(a);   // (the buffers of the last launch)
    if (a->last_mode != BGR_MODE_EXHAUSTIVE || !a->sh->exhaustive_paths || !a->last_n)
        return fail(BGR_E_ARG, "bgr_aligner_device_rows_view: the view is that of an exhaustive last launch on an aligner with bgr_aligner_exhaustive_paths_enable");
    const uint2* rows = nullptr;
    if (const int rc = last_rows(a, "bgr_aligner_device_rows_view", &rows); rc != BGR_OK) return rc;
    HIP_TRY(wait_stream(a));
    *d_view = const_cast<uint2*>(rows);
    return BGR_OK;
}

// results -> CSR on the device in two steps: the number of path ints of the launch (fetch_total), then the dense arrays and
// their copies into the caller's memory (fetch_copy: relative path_offsets[0..n], status[0..n), total ints at paths_out)
static int fetch_total(bgr_aligner* a, uint64_t n, uint64_t* total_out) {
    HIP_TRY(hipSetDevice(a->device));
    if (a->deep.open || a->deep_count.open) { const int src = settle_launch_sync(a); if (src != BGR_OK) return src; }
    else HIP_TRY(wait_stream(a));
    const uint64_t nb = (n + 4095) / 4096;
    HIP_TRY(a->fetch.csr_sums.ensure(nb * 4 + 64));
    HIP_TRY(a->fetch.csr_poffs.ensure((n + 1) * 8));
    HIP_TRY(a->fetch.csr_status.ensure(n));
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(static_cast<char*>(a->launch.small.p) + bgr::kSmallCsrTotal);
    hipError_t e = bgr::launch_csr(static_cast<const uint2*>(a->launch.results.p), static_cast<const int32_t*>(a->launch.arena.p), (uint32_t)n,
                                   static_cast<uint32_t*>(a->fetch.csr_sums.p), d_total, nullptr, nullptr, nullptr, 0, 0, a->last_arena_cap, a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("csr launch: ") + hipGetErrorString(e));
    uint64_t hs[bgr::kSmallCsrTotal / 8 + 1];  // the cursor block at the start, the path-int total at the end
    HIP_TRY(hipMemcpyAsync(hs, a->launch.small.p, sizeof(hs), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    const uint32_t* cur = reinterpret_cast<const uint32_t*>(hs);
    if (cur[bgr::kCurOverflow]) return fail(BGR_E_INTERNAL, "path arena overflow (internal sizing error)");
    *total_out = hs[bgr::kSmallCsrTotal / 8];
    return BGR_OK;
}
static int fetch_copy(bgr_aligner* a, uint64_t n, uint64_t total, int32_t* paths_out, uint64_t* path_offsets, uint8_t* status, bool with_end = true) {
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(static_cast<char*>(a->launch.small.p) + bgr::kSmallCsrTotal);
    HIP_TRY(a->fetch.csr_paths.ensure(total * 4 + 16));
    hipError_t e = bgr::launch_csr(static_cast<const uint2*>(a->launch.results.p), static_cast<const int32_t*>(a->launch.arena.p), (uint32_t)n,
                                   static_cast<uint32_t*>(a->fetch.csr_sums.p), d_total, static_cast<unsigned long long*>(a->fetch.csr_poffs.p),
                                   static_cast<int32_t*>(a->fetch.csr_paths.p), static_cast<uint8_t*>(a->fetch.csr_status.p), (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull), 1, a->last_arena_cap, a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("csr launch: ") + hipGetErrorString(e));
    // (with_end = false: entry n, the end of the last read, is left to the caller -- it is the first entry of the next piece)
    HIP_TRY(hipMemcpyAsync(path_offsets, a->fetch.csr_poffs.p, (n + (with_end ? 1 : 0)) * 8, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipMemcpyAsync(status, a->fetch.csr_status.p, n, hipMemcpyDeviceToHost, a->stream));
    if (total) HIP_TRY(hipMemcpyAsync(paths_out, a->fetch.csr_paths.p, total * 4, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return BGR_OK;
}

// what bgr_aligner_path_stats and bgr_aligner_path_diffs refuse of the last launch (a: the aligner that holds it)
static int path_rows_refusal(const bgr_aligner* a, uint64_t n, const std::string& who) {
    if (a->graph->header.has_exc) return fail(BGR_E_ARG, who + ": needs a graph of ACGT-only unitigs (the walk is read from the 2-bit store)");
    if (n != a->last_n) return fail(BGR_E_ARG, who + ": n_reads differs from the last bgr_align_device call");
    if (a->last_mode == BGR_MODE_EXHAUSTIVE && !a->sh->exhaustive_paths) return fail(BGR_E_ARG, who + ": the last launch was exhaustive; paths of the greedy modes only");
    return BGR_OK;
}

int bgr_aligner_path_stats(bgr_aligner* a, const void* d_reads, const void* d_read_offsets, uint64_t n, bgr_path_stat* out) {
    if (!a || (n && (!d_reads || !d_read_offsets || !out))) return fail(BGR_E_ARG, "bgr_aligner_path_stats: null argument");
    a = holder_of(a);   // (the rows of the last launch, on the stream that ran it)
    if (const int rc = path_rows_refusal(a, n, "bgr_aligner_path_stats"); rc != BGR_OK) return rc;
    if (n == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    static_assert(sizeof(bgr_path_stat) == 24, "six words per read, as the kernel writes them");
    HIP_TRY(a->fetch.path_stats.ensure(n * sizeof(bgr_path_stat)));
    const uint2* rows = nullptr;   // (an exhaustive launch: settled, and read through its view)
    if (const int rc = last_rows(a, "bgr_aligner_path_stats", &rows); rc != BGR_OK) return rc;
    hipError_t e = bgr::launch_path_stats(a->dg, static_cast<const uint8_t*>(d_reads), static_cast<const uint64_t*>(d_read_offsets), rows,
                                          static_cast<const int32_t*>(a->launch.arena.p), a->last_arena_cap, (uint32_t)n, static_cast<uint32_t*>(a->fetch.path_stats.p), a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("path stats launch: ") + hipGetErrorString(e));
    if (bgr::opt("test.count_with_path_stats")) {   // test hook: the counting kernels once over the rows the buffers hold now, the reads' characters from the caller's buffer
        BehindPasses c{a, a->last_arena_cap, static_cast<const uint64_t*>(d_read_offsets), n, a->last_total_bases};
        c.reads.ascii = static_cast<const uint8_t*>(d_reads); c.reads.ascii_bytes = a->last_total_bases;
        if (a->last_mode == BGR_MODE_EXHAUSTIVE) c.view = rows;
        LaunchMarks none{a, false};
        const int crc = queue_behind_passes(c, true, none);
        if (crc != BGR_OK) return crc;
    }
    HIP_TRY(hipMemcpyAsync(out, a->fetch.path_stats.p, n * sizeof(bgr_path_stat), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return BGR_OK;
}

// bgr_aligner_path_diffs: count, scan, fill (text_gaf.hip)
int bgr_aligner_path_diffs(bgr_aligner* a, const void* d_reads, const void* d_read_offsets, uint64_t n, uint64_t* diff_offsets, bgr_path_diff* out, uint64_t cap, uint64_t* n_out) {
    if (n_out) *n_out = 0;
    if (!a || !diff_offsets || !n_out || (cap && !out) || (n && (!d_reads || !d_read_offsets))) return fail(BGR_E_ARG, "bgr_aligner_path_diffs: null argument");
    a = holder_of(a);   // (the rows of the last launch, on the stream that ran it)
    if (const int rc = path_rows_refusal(a, n, "bgr_aligner_path_diffs"); rc != BGR_OK) return rc;
    diff_offsets[0] = 0;
    if (n == 0) return BGR_OK;
    if (a->last_total_bases >= (1ull << 32)) return fail(BGR_E_ARG, "bgr_aligner_path_diffs: launches of fewer than 2^32 bases (a read has at most one difference per base, and their offsets are scanned in 32 bits)");
    HIP_TRY(hipSetDevice(a->device));
    static_assert(sizeof(bgr_path_diff) == 8, "two words per difference, as the kernel writes them");
    // counts | offsets | offsets' unused twin (launch_scan2_u32 scans two arrays) | the scan's tile sums and the total
    const uint64_t words = n + 4, sums = 2ull * bgr::scan_tiles((uint32_t)n) + 16;
    HIP_TRY(a->fetch.path_diffs.ensure((3 * words + sums + 4) * 4));
    uint32_t* cnt = a->fetch.path_diffs.as<uint32_t>();
    uint32_t *doff = cnt + words, *twin = doff + words, *tile = twin + words, *total = tile + sums;
    const uint8_t* reads = static_cast<const uint8_t*>(d_reads);
    const uint64_t* offs = static_cast<const uint64_t*>(d_read_offsets);
    const uint2* rows = nullptr;   // (an exhaustive launch: settled, and read through its view)
    if (const int rc = last_rows(a, "bgr_aligner_path_diffs", &rows); rc != BGR_OK) return rc;
    hipError_t e = bgr::launch_path_diffs_count(a->dg, reads, offs, rows, a->launch.arena.as<int32_t>(), a->last_arena_cap, (uint32_t)n, cnt, a->stream);
    if (e == hipSuccess) e = bgr::launch_scan2_u32(cnt, cnt, doff, twin, (uint32_t)n, nullptr, tile, total, total + 1, a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("path diffs launches: ") + hipGetErrorString(e));
    std::vector<uint32_t> h(n + 1);
    HIP_TRY(hipMemcpyAsync(h.data(), doff, n * 4, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipMemcpyAsync(h.data() + n, total, 4, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    for (uint64_t i = 0; i <= n; ++i) diff_offsets[i] = h[i];
    const uint64_t all = h[n];
    *n_out = all;
    if (all > cap) return fail(BGR_E_CAPACITY, "bgr_aligner_path_diffs: out holds fewer differences than the launch has (*n says how many; the offsets are set)");
    if (all == 0) return BGR_OK;
    DevBuf& buf = a->fetch.path_stats;   // (the records: the buffer of bgr_aligner_path_stats' rows is free between calls)
    HIP_TRY(buf.ensure(all * sizeof(bgr_path_diff)));
    e = bgr::launch_path_diffs_fill(a->dg, reads, offs, rows, a->launch.arena.as<int32_t>(), (uint32_t)n, cnt, doff, buf.as<uint2>(), a->stream);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("path diffs fill launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, buf.p, all * sizeof(bgr_path_diff), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(wait_stream(a));
    return BGR_OK;
}

int bgr_aligner_fetch(bgr_aligner* a, uint64_t n, int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status) {
    if (!a || !path_offsets || !status || (paths_cap && !paths_out)) return fail(BGR_E_ARG, "bgr_aligner_fetch: null argument");
    a = holder_of(a);   // (the rows of the last launch, on the stream that ran it; a fetch into a larger buffer after BGR_E_CAPACITY finds them there again)
    if (n != a->last_n) return fail(BGR_E_ARG, "bgr_aligner_fetch: n_reads differs from the last bgr_align_device call");
    path_offsets[0] = 0;
    if (n == 0) return BGR_OK;
    uint64_t total = 0;
    int rc = fetch_total(a, n, &total);
    if (rc != BGR_OK) return rc;
    if (total > paths_cap) return fail(BGR_E_CAPACITY, "bgr_aligner_fetch: paths_out too small");
    return fetch_copy(a, n, total, paths_out, path_offsets, status);
}

// A batch of reads on the host up to (not including) the copies out: H2D of the characters and offsets into the aligner's input buffers, the mapping
// launch (not the public form: the copies are on a->stream).  rel: where the offsets are made relative when they do not start at 0 -- with `keep` in any
// case, and nothing is waited for: the vector outlives the copy, the caller's array need not
static int batch_launch(bgr_aligner* a, const bgr_params* p, const char* who, const char* reads, const uint64_t* read_offsets, uint64_t n, std::vector<uint64_t>& rel, bool keep) {
    const uint64_t base = read_offsets[0], total = read_offsets[n] - base;
    uint32_t max_len = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t l = read_offsets[i + 1] - read_offsets[i];
        if (l > 0x7FFFFFFFull) return fail(BGR_E_ARG, std::string(who) + ": read longer than 2^31 bases");
        max_len = std::max<uint32_t>(max_len, (uint32_t)l);
    }
    if (const int rc = settle_pending(a); rc != BGR_OK) return rc;   // (an exhaustive launch still to be counted reads the buffers that are written next)
    rel.resize(keep || base ? n + 1 : 0);
    for (uint64_t i = 0; i < rel.size(); ++i) rel[i] = read_offsets[i] - base;
    HIP_TRY(a->launch.in_reads.ensure(total + 16));
    HIP_TRY(a->launch.in_offs.ensure((n + 1) * 8));
    HIP_TRY(hipMemcpyAsync(a->launch.in_reads.p, reads + base, total, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(a->launch.in_offs.p, rel.empty() ? read_offsets : rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, a->stream));
    if (!keep) HIP_TRY(hipStreamSynchronize(a->stream));
    return align_device_impl(a, p, a->launch.in_reads.p, a->launch.in_offs.p, n, total, max_len, false);
}
static int batch_piece_launch(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n) {
    HIP_TRY(hipSetDevice(a->device));
    std::vector<uint64_t> rel;
    return batch_launch(a, p, "bgr_align_batch", reads, read_offsets, n, rel, false);
}

// A large batch in pieces on several streams (this aligner's and its twins', one host thread each): the copies of one piece run under the
// kernels of the others, and -- with more streams than two -- the link never waits for a stream that is busy fetching its results (two
// streams kept it 2/3 busy: 243 Mreads/s per 5 M-read call; kOverlapStreams = 4: see DESIGN 9).  A piece's place in paths_out is known
// once the pieces in front of it have counted their path ints (fetch_total); results are those of one launch over the whole batch.
static const uint64_t kOverlapMinReads = 512 * 1024;
static const unsigned kOverlapMaxStreams = 4, kOverlapMaxPieces = 2 * kOverlapMaxStreams;
static int align_batch_overlapped(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n,
                                  int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status) {
    unsigned n_streams = kOverlapMaxStreams;
    n_streams = (unsigned)std::min<int64_t>((int64_t)kOverlapMaxStreams, std::max<int64_t>(2, bgr::opt("overlap_streams")));  // (option overlap_streams: A/B measurements)
    const unsigned n_pieces = 2 * n_streams;
    bgr_aligner* al[kOverlapMaxStreams] = {a, nullptr, nullptr, nullptr};
    { const int rc = twins_setup(a, n_streams - 1); if (rc != BGR_OK) return rc; }
    for (unsigned t = 1; t < n_streams; ++t) al[t] = al[t - 1]->twin;
    uint64_t cut[kOverlapMaxPieces + 1];
    for (unsigned k = 0; k <= n_pieces; ++k) cut[k] = n * k / n_pieces;
    std::mutex mu;
    std::condition_variable cv;
    uint64_t totals[kOverlapMaxPieces];
    bool known[kOverlapMaxPieces];
    for (unsigned k = 0; k < n_pieces; ++k) { totals[k] = 0; known[k] = false; }
    int first_rc = BGR_OK;
    std::string first_err;
    auto give_up = [&](int rc, const char* msg) {
        std::lock_guard<std::mutex> l(mu);
        if (first_rc == BGR_OK) { first_rc = rc; first_err = msg ? msg : ""; }
        cv.notify_all();
    };
    auto work = [&](unsigned t) {
        for (unsigned k = t; k < n_pieces; k += n_streams) {
            { std::lock_guard<std::mutex> l(mu); if (first_rc != BGR_OK) return; }
            const uint64_t i0 = cut[k], cnt = cut[k + 1] - cut[k];
            uint64_t tot = 0;
            int rc = cnt ? batch_piece_launch(al[t], p, reads, read_offsets + i0, cnt) : BGR_OK;
            if (rc == BGR_OK && cnt) rc = fetch_total(al[t], cnt, &tot);
            if (rc != BGR_OK) { give_up(rc, bgr_last_error()); return; }
            uint64_t before = 0;
            {
                std::unique_lock<std::mutex> l(mu);
                totals[k] = tot;
                known[k] = true;
                cv.notify_all();
                cv.wait(l, [&] { if (first_rc != BGR_OK) return true; for (unsigned j = 0; j < k; ++j) if (!known[j]) return false; return true; });
                if (first_rc != BGR_OK) return;
                for (unsigned j = 0; j < k; ++j) before += totals[j];
            }
            if (before + tot > paths_cap) { give_up(BGR_E_CAPACITY, "bgr_align_batch: paths_out too small"); return; }
            if (cnt) {
                rc = fetch_copy(al[t], cnt, tot, paths_out ? paths_out + before : nullptr, path_offsets + i0, status + i0, false);
                if (rc != BGR_OK) { give_up(rc, bgr_last_error()); return; }
                if (before) for (uint64_t i = i0; i < i0 + cnt; ++i) path_offsets[i] += before;  // (entry i0 + cnt belongs to the next piece / the end)
            }
        }
    };
    std::vector<std::thread> helpers;
    try {
        for (unsigned t = 1; t < n_streams; ++t) helpers.emplace_back(work, t);
        work(0u);
    } catch (...) {  // (bad_alloc in a piece, or no thread to be had: the helpers that run must still be joined)
        give_up(BGR_E_INTERNAL, "bgr_align_batch: out of memory");
    }
    for (auto& h : helpers) h.join();
    if (first_rc != BGR_OK) return fail(first_rc, first_err);
    uint64_t all = 0;
    for (unsigned k = 0; k < n_pieces; ++k) all += totals[k];
    path_offsets[n] = all;
    forget_launch(a);  // several launches: bgr_aligner_fetch has nothing to re-read
    return BGR_OK;
}

int bgr_align_batch(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n,
                    int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status) {
    if (!a || !p || !path_offsets || (n && (!reads || !read_offsets || !status))) return fail(BGR_E_ARG, "bgr_align_batch: null argument");
    path_offsets[0] = 0;
    forget_launch(a);
    if (n == 0) return BGR_OK;
    HIP_TRY(hipSetDevice(a->device));
    const uint64_t base = read_offsets[0], total = read_offsets[n] - base;
    // One launch addresses its path arena with 32 bits: a batch beyond that (~13 M reads of 150 bp) is mapped in pieces.
    // (BGR_KNOB_BATCH_SPLIT_LIMIT: tests lower the limit to walk this path with small inputs)
    const uint64_t lim = a->sh->knob_split_limit ? std::max<uint64_t>(4096, a->sh->knob_split_limit) : 0xFFFFFFFFull - (256ull << 20);
    if (n > 1 && (2 * (total + 16 * n) >= lim || n >= 0x7FFFFFFFull)) {
        uint64_t w = 0;
        for (uint64_t i0 = 0; i0 < n;) {
            uint64_t i1 = i0 + 1;  // longest piece below half the limit (at least one read)
            while (i1 < n && 2 * ((read_offsets[i1 + 1] - read_offsets[i0]) + 16 * (i1 + 1 - i0)) < lim / 2 && i1 + 1 - i0 < (1ull << 30)) ++i1;
            int rc = bgr_align_batch(a, p, reads, read_offsets + i0, i1 - i0, paths_out ? paths_out + w : nullptr, paths_cap - w, path_offsets + i0, status + i0);
            if (rc != BGR_OK) return rc;
            const uint64_t got = path_offsets[i1];
            for (uint64_t i = i0; i <= i1; ++i) path_offsets[i] += w;
            w += got;
            i0 = i1;
        }
        forget_launch(a);  // several launches: bgr_aligner_fetch has nothing to re-read
        return BGR_OK;
    }
    // a large batch: in pieces on two streams, copies under kernels (BGR_KNOB_BATCH_OVERLAP = 1 turns it off)
    if (!a->is_twin && !a->sh->knob_overlap && n >= kOverlapMinReads) return align_batch_overlapped(a, p, reads, read_offsets, n, paths_out, paths_cap, path_offsets, status);
    int rc = batch_piece_launch(a, p, reads, read_offsets, n);
    if (rc != BGR_OK) return rc;
    return bgr_aligner_fetch(a, n, paths_out, paths_cap, path_offsets, status);
}

// ---- asynchronous form over host buffers ---------------------------------------------------------------------------------------
int bgr_align_batch_begin(bgr_aligner* a, const bgr_params* p, const char* reads, const uint64_t* read_offsets, uint64_t n, bgr_ticket* ticket) {
    if (!a || !p || !ticket || (n && (!reads || !read_offsets))) return fail(BGR_E_ARG, "bgr_align_batch_begin: null argument");
    if (a->ticket_open) return fail(BGR_E_ARG, "bgr_align_batch_begin: this aligner still has a batch in flight (wait for its ticket first)");
    ticket->aligner = a;
    ticket->n_reads = n;
    ticket->serial = ++a->ticket_serial;
    forget_launch(a);
    if (n == 0) { a->ticket_open = true; return BGR_OK; }
    HIP_TRY(hipSetDevice(a->device));
    const uint64_t base = read_offsets[0], total = read_offsets[n] - base;
    if (n >= 0x7FFFFFFFull || 2 * (total + 16 * n) >= 0xFFFFFFFFull - (256ull << 20))
        return fail(BGR_E_ARG, "bgr_align_batch_begin: batch too large for one launch (2 * (bases + 16 * reads) must stay below 2^32 - 2^28); bgr_align_batch cuts such a batch");
    const int rc = batch_launch(a, p, "bgr_align_batch_begin", reads, read_offsets, n, a->ticket_offs, true);   // (the offsets stay alive in the aligner for the asynchronous copy)
    if (rc != BGR_OK) return rc;
    a->ticket_open = true;
    return BGR_OK;
}

int bgr_align_batch_test(const bgr_ticket* t) {
    if (!t || !t->aligner) return fail(BGR_E_ARG, "bgr_align_batch_test: null ticket");
    bgr_aligner* a = t->aligner;
    if (!a->ticket_open || t->serial != a->ticket_serial) return fail(BGR_E_ARG, "bgr_align_batch_test: stale ticket");
    if (hipSetDevice(a->device) != hipSuccess) return fail(BGR_E_HIP, "hipSetDevice failed");
    bool idle = false;
    const int rc = stream_idle(a, &idle);
    return rc != BGR_OK ? rc : idle ? 1 : 0;
}

int bgr_align_batch_wait(const bgr_ticket* t, int32_t* paths_out, uint64_t paths_cap, uint64_t* path_offsets, uint8_t* status) {
    if (!t || !t->aligner || !path_offsets) return fail(BGR_E_ARG, "bgr_align_batch_wait: null argument");
    bgr_aligner* a = t->aligner;
    if (!a->ticket_open || t->serial != a->ticket_serial) return fail(BGR_E_ARG, "bgr_align_batch_wait: stale ticket (every begin is waited for once, in order)");
    path_offsets[0] = 0;
    if (t->n_reads == 0) { a->ticket_open = false; return BGR_OK; }
    const int rc = bgr_aligner_fetch(a, t->n_reads, paths_out, paths_cap, path_offsets, status);
    if (rc != BGR_E_CAPACITY) a->ticket_open = false;  // (too small a paths buffer: the results stay, wait again with a larger one)
    return rc;
}

int bgr_aligner_counters(bgr_aligner* a, uint64_t out[5]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_counters: null argument");
    HIP_TRY(hipSetDevice(a->device));
    for (uint32_t i = 0; i < bgr::kCounters; ++i) out[i] = 0;
    for (bgr_aligner* x = a; x; x = x->twin) {  // its own stream, and the pieces of overlapped batches its other streams mapped
        uint64_t t[bgr::kCounters];
        HIP_TRY(hipStreamSynchronize(x->stream));
        { const int src = settle_launch_sync(x); if (src != BGR_OK) return src; }  // (exhaustive mode: reads the last pass handed back are mapped -- and counted -- first)
        HIP_TRY(hipMemcpy(t, x->launch.small.as<char>() + bgr::kSmallCounters, sizeof(t), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < bgr::kCounters; ++i) out[i] += t[i];
    }
    return BGR_OK;
}

int bgr_aligner_reset_counters(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_counters: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    for (bgr_aligner* x = a; x; x = x->twin) {  // (each on its own stream: a fill on the null stream is not ordered with a non-blocking stream's kernels)
        HIP_TRY(hipMemsetAsync(x->launch.small.as<char>() + bgr::kSmallCounters, 0, bgr::kCounters * 8 + 8, x->stream));
        HIP_TRY(hipStreamSynchronize(x->stream));
    }
    return BGR_OK;
}

int bgr_aligner_kernel_time(bgr_aligner* a, uint64_t* launches, double* total_ms) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_kernel_time: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    if (launches) *launches = 0;
    if (total_ms) *total_ms = 0;
    for (bgr_aligner* x = a; x; x = x->twin) {  // its own stream, and the pieces of overlapped batches its other streams mapped
        if (const int src = settle_pending(x); src != BGR_OK) return src;
        const int rc = drain_timers(x);
        if (rc != BGR_OK) return rc;
        if (launches) *launches += x->t_launches;
        if (total_ms) *total_ms += x->t_ms;
    }
    return BGR_OK;
}

int bgr_aligner_kernel_times(bgr_aligner* a, uint64_t* launches, double slot_ms[8], const char* slot_names[8]) {
    if (!a || !slot_ms) return fail(BGR_E_ARG, "bgr_aligner_kernel_times: null argument");
    HIP_TRY(hipSetDevice(a->device));
    if (launches) *launches = 0;
    for (bgr_aligner* x = a; x; x = x->twin) {
        if (const int src = settle_pending(x); src != BGR_OK) return src;   // (the kernels behind an exhaustive launch's settling are that launch's)
        const int rc = drain_timers(x);
        if (rc != BGR_OK) return rc;
        if (launches) *launches += x->t_launches;
    }
    for (int j = 0; j < kTimerSlots; ++j) {
        slot_ms[j] = a->t_slot_ms[j];
        const char* name = a->t_slot_name[j];
        for (bgr_aligner* tw = a->twin; tw; tw = tw->twin) {  // (all streams run the same launch sequence: slot j is the same kernel)
            if (tw->t_slot_ms[j] <= 0) continue;
            slot_ms[j] += tw->t_slot_ms[j];
            if (!name) name = tw->t_slot_name[j];
        }
        if (slot_names) slot_names[j] = slot_ms[j] > 0 ? name : nullptr;
    }
    return BGR_OK;
}

int bgr_aligner_reset_kernel_time(bgr_aligner* a) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_reset_kernel_time: null aligner");
    HIP_TRY(hipSetDevice(a->device));
    int rc = drain_timers(a);
    if (rc != BGR_OK) return rc;
    a->t_launches = 0;
    a->t_ms = 0;
    for (double& x : a->t_slot_ms) x = 0;
    if (a->twin) return bgr_aligner_reset_kernel_time(a->twin);
    return BGR_OK;
}

int bgr_aligner_launch_info(bgr_aligner* a, uint32_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_launch_info: null argument");
    memcpy(out, holder_of(a)->last_launch, sizeof(a->last_launch));
    return BGR_OK;
}

#ifdef BGR_PHASE_TIMING
// diagnostic builds only (not part of include/bgreat_gpu.h): four u64 per wave of the last launch, the `part`-th such block of its buffer
static int debug_wave_block(bgr_aligner* a, uint64_t part, uint64_t* out, uint64_t cap_waves, uint64_t* n_waves) {
    if (!a || !n_waves) return BGR_E_ARG;
    a = holder_of(a);
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    *n_waves = a->wave_times_n;
    const uint64_t n = std::min(cap_waves, a->wave_times_n);
    if (n && out) HIP_TRY(hipMemcpy(out, a->launch.wave_times.as<char>() + part * a->wave_times_n * 32, n * 32, hipMemcpyDeviceToHost));
    return BGR_OK;
}
// the per-wave time stamps (100 MHz ticks)
int bgr_debug_wave_times(bgr_aligner* a, uint64_t* out, uint64_t cap_waves, uint64_t* n_waves) { return debug_wave_block(a, 0, out, cap_waves, n_waves); }
// the greedy multi kernel's anchor-scan counts per wave: {scan steps, items scanned, groups of items, 0}
int bgr_debug_scan_counts(bgr_aligner* a, uint64_t* out, uint64_t cap_waves, uint64_t* n_waves) { return debug_wave_block(a, 1, out, cap_waves, n_waves); }
#endif

int bgr_aligner_last_pass_runs(const bgr_aligner* a, uint32_t* runs, uint32_t* memo_cap) {
    if (!a) return fail(BGR_E_ARG, "bgr_aligner_last_pass_runs: null aligner");
    a = holder_of(a);
    if (runs) *runs = a->deep.runs;
    if (memo_cap) *memo_cap = a->deep.memo_cap;
    return BGR_OK;
}

int bgr_aligner_pass_counts(bgr_aligner* a, uint32_t out[4]) {
    if (!a || !out) return fail(BGR_E_ARG, "bgr_aligner_pass_counts: null argument");
    a = holder_of(a);   // (the cursor block of the last launch)
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    uint32_t cur[bgr::kCurWords];
    HIP_TRY(hipMemcpy(cur, a->launch.small.p, sizeof(cur), hipMemcpyDeviceToHost));
    static_assert(bgr::kCurFollowUps == bgr::list_word(bgr::List::kSearch), "out[0]: greedy mode's follow-up items, exhaustive mode's first list");
    out[0] = cur[bgr::kCurFollowUps]; out[1] = cur[bgr::list_word(bgr::List::kDepthFirst)];
    out[2] = cur[bgr::list_word(bgr::List::kFirst)]; out[3] = cur[bgr::list_word(bgr::List::kGeneral)];
    return BGR_OK;
}

int bgr_device_local_cpus(int device, char* cpulist_out, uint64_t cap) {
    if (!cpulist_out || cap < 2) return fail(BGR_E_ARG, "bgr_device_local_cpus: null argument");
    char bus[64];
    HIP_TRY(hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device));
    for (char* c = bus; *c; ++c) *c = (char)tolower(*c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return fail(BGR_E_IO, "bgr_device_local_cpus: cannot read " + path);
    const size_t got = fread(cpulist_out, 1, (size_t)cap - 1, f);
    fclose(f);
    cpulist_out[got] = 0;
    for (size_t i = 0; i < got; ++i) if (cpulist_out[i] == '\n') cpulist_out[i] = 0;
    if (!cpulist_out[0]) return fail(BGR_E_IO, "bgr_device_local_cpus: empty cpulist");
    return BGR_OK;
}

int bgr_device_alloc(int device, uint64_t bytes, void** out) {
    if (!out) return fail(BGR_E_ARG, "bgr_device_alloc: null argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
    return BGR_OK;
}
int bgr_device_free(int device, void* p) {
    if (!p) return BGR_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(p));
    return BGR_OK;
}
int bgr_device_upload(int device, void* dst_device, const void* src_host, uint64_t bytes) {
    if (bytes && (!dst_device || !src_host)) return fail(BGR_E_ARG, "bgr_device_upload: null argument");
    HIP_TRY(hipSetDevice(device));
    if (bytes) { HIP_TRY(hipMemcpy(dst_device, src_host, bytes, hipMemcpyHostToDevice)); HIP_TRY(hipStreamSynchronize(nullptr)); }  // (the callers' kernels run on non-blocking streams)
    return BGR_OK;
}
int bgr_device_download(int device, void* dst_host, const void* src_device, uint64_t bytes) {
    if (bytes && (!dst_host || !src_device)) return fail(BGR_E_ARG, "bgr_device_download: null argument");
    HIP_TRY(hipSetDevice(device));
    if (bytes) HIP_TRY(hipMemcpy(dst_host, src_device, bytes, hipMemcpyDeviceToHost));
    return BGR_OK;
}

// Page-locked host memory.  hipHostMalloc pins 4 KB pages at ~4.4 GB/s on this platform, from any number of threads; an anonymous
// mapping with transparent huge pages asked for, touched once per 2 MB and then registered pins at ~26 GB/s (tools/ubench/pin_alloc.hip) --
// bgr_align_all takes ~0.7 GB of staging sets while its pipeline ramps up, 0.17 s of a 0.6 s run of 100 M reads.  Buffers of 2 MB and
// more go that way (hipHostMalloc when anything in it fails); the registry tells bgr_host_free how a pointer was obtained.
// (never destroyed: the pipeline's cache of staging sets frees its buffers from a static destructor of its own, in whatever order)
static std::mutex& g_host_m = *new std::mutex;
static std::map<void*, uint64_t>& g_host_mapped = *new std::map<void*, uint64_t>;  // registered anonymous mappings: pointer -> mapped bytes

int bgr_host_alloc(uint64_t bytes, void** out) {
    if (!out) return fail(BGR_E_ARG, "bgr_host_alloc: null argument");
    void* p = nullptr;
    if (bytes >= (2ull << 20) && bgr::opt("huge_pinned")) {
        const uint64_t len = (bytes + (2ull << 20) - 1) & ~((2ull << 20) - 1);
        void* m = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m != MAP_FAILED) {
            (void)madvise(m, len, MADV_HUGEPAGE);
            for (uint64_t o = 0; o < len; o += 2ull << 20) static_cast<volatile char*>(m)[o] = 0;  // fault the (huge) pages in before they are pinned
            if (hipHostRegister(m, len, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> l(g_host_m);
                g_host_mapped[m] = len;
                *out = m;
                return BGR_OK;
            }
            (void)hipGetLastError();
            munmap(m, len);
        }
    }
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    *out = p;
    return BGR_OK;
}

int bgr_host_free(void* p) {
    if (!p) return BGR_OK;
    uint64_t len = 0;
    {
        std::lock_guard<std::mutex> l(g_host_m);
        auto it = g_host_mapped.find(p);
        if (it != g_host_mapped.end()) { len = it->second; g_host_mapped.erase(it); }
    }
    if (len) {
        hipError_t e = hipHostUnregister(p);
        munmap(p, len);
        if (e != hipSuccess) return fail(BGR_E_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e));
        return BGR_OK;
    }
    hipError_t e = hipHostFree(p);
    if (e != hipSuccess) return fail(BGR_E_HIP, std::string("hipHostFree: ") + hipGetErrorString(e));
    return BGR_OK;
}

// ---- read files / output records (host) ---------------------------------------------------------------
struct bgr_readset { bgr::ReadSet rs; };

int bgr_readset_load(const char* path, int fastq, uint32_t k, bgr_readset** out) {
    return bgr_readset_load_parallel(path, fastq, k, 1, 0, out);
}

int bgr_readset_load_parallel(const char* path, int fastq, uint32_t k, uint32_t threads, uint64_t chunk_bytes, bgr_readset** out) {
    if (!path || !out) return fail(BGR_E_ARG, "bgr_readset_load: null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(BGR_E_IO, std::string("cannot open read file ") + path);
    std::vector<char> buf;
    char tmp[1 << 16];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    bgr_readset* r = new bgr_readset();
    r->rs.clear();
    bgr::parse_reads_parallel(buf.data(), buf.size(), fastq != 0, k, threads ? threads : 1, chunk_bytes ? chunk_bytes : (8u << 20), r->rs);
    *out = r;
    return BGR_OK;
}
uint64_t bgr_readset_count(const bgr_readset* rs) { return rs ? rs->rs.count() : 0; }
int bgr_readset_view(const bgr_readset* rs, const char** reads, const uint64_t** read_offsets, const char** headers, const uint64_t** header_offsets) {
    if (!rs) return fail(BGR_E_ARG, "bgr_readset_view: null readset");
    if (reads) *reads = rs->rs.reads.data();
    if (read_offsets) *read_offsets = rs->rs.read_offs.data();
    if (headers) *headers = rs->rs.headers.data();
    if (header_offsets) *header_offsets = rs->rs.header_offs.data();
    return BGR_OK;
}
void bgr_readset_destroy(bgr_readset* rs) { delete rs; }

int bgr_write_records(void* paths_file, void* notaligned_file, uint64_t n, const char* headers, const uint64_t* hoffs,
                      const char* reads, const uint64_t* roffs, const int32_t* paths, const uint64_t* poffs) {
    if (!paths_file || !notaligned_file || (n && (!headers || !hoffs || !reads || !roffs || !poffs))) return fail(BGR_E_ARG, "bgr_write_records: null argument");
    FILE* pf = static_cast<FILE*>(paths_file);
    FILE* nf = static_cast<FILE*>(notaligned_file);
    std::string pbuf, nbuf;
    pbuf.reserve(1 << 20);
    nbuf.reserve(1 << 20);
    char num[16];
    for (uint64_t i = 0; i < n; ++i) {
        const char* h = headers + hoffs[i];
        size_t hn = hoffs[i + 1] - hoffs[i];
        if (poffs[i + 1] > poffs[i]) {  // alignerGreedy.cpp:406-411 + printPath aligner.cpp:600-609
            pbuf.append(h, hn);
            pbuf.push_back('\n');
            for (uint64_t j = poffs[i]; j < poffs[i + 1]; ++j) {
                int32_t v = paths[j];
                uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
                int len = 0;
                do { num[len++] = (char)('0' + u % 10); u /= 10; } while (u);
                if (v < 0) pbuf.push_back('-');
                while (len) pbuf.push_back(num[--len]);
                pbuf.push_back('.');
            }
            pbuf.push_back('\n');
            if (pbuf.size() > (1 << 20) - 4096) { if (fwrite(pbuf.data(), 1, pbuf.size(), pf) != pbuf.size()) return fail(BGR_E_IO, "write to paths file failed"); pbuf.clear(); }
        } else {  // alignerGreedy.cpp:421-427
            nbuf.append(h, hn);
            nbuf.push_back('\n');
            nbuf.append(reads + roffs[i], roffs[i + 1] - roffs[i]);
            nbuf.push_back('\n');
            if (nbuf.size() > (1 << 20) - 4096) { if (fwrite(nbuf.data(), 1, nbuf.size(), nf) != nbuf.size()) return fail(BGR_E_IO, "write to notAligned file failed"); nbuf.clear(); }
        }
    }
    if (!pbuf.empty() && fwrite(pbuf.data(), 1, pbuf.size(), pf) != pbuf.size()) return fail(BGR_E_IO, "write to paths file failed");
    if (!nbuf.empty() && fwrite(nbuf.data(), 1, nbuf.size(), nf) != nbuf.size()) return fail(BGR_E_IO, "write to notAligned file failed");
    return BGR_OK;
}

}  // extern "C"

// pipeline_support.h -- part of the translation unit pipeline.cpp (included by it alone): what the stages of the host pipeline
// stand on -- the pool of worker threads, the bounded channel, the page-locked buffer sets and their cache between runs.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <ctime>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/bgreat_gpu.h"
#include "read_pack.h"

namespace {

// Persistent workers shared by the parse, gather and format stages (a batch is a few hundred thousand reads: spawning
// threads per stage and batch cost more than the work).  run(n, fn): fn(0..n-1) on the workers and the calling
// thread, returns when all are done; concurrent run() calls from different stage threads interleave.
class WorkerPool {
public:
    explicit WorkerPool(unsigned n) {
        for (unsigned i = 0; i + 1 < n; ++i) ts_.emplace_back([this]() { loop(); });
    }
    ~WorkerPool() {
        { std::lock_guard<std::mutex> l(m_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : ts_) t.join();
    }
    // tag: which stage the work belongs to (BGREAT_TIMING: thread CPU seconds per stage, cpu_us)
    template <typename F>
    void run(size_t n, F fn, int tag = 0) {
        if (n == 0) return;
        if (n == 1 || ts_.empty()) { const uint64_t c0 = cpu_now(); for (size_t i = 0; i < n; ++i) fn(i); cpu_us[tag] += cpu_now() - c0; return; }
        Job job;
        job.n = n;
        job.tag = tag;
        job.fn = [&fn](size_t i) { fn(i); };
        const size_t helpers = std::min<size_t>(ts_.size(), n - 1);
        job.pending = helpers;
        {
            std::lock_guard<std::mutex> l(m_);
            for (size_t i = 0; i < helpers; ++i) q_.push_back(&job);
        }
        cv_.notify_all();
        work(job);
        std::unique_lock<std::mutex> l(job.m);
        job.cv.wait(l, [&job] { return job.pending == 0; });
    }
private:
    struct Job {
        size_t n = 0;
        std::atomic<size_t> next{0};
        std::function<void(size_t)> fn;
        std::mutex m;
        std::condition_variable cv;
        size_t pending = 0;
        int tag = 0;
    };
    void work(Job& j) {
        const uint64_t c0 = cpu_now();
        for (size_t i; (i = j.next.fetch_add(1)) < j.n;) j.fn(i);
        cpu_us[j.tag] += cpu_now() - c0;
    }
    void loop() {
        for (;;) {
            Job* j = nullptr;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                j = q_.front();
                q_.pop_front();
            }
            work(*j);
            std::lock_guard<std::mutex> l(j->m);  // notify under the lock: the job lives on the caller's stack
            if (--j->pending == 0) j->cv.notify_one();
        }
    }
    std::vector<std::thread> ts_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Job*> q_;
    bool stop_ = false;
public:
    bool timing = false;
    std::atomic<uint64_t> cpu_us[8] = {};
    uint64_t cpu_now() const {  // CPU time of the calling thread, microseconds (0 unless timing)
        if (!timing) return 0;
        timespec ts;
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
        return (uint64_t)ts.tv_sec * 1000000ull + (uint64_t)ts.tv_nsec / 1000;
    }
};

template <typename T>
class Channel {  // bounded FIFO
public:
    explicit Channel(size_t cap) : cap_(cap) {}
    bool push(T v) {
        std::unique_lock<std::mutex> l(m_);
        cv_space_.wait(l, [this] { return q_.size() < cap_ || closed_; });
        if (closed_) return false;
        q_.push_back(std::move(v));
        cv_item_.notify_one();
        return true;
    }
    bool try_pop(T& v) {
        std::lock_guard<std::mutex> l(m_);
        if (q_.empty()) return false;
        v = std::move(q_.front());
        q_.pop_front();
        cv_space_.notify_one();
        return true;
    }
    bool pop(T& v) {
        std::unique_lock<std::mutex> l(m_);
        cv_item_.wait(l, [this] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        v = std::move(q_.front());
        q_.pop_front();
        cv_space_.notify_one();
        return true;
    }
    void close() {
        std::lock_guard<std::mutex> l(m_);
        closed_ = true;
        cv_item_.notify_all();
        cv_space_.notify_all();
    }
private:
    std::mutex m_;
    std::condition_variable cv_item_, cv_space_;
    std::deque<T> q_;
    size_t cap_;
    bool closed_ = false;
};

struct HostBuf {  // grow-only host buffer; `pinned` = page-locked (20 GB/s to allocate on an idle process, several times slower
                  // while parser threads are faulting the input file in: the pool is sized and allocated before they start)
    void* p = nullptr;
    uint64_t cap = 0;
    bool pinned;
    explicit HostBuf(bool pin) : pinned(pin) {}
    void release() {
        if (!p) return;
        if (pinned) bgr_host_free(p); else free(p);
        p = nullptr; cap = 0;
    }
    bool ensure(uint64_t bytes) {
        if (bytes <= cap) return true;
        release();
        uint64_t want = bytes + bytes / 4 + 4096;
        if (pinned) { if (bgr_host_alloc(want, &p) != BGR_OK) return false; }
        else { p = malloc(want); if (!p) return false; }
        cap = want;
        return true;
    }
    ~HostBuf() { release(); }
};

struct Pinned {  // the page-locked buffers of one batch in flight: sources / targets of the async copies
    // reads travel as 2-bit planes (read_pack.h): fw3 words, N bitmap, and the N-mask words of the few reads with an N
    HostBuf fw3{true}, hasn{true}, nm_idx{true}, nm_val{true}, offs{true}, paths{true}, poffs{true}, status{true};
    // text route (bgr_align_fasta_text): the piece of the file as it is, and the two record streams as they come back
    HostBuf text{true}, ptext{true}, ntext{true};
    HostBuf info{true};  // text route under -b with progress blocks: one word per record of the piece (bgr_text_batch.record_info_out)
    std::vector<bgr_text_stage*> stages;  // per device of the run: where this set's piece waits in HBM (bgr_text_stage_upload), made on first use
    uint64_t nm_count = 0;
    uint32_t max_len = 0;
    ~Pinned() { for (bgr_text_stage* st : stages) bgr_text_stage_destroy(st); }
};
using PinChannel = Channel<std::unique_ptr<Pinned>>;

// Page-locked buffers cost ~0.2 s per GB to allocate: a finished run leaves its sets here for the next bgr_align_all of the
// process (bgr_host_cache_release frees them).
// (heap objects that are never destroyed: a static destructor would release page-locked memory, streams and HBM buffers after the HIP
// runtime's own teardown at exit; a process that wants them gone calls bgr_host_cache_release -- the CLI does at the end of main)
std::mutex& g_pin_cache_m = *new std::mutex;
std::vector<std::unique_ptr<Pinned>>& g_pin_cache = *new std::vector<std::unique_ptr<Pinned>>;

// What the pin-allocator thread of a run makes: `n_sets` sets, the first `n_sized` of them with buffers of the estimated sizes -- a piece
// of `piece` bytes and two streams of `stream` bytes on the text route, else `reads` reads of `bytes` bytes in all.
struct PinPlan {
    bool text_route = false;
    size_t n_sets = 0, n_sized = 0;
    uint64_t piece = 0, stream = 0, reads = 0, bytes = 0;
};

// The page-locked buffers cost ~0.2 s per GB to allocate, so they are few (one set per batch between gather and
// format), sized from the input up front, allocated by their own thread while the parsers already run, and reused.
void fill_pin_pool(PinChannel& free_pins, const PinPlan& pl) {
    for (size_t i = 0; i < pl.n_sets; ++i) {
        std::unique_ptr<Pinned> pn;
        {
            std::lock_guard<std::mutex> l(g_pin_cache_m);  // a set left by an earlier run of this process
            if (!g_pin_cache.empty()) { pn = std::move(g_pin_cache.back()); g_pin_cache.pop_back(); }
        }
        if (!pn) pn = std::make_unique<Pinned>();
        if (i < pl.n_sized) {  // best effort: the stages grow what turns out too small
            if (pl.text_route) (void)(pn->text.ensure(pl.piece + 64) && pn->ptext.ensure(pl.stream) && pn->ntext.ensure(pl.stream));
            else (void)(pn->fw3.ensure(bgr::packed_plane_words(pl.reads, pl.bytes) * 8) && pn->hasn.ensure((pl.reads / 32 + 2) * 4) && pn->offs.ensure((pl.reads + 1) * 8) &&
                        pn->paths.ensure((8 * pl.reads + 4096) * 4) && pn->poffs.ensure((pl.reads + 1) * 8) && pn->status.ensure(pl.reads + 1));
        }
        if (!free_pins.push(std::move(pn))) break;
    }
}

// The end of a run: its page-locked sets wait for the next run of this process (bgr_host_cache_release).
void park_pin_sets(PinChannel& free_pins) {
    std::unique_ptr<Pinned> pn;
    std::lock_guard<std::mutex> l(g_pin_cache_m);
    while (free_pins.try_pop(pn)) if (g_pin_cache.size() < 96) g_pin_cache.push_back(std::move(pn));  // (the lanes of a split run on eight devices hold 64 sets)
}

}  // namespace

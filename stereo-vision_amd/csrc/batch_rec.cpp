// The lockstep machinery every batched entry shares (batch_rec.h): the recorder and its per-thread instances, the
// helper pool of the per-object host work, the stream wait and the count of threads inside a compute entry.
#include "batch_rec.h"

#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "svh_config.h"

namespace svh {

// Threads that are inside a compute entry of the Matcher / visual odometry right now (svh_matcher_push_back,
// svh_matcher_match_features, svh_vo_process, svh_vo_estimate_motion).  One or two = a single sequence (the
// latency path: spin on the stream, triangulate the outlier vote on the helper pool); more = several sequences
// share this GPU and the host cores: waits sleep between polls and the helper pool is left alone.  What counts
// is concurrent ACTIVITY, not how many objects exist (a process may hold many Matchers and drive one).
// SVH_MATCHER_WAIT=0 (spin) / 1 (sleep-poll) overrides the choice.
static std::atomic<int> g_active_callers{0};
static thread_local int t_entry_depth = 0;   // svh_vo_process calls the Matcher's entries: a thread counts once
ActiveCaller::ActiveCaller() {
    if (t_entry_depth++ == 0) g_active_callers.fetch_add(1, std::memory_order_relaxed);
}
ActiveCaller::~ActiveCaller() {
    if (--t_entry_depth == 0) g_active_callers.fetch_sub(1, std::memory_order_relaxed);
}
int wait_stream(void* stream) {
    hipStream_t s = (hipStream_t)stream;
    static const int forced = svh::env("SVH_MATCHER_WAIT") ? atoi(svh::env("SVH_MATCHER_WAIT")) : -1;   // 0 spin, 1 sleep-poll
    const bool poll = forced >= 0 ? forced == 1 : g_active_callers.load(std::memory_order_relaxed) > 2;
    if (!poll) return (int)hipStreamSynchronize(s);
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return (int)e;
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}
int active_callers() { return g_active_callers.load(std::memory_order_relaxed); }

thread_local BatchRec* t_rec = nullptr;

static std::atomic<int64_t> g_lockstep_counts[3];
void lockstep_count(int which, int64_t by) { g_lockstep_counts[which].fetch_add(by, std::memory_order_relaxed); }

hipError_t BatchRec::flush(hipStream_t s) {
    cursor = 0;
    if (slots.empty()) return hipSuccess;
    auto al = [](size_t n) { return (n + 255) & ~(size_t)255; };
    size_t need = 0;
    for (const Slot& sl : slots) need += al(sl.jobs.size());
    if (used + need > d_arena.cap) {
        // the arena may still be read by launches in flight: wait, then grow (a failed allocation leaves an arena of
        // size 0: the next flush allocates again)
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        const size_t want = std::max<size_t>(2 * (used + need), 256 * 1024);
        used = 0;
        if ((e = h_arena.grow(want)) != hipSuccess || (e = d_arena.grow(want)) != hipSuccess) {
            h_arena.release();
            d_arena.release();
            return e;
        }
    }
    size_t off = used;
    std::vector<size_t> at;
    for (const Slot& sl : slots) {
        memcpy(h_arena + off, sl.jobs.data(), sl.jobs.size());
        at.push_back(off);
        off += al(sl.jobs.size());
    }
    hipError_t e = hipMemcpyAsync(d_arena + used, h_arena + used, need, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    int64_t launches = 0;
    for (size_t i = 0; i < slots.size(); i++) {
        const Slot& sl = slots[i];
        if (sl.njobs > 0) {
            sl.fn(d_arena + at[i], sl.njobs, sl.gx, sl.gy, sl.lds, s);
            launches++;
        }
    }
    lockstep_count(2, launches);
    used += need;
    slots.clear();
    if (track) {
        last_stream = s;
        flush_pending = true;
    }
    return hipGetLastError();
}

hipError_t BatchRec::ensure_side() {
    for (int i = 0; i < kSide; i++) {
        if (side[i]) continue;
        hipError_t e = hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking);
        if (e != hipSuccess) return e;
        e = hipEventCreateWithFlags(&side_done[i], hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t BatchRec::join_side(hipStream_t s) {
    for (int i = 0; i < kSide; i++) {
        if (!side[i]) continue;
        hipError_t e = hipEventRecord(side_done[i], side[i]);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, side_done[i], 0);
        if (e != hipSuccess) {
            // (seen once in a while with several threads in the runtime: "event last recorded in a capturing
            // stream"; the host waits for the side stream instead)
            (void)hipGetLastError();
            e = hipStreamSynchronize(side[i]);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

void BatchRec::release() {
    h_arena.release();
    d_arena.release();
    for (int i = 0; i < kSide; i++) {
        if (side[i]) (void)hipStreamDestroy(side[i]);
        if (side_done[i]) (void)hipEventDestroy(side_done[i]);
        side[i] = nullptr;
        side_done[i] = nullptr;
    }
    flush_pending = false;
}

// The calling thread's recorder FOR A DEVICE (arena, side streams and events live on the device that was current
// when they were created; they are kept for the thread's lifetime).  Round 5: one recorder per (thread, device) --
// a thread that drove a lockstep batch on GPU 0 and then one on GPU 1 used to launch the second batch's kernels with
// a job table in GPU 0's memory.
namespace {
BatchRec& recorder_of(std::map<int, std::unique_ptr<BatchRec>>& recs, int device) {
    std::unique_ptr<BatchRec>& r = recs[device];
    if (!r) r.reset(new BatchRec());
    return *r;
}
}   // namespace
BatchRec& batch_recorder(int device) {
    static thread_local std::map<int, std::unique_ptr<BatchRec>> recs;
    return recorder_of(recs, device);
}
// a second one for svh_matcher_prefetch_batch: its launches are still in flight when the thread records the next
// phases of the frame before
BatchRec& prefetch_recorder(int device) {
    static thread_local std::map<int, std::unique_ptr<BatchRec>> recs;
    BatchRec& rec = recorder_of(recs, device);
    rec.track = true;
    return rec;
}

hipError_t BatchRec::reuse() {
    // (a stream wait, not an event: events recorded on this thread and waited for on streams that another thread
    // synchronises at the same moment came back as "event last recorded in a capturing stream" now and then)
    if (flush_pending) {
        const hipError_t e = hipStreamSynchronize(last_stream);
        if (e != hipSuccess) return e;
        flush_pending = false;
    }
    used = 0;
    return hipSuccess;
}

// Parked helper threads for the per-object HOST work of a batch call (outlier votes, prior statistics, row packing):
// parallel_for(n, fn) runs fn(0..n-1) on the helpers and the caller, returns when all are done.
// Several calls may be in flight at once (the prefetch thread packing frame t+1 while the caller votes on frame t,
// two calling threads with their own objects): every call is a job on the pool's list, the helpers take tasks from
// the jobs in turn, a caller works on its OWN job only (it returns as soon as that job is done).  Until round 5's
// last session the calls took turns on a mutex: the packing of the next frame and the votes of this one -- both on
// the critical path of a pipelined lockstep call -- waited for each other with helpers idle in the tail of either.
// SVH_POOL_SERIAL=1 keeps the take-turns form (A/B).
namespace {
class BatchPool {
    struct Job {
        const std::function<void(int)>* fn;
        int n;
        int next = 0, done = 0;
    };

public:
    void parallel_for(int n, const std::function<void(int)>& fn) {
        if (n <= 1) {
            for (int i = 0; i < n; i++) fn(i);
            return;
        }
        static const bool serial = svh::env("SVH_POOL_SERIAL") && atoi(svh::env("SVH_POOL_SERIAL")) != 0;
        std::unique_lock<std::mutex> one_call(call_mu_, std::defer_lock);
        if (serial) one_call.lock();
        Job job{&fn, n};
        {
            std::lock_guard<std::mutex> lk(mu_);
            const int want = std::min(n - 1, max_threads());
            while ((int)threads_.size() < want) threads_.emplace_back(&BatchPool::run, this);
            jobs_.push_back(&job);
        }
        cv_.notify_all();
        std::unique_lock<std::mutex> lk(mu_);
        while (job.next < job.n) {            // the caller's share of its own job
            const int i = take(&job);
            lk.unlock();
            fn(i);
            lk.lock();
            job.done++;
        }
        cv_done_.wait(lk, [&] { return job.done == job.n; });   // (the job left the list with its last task)
    }
    static BatchPool& get() {
        static BatchPool* p = new BatchPool();   // leaked on purpose: its threads outlive static destruction
        return *p;
    }

private:
    static int max_threads() {
        static const int n = std::max(1, std::min(15, (int)std::thread::hardware_concurrency() - 1));
        return n;
    }
    // mu_ held: next task of the job; a job whose tasks are all handed out leaves the list
    int take(Job* j) {
        const int i = j->next++;
        if (j->next == j->n) jobs_.erase(std::find(jobs_.begin(), jobs_.end(), j));
        return i;
    }
    void run() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return !jobs_.empty(); });
            Job* j = jobs_[turn_++ % jobs_.size()];   // the jobs in turn: neither call starves the other
            const int i = take(j);
            const std::function<void(int)>* fn = j->fn;
            lk.unlock();
            (*fn)(i);
            lk.lock();
            // (the job lives on its caller's stack until done == n, and this is the helper's last touch of it)
            if (++j->done == j->n) cv_done_.notify_all();
        }
    }
    std::mutex mu_, call_mu_;
    std::condition_variable cv_, cv_done_;
    std::vector<std::thread> threads_;
    std::vector<Job*> jobs_;      // jobs with tasks left to hand out
    size_t turn_ = 0;
};
}  // namespace
thread_local bool t_in_batch = false;

void batch_parallel_for(int n, const std::function<void(int)>& fn) {
    InBatchScope caller;
    BatchPool::get().parallel_for(n, [&](int i) {
        InBatchScope helper;
        fn(i);
    });
}

}  // namespace svh

extern "C" void svh_test_lockstep_counts(int64_t out[3]) {
    if (!out) return;
    for (int k = 0; k < 3; k++) out[k] = svh::g_lockstep_counts[k].load(std::memory_order_relaxed);
}

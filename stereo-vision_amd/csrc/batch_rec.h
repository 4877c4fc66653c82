// Batched launches for K Matcher / visual-odometry objects driven in lockstep (svh_matcher_*_batch,
// svh_vo_process_batch, svh_vo_mono_*_batch): while a recorder is installed on the calling thread, the kernel launchers
// (mlaunch_*, vlaunch_*) do not launch -- they append their arguments as one JOB to the recorder's slot for
// that call position.  Every object issues the same sequence of launcher calls (same parameters and image
// size: the batch entries check it), so slot c holds the K jobs of the c-th call, and flush() turns each slot
// into ONE launch of the kernel's batched form (blockIdx.z = job, grid = the largest job's).  A frame of K
// sequences then costs ~25 launches instead of ~45 K.
//
// This header and batch_rec.cpp are the one home of what the lockstep entries share on the host:
//   BatchRec, batch_recorder / prefetch_recorder   the recorder and the calling thread's instances per device
//   RecordingScope, InBatchScope                   the only code that sets t_rec / t_in_batch
//   run_recorded                                   ONE device phase of a lockstep entry: record, flush, wait -- with
//                                                  the one fallback for a sequence mismatch and the one rule for what
//                                                  an error leaves behind
//   check_batch                                    the checks in front of every batch entry
//   batch_parallel_for                             the per-object host work on the parked helper threads
//   wait_stream, ActiveCaller                      the stream wait, chosen by how many threads are inside an entry
#ifndef SVH_BATCH_REC_H
#define SVH_BATCH_REC_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "hip_guard.h"

namespace svh {

// launches the batched form of one kernel: jobs = device copy of the job table
typedef void (*BatchLaunchFn)(const void* jobs, int njobs, unsigned gx, unsigned gy, size_t lds, hipStream_t s);

struct BatchRec {
    struct Slot {
        BatchLaunchFn fn = nullptr;
        unsigned gx = 0, gy = 1;
        size_t lds = 0, job_bytes = 0;
        int njobs = 0;
        std::vector<uint8_t> jobs;
    };
    std::vector<Slot> slots;
    int cursor = 0;           // call position of the object being recorded
    bool broken = false;      // an object issued a different call sequence than the first one, or a job has no batched form
    // side streams (+ one event each) for work a lockstep call issues outside the recorded sequence: the image
    // uploads, several in flight at once
    static constexpr int kSide = 3;
    hipStream_t side[kSide] = {nullptr, nullptr, nullptr};
    hipEvent_t side_done[kSide] = {nullptr, nullptr, nullptr};
    // a recorder whose launches outlive the call that flushed them (prefetch): flush() notes its stream, reuse()
    // waits for that stream before the arena is written again
    bool track = false, flush_pending = false;
    hipStream_t last_stream = nullptr;
    hipError_t reuse();
    hipError_t ensure_side();                 // creates them on first use (current device)
    hipError_t join_side(hipStream_t s);      // s waits for everything issued on the side streams so far
    PinnedBuf<uint8_t> h_arena;   // pinned staging of the job tables
    HipBuf<uint8_t> d_arena;      // (same size, or both empty)
    size_t used = 0;              // advances per flush, reset by synced()

    void begin_object() { cursor = 0; }
    void reset() {   // forget recorded jobs (a new phase, or after a mismatch)
        slots.clear();
        cursor = 0;
        broken = false;
    }
    template <class J>
    void add(BatchLaunchFn fn, const J& job, unsigned gx, unsigned gy = 1, size_t lds = 0) {
        if ((size_t)cursor == slots.size()) {
            slots.emplace_back();
            slots.back().fn = fn;
            slots.back().job_bytes = sizeof(J);
        }
        Slot& s = slots[cursor++];
        if (s.fn != fn || s.job_bytes != sizeof(J)) {
            broken = true;
            return;
        }
        s.gx = gx > s.gx ? gx : s.gx;
        s.gy = gy > s.gy ? gy : s.gy;
        s.lds = lds > s.lds ? lds : s.lds;
        const size_t at = s.jobs.size();
        s.jobs.resize(at + sizeof(J));
        memcpy(s.jobs.data() + at, &job, sizeof(J));
        s.njobs++;
    }
    // job tables -> device (one copy), one launch per slot, slots cleared.  hipSuccess or the first error
    hipError_t flush(hipStream_t s);
    void synced() { used = 0; }   // the stream was waited for: the arena may be reused from its start
    void release();   // frees the arena and the side streams
    ~BatchRec() { release(); }
    BatchRec() = default;
    BatchRec(const BatchRec&) = delete;
    BatchRec& operator=(const BatchRec&) = delete;
};

// non-null: the launchers record into it.  Set by RecordingScope only
extern thread_local BatchRec* t_rec;
struct RecordingScope {   // `rec` is the calling thread's recorder until the scope ends, however it ends
    explicit RecordingScope(BatchRec& rec) { t_rec = &rec; }
    ~RecordingScope() { t_rec = nullptr; }
    RecordingScope(const RecordingScope&) = delete;
    RecordingScope& operator=(const RecordingScope&) = delete;
};
// inside a batch call: the outlier vote does not fork (the pool is the parallelism).  Set by InBatchScope only
extern thread_local bool t_in_batch;
struct InBatchScope {
    const bool was = t_in_batch;
    InBatchScope() { t_in_batch = true; }
    ~InBatchScope() { t_in_batch = was; }
    InBatchScope(const InBatchScope&) = delete;
    InBatchScope& operator=(const InBatchScope&) = delete;
};
// the calling thread's recorder for a device (arena and side streams are kept for the thread's lifetime)
BatchRec& batch_recorder(int device);
BatchRec& prefetch_recorder(int device);
// fn(0..n-1) on the library's parked helper threads and the caller (each inside an InBatchScope); returns when all
// are done
void batch_parallel_for(int n, const std::function<void(int)>& fn);

// Wait for a stream of a Matcher / visual-odometry object.  One or two threads inside the library's compute
// entries at this moment: the driver's spinning wait (lowest latency for the single-sequence case of
// stereomapper).  Three or more (K independent sequences driven concurrently on one GPU): polling with short
// sleeps, so that K host threads do not burn K cores spinning on a GPU they share.  The count is of
// concurrent callers (ActiveCaller below), not of objects that exist; SVH_MATCHER_WAIT=0/1 overrides.
int wait_stream(void* stream);   // returns a hipError_t value
// RAII marker of a thread inside a compute entry
struct ActiveCaller {
    ActiveCaller();
    ~ActiveCaller();
    ActiveCaller(const ActiveCaller&) = delete;
    ActiveCaller& operator=(const ActiveCaller&) = delete;
};
int active_callers();   // threads inside an entry right now

// What differs between the device phases of the lockstep entries (everything else is run_recorded):
struct Phase {
    const char* entry;           // whose line on stderr a failed HIP call gets ("Matcher", "VisualOdometry", ...)
    FiKind wait_kind;            // the fault hook's kind of the phase's stream waits (hip_guard.h: FI_none in the Matcher
                                 // and the stereo visual odometry, FI_wait in the mono one; their positions are fixed)
    // false (svh_matcher_prefetch_batch): the launches outlive the call.  Nothing is waited for, the recorder notes the
    // stream for its reuse() instead, and an error leaves the stream as it is
    bool wait = true;
    hipEvent_t ev[2] = {nullptr, nullptr};   // non-null (the mono phase times): recorded on the stream around the flush
    double* t_host = nullptr;    // non-null (SVH_MATCHER_TIMING): now_ms() after the recording [0], the flush [1], the end [2]
};
inline int phase_wait(const Phase& ph, hipStream_t s) {
    if (ph.wait_kind == FI_wait) SVH_HIP_TRY(ph.entry, wait, (hipError_t)wait_stream(s));
    else SVH_HIP_TRY(ph.entry, none, (hipError_t)wait_stream(s));
    return SVH_OK;
}

// the counters behind svh_test_lockstep_counts (hip_guard.h): 0 phases flushed, 1 phases one by one, 2 batched launches
void lockstep_count(int which, int64_t by = 1);

// One recorded device phase over the objects live[0..n-1] (null: 0..n-1) on stream `s`:
//   1. rec.reset(); enqueue(i) of every object behind begin_object(), with `rec` installed.  enqueue returns an SVH_*
//      code and issues the object's launcher calls -- into the recorder, or, called without one, on the object's own
//      stream.  An error ends the phase.
//   2. All objects issued the same sequence: flush(s) (kind copy), wait for s, synced().
//      They did not, or a launcher found a job that has no batched form (rec.broken: mlaunch_bin_index sets it when a
//      table's bin index needs more than the 156 KiB of LDS a recorded batch gets -- about 38 000 features, a 640 x 480
//      frame at full resolution with nms_n = 2 has 45 000): reset(), undo(), wait for s (work the caller issued on it
//      outside the recorder), then object by object enqueue(i) outside the recorder and wait_own(i), the wait for
//      object i's own stream(s).
//   3. hipGetLastError() (kind launch).
// Returns SVH_OK, kOneByOne (> 0) after the one-by-one pass, or the error (< 0).
// undo() takes back what the recording pass pretended (svh_matcher_match_features_batch: bin indices marked as built
// although no kernel built them); it runs before the one-by-one pass and on every failing exit.
// What an error leaves behind, whichever step failed: t_rec cleared, `s` synchronised (unguarded: no counter of the
// fault hook moves), the recorder reset() and synced() -- streams drained, objects usable.  With ph.wait == false
// the recorded pass neither waits nor calls synced(), the one-by-one pass still waits for s first (as the prefetch always
// did) but calls no wait_own, step 3 is left out (flush has checked its own launches), and an error only resets the
// recorder: reuse() waits before the arena is written again.
enum { kOneByOne = 1 };
template <class Enqueue, class WaitOwn, class Undo>
int run_recorded(BatchRec& rec, hipStream_t s, const int* live, int n, const Phase& ph, Enqueue enqueue,
                 WaitOwn wait_own, Undo undo) {
    struct OnError {
        BatchRec& rec;
        hipStream_t s;
        const bool wait;
        Undo& undo;
        bool armed = true;
        ~OnError() {
            if (!armed) return;
            rec.reset();
            if (wait) {
                (void)hipStreamSynchronize(s);
                rec.synced();
            }
            undo();
        }
    } on_error{rec, s, ph.wait, undo};
    rec.reset();
    int rc = SVH_OK;
    {
        RecordingScope recording(rec);
        for (int j = 0; j < n && !rc; j++) {
            rec.begin_object();
            rc = enqueue(live ? live[j] : j);
        }
    }
    if (rc) return rc;
    if (ph.t_host) ph.t_host[0] = now_ms();
    const bool one_by_one = rec.broken;
    if (one_by_one) {
        lockstep_count(1);
        rec.reset();
        undo();
        if ((rc = phase_wait(ph, s))) return rc;
        for (int j = 0; j < n; j++) {
            const int i = live ? live[j] : j;
            if ((rc = enqueue(i))) return rc;
            if (ph.wait && (rc = wait_own(i))) return rc;
        }
        if (ph.t_host) ph.t_host[1] = now_ms();
    } else {
        if (ph.ev[0]) (void)hipEventRecord(ph.ev[0], s);
        SVH_HIP_TRY(ph.entry, copy, rec.flush(s));   // (its one copy is the upload of the job tables)
        lockstep_count(0);
        if (ph.ev[1]) (void)hipEventRecord(ph.ev[1], s);
        if (ph.t_host) ph.t_host[1] = now_ms();
        if (ph.wait) {
            if ((rc = phase_wait(ph, s))) return rc;
            rec.synced();
        }
    }
    if (ph.wait) SVH_HIP_TRY(ph.entry, launch, hipGetLastError());
    if (ph.t_host) ph.t_host[2] = now_ms();
    on_error.armed = false;
    return one_by_one ? kOneByOne : SVH_OK;
}
inline void no_undo() {}

// The checks in front of a batch entry over objs[0..K-1] (`what`: "matcher", "object" in the message).  A null object
// and the same object twice are refused with SVH_ERR_BAD_ARG.  *uniform: all objects are on objs[0]'s device and
// same(i) -- the caller's "object i is configured like object 0" -- holds for each; such a batch can run in lockstep.
// stop_when_mixed (svh_matcher_push_back_batch, svh_matcher_match_features_batch): the objects behind the first one
// that differs are not looked at, their own entries refuse them when the batch runs one by one.
template <class T, class Same>
int check_batch(T* const* objs, int K, const char* what, bool* uniform, Same same, bool stop_when_mixed = false) {
    *uniform = true;
    for (int i = 0; i < K && (*uniform || !stop_when_mixed); i++) {
        if (!objs[i]) return fail(SVH_ERR_BAD_ARG, std::string("null ") + what + " in the batch");
        for (int j = 0; j < i; j++)
            if (objs[j] == objs[i]) return fail(SVH_ERR_BAD_ARG, std::string("the same ") + what + " twice in one batch");
        *uniform = *uniform && objs[i]->device == objs[0]->device && same(i);
    }
    return SVH_OK;
}

}  // namespace svh
#endif

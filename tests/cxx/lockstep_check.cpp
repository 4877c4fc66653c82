// Stand-alone CPU check of the lockstep machinery (stereo-vision_amd/csrc/batch_rec.h, batch_rec.cpp): the recorder,
// run_recorded -- its success path, its fallback for a call-sequence mismatch and what its error exits leave behind --
// and check_batch.  The HIP runtime entry points that the machinery references are host stubs defined here (malloc for
// the arenas, memcpy for the one copy, dummies for streams and events), so the program links no HIP runtime and runs
// without a GPU.  Two fake BatchLaunchFn log every batched launch and read every job back from the "device" table.
// Exit status 0: every check held; the failed checks are printed otherwise.  tests/test_lockstep_core.py builds and runs it,
// plain and under the address and undefined-behaviour sanitizers.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../stereo-vision_amd/csrc/batch_rec.h"
#include "../../stereo-vision_amd/csrc/svh_config.h"

// ---- the stub device layer
static int g_fail_copy = 0, g_fail_sync = 0;   // the next such call fails (once)
static int g_syncs = 0, g_copies = 0;
extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
    g_copies++;
    if (g_fail_copy) return g_fail_copy = 0, hipErrorUnknown;
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { *s = reinterpret_cast<hipStream_t>(new int(0)); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { delete reinterpret_cast<int*>(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) {
    g_syncs++;
    if (g_fail_sync) return g_fail_sync = 0, hipErrorUnknown;
    return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(new int(0)); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<int*>(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
}
namespace svh {
const char* env(const char*) { return nullptr; }   // no switch set
static std::vector<int> g_kinds;                    // the fault hook: fails nothing, notes the kind of every guarded call
bool fi_armed() { return true; }
bool fi_hit(FiKind kind) { return g_kinds.push_back(kind), false; }
}   // namespace svh

using namespace svh;

static int g_bad = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #cond);               \
            g_bad++;                                                       \
        }                                                                  \
    } while (0)

// ---- two launchers with two job types, as a .hip file's mlaunch_* would issue them
struct JobA { int32_t obj, pos; };
struct JobB { int32_t obj, pos; double pad[3]; };
struct Launch {
    int fn, njobs;
    unsigned gx, gy;
    size_t lds;
    const void* table;
    std::vector<int32_t> obj, pos;   // read back from the table
};
static std::vector<Launch> g_launched;   // through the batched form
template <class J, int F>
static void fake_batch(const void* jobs, int njobs, unsigned gx, unsigned gy, size_t lds, hipStream_t) {
    Launch l{F, njobs, gx, gy, lds, jobs, {}, {}};
    for (int k = 0; k < njobs; k++) {
        l.obj.push_back(static_cast<const J*>(jobs)[k].obj);
        l.pos.push_back(static_cast<const J*>(jobs)[k].pos);
    }
    g_launched.push_back(l);
}
static const BatchLaunchFn fnA = fake_batch<JobA, 0>, fnB = fake_batch<JobB, 1>;

struct Counts { int recorded = 0, plain = 0, waits = 0; };
static std::vector<Counts> g_obj;
static int g_undo = 0;
template <class J>
static void launcher(BatchLaunchFn fn, int obj, int pos, unsigned gx, unsigned gy, size_t lds) {
    J j{};
    j.obj = obj, j.pos = pos;
    if (t_rec) return t_rec->add(fn, j, gx, gy, lds);
    g_obj[obj].plain++;   // (the plain launch on the object's own stream)
}
static unsigned gx_of(int i, int c) { return 1 + (unsigned)((i * 7 + c * 3) % 11); }
static unsigned gy_of(int i, int c) { return 1 + (unsigned)((i * 5 + c) % 4); }
static size_t lds_of(int i, int c) { return 64 * (size_t)((i * 3 + c * 5) % 9); }

// what to break: object `odd` issues at position 1 another function (1) or the same function with another job size (2)
static int g_odd = -1, g_how = 0, g_fail_at = -1;
static int enqueue(int i) {
    if (i == g_fail_at) return SVH_ERR_BAD_DIMS;
    if (t_rec) g_obj[i].recorded++;
    launcher<JobA>(fnA, i, 0, gx_of(i, 0), gy_of(i, 0), lds_of(i, 0));
    if (i == g_odd && g_how == 1) launcher<JobA>(fnA, i, 1, gx_of(i, 1), gy_of(i, 1), lds_of(i, 1));
    else if (i == g_odd && g_how == 2) launcher<JobA>(fnB, i, 1, gx_of(i, 1), gy_of(i, 1), lds_of(i, 1));
    else launcher<JobB>(fnB, i, 1, gx_of(i, 1), gy_of(i, 1), lds_of(i, 1));
    launcher<JobA>(fnA, i, 2, gx_of(i, 2), gy_of(i, 2), lds_of(i, 2));
    return SVH_OK;
}
static int wait_own(int i) {
    g_obj[i].waits++;
    return SVH_OK;
}
static void undo() { g_undo++; }
static void fresh(int K) {
    g_launched.clear();
    g_kinds.clear();
    g_obj.assign(K, Counts());
    g_undo = 0;
    g_odd = g_fail_at = -1;
    g_how = 0;
}

static hipStream_t const kStream = reinterpret_cast<hipStream_t>(0x10);
static const Phase kPhase{"lockstep_check", FI_wait};

// one launch per call position, jobs in object order, grid and LDS the maxima, tables 256-aligned from `first`
static void check_success_launches(const BatchRec& rec, int K, size_t first) {
    CHECK(g_launched.size() == 3);
    size_t off = first;
    for (size_t c = 0; c < g_launched.size() && c < 3; c++) {
        const Launch& l = g_launched[c];
        CHECK(l.fn == (c == 1 ? 1 : 0));
        CHECK(l.njobs == K && (int)l.obj.size() == K);
        unsigned gx = 0, gy = 0;
        size_t lds = 0;
        for (int i = 0; i < K; i++) {
            CHECK(l.obj[i] == i && l.pos[i] == (int)c);
            gx = gx_of(i, c) > gx ? gx_of(i, c) : gx;
            gy = gy_of(i, c) > gy ? gy_of(i, c) : gy;
            lds = lds_of(i, c) > lds ? lds_of(i, c) : lds;
        }
        CHECK(l.gx == gx && l.gy == gy && l.lds == lds);
        const size_t at = (size_t)(static_cast<const uint8_t*>(l.table) - rec.d_arena.p);
        CHECK(at % 256 == 0 && at == off);
        off += ((size_t)K * (c == 1 ? sizeof(JobB) : sizeof(JobA)) + 255) & ~(size_t)255;
    }
}
static void check_left_clean(const BatchRec& rec) {
    CHECK(t_rec == nullptr);
    CHECK(rec.slots.empty() && rec.cursor == 0 && !rec.broken && rec.used == 0);
}

static void success_path(BatchRec& rec, int K) {
    fresh(K);
    const int syncs = g_syncs;
    CHECK(run_recorded(rec, kStream, nullptr, K, kPhase, enqueue, wait_own, undo) == SVH_OK);
    check_success_launches(rec, K, 0);
    check_left_clean(rec);
    CHECK(g_undo == 0);
    for (int i = 0; i < K; i++) CHECK(g_obj[i].recorded == 1 && g_obj[i].plain == 0 && g_obj[i].waits == 0);
    CHECK(g_syncs >= syncs + 1);   // the phase's stream was waited for
    CHECK((g_kinds == std::vector<int>{FI_copy, FI_wait, FI_launch}));   // the guarded calls of a phase, in order
    // ... and with the Matcher's and the stereo visual odometry's kind of wait, which the fault hook does not count
    fresh(K);
    CHECK(run_recorded(rec, kStream, nullptr, K, Phase{"lockstep_check", FI_none}, enqueue, wait_own, undo) == SVH_OK);
    CHECK((g_kinds == std::vector<int>{FI_copy, FI_launch}));
    check_success_launches(rec, K, 0);
}

// the recorder itself: phases that share the arena, its reuse after synced(), its growth
static void arena_rules() {
    BatchRec rec;
    const int K = 5;
    fresh(K);
    auto record = [&]() {
        RecordingScope recording(rec);
        for (int i = 0; i < K; i++) {
            rec.begin_object();
            CHECK(t_rec == &rec);
            enqueue(i);
        }
    };
    record();
    CHECK(t_rec == nullptr);
    CHECK(rec.flush(kStream) == hipSuccess);
    const size_t used1 = rec.used;
    CHECK(used1 > 0 && used1 % 256 == 0 && rec.d_arena.cap >= 256 * 1024);
    check_success_launches(rec, K, 0);
    std::vector<uint8_t> first(rec.d_arena.p, rec.d_arena.p + used1);
    // a second phase before synced(): behind the first phase's tables, which stay as they are
    g_launched.clear();
    record();
    CHECK(rec.flush(kStream) == hipSuccess);
    check_success_launches(rec, K, used1);
    CHECK(rec.used == 2 * used1 && memcmp(first.data(), rec.d_arena.p, used1) == 0);
    // after synced(): from the start again
    rec.synced();
    g_launched.clear();
    record();
    CHECK(rec.flush(kStream) == hipSuccess);
    check_success_launches(rec, K, 0);
    CHECK(rec.used == used1);
    // more jobs than the arena's 256 KB floor holds (on top of what is in use): it grows, no recorded job is lost
    struct JobBig { int32_t obj, pos; uint8_t pad[4088]; };
    const size_t cap0 = rec.d_arena.cap;
    const int big = 100;
    g_launched.clear();
    {
        RecordingScope recording(rec);
        for (int i = 0; i < big; i++) {
            rec.begin_object();
            for (int c = 0; c < 2; c++) {
                JobBig j{};
                j.obj = i, j.pos = c;
                rec.add(fake_batch<JobBig, 2>, j, 1 + i, 1, 0);
            }
        }
    }
    CHECK(rec.flush(kStream) == hipSuccess);
    CHECK(rec.d_arena.cap > cap0 && rec.d_arena.cap >= 2 * big * sizeof(JobBig) && rec.h_arena.cap == rec.d_arena.cap);
    CHECK(g_launched.size() == 2);
    for (size_t c = 0; c < g_launched.size(); c++) {
        const Launch& l = g_launched[c];
        CHECK(l.njobs == big && l.gx == (unsigned)big);
        for (int i = 0; i < big; i++) CHECK(l.obj[i] == i && l.pos[i] == (int)c);
    }
    CHECK(rec.ensure_side() == hipSuccess && rec.join_side(kStream) == hipSuccess);
    rec.release();
    CHECK(rec.d_arena.p == nullptr && rec.side[0] == nullptr);
}

static void mismatch(BatchRec& rec, int K, int how) {
    fresh(K);
    g_odd = 2, g_how = how;
    int seen_rec_outside = 0;
    auto enq = [&](int i) {
        if (g_obj[i].recorded == 1 && t_rec != nullptr) seen_rec_outside++;   // the second call of an object: no recorder
        return enqueue(i);
    };
    int undo_before_plain = -1;
    auto und = [&]() {
        int plain = 0;
        for (const Counts& c : g_obj) plain += c.plain;
        if (g_undo == 0) undo_before_plain = plain;
        g_undo++;
    };
    CHECK(run_recorded(rec, kStream, nullptr, K, kPhase, enq, wait_own, und) == kOneByOne);
    CHECK(g_launched.empty());            // nothing through the batched form
    CHECK(seen_rec_outside == 0);
    CHECK(g_undo == 1 && undo_before_plain == 0);   // once, before the one-by-one pass
    for (int i = 0; i < K; i++) CHECK(g_obj[i].recorded == 1 && g_obj[i].plain == 3 && g_obj[i].waits == 1);
    check_left_clean(rec);
    success_path(rec, K);
}

enum { ENQUEUE_FAILS, FLUSH_FAILS, WAIT_FAILS };
static void error_exit(BatchRec& rec, int K, int what, int at) {
    fresh(K);
    int want = SVH_ERR_HIP;
    if (what == ENQUEUE_FAILS) g_fail_at = at, want = SVH_ERR_BAD_DIMS;
    if (what == FLUSH_FAILS) g_fail_copy = 1;
    if (what == WAIT_FAILS) g_fail_sync = 1;
    const int syncs = g_syncs;
    CHECK(!t_in_batch);
    {
        InBatchScope in_batch;
        CHECK(run_recorded(rec, kStream, nullptr, K, kPhase, enqueue, wait_own, undo) == want);
        CHECK(t_in_batch);
    }
    CHECK(!t_in_batch);
    CHECK(g_fail_copy == 0 && g_fail_sync == 0);   // (the armed failure was met)
    check_left_clean(rec);
    CHECK(g_undo == 1);
    CHECK(g_syncs >= syncs + 1 + (what == WAIT_FAILS));   // drained, behind the failed wait too
    if (what != WAIT_FAILS) CHECK(g_launched.empty());
    for (int i = 0; i < K; i++) CHECK(g_obj[i].plain == 0 && g_obj[i].waits == 0);
    success_path(rec, K);
}

struct Obj { int device, cfg; };
static void validation() {
    Obj a{0, 1}, b{0, 1}, c{0, 1}, other_dev{1, 1}, other_cfg{0, 2};
    bool uniform = false;
    auto run = [&](std::vector<Obj*> v, bool stop = false) {
        Obj* const* o = v.data();
        return check_batch(o, (int)v.size(), "object", &uniform, [&](int i) { return o[i]->cfg == o[0]->cfg; }, stop);
    };
    CHECK(run({nullptr, &a, &b}) == SVH_ERR_BAD_ARG);
    CHECK(run({&a, &b, nullptr}) == SVH_ERR_BAD_ARG);
    CHECK(std::string(svh_last_error()).find("null object") != std::string::npos);
    CHECK(run({&a, &b, &a}) == SVH_ERR_BAD_ARG);
    CHECK(std::string(svh_last_error()).find("twice") != std::string::npos);
    CHECK(run({&a}) == SVH_OK && uniform);
    CHECK(run({}) == SVH_OK && uniform);
    CHECK(run({&a, &b, &c}) == SVH_OK && uniform);
    CHECK(run({&a, &b, &other_dev}) == SVH_OK && !uniform);
    CHECK(run({&a, &other_cfg, &b}) == SVH_OK && !uniform);
    // every object is looked at, also behind one that differs ...
    CHECK(run({&a, &other_dev, nullptr}) == SVH_ERR_BAD_ARG);
    CHECK(run({&a, &other_cfg, &a}) == SVH_ERR_BAD_ARG);
    // ... unless the entry leaves those to the single calls it falls back to
    CHECK(run({&a, &other_dev, nullptr}, true) == SVH_OK && !uniform);
    CHECK(run({&a, nullptr, &other_dev}, true) == SVH_ERR_BAD_ARG);
}

int main() {
    arena_rules();
    BatchRec& rec = batch_recorder(0);
    CHECK(&rec == &batch_recorder(0) && &rec != &batch_recorder(1) && &rec != &prefetch_recorder(0));
    for (int K : {1, 2, 5}) success_path(rec, K);
    for (int how : {1, 2}) mismatch(rec, 5, how);
    for (int at : {0, 2, 4}) error_exit(rec, 5, ENQUEUE_FAILS, at);
    error_exit(rec, 5, FLUSH_FAILS, 0);
    error_exit(rec, 5, WAIT_FAILS, 0);
    // the live list: objects 1 and 3 of 5
    {
        fresh(5);
        const int live[2] = {1, 3};
        CHECK(run_recorded(rec, kStream, live, 2, kPhase, enqueue, wait_own, undo) == SVH_OK);
        CHECK(g_launched.size() == 3 && g_launched[0].njobs == 2 && g_launched[0].obj[0] == 1 && g_launched[0].obj[1] == 3);
        CHECK(g_obj[0].recorded == 0 && g_obj[1].recorded == 1 && g_obj[3].recorded == 1);
    }
    // a phase that is not waited for (the prefetch): no wait, the arena is kept until reuse()
    {
        fresh(2);
        BatchRec& pr = prefetch_recorder(0);
        Phase ph{"lockstep_check", FI_wait};
        ph.wait = false;
        CHECK(run_recorded(pr, kStream, nullptr, 2, ph, enqueue, wait_own, undo) == SVH_OK);   // (allocates the arena)
        CHECK(pr.reuse() == hipSuccess);
        fresh(2);
        const int syncs = g_syncs;
        CHECK(run_recorded(pr, kStream, nullptr, 2, ph, enqueue, wait_own, undo) == SVH_OK);
        CHECK(g_launched.size() == 3 && pr.used > 0 && pr.flush_pending && pr.last_stream == kStream);
        CHECK(g_syncs == syncs && g_obj[0].waits == 0 && g_kinds == std::vector<int>{FI_copy});
        const int before = g_syncs;
        CHECK(pr.reuse() == hipSuccess && pr.used == 0 && !pr.flush_pending && g_syncs == before + 1);
    }
    // the helper pool: every index once, inside a batch scope
    {
        std::vector<int> hit(64, 0), in(64, 0);
        batch_parallel_for(64, [&](int i) { hit[i]++, in[i] = t_in_batch; });
        for (int i = 0; i < 64; i++) CHECK(hit[i] == 1 && in[i] == 1);
        CHECK(!t_in_batch);
    }
    validation();
    printf("lockstep_check: %d failed checks\n", g_bad);
    return g_bad ? 1 : 0;
}

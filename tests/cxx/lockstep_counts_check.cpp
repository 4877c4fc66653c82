// Stand-alone CPU check of the lockstep counters (svh_test_lockstep_counts, declared in csrc/hip_guard.h and kept in
// csrc/batch_rec.cpp): a recorded phase over K = 1, 2, 5 objects is counted as ONE flushed phase with a number of batched
// launches that does not depend on K, a call-sequence mismatch as ONE fallback with no launch, a phase that fails before
// its flush as nothing.  The device layer is the stub of lockstep_check.cpp in its smallest form: no HIP runtime is
// linked, nothing needs a GPU.  tests/test_lockstep_device.py builds and runs it, plain and under the address and
// undefined-behaviour sanitizers.  Exit status 0 and "lockstep_counts_check: 0 failed checks": every check held.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../stereo-vision_amd/csrc/batch_rec.h"
#include "../../stereo-vision_amd/csrc/svh_config.h"

// ---- the stub device layer
static int g_fail_copy = 0;   // the next copy fails (once)
extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
    if (g_fail_copy) return g_fail_copy = 0, hipErrorUnknown;
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { *s = reinterpret_cast<hipStream_t>(new int(0)); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { delete reinterpret_cast<int*>(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(new int(0)); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<int*>(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
}
namespace svh {
const char* env(const char*) { return nullptr; }   // no switch set
bool fi_armed() { return false; }
bool fi_hit(FiKind) { return false; }
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

struct JobA { int32_t obj, pos; };
struct JobB { int32_t obj, pos; double pad[3]; };
static int g_launches = 0, g_jobs = 0, g_plain = 0;
static void batch_a(const void*, int njobs, unsigned, unsigned, size_t, hipStream_t) { g_launches++, g_jobs += njobs; }
static void batch_b(const void*, int njobs, unsigned, unsigned, size_t, hipStream_t) { g_launches++, g_jobs += njobs; }

// three launcher calls per object; object `g_odd` issues another kernel at position 1 (a sequence mismatch); object
// `g_short` leaves out its last call (a job table with fewer jobs than objects is still one launch)
static int g_odd = -1, g_short = -1, g_fail_at = -1;
template <class J>
static void launcher(BatchLaunchFn fn, int obj, int pos) {
    J j{};
    j.obj = obj, j.pos = pos;
    if (t_rec) return t_rec->add(fn, j, 1u + (unsigned)obj, 1, 0);
    g_plain++;
}
static int enqueue(int i) {
    if (i == g_fail_at) return SVH_ERR_BAD_DIMS;
    launcher<JobA>(batch_a, i, 0);
    if (i == g_odd) launcher<JobA>(batch_a, i, 1);
    else launcher<JobB>(batch_b, i, 1);
    if (i != g_short) launcher<JobA>(batch_a, i, 2);
    return SVH_OK;
}
static int wait_own(int) { return SVH_OK; }

struct Delta {
    int64_t at[3];
    Delta() { svh_test_lockstep_counts(at); }
    bool is(int64_t flushed, int64_t fallback, int64_t launches) {
        int64_t now[3];
        svh_test_lockstep_counts(now);
        const bool ok = now[0] - at[0] == flushed && now[1] - at[1] == fallback && now[2] - at[2] == launches;
        if (!ok)
            printf("  counters moved by (%lld, %lld, %lld)\n", (long long)(now[0] - at[0]), (long long)(now[1] - at[1]),
                   (long long)(now[2] - at[2]));
        memcpy(at, now, sizeof(at));
        return ok;
    }
};

int main() {
    hipStream_t const stream = reinterpret_cast<hipStream_t>(0x10);
    const Phase phase{"lockstep_counts_check", FI_wait};
    BatchRec rec;
    int64_t start[3] = {-1, -1, -1};
    svh_test_lockstep_counts(start);
    CHECK(start[0] == 0 && start[1] == 0 && start[2] == 0);
    svh_test_lockstep_counts(nullptr);   // (ignored)
    // a recorded phase: one flush, three launches, whatever K is
    const int Ks[3] = {1, 2, 5};
    for (int K : Ks) {
        Delta d;
        g_launches = g_jobs = g_plain = 0;
        CHECK(run_recorded(rec, stream, nullptr, K, phase, enqueue, wait_own, no_undo) == SVH_OK);
        CHECK(d.is(1, 0, 3));
        CHECK(g_launches == 3 && g_jobs == 3 * K && g_plain == 0);
    }
    // a subset of the objects (live list), one of them one call short: still one phase and three launches
    {
        const int live[3] = {4, 0, 2};
        Delta d;
        g_launches = g_jobs = g_plain = 0;
        g_short = 2;
        CHECK(run_recorded(rec, stream, live, 3, phase, enqueue, wait_own, no_undo) == SVH_OK);
        g_short = -1;
        CHECK(d.is(1, 0, 3));
        CHECK(g_launches == 3 && g_jobs == 8);
    }
    // a phase over no object: flushed, no launch
    {
        Delta d;
        CHECK(run_recorded(rec, stream, nullptr, 0, phase, enqueue, wait_own, no_undo) == SVH_OK);
        CHECK(d.is(1, 0, 0));
    }
    // a sequence mismatch: one fallback, no batched launch, every object launched plainly
    {
        Delta d;
        g_launches = g_jobs = g_plain = 0;
        g_odd = 1;
        CHECK(run_recorded(rec, stream, nullptr, 5, phase, enqueue, wait_own, no_undo) == kOneByOne);
        g_odd = -1;
        CHECK(d.is(0, 1, 0));
        CHECK(g_launches == 0 && g_plain == 15);
    }
    // an enqueue that fails, and a flush whose copy fails: neither a flushed phase nor a fallback, nothing launched
    {
        Delta d;
        g_launches = 0;
        g_fail_at = 3;
        CHECK(run_recorded(rec, stream, nullptr, 5, phase, enqueue, wait_own, no_undo) == SVH_ERR_BAD_DIMS);
        g_fail_at = -1;
        CHECK(d.is(0, 0, 0));
        g_fail_copy = 1;
        CHECK(run_recorded(rec, stream, nullptr, 5, phase, enqueue, wait_own, no_undo) == SVH_ERR_HIP);
        CHECK(d.is(0, 0, 0));
        CHECK(g_launches == 0);
        // ... and the next phase counts as usual
        CHECK(run_recorded(rec, stream, nullptr, 5, phase, enqueue, wait_own, no_undo) == SVH_OK);
        CHECK(d.is(1, 0, 3));
    }
    // the recorder alone (no run_recorded): its launches are counted, no phase is
    {
        Delta d;
        {
            RecordingScope recording(rec);
            for (int i = 0; i < 2; i++) {
                rec.begin_object();
                enqueue(i);
            }
        }
        CHECK(rec.flush(stream) == hipSuccess);
        rec.synced();
        CHECK(d.is(0, 0, 3));
    }
    printf("lockstep_counts_check: %d failed checks\n", g_bad);
    return g_bad ? 1 : 0;
}

// What every host engine of libsvhip.so shares around a HIP call (svh_error.cpp): the text behind svh_last_error(), the
// one guard macro with its fault hook, and the owner of a device or pinned buffer.  Host code only.
#ifndef SVH_HIP_GUARD_H
#define SVH_HIP_GUARD_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/svh.h"

namespace svh {

int fail(int code, const std::string& msg);   // records the text behind svh_last_error(), returns `code`
double now_ms();                              // steady clock
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// ---------------------------------------------------------------- fault injection (tests)
// TEST HOOK, not part of the public C-ABI (include/svh.h does not declare it; tests bind it by name, the sanitizer
// drivers pass their SVH_TEST_FAIL_AT on): svh_test_fail_at("<kind>:<n>[:<count>]") arms it, "" / NULL disarms; the
// library itself never reads a specification from the environment.  The n-th (1-based) guarded call of that kind in
// this process, counted from the moment the specification is set, is NOT issued and reports an error instead, and so
// do the count-1 calls of the kind after it (count 0: every one from the n-th on).  The kind of a call is GIVEN at its
// call site, as the second argument of the guard, never matched from its text:
//   malloc  an allocation: hipMalloc / hipHostMalloc, directly or through HipBuf::grow (only a grow that allocates)
//   copy    hipMemcpy*Async / hipMemset*Async, and a recorder's flush (its one upload, then the phase's launches)
//   launch  the hipGetLastError() after a phase's launches
//   wait    stream / event waits (and queries in sleep-polls).  NOT every wait: the `(hipError_t)wait_stream(...)` sites
//           of the Matcher, the stereo visual odometry and the host-table Reconstruction are `none` on purpose -- they
//           never counted, and the positions the fault tests arm (n-th wait of a call) are fixed on that.  Do not
//           "correct" them without re-deriving those positions
//   none    everything else: guarded, never injected
// Boundary behaviour under a failure (tests/test_faults_gpu.py): the entry returns SVH_ERR_HIP, svh_last_error()
// names the call, one line goes to stderr, the lane / object is usable for the next call, nothing leaks.
enum FiKind { FI_none = -1, FI_malloc, FI_launch, FI_copy, FI_wait, FI_KINDS };
bool fi_armed();             // one relaxed load
bool fi_hit(FiKind kind);    // counts the call; true: it is the one to fail
// "svhip: <entry>: <last error>" on stderr, once per failing call
void report_hip_failure(const char* entry);
// a failed guarded call: svh_last_error() becomes "<expr>: <hipGetErrorString | injected failure (SVH_TEST_FAIL_AT)>",
// the stderr line is printed here under `entry` (null: the caller reports at its own entry), returns SVH_ERR_HIP
int hip_failed(const char* entry, const char* expr_text, bool injected, hipError_t e);

// Owner of one device (Pinned = false) or pinned host buffer.  Pointer and capacity (bytes) change together, so a
// growth that fails leaves "nothing allocated", which the next call repairs, never a stale pointer behind a capacity
// that says "fits".  A grow() within the capacity issues no HIP call at all (hipFree synchronises the device).  The
// destructor frees on the current device: an object's destroy selects its device and drains its stream first.
// Every device and pinned buffer of every host engine is one of these, and hipMalloc / hipHostMalloc / hipFree /
// hipHostFree are called here only: an engine has no list of buffers to free.  A set of buffers that follows a geometry
// (a Matcher view, a map, an ELAS lane) is a struct of owners, and "release" is the assignment of a fresh one.
template <typename T, bool Pinned = false>
struct HipBuf {
    T* p = nullptr;
    size_t cap = 0;   // bytes
    HipBuf() = default;
    HipBuf(const HipBuf&) = delete;
    HipBuf& operator=(const HipBuf&) = delete;
    HipBuf(HipBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    HipBuf& operator=(HipBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~HipBuf() { release(); }
    operator T*() const { return p; }
    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    // room for `bytes`; the contents are discarded when it has to allocate
    hipError_t grow(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p, bytes) : hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) p = nullptr;
        else cap = bytes;
        return e;
    }
};
template <typename T>
using PinnedBuf = HipBuf<T, true>;

}   // namespace svh
extern "C" int32_t svh_test_fail_at(const char* spec);
// TEST TAP of the lockstep machinery (batch_rec.cpp), bound by name like the hook above; process-wide, never reset:
//   out[0]  recorded phases that were flushed as batched launches (run_recorded)
//   out[1]  recorded phases that fell back to one-by-one (a call-sequence mismatch, or a job without a batched form)
//   out[2]  batched launches issued by BatchRec::flush
// A loop over the single entries moves none of them, so a parity test that also reads these shows lockstep happened.
extern "C" void svh_test_lockstep_counts(int64_t out[3]);
// TEST TAP of the ELAS engine's downward map copies (elas_engine.cpp, copy_map), bound by name like the hook above;
// process-wide: out[0] = bytes, out[1] = number of device-to-host map copies issued since the start or the last reset
// (a strided copy of several maps counts once); reset != 0 clears both after reading.  Parity of the 16-bit outputs
// cannot show that fewer bytes crossed PCIe (a library that downloaded floats and converted on the host would pass);
// this does.
extern "C" void svh_test_d2h_map_bytes(int64_t out[2], int32_t reset);
// TEST ACCESS to the device-frame path of the Matcher (matcher_engine.cpp), bound by name like the hook above:
//   svh_test_pack_rows      k_pack_rows alone: src_dev = h rows of w bytes, pitch apart, in device memory; bpl * h bytes
//                           (bpl a multiple of 16, >= w) come back in dst_host
//   svh_test_matcher_image  the packed image of a view as it lies on the device, h rows of bpl bytes; view = 2 * current
//                           + right (0 previous left .. 3 current right).  Returns the byte count (buf NULL: only that),
//                           0 for a view without a frame, or a negative SVH_ERR_*
//   svh_test_matcher_gain   Matcher::getGain over the object's two left frames for CALLER-GIVEN matches (real ones never
//                           reach the window clamps); path 0 = the host loop (needs host-pushed frames), 1 = k_gain.
//                           NaN, with svh_last_error() set, when it cannot run
extern "C" int32_t svh_test_pack_rows(const uint8_t* src_dev, int32_t w, int32_t h, int32_t pitch, int32_t bpl,
                                      uint8_t* dst_host);
extern "C" int64_t svh_test_matcher_image(svh_matcher* m, int32_t view, uint8_t* buf, size_t cap);
extern "C" float svh_test_matcher_gain(svh_matcher* m, const svh_p_match* matches, int32_t nm, const int32_t* inliers,
                                       int32_t n, int32_t path);
// TEST ACCESS to the arithmetic of the map view's thinning (view_engine.cpp), bound by name like the hook above; host code,
// needs no device: csrc/view_thin_core.h evaluated on n points (x, y, z, val).  key[i] = the voxel key, all ones for a
// point that falls into no voxel; home[i] = the slot its probe starts at in a table for n points, 0xFFFFFFFF for such a
// point; *capacity = that table's slots.  Any of the three outputs may be NULL
extern "C" int32_t svh_test_thin_keys(const float* xyzv, int64_t n, float voxel, uint64_t* key, uint32_t* home,
                                      uint64_t* capacity);
// TEST ACCESS to the arithmetic of the ground grid (grid_engine.cpp), bound by name like the hook above; host code, needs
// no device: csrc/grid_core.h evaluated with the parameters `p` (checked as svh_grid_create checks them).
//   svh_test_grid_points    per point (x, y, z, val): fate (0 low, 1 overhead, 2 outside, 3 unplaced), cell = ib * nx + ia
//                           (all ones when outside or unplaced) and, for a low point (else 0), the key of its height, the
//                           height in 1/1024 and the intensity byte.  Any output may be NULL
//   svh_test_grid_finalise  per accumulated cell: HMIN, HMAX, HMEAN, INTENSITY, CLASS and rgb[9] = its colour in the modes
//                           class, height, intensity.  Any output may be NULL
struct svh_grid_params;
extern "C" int32_t svh_test_grid_points(const svh_grid_params* p, const float* xyzv, int64_t n, int32_t* fate, uint32_t* cell,
                                        uint32_t* key, int32_t* q, uint8_t* v);
extern "C" int32_t svh_test_grid_finalise(const svh_grid_params* p, int64_t ncells, const int32_t* count,
                                          const int32_t* overhead, const uint32_t* kmin, const uint32_t* kmax,
                                          const int64_t* hsum, const uint64_t* vsum, float* hmin, float* hmax, float* hmean,
                                          uint8_t* intensity, uint8_t* cls, uint8_t* rgb);
//   svh_test_grid_trav        the traversability layer of a window of p->nx x p->nz cells from its CLASS, HMEAN and STATE
//                             planes: FLAGS, DIST2, COST and rgb[3] per cell = the cost colour (cell order).  Any output may
//                             be NULL
//   svh_test_grid_cost_table  the cost table of parameters `t` for a cell side: *reach, and the first min(reach^2 + 1, cap)
//                             bytes
struct svh_grid_trav_params;
extern "C" int32_t svh_test_grid_trav(const svh_grid_params* p, const svh_grid_trav_params* t, const uint8_t* cls,
                                      const float* hmean, const uint8_t* state, uint8_t* flags, int32_t* dist2, uint8_t* cost,
                                      uint8_t* rgb);
extern "C" int32_t svh_test_grid_cost_table(float cell, const svh_grid_trav_params* t, int32_t* reach, uint8_t* table,
                                            int64_t cap);

//   svh_test_grid_plan         csrc/grid_plan_core.h on the host: POT and DIR of a window of nx x nz cells under the offsets
//                              (oa, ob) from its COST plane and n goals (global cells), by the header's heap Dijkstra;
//                              returns the number of goals that count
//   svh_test_grid_path         the header's walk over a DIR plane from the window cell (a, b): *len cells, the first
//                              min(*len, cap) of them as global cells
//   svh_test_grid_plan_tile    the tile side the planner's kernels were built with
//   svh_test_grid_plan_device  NEEDS A DEVICE: the planner's kernels and round loop on a caller's COST plane (offsets 0);
//                              out[0] goals that counted, out[1] cells reached, out[2] rounds
struct svh_grid_plan_params;
extern "C" int32_t svh_test_grid_plan(const svh_grid_plan_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                                      const uint8_t* cost, const int32_t* goals, int32_t n, int32_t* pot, uint8_t* dir);
extern "C" int32_t svh_test_grid_path(int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* dir, int32_t a, int32_t b,
                                      int32_t* cells, int64_t cap, int64_t* len);
extern "C" int32_t svh_test_grid_plan_tile(void);
//   svh_test_grid_plan_rounds_per_wait  a measurement's switch: the rounds the host loop enqueues per wait become n (1..64,
//                              anything else only reads); returns what they were (4 unless changed)
extern "C" int32_t svh_test_grid_plan_rounds_per_wait(int32_t n);
extern "C" int32_t svh_test_grid_plan_device(int32_t nx, int32_t nz, const svh_grid_plan_params* p, const uint8_t* cost,
                                             const int32_t* goals, int32_t n, int32_t* pot, uint8_t* dir, int64_t out[3]);

//   svh_test_grid_front               csrc/grid_front_core.h on the host: FRONT and LABEL of a window of nx x nz cells under the
//                              offsets (oa, ob) from its STATE and COST planes, the first min(*n, cap) records of the kept
//                              components (*n of them) and stats[5]; flags, label, recs and stats may be NULL
//   svh_test_grid_front_device        NEEDS A DEVICE: the same through the kernels of csrc/grid_front_kernels.hip
//   svh_test_grid_front_label_device  NEEDS A DEVICE: the labelling stage alone (tile, merge, flatten) on an arbitrary mask
//                              (uint8, nonzero: a cell to label): LABEL; *launches = the kernels launched
//   svh_test_grid_front_tile   the tile side the labelling kernel was built with
struct svh_grid_front_params;
extern "C" int32_t svh_test_grid_front(const svh_grid_front_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state,
                                       const uint8_t* cost, uint8_t* flags, int32_t* label, int32_t* recs, int64_t cap, int64_t* n,
                                       int64_t* stats);
extern "C" int32_t svh_test_grid_front_device(const svh_grid_front_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                                              const uint8_t* state, const uint8_t* cost, uint8_t* flags, int32_t* label, int32_t* recs,
                                              int64_t cap, int64_t* n, int64_t* stats);
extern "C" int32_t svh_test_grid_front_label_device(int32_t nx, int32_t nz, const uint8_t* mask, int32_t* label, int64_t* launches);
extern "C" int32_t svh_test_grid_front_tile(void);

// The guard of every HIP call of the host engines: `kind` is one of none, malloc, copy, launch, wait (see above); a
// disarmed hook costs one relaxed load.  Returns hip_failed(...) out of the enclosing function on failure.
#define SVH_HIP_TRY(entry, kind, expr)                                                                  \
    do {                                                                                                \
        const bool inj_ = svh::FI_##kind != svh::FI_none && svh::fi_armed() && svh::fi_hit(svh::FI_##kind); \
        const hipError_t e_ = inj_ ? hipErrorUnknown : (expr);                                          \
        if (e_ != hipSuccess) return svh::hip_failed(entry, #expr, inj_, e_);                           \
    } while (0)
// ... and of a buffer's growth: counted (kind malloc) only when it allocates
#define SVH_HIP_GROW(entry, buf, bytes)                                                                 \
    do {                                                                                                \
        if ((buf).cap < (size_t)(bytes)) SVH_HIP_TRY(entry, malloc, (buf).grow(bytes));                 \
    } while (0)
// ... to `count` elements, at least one: kernels receive the pointer of an empty table too
#define SVH_HIP_GROW_N(entry, buf, count) \
    SVH_HIP_GROW(entry, buf, ((size_t)(count) > 0 ? (size_t)(count) : 1) * sizeof(*(buf).p))

#endif

// Sanitizer driver for the threaded HOST logic of the Matcher / visual-odometry engines
// (matcher_engine.cpp, vo_engine.cpp, batch_rec.cpp: ring buffer, pinned count read-backs, sleep-polling waits chosen by the
// number of concurrent callers, helper-pool bypass of the outlier vote, bucketing, RANSAC bookkeeping) with
// a STUB device layer: this file defines the HIP entry points those files use (host memory, streams
// that complete after a few queries) and their kernel launchers (deterministic synthetic feature tables,
// matches and motion results of realistic sizes).  No GPU, no libamdhip64: CPU only.
//   make -C stereo-vision_amd sanitize_viso    builds it with -fsanitize=thread and with
//                                              -fsanitize=address,undefined and runs both, K = 16 sequences
// What is checked: data races and memory errors of K VisualOdometryStereo objects driven from K threads at
// once (SURVEY 8(e) "replicas only"), one thread that creates and destroys Matchers meanwhile, and two threads
// that each drive K/2 objects in lockstep through svh_vo_process_batch (recorder, helper pool, phase barriers), and
// two threads that each drive a Reconstruction (track table, undo of a failed update, growth of the resident arrays),
// one thread with a resident-table Reconstruction beside a host-table one and one with three resident objects in lockstep
// (svh_recon_update_batch: double-buffered table, job table, an object sitting out, the way back from a failed batch),
// and two threads that each drive PlaneEstimation objects (single calls on host maps and a batch of three; the cache
// of raw draws, the transaction of a failed call, svh_plane_release), and two threads that each drive three
// VisualOdometryMono objects in lockstep (svh_vo_mono_process_batch with per-object replace, the pipelined loop and
// svh_vo_mono_process_matches_batch with lists of different lengths: the per-phase live lists, the host steps on the
// helper pool, the drain behind a failed phase).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../include/svh_plane.h"
#include "../stereo-vision_amd/csrc/hip_guard.h"
#include "../stereo-vision_amd/csrc/matcher_internal.h"
#include "../stereo-vision_amd/csrc/plane_internal.h"
#include "../stereo-vision_amd/csrc/recon_internal.h"
#include "../stereo-vision_amd/csrc/vo_internal.h"

// ---------------------------------------------------------------- stub HIP runtime
struct StubStream {
    std::atomic<int> pending{0};   // queries that still answer "not ready"
};
extern "C" {
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMalloc(void** p, size_t n) { *p = calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { *p = calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) {
    memcpy(d, s, n);
    if (st) reinterpret_cast<StubStream*>(st)->pending.store(2, std::memory_order_relaxed);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { *s = reinterpret_cast<hipStream_t>(new StubStream()); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { delete reinterpret_cast<StubStream*>(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { if (s) reinterpret_cast<StubStream*>(s)->pending.store(0, std::memory_order_relaxed); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(new int(0)); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<int*>(e); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = reinterpret_cast<hipEvent_t>(new int(0)); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.01f; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t s) {
    if (!s) return hipSuccess;
    StubStream* q = reinterpret_cast<StubStream*>(s);
    const int left = q->pending.load(std::memory_order_relaxed);
    if (left > 0) { q->pending.store(left - 1, std::memory_order_relaxed); return hipErrorNotReady; }
    return hipSuccess;
}
}

namespace svh {
// fault injection under the sanitizers: SVH_SAN_FAIL_EVERY=n makes every n-th HIP call the engines check fail
// (any kind), so that their error paths -- early returns out of recording passes, helper-pool phases, the prefetch
// hand-over -- run under TSan / ASan with 16 threads around them.  This program's own policy behind the shared
// declarations of hip_guard.h (the library's own hook, svh_fault_hook.cpp, is not linked)
static const long g_fi_every = getenv("SVH_SAN_FAIL_EVERY") ? atol(getenv("SVH_SAN_FAIL_EVERY")) : 0;
static std::atomic<long> g_fi_n{0};
bool fi_armed() { return g_fi_every > 0; }
bool fi_hit(FiKind) { return g_fi_every > 0 && (g_fi_n.fetch_add(1) + 1) % g_fi_every == 0; }

// ---------------------------------------------------------------- stub launchers
static uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }
// (the stub launchers run at once even while a batch is being recorded: the recorder stays empty, its flush is a no-op)
void mlaunch_upload(void*, const uint8_t* pinned, uint8_t* dev, size_t bytes) { memcpy(dev, pinned, bytes); }
void mlaunch_copy(void*, void* dst, const void* src, size_t bytes, int) { memcpy(dst, src, bytes); }
// a "device" frame is host memory here: the rows at bpl, zero behind w -- what k_pack_rows writes
void mlaunch_pack_rows(void*, const uint8_t* src, int w, int h, int pitch, uint8_t* dst, int bpl) {
    for (int v = 0; v < h; v++) {
        memcpy(dst + (size_t)v * bpl, src + (size_t)v * pitch, (size_t)w);
        memset(dst + (size_t)v * bpl + w, 0, (size_t)(bpl - w));
    }
}
// k_gain's indexing on the CPU (the sanitizers see every load of the two windows): row H is not loaded
void mlaunch_gain(void*, const GainView& prev, const GainView& cur, const float4* in, GainOut* out, int n) {
    auto mean = [](const GainView& V, float u, float v) {
        auto cl = [](int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); };
        const int u0 = cl((int)u - 3, V.W), u1 = cl((int)u + 3, V.W), v0 = cl((int)v - 3, V.H), v1 = cl((int)v + 3, V.H);
        uint32_t s = 0;
        for (int y = v0; y <= v1 && y < V.h; y++)
            for (int x = u0; x <= u1; x++) s += V.I[(size_t)y * V.bpl + x];
        return (float)s / (float)((u1 - u0 + 1) * (v1 - v0 + 1));
    };
    for (int q = 0; q < n; q++) {
        const float mp = mean(prev, in[q].x, in[q].y), mc = mean(cur, in[q].z, in[q].w);
        out[q].use = mp > 10 ? 1 : 0;
        out[q].ratio = out[q].use ? mc / mp : 0.f;
    }
}
void mlaunch_fill(void*, void* dst, int v, size_t bytes) { memset(dst, v, bytes); }
void mlaunch_half(void*, const uint8_t*, int, uint8_t*, int, int, int) {}
void mlaunch_filters(void*, const uint8_t*, int, int, int, uint8_t*, uint8_t*, int16_t*, int16_t*) {}
void mlaunch_half_filters(void*, const uint8_t*, int, int, int, uint8_t*, int, int, int, uint8_t*, uint8_t*) {}
int mnms_blocks(int extent, int n, int margin) { const int e = extent - 2 * margin; return e <= 0 ? 0 : (e + n) / (n + 1); }
void mlaunch_features(void*, const int16_t*, const int16_t*, const uint8_t* du, const uint8_t*, int w, int h, int, int n,
                      int, int margin, int scale, int4*, int32_t*, int32_t*, int32_t* table, int32_t* count) {
    // a plausible table: one feature per second NMS block, classes cycling, descriptor words from a hash
    const int bx = mnms_blocks(w, n, margin), by = mnms_blocks(h, n, margin);
    int k = 0;
    const uint32_t seed = mix((uint32_t)(uintptr_t)du ^ (uint32_t)n);
    for (int y = 0; y < by; y++)
        for (int x = (y & 1); x < bx; x += 2) {
            int32_t* r = table + 12 * k;
            r[0] = (margin + x * (n + 1) + (int)(mix(seed + k) % (unsigned)(n + 1))) * scale;
            r[1] = (margin + y * (n + 1) + (int)(mix(seed + 7 * k) % (unsigned)(n + 1))) * scale;
            r[2] = 0;
            r[3] = k & 3;
            for (int q = 4; q < 12; q++) r[q] = (int32_t)mix(seed + 13 * k + q);
            k++;
        }
    *count = k;
}
void mlaunch_features2(void* st, const int16_t* f1, const int16_t* f2, const uint8_t* du, const uint8_t* dv, int w, int h,
                       int bpl, int tau, int margin, int scale, int n_a, int4* sa, int32_t* fa, int32_t* oa, int32_t* ta,
                       int32_t* ca, int n_b, int4* sb, int32_t* fb, int32_t* ob, int32_t* tb, int32_t* cb, int32_t* host_counts) {
    mlaunch_features(st, f1, f2, du, dv, w, h, bpl, n_a, tau, margin, scale, sa, fa, oa, ta, ca);
    mlaunch_features(st, f1, f2, du, dv, w, h, bpl, n_b, tau, margin, scale, sb, fb, ob, tb, cb);
    host_counts[0] = *ca;
    host_counts[1] = *cb;
}
void mlaunch_bin_index(void*, const BinJobs&, int, int, int, int, int, int32_t*) {}
void mlaunch_match(void*, const MatchParams& P, const FeatView& m1p, const FeatView&, const FeatView& m1c,
                   const FeatView&, int nquery_cap, const float*, int, svh_p_match*, int32_t*, int32_t*,
                   svh_p_match* out, int32_t* out_count, int32_t* out_count_host) {
    // every third feature of the current left image "matches": consistent small flow and disparity
    const int nc = *m1c.count, np = *m1p.count;
    int k = 0;
    for (int i = 0; i < nc && k < nquery_cap; i += 3) {
        const int32_t* r = m1c.rec + 12 * i;
        svh_p_match m;
        memset(&m, 0, sizeof(m));
        const float d = 8.f + (float)(mix((uint32_t)i) % 40u), fu = (float)(mix((uint32_t)i * 3u) % 5u) - 2.f;
        m.u1c = (float)r[0]; m.v1c = (float)r[1]; m.i1c = i;
        m.u2c = m.u1c - d;   m.v2c = m.v1c;       m.i2c = i;
        m.u1p = m.u1c + fu;  m.v1p = m.v1c + 1.f; m.i1p = np > 0 ? i % np : 0;
        m.u2p = m.u1p - d;   m.v2p = m.v1p;       m.i2p = m.i1p;
        if (P.method < 2) { m.u2c = m.u2p = -1; m.v2c = m.v2p = -1; m.i2c = m.i2p = -1; }
        out[k++] = m;
    }
    *out_count = k;
    if (out_count_host) *out_count_host = k;
}
void mlaunch_refine(void*, svh_p_match* m, const int32_t* count, int, int, int, const SobelView&, const SobelView&,
                    const SobelView&, const SobelView&, int parabolic, int32_t*, svh_p_match* compacted,
                    int32_t* compacted_count) {
    if (!parabolic) return;
    memcpy(compacted, m, sizeof(svh_p_match) * (size_t)*count);
    *compacted_count = *count;
}
void vlaunch_estimate(void*, const svh_p_match*, int N, const int32_t*, int, const VoCalib&, double*, int32_t*, uint8_t*,
                      double*, double*, VoResult* out, int32_t* out_inliers) {
    out->success = N >= 6;
    out->n_inliers = N / 2;
    out->best = N >= 6 ? 0 : -1;
    for (int k = 0; k < 6; k++) out->tr[k] = 1e-3 * (k + 1);
    for (int i = 0; i < N / 2; i++) out_inliers[i] = 2 * i;
}
// VisualOdometryMono (vo_mono_engine.cpp): every second match an inlier of hypothesis 0, candidate 0 puts the points
// in front at growing depth
void mlaunch_ransac(void*, const float*, int32_t N, const int32_t*, int32_t iters, double, double*, int32_t*,
                    int32_t* out_sel, uint8_t* out_flags, int32_t* out_counts) {
    for (int32_t h = 0; h < iters; h++) out_counts[h] = h == 0 ? (N + 1) / 2 : 0;
    for (int32_t i = 0; i < N; i++) out_flags[i] = i % 2 == 0;
    out_sel[0] = 0;
    out_sel[1] = (N + 1) / 2;
}
void mlaunch_chiral(void*, const float*, int32_t N, const double*, double*, uint8_t*, double* out_X,
                    int32_t* out_cand) {
    out_cand[0] = 0;
    for (int k = 0; k < 4; k++) out_cand[1 + k] = k == 0 ? N : 0;
    for (int32_t i = 0; i < N; i++) {
        out_X[i] = 0.1 * i;
        out_X[N + i] = 0.5;
        out_X[2 * N + i] = 1.0 + i;
        out_X[3 * N + i] = 1.0;
    }
}
void mlaunch_plane(void*, const double* d, int32_t n, double, double, double* sums) {
    for (int32_t i = 0; i < n; i++) sums[i] = 1.0 + (d[i] > 0);
}
// Reconstruction (recon_engine.cpp): every third lost track of two or more frames is accepted at its first pixel
void rlaunch_tracks(void*, const int32_t* offs, const int32_t*, const int32_t*, const float* px, int32_t n_lost, int32_t,
                    const double*, int32_t, const recon::Settings&, int32_t* code, float* xyz, float* points,
                    int32_t n_points, int32_t* out_code, float* out_xyz, int32_t* out_count) {
    for (int32_t t = 0; t < n_lost; t++) {
        const bool take = t % 3 == 0 && offs[t + 1] - offs[t] >= 2;
        code[t] = out_code[t] = take ? 6 : 5;
        for (int k = 0; k < 3; k++) xyz[3 * t + k] = out_xyz[3 * t + k] = k < 2 ? px[2 * offs[t] + k] : 1.f;
        if (take) {
            for (int k = 0; k < 3; k++) points[3 * (size_t)n_points + k] = xyz[3 * t + k];
            n_points++;
        }
    }
    out_count[0] = n_points;
}
// the resident form (recon_internal.h): the seven kernels' work over each job, serially, with the outcome rule above
void rlaunch_resident(void*, const ReconJob* jobs, int32_t K, int32_t, int32_t, int32_t, uint32_t) {
    for (int32_t k = 0; k < K; k++) {
        const ReconJob& a = jobs[k];
        for (int seg = 0; seg < 2; seg++)
            if (a.up_bytes[seg]) memcpy(a.up_dst[seg], a.up_src[seg], a.up_bytes[seg]);
        for (int32_t i = 0; i < a.tbl; i++) a.track_idx[i] = -1;
        for (int32_t t = 0; t < a.n_old; t++) a.claim[t] = INT32_MAX;
        for (int i = 0; i < RT_HDR; i++) a.hdr[i] = 0;
        for (int32_t t = 0; t < a.n_old; t++)
            if (a.a_last[t] >= 0 && a.a_last[t] < a.tbl && a.track_idx[a.a_last[t]] < t) a.track_idx[a.a_last[t]] = t;
        for (int32_t i = 0; i < a.n; i++) {
            int32_t idx = -1;
            if (a.m[i].i1p < 0 || a.m[i].i1p >= a.max_index || a.m[i].i1c < 0 || a.m[i].i1c >= a.max_index)
                a.hdr[RT_ERROR] |= RT_BAD_INDEX;
            else
                idx = a.track_idx[a.m[i].i1p];
            if (idx >= 0 && a.claim[idx] > i) a.claim[idx] = i;
            a.midx[i] = idx;
        }
        int32_t nb = 0, px = 0, n_lost = 0, points = a.n_points;
        if (!a.hdr[RT_ERROR]) {
            auto put = [&](const float* from, int32_t len, const svh_p_match& q, int32_t first) {
                a.b_offs[nb] = px;
                if (from) memcpy(a.b_px + 2 * (size_t)px, from, 8 * (size_t)len);
                px += len;
                if (!from) { a.b_px[2 * (size_t)px] = q.u1p; a.b_px[2 * (size_t)px + 1] = q.v1p; px++; }
                a.b_px[2 * (size_t)px] = q.u1c; a.b_px[2 * (size_t)px + 1] = q.v1c; px++;
                a.b_first[nb] = first;
                a.b_last[nb++] = q.i1c;
            };
            for (int32_t t = 0; t < a.n_old; t++) {
                if (a.claim[t] != INT32_MAX)
                    put(a.a_px + 2 * (size_t)a.a_offs[t], a.a_offs[t + 1] - a.a_offs[t], a.m[a.claim[t]], a.a_first[t]);
                else
                    a.lost[n_lost++] = t;
            }
            a.hdr[RT_EXTENDED] = nb;
            for (int32_t i = 0; i < a.n; i++)
                if (!(a.midx[i] >= 0 && a.claim[a.midx[i]] == i)) put(nullptr, 0, a.m[i], a.frame_prev);
            a.b_offs[nb] = px;
            a.hdr[RT_CREATED] = nb - a.hdr[RT_EXTENDED];
            a.hdr[RT_LOST] = n_lost;
            a.hdr[RT_PIXELS] = px;
            for (int32_t g = 0; g < n_lost; g++) {
                const int32_t t = a.lost[g];
                const bool take = g % 3 == 0 && a.a_offs[t + 1] - a.a_offs[t] >= 2;
                a.code[g] = a.out_code[g] = take ? 6 : 5;
                for (int c = 0; c < 3; c++)
                    a.xyz[3 * g + c] = a.out_xyz[3 * g + c] = c < 2 ? a.a_px[2 * (size_t)a.a_offs[t] + c] : 1.f;
                if (take) {
                    for (int c = 0; c < 3; c++) a.points[3 * (size_t)points + c] = a.xyz[3 * g + c];
                    points++;
                }
            }
        }
        for (int i = 0; i < RT_HDR; i++) a.out_hdr[i] = i == RT_POINTS ? points : a.hdr[i];
    }
}
// PlaneEstimation (plane_engine.cpp): the kernels' work with plane_core.h on the host ("device" memory is host memory)
void planelaunch_grid(void*, const PlaneDev& P, int32_t nmaps, const plane::Lattice& L, int32_t step, int32_t row0) {
    for (int32_t m = 0; m < nmaps; m++) {
        int32_t n = 0;
        for (int32_t t = 0; t < L.nu * L.nv; t++) {
            const int32_t u = plane::cell_u(L, t), v = plane::cell_v(L, t);
            const float d = P.maps[m][(size_t)(v - row0) * step + u];
            if (!plane::cell_kept(d)) continue;
            const size_t at = (size_t)m * P.cap + n++;
            P.lu[at] = (float)u; P.lv[at] = (float)v; P.ld[at] = d;
        }
        P.n_list[m] = n;
    }
}
void planelaunch_vote(void*, const PlaneDev& P, int32_t nmaps, int32_t, double thr) {
    for (int32_t m = 0; m < nmaps; m++) {
        const size_t o = (size_t)m * P.cap;
        const int32_t n = P.n_list[m];
        int32_t best = -1, best_count = 0;
        for (int32_t h = 0; h < P.S; h++) {
            const int32_t* s = P.samples + ((size_t)m * P.S + h) * 4;
            double* abc = P.planes + ((size_t)m * P.S + h) * 3;
            plane::fit_indexed(P.lu + o, P.lv + o, P.ld + o, s + 1, s[0], abc);
            int32_t c = 0;
            for (int32_t i = 0; i < n; i++)
                c += plane::is_inlier(abc[0], abc[1], abc[2], P.lu[o + i], P.lv[o + i], P.ld[o + i], thr);
            P.counts[(size_t)m * P.S + h] = c;
            if (c > best_count) { best_count = c; best = h; }
        }
        int32_t k = 0;
        if (best >= 0) {
            const double* abc = P.planes + ((size_t)m * P.S + best) * 3;
            for (int32_t i = 0; i < n; i++)
                if (plane::is_inlier(abc[0], abc[1], abc[2], P.lu[o + i], P.lv[o + i], P.ld[o + i], thr)) P.inl[o + k++] = i;
        }
        P.sel[2 * m] = best;
        P.sel[2 * m + 1] = k;
    }
}
}  // namespace svh

// ---------------------------------------------------------------- driver
int main(int argc, char** argv) {
    const int K = argc > 1 ? atoi(argv[1]) : 16, frames = argc > 2 ? atoi(argv[2]) : 12;
    const int W = 640, H = 200;
    std::atomic<int> bad{0};
    // a check of this driver that did not hold: counted, and named on stderr by its line
#define BAD() (fprintf(stderr, "sanitize_viso: check at line %d failed\n", __LINE__), bad++)
    std::atomic<long> matches{0}, injected{0};
    const bool inject = svh::fi_armed();
    // a negative return is a failure of the run -- unless failures are being injected: then it must be SVH_ERR_HIP
    // (or the bad-argument answer of an entry whose hand-over was lost with the failed call), and is counted
    auto check = [&](int32_t rc) {
        if (rc >= 0) return;
        if (inject && (rc == SVH_ERR_HIP || rc == SVH_ERR_BAD_ARG)) injected++;
        else BAD();
    };
    // Every 1st, 2nd or 3rd call fails: first, on this thread alone (the failing calls are then the same in every run), a
    // fresh Matcher, a fresh stereo object and a fresh mono object, each driven eight times -- their first allocations
    // fail one after the other, the mono engine's first-call block (stream, then three buffers) among them, and the
    // calls after a failed one must not trust what it left behind
    if (inject && svh::g_fi_every <= 3) {
        std::vector<uint8_t> I((size_t)W * H);
        for (size_t i = 0; i < I.size(); i++) I[i] = (uint8_t)(svh::mix((uint32_t)i) >> 24);
        const int32_t dims[3] = {W, H, W};
        svh_matcher_params mp;
        svh_matcher_params_default(&mp);
        svh_matcher* m = svh_matcher_create(&mp);
        svh_vo_params sp;
        svh_vo_params_default(&sp);
        sp.f = 645.2; sp.cu = 320.0; sp.cv = 100.0; sp.base = 0.57;
        svh_vo* st = svh_vo_create(&sp);
        svh_vo_mono_params op;
        svh_vo_mono_params_default(&op);
        op.f = 645.2; op.cu = 320.0; op.cv = 100.0; op.height = 1.6; op.pitch = -0.08;
        op.ransac_iters = 50;
        op.motion_threshold = 1e6;
        svh_vo* mono = svh_vo_mono_create(&op);
        if (!m || !st || !mono) BAD();
        std::vector<svh_p_match> pm(40);
        for (int k = 0; k < 40; k++) {
            memset(&pm[k], 0, sizeof(pm[k]));
            pm[k].u1p = (float)(svh::mix((uint32_t)k) % 600u); pm[k].v1p = (float)(svh::mix((uint32_t)(3 * k)) % 180u);
            pm[k].u1c = pm[k].u1p + 2.f + (float)(k % 3); pm[k].v1c = pm[k].v1p + 1.f;
        }
        for (int r = 0; r < 8 && m && st && mono; r++) {
            check(svh_matcher_push_back(m, I.data(), I.data(), dims, 0));
            check(svh_matcher_match_features(m, 2, nullptr));
            check(svh_vo_process(st, I.data(), I.data(), dims, 0));
            check(svh_vo_process_matches(mono, pm.data(), 40));
            check(svh_vo_mono_process(mono, I.data(), dims, 0));
        }
        svh_matcher_destroy(m);
        svh_vo_destroy(st);
        svh_vo_destroy(mono);
    }
    auto sequence = [&](int id) {
        svh_vo_params p;
        svh_vo_params_default(&p);
        p.f = 645.2; p.cu = 320.0; p.cv = 100.0; p.base = 0.57;
        svh_vo* vo = svh_vo_create(&p);
        if (!vo) { BAD(); return; }
        std::vector<uint8_t> I1((size_t)W * H), I2((size_t)W * H);
        const int32_t dims[3] = {W, H, W};
        for (int f = 0; f < frames; f++) {
            for (size_t i = 0; i < I1.size(); i++) {
                I1[i] = (uint8_t)(svh::mix((uint32_t)(i + 977 * f + 31 * id)) >> 24);
                I2[i] = (uint8_t)(svh::mix((uint32_t)(i + 977 * f + 31 * id + 5)) >> 24);
            }
            // host and device pushes alternate on one object (a "device" frame is host memory under the stub layer);
            // the gain then takes the host loop or the k_gain path, and a few indices lie past the match list
            if (f & 1) check(svh_vo_process_device(vo, I1.data(), I2.data(), dims, 0));
            else check(svh_vo_process(vo, I1.data(), I2.data(), dims, 0));
            matches += svh_vo_num_matches(vo);
            std::vector<int32_t> inl((size_t)svh_vo_get_inliers(vo, nullptr, 0) + 2, 1 << 20);
            (void)svh_vo_get_inliers(vo, inl.data(), (int32_t)inl.size() - 2);
            matches += svh_vo_get_gain(vo, inl.data(), (int32_t)inl.size()) > 0 ? 1 : 0;
        }
        svh_vo_destroy(vo);
    };
    std::vector<std::thread> th;
    for (int k = 0; k < K; k++) th.emplace_back(sequence, k);
    // a Matcher used on its own from one more thread, created and destroyed over and over meanwhile
    th.emplace_back([&] {
        for (int r = 0; r < 3 * frames; r++) {
            svh_matcher_params mp;
            svh_matcher_params_default(&mp);
            svh_matcher* m = svh_matcher_create(&mp);
            std::vector<uint8_t> I((size_t)W * H, (uint8_t)(r * 7));
            const int32_t dims[3] = {W, H, W};
            for (int f = 0; f < 2; f++) {
                check(svh_matcher_push_back(m, I.data(), I.data(), dims, 0));
                check(svh_matcher_match_features(m, 2, nullptr));
            }
            svh_matcher_destroy(m);
        }
    });
    // two more threads, each driving K/2 objects in lockstep (svh_vo_process_batch: recorder, helper pool, phases)
    auto lockstep = [&](int id) {
        const int n = K / 2 > 1 ? K / 2 : 2;
        svh_vo_params p;
        svh_vo_params_default(&p);
        p.f = 645.2; p.cu = 320.0; p.cv = 100.0; p.base = 0.57;
        std::vector<svh_vo*> vs(n);
        for (int i = 0; i < n; i++) vs[i] = svh_vo_create(&p);
        // two sets of image buffers: a frame handed over early is read (prefetch thread) until it is TAKEN by the
        // next call, so the caller fills the other set meanwhile -- the contract of svh_vo_prefetch_batch
        std::vector<std::vector<uint8_t>> Ia[2], Ib[2];
        for (int q = 0; q < 2; q++) {
            Ia[q].assign(n, std::vector<uint8_t>((size_t)W * H));
            Ib[q] = Ia[q];
        }
        std::vector<const uint8_t*> p1(n), p2(n);
        std::vector<int32_t> ok(n);
        const int32_t dims[3] = {W, H, W};
        for (int f = 0; f < frames; f++) {
            std::vector<std::vector<uint8_t>>&I1 = Ia[f & 1], &I2 = Ib[f & 1];
            for (int i = 0; i < n; i++) {
                for (size_t j = 0; j < I1[i].size(); j++) {
                    I1[i][j] = (uint8_t)(svh::mix((uint32_t)(j + 977 * f + 31 * i + 7777 * id)) >> 24);
                    I2[i][j] = (uint8_t)(svh::mix((uint32_t)(j + 977 * f + 31 * i + 7777 * id + 5)) >> 24);
                }
                p1[i] = I1[i].data();
                p2[i] = I2[i].data();
            }
            // thread 1: images with the call; thread 2: the pipelined loop (frame f handed over one call earlier)
            if (id == 1) {
                check(svh_vo_process_batch(vs.data(), n, p1.data(), p2.data(), dims, 0, ok.data()));
            } else {
                if (f == 0) {
                    check(svh_vo_prefetch_batch(vs.data(), n, p1.data(), p2.data(), dims));
                } else {
                    // (processes frame f - 1, hands over frame f)
                    const int32_t rc = svh_vo_process_next_batch(vs.data(), n, p1.data(), p2.data(), dims, 0, ok.data());
                    check(rc);
                    // a failed call may have lost the hand-over of frame f: hand it over again (refused when it is pending)
                    if (rc < 0 && inject) (void)svh_vo_prefetch_batch(vs.data(), n, p1.data(), p2.data(), dims);
                }
            }
            for (int i = 0; i < n; i++) matches += svh_vo_num_matches(vs[i]);
        }
        for (svh_vo* v : vs) svh_vo_destroy(v);
    };
    th.emplace_back(lockstep, 1);
    th.emplace_back(lockstep, 2);
    // two Reconstruction objects on threads of their own: tracks that live one to five frames, an empty update
    auto reconstruct = [&](int id) {
        svh_recon* r = svh_recon_create();
        if (!r) { BAD(); return; }
        const double Tr[16] = {1, 0, 0, 0.05, 0, 1, 0, 0, 0, 0, 1, -0.8, 0, 0, 0, 1};
        if (svh_recon_update(r, nullptr, 0, Tr, 1, 2, 30, 2) != SVH_ERR_BAD_ARG) BAD();   // not calibrated yet
        check(svh_recon_set_calibration(r, 645.2, 635.9, 194.1));
        if (svh_recon_set_calibration(r, 645.2, 635.9, 194.1) != SVH_ERR_BAD_ARG) BAD();
        const int n = 600;
        for (int f = 0; f < 3 * frames; f++) {
            std::vector<svh_p_match> m;
            for (int i = 0; i < n && f % 7 != 5; i++) {
                if (svh::mix((uint32_t)(i + 131 * f + 7 * id)) % 5u == 0) continue;   // this feature is not matched now
                svh_p_match q;
                memset(&q, 0, sizeof(q));
                q.u1p = 10.f + i + f; q.v1p = 20.f + (i % 37); q.i1p = i;
                q.u1c = q.u1p + 1.f;  q.v1c = q.v1p;           q.i1c = i;
                m.push_back(q);
            }
            check(svh_recon_update(r, m.data(), (int32_t)m.size(), Tr, 1, 2, 30, 2));
            std::vector<float> p(3 * (size_t)svh_recon_num_points(r) + 3);
            check(svh_recon_get_points(r, p.data(), svh_recon_num_points(r)));
            matches += svh_recon_num_tracks(r);
        }
        svh_recon_destroy(r);
    };
    th.emplace_back(reconstruct, 1);
    th.emplace_back(reconstruct, 2);
    // the resident form: one thread with a resident object next to a host-table object fed the same updates (their
    // track and point counts must agree), one thread with three resident objects in lockstep, one of which sits every
    // fourth update out, and a batch that is refused
    auto recon_matches = [&](int f, int id, int n) {
        std::vector<svh_p_match> m;
        for (int i = 0; i < n && f % 7 != 5; i++) {
            if (svh::mix((uint32_t)(i + 131 * f + 7 * id)) % 5u == 0) continue;
            svh_p_match q;
            memset(&q, 0, sizeof(q));
            q.u1p = 10.f + i + f; q.v1p = 20.f + (i % 37); q.i1p = i;
            q.u1c = q.u1p + 1.f;  q.v1c = q.v1p;           q.i1c = i % 3 ? i : i + 1;   // some tracks end on one index
            m.push_back(q);
        }
        return m;
    };
    auto resident = [&](int id) {
        const double Tr[16] = {1, 0, 0, 0.05, 0, 1, 0, 0, 0, 0, 1, -0.8, 0, 0, 0, 1};
        svh_recon* r = svh_recon_create_resident();
        svh_recon* h = svh_recon_create();
        if (!r || !h) { BAD(); return; }
        if (svh_recon_update(r, nullptr, 0, Tr, 1, 2, 30, 2) != SVH_ERR_BAD_ARG) BAD();   // not calibrated yet
        check(svh_recon_set_calibration(r, 645.2, 635.9, 194.1));
        check(svh_recon_set_calibration(h, 645.2, 635.9, 194.1));
        bool in_step = true;
        for (int f = 0; f < 3 * frames; f++) {
            const std::vector<svh_p_match> m = recon_matches(f, id, 600);
            int32_t a, b;
            // (an update that failed is given again: both objects then stay in step)
            for (int k = 0; k < 50 && (a = svh_recon_update(r, m.data(), (int32_t)m.size(), Tr, 1, 2, 30, 2)) == SVH_ERR_HIP; k++) {}
            for (int k = 0; k < 50 && (b = svh_recon_update(h, m.data(), (int32_t)m.size(), Tr, 1, 2, 30, 2)) == SVH_ERR_HIP; k++) {}
            check(a);
            check(b);
            // (fifty failures in a row happen when every n-th call fails for a small n and this thread is the only one
            // left counting: each attempt then fails at the same call.  One object missed an update the other took:
            // their counts are no longer comparable)
            if (a < 0 || b < 0) in_step = false;
            if (in_step && a == SVH_OK && b == SVH_OK &&
                (svh_recon_num_tracks(r) != svh_recon_num_tracks(h) || svh_recon_num_points(r) != svh_recon_num_points(h)))
                BAD();
            std::vector<float> p(3 * (size_t)svh_recon_num_points(r) + 3);
            check(svh_recon_get_points(r, p.data(), svh_recon_num_points(r)));
            matches += svh_recon_num_tracks(r);
        }
        svh_recon_destroy(r);
        svh_recon_destroy(h);
    };
    th.emplace_back(resident, 3);
    auto recon_batch = [&](int id) {
        double Tr[3 * 16];
        for (int i = 0; i < 3; i++) {
            const double one[16] = {1, 0, 0, 0.05, 0, 1, 0, 0, 0, 0, 1, -0.8 - 0.1 * i, 0, 0, 0, 1};
            memcpy(Tr + 16 * i, one, sizeof(one));
        }
        svh_recon* rs[3] = {svh_recon_create_resident(), svh_recon_create_resident(), svh_recon_create_resident()};
        svh_recon* h = svh_recon_create();
        if (!rs[0] || !rs[1] || !rs[2] || !h) { BAD(); return; }
        for (svh_recon* r : rs) check(svh_recon_set_calibration(r, 645.2, 635.9, 194.1));
        check(svh_recon_set_calibration(h, 645.2, 635.9, 194.1));
        for (int f = 0; f < 3 * frames; f++) {
            std::vector<svh_p_match> m[3] = {recon_matches(f, id, 600), recon_matches(f, id + 1, 450), recon_matches(f, id + 2, 90)};
            static const svh_p_match none = {};
            const svh_p_match* mp[3];
            for (int i = 0; i < 3; i++) mp[i] = m[i].empty() ? &none : m[i].data();   // (empty: an update all the same)
            if (f % 4 == 3) mp[1] = nullptr;                                          // sits this one out
            const int32_t n[3] = {(int32_t)m[0].size(), (int32_t)m[1].size(), (int32_t)m[2].size()};
            int32_t st[3] = {0, 0, 0};
            const int32_t before = svh_recon_num_tracks(rs[1]);
            const int32_t rc = svh_recon_update_batch(rs, mp, n, Tr, 3, 1, 2, 30, 2, st);
            check(rc);
            if (rc == SVH_OK && f % 4 == 3 && svh_recon_num_tracks(rs[1]) != before) BAD();
            svh_recon* mixed[2] = {rs[0], h};
            if (svh_recon_update_batch(mixed, mp, n, Tr, 2, 1, 2, 30, 2, st) != SVH_ERR_BAD_ARG) BAD();
            matches += svh_recon_num_tracks(rs[2]);
        }
        for (svh_recon* r : rs) svh_recon_destroy(r);
        svh_recon_destroy(h);
    };
    th.emplace_back(recon_batch, 4);
    // two threads with PlaneEstimation objects: a road (d grows with v) with a hashed ripple, host maps, changing
    // seeds, a batch of three objects over the same map, release in between
    auto planes = [&](int id) {
        const int w = 320, h = 120;
        std::vector<float> D((size_t)w * h);
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++)
                D[(size_t)v * w + u] =
                    v < 50 ? 0.f : 0.3f * (v - 45) + 0.001f * (float)(svh::mix((uint32_t)(u + w * v + id)) % 1000u);
        svh_plane_params prm;
        svh_plane_params_default(&prm);
        prm.num_samples = 200;
        svh_plane* p[3] = {svh_plane_create(&prm), svh_plane_create(&prm), svh_plane_create(&prm)};
        if (!p[0] || !p[1] || !p[2]) { BAD(); return; }
        if (svh_plane_estimate(p[0], D.data(), 0, w, h, w - 1, 700, 160, 60, 0.5f, 1) != SVH_ERR_BAD_ARG) BAD();
        for (int f = 0; f < frames; f++) {
            const int32_t rc = svh_plane_estimate(p[0], D.data(), 0, w, h, w, 700, 160, 60, 0.5f, (uint32_t)(f / 2 + id));
            check(rc);
            double abc[3];
            svh_plane_get_plane_dsi(p[0], abc);
            if (rc == SVH_OK && !(abc[1] > 0.2 && abc[1] < 0.4)) BAD();
            const float* maps[3] = {D.data(), D.data(), D.data()};
            const uint32_t seeds[3] = {1, 2, (uint32_t)f};
            int32_t st[3];
            check(svh_plane_estimate_batch(p, maps, 3, w, h, w, 700, 160, 60, 0.5f, seeds, st));
            if (f % 4 == 3) (void)svh_plane_release(p[f % 3]);
            matches += svh_plane_get_best(p[1], nullptr, nullptr, 0);
        }
        for (svh_plane* q : p) svh_plane_destroy(q);
    };
    th.emplace_back(planes, 1);
    th.emplace_back(planes, 2);
    // two threads with three mono objects each in lockstep; thread 1 with private streams (parallel preparation),
    // thread 2 with libc rand() and the pipelined loop
    auto mono = [&](int id) {
        svh_vo_mono_params p;
        svh_vo_mono_params_default(&p);
        p.f = 645.2; p.cu = 320.0; p.cv = 100.0; p.height = 1.6; p.pitch = -0.08;
        p.ransac_iters = 50;
        p.motion_threshold = 1e6;
        svh_vo* vs[3];
        for (int i = 0; i < 3; i++) {
            vs[i] = svh_vo_mono_create(&p);
            if (!vs[i]) { BAD(); return; }
            if (id == 1) svh_vo_set_private_rand(vs[i], 1, (uint32_t)i);
        }
        std::vector<std::vector<uint8_t>> I[2];
        for (int q = 0; q < 2; q++) I[q].assign(3, std::vector<uint8_t>((size_t)W * H));
        const uint8_t* ptr[3];
        int32_t ok[3] = {0, 0, 0}, replace[3] = {0, 0, 0};
        const int32_t dims[3] = {W, H, W};
        for (int f = 0; f < frames; f++) {
            for (int i = 0; i < 3; i++) {
                std::vector<uint8_t>& img = I[f & 1][i];
                for (size_t j = 0; j < img.size(); j++) img[j] = (uint8_t)(svh::mix((uint32_t)(j + 977 * f + 31 * i + 9001 * id)) >> 24);
                ptr[i] = img.data();
                replace[i] = f > 1 && (f + i) % 3 == 0;
            }
            if (id == 1) {
                check(svh_vo_mono_process_batch(vs, 3, ptr, dims, replace, ok));
            } else if (f == 0) {
                check(svh_vo_mono_prefetch_batch(vs, 3, ptr, dims));
            } else {
                const int32_t rc = svh_vo_mono_process_next_batch(vs, 3, ptr, dims, replace, ok);
                check(rc);
                if (rc < 0 && inject) (void)svh_vo_mono_prefetch_batch(vs, 3, ptr, dims);
            }
            // the estimate alone: 9 (leaves at once), 40 and 300 matches side by side
            std::vector<svh_p_match> m[3];
            const int nm[3] = {9, 40, 300};
            const svh_p_match* mp[3];
            int32_t n[3];
            for (int i = 0; i < 3; i++) {
                for (int k = 0; k < nm[i]; k++) {
                    svh_p_match q;
                    memset(&q, 0, sizeof(q));
                    q.u1p = (float)(svh::mix((uint32_t)(k + 17 * f + i)) % 600u); q.v1p = (float)(svh::mix((uint32_t)(3 * k + f)) % 180u);
                    q.u1c = q.u1p + 2.f + (float)(k % 3); q.v1c = q.v1p + 1.f;
                    m[i].push_back(q);
                }
                mp[i] = m[i].data();
                n[i] = nm[i];
            }
            const int32_t rc = svh_vo_mono_process_matches_batch(vs, 3, mp, n, ok);
            check(rc);
            if (rc >= 0 && ok[0] != 0) BAD();   // (N < 10 never succeeds)
            int32_t votes[64];
            for (int i = 0; i < 3; i++) matches += svh_vo_mono_get_votes(vs[i], votes, 64) + svh_vo_get_inliers(vs[i], nullptr, 0);
        }
        for (svh_vo* v : vs) svh_vo_destroy(v);
    };
    th.emplace_back(mono, 1);
    th.emplace_back(mono, 2);
    for (std::thread& t : th) t.join();
    printf("sanitize_viso: %d sequences x %d frames + 1 Matcher thread + 2 lockstep threads, %ld matches seen, %d failures"
           ", %ld injected HIP failures reported\n", K, frames, matches.load(), bad.load(), injected.load());
    return bad.load() ? 1 : 0;
}

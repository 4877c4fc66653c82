// VisualOdometryMono::estimateMotion (libviso2/src/viso_mono.cpp:40-159) for the svh_vo_mono_* entries of
// vo_engine.cpp.  Three device phases, each ended by one stream wait:
//   1. RANSAC: 2000 hypotheses (8x9 SVD, rank-2 SVD, Sampson vote over all N) and the winner's inlier flags
//      (k_mono_hyp, k_mono_vote, k_mono_select);
//   2. chirality: 4 x N triangulations (4x4 SVDs) and the candidate with the most points in front
//      (k_mono_chiral, k_mono_pick);
//   3. the ground-plane vote, O(n^2) exp (k_mono_plane).
// Between them the host does the once-per-frame steps that are a handful of small matrices or a single pass:
// normalisation and the random samples (before 1), the k x 9 refit of F on the inliers, E and the four R|t
// candidates (between 1 and 2), the median and the plane distances (between 2 and 3), the scale and the angles
// (after 3).  The matrix steps use the same mono_core.h functions as the kernels.  There is no CPU path for the
// device phases.
// The estimate is written as steps -- mono_prepare, then per phase mono_enqueue, the wait and mono_after -- which the
// single call (mono_estimate) runs for one object and the lockstep entries (mono_run_batch) for K objects together:
// per phase ONE recorded pass over the objects still alive (batch_rec.h: one launch per kernel, blockIdx.z = object),
// one stream wait, then the host step of every live object on the helper threads.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/svh.h"
#include "batch_rec.h"
#include "hip_guard.h"
#include "matcher_internal.h"
#include "mono_core.h"
#include "vo_internal.h"

namespace svh {

#define MONO_TRY(kind, expr) SVH_HIP_TRY("VisualOdometryMono", kind, expr)
#define MONO_GROW(buf, bytes) SVH_HIP_GROW("VisualOdometryMono", buf, bytes)

struct MonoVo {
    svh_vo_mono_params p;
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<int32_t> votes;   // per-hypothesis inlier counts of the last estimate (svh_vo_mono_get_votes)
    bool timing = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms[3] = {0, 0, 0};     // device time of the three phases of the last estimate (timing on)
    // pinned host memory (every buffer carries 16 bytes of slack: the upload kernel moves whole 16-byte words)
    PinnedBuf<uint8_t> h_in;      // [normalised matches 16N | matches 16N | samples 32 iters] -> d_in
    PinnedBuf<int32_t> h_sel;     // {winner, its count} (2) | {candidate, 4 counts} (at +4)
    PinnedBuf<uint8_t> h_flags;   // N
    PinnedBuf<int32_t> h_counts;  // iters
    PinnedBuf<double> h_cams;     // 60 -> d_cams
    PinnedBuf<double> h_X;        // 4 N
    PinnedBuf<double> h_d;        // n -> d_d
    PinnedBuf<double> h_sums;     // n
    // device memory
    HipBuf<uint8_t> d_in, d_front;
    HipBuf<double> d_F, d_cams, d_X, d_d;
    HipBuf<int32_t> d_counts;
    // the estimate in flight, from mono_prepare to the last mono_after
    int32_t N = 0, iters = 0, n = 0;
    std::vector<float> q;         // normalised matches, 4 N
    double T[18];                 // Tp | Tc
    double Ra[9], Rb[9], t[3];    // EtoRt's candidates: (Ra,t) (Ra,-t) (Rb,t) (Rb,-t)
    int32_t cand = -1;            // the one with the most points in front
    double weight = 0, thr = 0;   // of the plane vote
};

namespace {

// room for `n` elements and the slack
template <typename T, bool Pinned>
size_t padded(const HipBuf<T, Pinned>&, size_t n) { return n * sizeof(T) + 16; }
#define MONO_ROOM(buf, n) MONO_GROW(buf, padded(buf, n))

// every item is checked on its own: a call that failed half way leaves nothing the next call would trust
int ensure(MonoVo* M, int32_t N, int32_t iters) {
    MONO_TRY(none, hipSetDevice(M->device));
    if (!M->stream) MONO_TRY(none, hipStreamCreateWithFlags(&M->stream, hipStreamNonBlocking));
    MONO_ROOM(M->h_sel, 16);
    MONO_ROOM(M->h_cams, 60);
    MONO_ROOM(M->d_cams, 60);
    for (int i = 0; i < 2; i++)
        if (!M->ev[i]) MONO_TRY(none, hipEventCreate(&M->ev[i]));
    const size_t n = (size_t)N, it = (size_t)iters;
    MONO_ROOM(M->h_in, 32 * n + 32 * it);
    MONO_ROOM(M->d_in, 32 * n + 32 * it);
    MONO_ROOM(M->h_flags, n);
    MONO_ROOM(M->h_counts, it);
    MONO_ROOM(M->h_X, 4 * n);
    MONO_ROOM(M->h_d, n);
    MONO_ROOM(M->h_sums, n);
    MONO_ROOM(M->d_F, 9 * it);
    MONO_ROOM(M->d_counts, it);
    MONO_ROOM(M->d_X, 16 * n);
    MONO_ROOM(M->d_front, 4 * n);
    MONO_ROOM(M->d_d, n);
    return SVH_OK;
}

void mark(MonoVo* M, int i) {
    if (M->timing) (void)hipEventRecord(M->ev[i], M->stream);
}

// the stream wait that ends device phase `phase` (its events: ev[0] before, ev[1] after)
int wait(MonoVo* M, int phase) {
    MONO_TRY(wait, (hipError_t)wait_stream(M->stream));
    MONO_TRY(launch, hipGetLastError());
    if (M->timing) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, M->ev[0], M->ev[1]) == hipSuccess) M->ms[phase] = ms;
    }
    return SVH_OK;
}

double det3(const double* A) {
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) +
           A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// F of the given matches (fundamentalMatrix, viso_mono.cpp:234-265) on the host: the k x 9 refit on the inliers
void refit(const float* q, const std::vector<int32_t>& active, double* F) {
    const int k = (int)active.size();
    std::vector<double> U((size_t)k * 9), V(81), w(9), rv1(9);
    for (int r = 0; r < k; r++) {
        const float* m = q + 4 * (size_t)active[r];
        mono::f_row(m[0], m[1], m[2], m[3], &U[9 * (size_t)r], 1);
    }
    const mono::Mat Um{U.data(), 9, 1}, Vm{V.data(), 9, 1};
    const mono::Vec wv{w.data(), 1}, rv{rv1.data(), 1};
    mono::svd(k, 9, Um, Vm, wv, rv);
    double f[9];
    for (int i = 0; i < 9; i++) f[i] = Vm(i, 8);
    const mono::Mat U3{U.data(), 3, 1}, V3{V.data(), 3, 1};
    for (int i = 0; i < 9; i++) U3(i / 3, i % 3) = f[i];
    mono::svd(3, 3, U3, V3, wv, rv);
    mono::rank2(U3, V3, wv, F);
}

// svd of a 3x3 matrix: U, w, V (row major)
void svd3(const double* A, double* U, double* w, double* V) {
    double rv1[3];
    for (int i = 0; i < 9; i++) U[i] = A[i];
    mono::svd(3, 3, mono::Mat{U, 3, 1}, mono::Mat{V, 3, 1}, mono::Vec{w, 1}, mono::Vec{rv1, 1});
}

void transpose3(const double* A, double* T) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[3 * j + i] = A[3 * i + j];
}

}  // namespace

MonoVo* mono_create(const svh_vo_mono_params& p, int device) {
    MonoVo* M = new MonoVo();
    M->p = p;
    M->device = device;
    return M;
}

void mono_destroy(MonoVo* M) {
    if (!M) return;
    if (M->stream) {
        (void)hipSetDevice(M->device);
        (void)hipStreamSynchronize(M->stream);
        for (int i = 0; i < 2; i++)
            if (M->ev[i]) (void)hipEventDestroy(M->ev[i]);
        (void)hipStreamDestroy(M->stream);
    }
    delete M;   // (its buffers free themselves, on the device selected above)
}

bool mono_same_params(const MonoVo* a, const MonoVo* b) {
    return memcmp(&a->p, &b->p, sizeof(a->p)) == 0 && a->device == b->device;
}

int32_t mono_votes(MonoVo* M, int32_t* out, int32_t cap) {
    for (int32_t i = 0; i < (int32_t)M->votes.size() && i < cap && out; i++) out[i] = M->votes[i];
    return (int32_t)M->votes.size();
}

void mono_clear(MonoVo* M) {
    M->votes.clear();
    M->ms[0] = M->ms[1] = M->ms[2] = 0;
}

void mono_set_timing(MonoVo* M, bool on) { M->timing = on; }

int32_t mono_timing(MonoVo* M, double* ms3) {
    for (int i = 0; i < 3 && ms3; i++) ms3[i] = M->ms[i];
    return 3;
}

// The host part in front of phase 1: the early exits, buffers, the random samples, staging.  1: there is device work,
// 0: the reference's empty vector, < 0 on error.  `inliers` is the object's getInlierIndices() state: cleared only
// where the reference clears it.  The only step of an estimate that draws random numbers.
int mono_prepare(MonoVo* M, const svh_p_match* pm, int32_t N, RandStream& rng, std::vector<int32_t>& inliers) {
    const svh_vo_mono_params& P = M->p;
    if (N < 10) return 0;   // viso_mono.cpp:44-46: before inliers.clear()
    std::vector<float>& q = M->q;
    q.resize((size_t)N * 4);
    for (int32_t i = 0; i < N; i++) {
        q[4 * i + 0] = pm[i].u1p;
        q[4 * i + 1] = pm[i].v1p;
        q[4 * i + 2] = pm[i].u1c;
        q[4 * i + 3] = pm[i].v1c;
    }
    const std::vector<float> orig = q;
    if (!mono::normalize(q.data(), N, M->T)) return 0;
    inliers.clear();
    M->votes.clear();
    M->ms[0] = M->ms[1] = M->ms[2] = 0;
    const int32_t iters = P.ransac_iters > 0 ? P.ransac_iters : 0;
    const int rc = ensure(M, N, iters);
    if (rc) return rc;
    M->N = N;
    M->iters = iters;

    // ---- phase 1: RANSAC on the device.  getRandomSample(N, 8) per iteration (viso.cpp:130-153): eight draws
    // without replacement, each indexing the list of the indices not chosen yet
    memcpy(M->h_in, q.data(), 16 * (size_t)N);
    memcpy(M->h_in + 16 * (size_t)N, orig.data(), 16 * (size_t)N);
    int32_t* samples = reinterpret_cast<int32_t*>(M->h_in + 32 * (size_t)N);
    for (int32_t k = 0; k < iters; k++) {
        int32_t chosen[8];
        for (int s = 0; s < 8; s++) {
            const int32_t j = rng.next() % (N - s);
            int32_t idx = j;   // the j-th smallest index not chosen yet
            bool moved = true;
            while (moved) {
                moved = false;
                int32_t below = 0;
                for (int r = 0; r < s; r++) below += chosen[r] <= idx;
                if (idx != j + below) {
                    idx = j + below;
                    moved = true;
                }
            }
            chosen[s] = idx;
            samples[8 * k + s] = idx;
        }
    }
    return 1;
}

// The upload and the kernels of device phase 0 / 1 / 2 on the object's stream, or into the calling thread's recorder
void mono_enqueue(MonoVo* M, int phase) {
    const svh_vo_mono_params& P = M->p;
    const int32_t N = M->N, iters = M->iters;
    const float* d_q = reinterpret_cast<const float*>(M->d_in.p);
    const float* d_m = reinterpret_cast<const float*>(M->d_in + 16 * (size_t)N);
    if (phase == 0) {
        mlaunch_upload(M->stream, M->h_in, M->d_in, 32 * (size_t)N + up16(32 * (size_t)iters));
        mlaunch_ransac(M->stream, d_q, N, reinterpret_cast<const int32_t*>(M->d_in + 32 * (size_t)N), iters,
                       P.inlier_threshold, M->d_F, M->d_counts, M->h_sel, M->h_flags, M->h_counts);
    } else if (phase == 1) {
        mlaunch_upload(M->stream, reinterpret_cast<const uint8_t*>(M->h_cams.p), reinterpret_cast<uint8_t*>(M->d_cams.p),
                       60 * sizeof(double));
        mlaunch_chiral(M->stream, d_m, N, M->d_cams, M->d_X, M->d_front, M->h_X, M->h_sel + 4);
    } else {
        mlaunch_upload(M->stream, reinterpret_cast<const uint8_t*>(M->h_d.p), reinterpret_cast<uint8_t*>(M->d_d.p),
                       up16(8 * (size_t)M->n));
        mlaunch_plane(M->stream, M->d_d, M->n, M->weight, M->thr, M->h_sums);
    }
}

namespace {

// after phase 0: votes, the inlier list, then the refit, E, the four R|t and the cameras of phase 1
int after_ransac(MonoVo* M, std::vector<int32_t>& inliers) {
    const svh_vo_mono_params& P = M->p;
    const int32_t N = M->N;
    const std::vector<float>& q = M->q;
    const double* T = M->T;
    M->votes.assign(M->h_counts.p, M->h_counts.p + M->iters);
    for (int32_t i = 0; i < N; i++)
        if (M->h_flags[i]) inliers.push_back(i);
    if (inliers.size() < 10) return 0;   // :73-74

    // ---- refit F on all inliers, denormalise, E with rank 2, the four R|t of EtoRt (:76-86, :316-361)
    double F[9], A[9], E[9], TcT[9], KT[9];
    refit(q.data(), inliers, F);
    const double K[9] = {P.f, 0, P.cu, 0, P.f, P.cv, 0, 0, 1};
    transpose3(T + 9, TcT);
    mono::mul3(TcT, F, A, false);
    mono::mul3(A, T, F, false);   // F = ~Tc * F * Tp
    transpose3(K, KT);
    mono::mul3(KT, F, A, false);
    mono::mul3(A, K, E, false);   // E = ~K * F * K
    {
        double U[9], w[3], V[9];
        svd3(E, U, w, V);
        mono::rank2(mono::Mat{U, 3, 1}, mono::Mat{V, 3, 1}, mono::Vec{w, 1}, E);
    }
    double U[9], S[3], V[9], VT[9];
    double *Ra = M->Ra, *Rb = M->Rb, *t = M->t;
    svd3(E, U, S, V);
    transpose3(V, VT);
    {
        const double W[9] = {0, -1, 0, +1, 0, 0, 0, 0, 1};
        const double Z[9] = {0, +1, 0, -1, 0, 0, 0, 0, 0};
        double WT[9], UT[9], Tm[9];
        transpose3(W, WT);
        transpose3(U, UT);
        mono::mul3(U, Z, A, false);
        mono::mul3(A, UT, Tm, false);
        mono::mul3(U, W, A, false);
        mono::mul3(A, VT, Ra, false);
        mono::mul3(U, WT, A, false);
        mono::mul3(A, VT, Rb, false);
        t[0] = Tm[7];
        t[1] = Tm[2];
        t[2] = Tm[3];
    }
    if (det3(Ra) < 0)
        for (int i = 0; i < 9; i++) Ra[i] = -Ra[i];
    if (det3(Rb) < 0)
        for (int i = 0; i < 9; i++) Rb[i] = -Rb[i];
    const double* Rc[4] = {Ra, Ra, Rb, Rb};
    const double sg[4] = {1, -1, 1, -1};
    double* cams = M->h_cams;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) cams[4 * i + j] = j < 3 ? K[3 * i + j] : 0.0;   // P1 = [K | 0]
    for (int c = 0; c < 4; c++) {
        double Rt[12];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) Rt[4 * i + j] = Rc[c][3 * i + j];
            Rt[4 * i + 3] = sg[c] < 0 ? -t[i] : t[i];
        }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) {
                double s = 0.0;
                for (int k = 0; k < 3; k++) s += K[3 * i + k] * Rt[4 * k + j];
                cams[12 + 12 * c + 4 * i + j] = s;   // P2 = K * [R | t]
            }
    }
    return 1;
}

// after phase 1 (chirality): the candidate, then the points in front, their median and the plane distances
int after_chiral(MonoVo* M) {
    const svh_vo_mono_params& P = M->p;
    const int32_t N = M->N;
    // no candidate with a point in front of both cameras: the reference leaves X empty and exits in getMat
    // (matrix.cpp:127-137); here the estimate fails
    M->cand = M->h_sel[4];
    if (M->cand < 0) return 0;

    // ---- points in front of the first camera, their median distance, plane distances (:88-122)
    const double* X = M->h_X;
    std::vector<int32_t> pos;
    for (int32_t i = 0; i < N; i++)
        if (X[2 * (size_t)N + i] > 0) pos.push_back(i);
    const int32_t n = (int32_t)pos.size();
    if (n < 10) return 0;
    std::vector<double> dist(n);
    for (int32_t i = 0; i < n; i++)
        dist[i] = fabs(X[pos[i]]) + fabs(X[(size_t)N + pos[i]]) + fabs(X[2 * (size_t)N + pos[i]]);
    std::nth_element(dist.begin(), dist.begin() + n / 2, dist.end());
    const double median = dist[n / 2];
    if (median > P.motion_threshold) return 0;
    const double n0 = cos(-P.pitch), n1 = sin(-P.pitch);
    double* d = M->h_d;
    for (int32_t i = 0; i < n; i++) {
        double s = 0.0;
        s += n0 * X[(size_t)N + pos[i]];
        s += n1 * X[2 * (size_t)N + pos[i]];
        d[i] = s;   // ~n * x_plane
    }
    const double sigma = median / 50.0;
    M->n = n;
    M->weight = 1.0 / (2.0 * sigma * sigma);
    M->thr = median / P.motion_threshold;
    return 1;
}

// after phase 2 (the plane vote): the best plane point, scale, angles
int after_plane(MonoVo* M, double* tr6) {
    const svh_vo_mono_params& P = M->p;
    const int32_t n = M->n;
    const double* d = M->h_d;
    const double thr = M->thr;
    const double* R = M->cand < 2 ? M->Ra : M->Rb;
    const double ts = (M->cand & 1) ? -1.0 : 1.0;
    const double* t = M->t;
    double best_sum = 0;
    int32_t best_idx = 0;
    for (int32_t i = 0; i < n; i++)
        if (d[i] > thr && M->h_sums[i] > best_sum) {
            best_sum = M->h_sums[i];
            best_idx = i;
        }
    // t = t*height/d(best_idx): the reference exits inside Matrix::operator/ (matrix.cpp:497-503) when
    // |d| < 1e-20; here the estimate fails instead
    const double db = d[best_idx];
    if (fabs(db) < 1e-20) return 0;
    double tt[3];
    for (int i = 0; i < 3; i++) tt[i] = ((ts < 0 ? -t[i] : t[i]) * P.height) / db;
    const double ry = asin(R[2]);
    const double rx = asin(-R[5] / cos(ry));
    const double rz = asin(-R[1] / cos(ry));
    tr6[0] = rx;
    tr6[1] = ry;
    tr6[2] = rz;
    tr6[3] = tt[0];
    tr6[4] = tt[1];
    tr6[5] = tt[2];
    return 1;
}

}  // namespace

// The host side after the wait that ended `phase`: its results, its exits, and what the next phase needs.  1: go on
// (after the last phase: tr6 is the motion), 0: the reference's empty vector.  Draws no random numbers.
int mono_after(MonoVo* M, int phase, std::vector<int32_t>& inliers, double* tr6) {
    return phase == 0 ? after_ransac(M, inliers) : (phase == 1 ? after_chiral(M) : after_plane(M, tr6));
}

// estimateMotion: 1 + tr6 (rx, ry, rz, tx, ty, tz), 0 for the reference's empty vector, < 0 on error.
int mono_estimate(MonoVo* M, const svh_p_match* pm, int32_t N, RandStream& rng, std::vector<int32_t>& inliers,
                  double* tr6) {
    int rc = mono_prepare(M, pm, N, rng, inliers);
    for (int phase = 0; phase < 3 && rc > 0; phase++) {
        mark(M, 0);
        mono_enqueue(M, phase);
        mark(M, 1);
        if ((rc = wait(M, phase))) {
            (void)hipStreamSynchronize(M->stream);   // (nothing of this estimate stays in flight behind an error)
            return rc;
        }
        rc = mono_after(M, phase, inliers, tr6);
    }
    return rc;
}

// The device phases of K prepared objects in lockstep.  state[i] > 0 on entry: object i passed mono_prepare; on
// return state[i] is what mono_estimate would have returned for it.  Objects share parameters and device (the
// callers check); the recorded launches of a phase go to the first live object's stream.
int mono_run_batch(MonoVo* const* Ms, int32_t K, int* state, std::vector<int32_t>* const* inliers, double* tr6) {
    std::vector<int> live;
    for (int i = 0; i < K; i++)
        if (state[i] > 0) live.push_back(i);
    if (live.empty()) return SVH_OK;
    MonoVo* M0 = Ms[live[0]];
    MONO_TRY(none, hipSetDevice(M0->device));
    BatchRec& rec = batch_recorder(M0->device);
    hipStream_t s = M0->stream;
    for (int phase = 0; phase < 3 && !live.empty(); phase++) {
        bool timing = false;
        for (int i : live) timing = timing || Ms[i]->timing;
        Phase ph{"VisualOdometryMono", FI_wait};
        if (timing) ph.ev[0] = M0->ev[0], ph.ev[1] = M0->ev[1];
        const int rc = run_recorded(
            rec, s, live.data(), (int)live.size(), ph,
            [&](int i) -> int {   // (without a recorder: on the object's own stream, between its own events)
                const bool own = t_rec == nullptr;
                if (own) mark(Ms[i], 0);
                mono_enqueue(Ms[i], phase);
                if (own) mark(Ms[i], 1);
                return SVH_OK;
            },
            [&](int i) -> int {
                const int r = wait(Ms[i], phase);
                if (r) (void)hipStreamSynchronize(Ms[i]->stream);
                return r;
            },
            no_undo);
        if (rc < 0) return rc;
        float ms = 0;   // (one by one: every object has its own phase time)
        if (timing && rc != kOneByOne && hipEventElapsedTime(&ms, M0->ev[0], M0->ev[1]) == hipSuccess)
            for (int i : live) Ms[i]->ms[phase] = ms;   // the phase's time for the whole batch
        batch_parallel_for((int)live.size(), [&](int j) {
            const int i = live[j];
            state[i] = mono_after(Ms[i], phase, *inliers[i], tr6 + 6 * (size_t)i);
        });
        std::vector<int> next;
        for (int i : live)
            if (state[i] > 0) next.push_back(i);
        live.swap(next);
    }
    return SVH_OK;
}

}  // namespace svh

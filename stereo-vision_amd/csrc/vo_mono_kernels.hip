// VisualOdometryMono::estimateMotion on the device (libviso2/src/viso_mono.cpp:40-400)
//
// k_mono_hyp     one lane per RANSAC hypothesis: the 8x9 constraint matrix of its 8 samples, its SVD, the 3x3 SVD
//                of F and the rank-2 product (viso_mono.cpp:234-265).  The SVD state of a lane (U 8x9, V 9x9, w,
//                rv1: 171 doubles) lives in LDS, interleaved across the lanes of the workgroup (mono_core.h).
// k_mono_vote    one wave per hypothesis: the Sampson test of getInlier (:267-314) over all N normalised matches,
//                counted with ballot + popcount.
// k_mono_select  one workgroup: the first hypothesis with the most inliers (the reference keeps a set only when it
//                is strictly larger, :66-67) and its inlier flags, in match order, into pinned host memory.
// k_mono_chiral  one lane per (R|t candidate, match): the 4x4 SVD of triangulateChieral (:363-400) and whether the
//                point lies in front of both cameras.
// k_mono_pick    one workgroup: the first candidate with the most points in front (EtoRt, :345-358) and its points
//                divided by their fourth coordinate (X/X.getMat(3,0,3,-1), matrix.cpp:472-485: a zero divisor
//                leaves 0) into pinned host memory.
// k_mono_plane   one lane per point i of the ground-plane vote (:124-138): the sum over j in ascending order of
//                exp(-dist*dist*weight).  exp is the device libm's; it can differ from glibc's in the last bit, so
//                the sums can, and the plane chosen would differ only if two sums were that close (none is in the
//                fixtures: the GPU tests compare best_idx through the motion).
// All arithmetic is fp64 in the reference's operation order (mono_core.h), no FMA contraction (-ffp-contract=off).
// Each kernel has a batched form k_mono_*_b for K objects driven in lockstep (svh_vo_mono_*_batch): one job per
// object in a table in device memory, blockIdx.z = job.  The results of a job go to that object's own pinned buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "job_kernel.h"
#include "mono_core.h"
#include "vo_internal.h"

namespace svh {

namespace {

using mono::Mat;
using mono::Vec;

constexpr int HYP_LANES = 32;     // lanes (hypotheses) per workgroup of k_mono_hyp: 171 x 8 B x 32 = 43.8 KB LDS
constexpr int HYP_SLAB = 171;     // U 72 | V 81 | w 9 | rv1 9
constexpr int CHI_LANES = 64;     // lanes per workgroup of k_mono_chiral: 40 x 8 B x 64 = 20 KB LDS
constexpr int CHI_SLAB = 40;      // J 16 | V 16 | w 4 | rv1 4

// Every kernel is a __device__ body with two entries made by one SVH_JOB_KERNEL line (job_kernel.h): the plain form
// takes its job by value, the batched form `_b` reads job blockIdx.z of a table in device memory, grid x is the largest
// job's and blocks beyond a job's own extent return at once (the line's last argument).  Both run the same body, so a
// batched lane computes bit for bit what the single launch computes.

struct MonoHypJob { const float4* q; const int32_t* samples; double* F; int32_t N, iters; };
struct MonoVoteJob { const float4* q; const double* F; int32_t* counts; double thr; int32_t N, iters; };
struct MonoSelectJob {
    const int32_t* counts; const double* F; const float4* q; int32_t* out_sel; uint8_t* out_flags; int32_t* out_counts;
    double thr; int32_t N, iters;
};
struct MonoChiralJob { const float4* m; const double* cams; double* X; uint8_t* front; int32_t N; };
struct MonoPickJob { const double* X; const uint8_t* front; double* out_X; int32_t* out_cand; int32_t N; };
struct MonoPlaneJob { const double* d; double* sums; double weight, thr; int32_t n; };
__device__ __forceinline__ MonoHypJob globalise(MonoHypJob a) { all_global(a.q, a.samples, a.F); return a; }
__device__ __forceinline__ MonoVoteJob globalise(MonoVoteJob a) { all_global(a.q, a.F, a.counts); return a; }
__device__ __forceinline__ MonoSelectJob globalise(MonoSelectJob a) {
    all_global(a.counts, a.F, a.q, a.out_sel, a.out_flags, a.out_counts);
    return a;
}
__device__ __forceinline__ MonoChiralJob globalise(MonoChiralJob a) { all_global(a.m, a.cams, a.X, a.front); return a; }
__device__ __forceinline__ MonoPickJob globalise(MonoPickJob a) {
    all_global(a.X, a.front, a.out_X, a.out_cand);
    return a;
}
__device__ __forceinline__ MonoPlaneJob globalise(MonoPlaneJob a) { all_global(a.d, a.sums); return a; }

__device__ __forceinline__ void d_mono_hyp(double* slab, const float4* __restrict__ q, int32_t N,
                                           const int32_t* __restrict__ samples, int32_t iters,
                                           double* __restrict__ Fout) {
    const int lane = threadIdx.x;
    const int h = blockIdx.x * HYP_LANES + lane;
    if (h >= iters) return;
    double* base = slab + lane;
    const Mat U{base, 9, HYP_LANES}, V{base + 72 * HYP_LANES, 9, HYP_LANES};
    const Vec w{base + 153 * HYP_LANES, HYP_LANES}, rv1{base + 162 * HYP_LANES, HYP_LANES};
    for (int r = 0; r < 8; r++) {
        int32_t s = samples[8 * h + r];
        s = s < 0 ? 0 : (s >= N ? N - 1 : s);   // (drawn on the host below N; clamped so a bad draw cannot read out of bounds)
        const float4 m = q[s];
        mono::f_row(m.x, m.y, m.z, m.w, &U(r, 0), HYP_LANES);
    }
    mono::svd(8, 9, U, V, w, rv1);
    double F[9];
    for (int i = 0; i < 9; i++) F[i] = V(i, 8);   // Matrix::reshape of the last column of V
    const Mat U3{base, 3, HYP_LANES}, V3{base + 72 * HYP_LANES, 3, HYP_LANES};
    for (int i = 0; i < 9; i++) U3(i / 3, i % 3) = F[i];
    mono::svd(3, 3, U3, V3, w, rv1);
    mono::rank2(U3, V3, w, F);
    for (int i = 0; i < 9; i++) Fout[9 * (size_t)h + i] = F[i];
}
__device__ __forceinline__ void d_mono_hyp(const MonoHypJob& a, unsigned, unsigned) {
    __shared__ double slab[HYP_SLAB * HYP_LANES];
    d_mono_hyp(slab, a.q, a.N, a.samples, a.iters, a.F);
}
SVH_JOB_KERNEL(kd_mono_hyp, , k_mono_hyp, k_mono_hyp_b, MonoHypJob, HYP_LANES, 1, d_mono_hyp,
               (int)(blockIdx.x * HYP_LANES) < a.iters)

__device__ __forceinline__ void d_mono_vote(const float4* __restrict__ q, int32_t N, const double* __restrict__ Fs,
                                            double thr, int32_t* __restrict__ counts) {
    const int h = blockIdx.x;
    double F[9];
    for (int i = 0; i < 9; i++) F[i] = Fs[9 * (size_t)h + i];
    int32_t c = 0;
    for (int32_t base = 0; base < N; base += 64) {
        const int32_t i = base + (int32_t)threadIdx.x;
        bool in = false;
        if (i < N) {
            const float4 m = q[i];
            in = mono::sampson_inlier(F, m.x, m.y, m.z, m.w, thr);
        }
        c += __popcll(__ballot(in));
    }
    if (threadIdx.x == 0) counts[h] = c;
}
__device__ __forceinline__ void d_mono_vote(const MonoVoteJob& a, unsigned, unsigned) {
    d_mono_vote(a.q, a.N, a.F, a.thr, a.counts);
}
SVH_JOB_KERNEL(kd_mono_vote, , k_mono_vote, k_mono_vote_b, MonoVoteJob, 64, 1, d_mono_vote, (int)blockIdx.x < a.iters)

__device__ __forceinline__ void d_mono_select(const int32_t* __restrict__ counts, int32_t iters,
                                              const double* __restrict__ Fs, const float4* __restrict__ q, int32_t N,
                                              double thr, int32_t* __restrict__ out_sel,
                                              uint8_t* __restrict__ out_flags, int32_t* __restrict__ out_counts) {
    __shared__ int32_t s_cnt[256], s_idx[256];
    int32_t bc = -1, bi = 0;
    for (int32_t h = threadIdx.x; h < iters; h += 256) {
        const int32_t c = counts[h];
        out_counts[h] = c;
        if (c > bc) { bc = c; bi = h; }   // ascending h per lane: the first of a lane's maxima
    }
    s_cnt[threadIdx.x] = bc;
    s_idx[threadIdx.x] = bi;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const int32_t oc = s_cnt[threadIdx.x + st], oi = s_idx[threadIdx.x + st];
            if (oc > s_cnt[threadIdx.x] || (oc == s_cnt[threadIdx.x] && oi < s_idx[threadIdx.x])) {
                s_cnt[threadIdx.x] = oc;
                s_idx[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    const int32_t best = s_idx[0], most = s_cnt[0];
    double F[9];
    if (most > 0)
        for (int i = 0; i < 9; i++) F[i] = Fs[9 * (size_t)best + i];
    for (int32_t i = threadIdx.x; i < N; i += 256) {
        const float4 m = q[i];
        // (no hypothesis with an inlier, or none at all: the reference's set stays empty)
        out_flags[i] = most > 0 && mono::sampson_inlier(F, m.x, m.y, m.z, m.w, thr);
    }
    if (threadIdx.x == 0) {
        out_sel[0] = best;
        out_sel[1] = most;
    }
}
__device__ __forceinline__ void d_mono_select(const MonoSelectJob& a, unsigned, unsigned) {
    d_mono_select(a.counts, a.iters, a.F, a.q, a.N, a.thr, a.out_sel, a.out_flags, a.out_counts);
}
SVH_JOB_KERNEL(kd_mono_select, , k_mono_select, k_mono_select_b, MonoSelectJob, 256, 1, d_mono_select, true)

__device__ __forceinline__ void d_mono_chiral(double* slab, const float4* __restrict__ m, int32_t N,
                                              const double* __restrict__ cams, double* __restrict__ X,
                                              uint8_t* __restrict__ front) {
    const int lane = threadIdx.x;
    const int32_t g = blockIdx.x * CHI_LANES + lane;
    if (g >= 4 * N) return;
    const int cand = g / N, i = g - cand * N;
    double* base = slab + lane;
    const Mat J{base, 4, CHI_LANES}, V{base + 16 * CHI_LANES, 4, CHI_LANES};
    const Vec w{base + 32 * CHI_LANES, CHI_LANES}, rv1{base + 36 * CHI_LANES, CHI_LANES};
    const float4 p = m[i];
    double x[4];
    const bool ok = mono::triangulate(cams, cams + 12 + 12 * cand, p.x, p.y, p.z, p.w, J, V, w, rv1, x);
    for (int r = 0; r < 4; r++) X[((size_t)cand * 4 + r) * N + i] = x[r];
    front[g] = ok;
}
__device__ __forceinline__ void d_mono_chiral(const MonoChiralJob& a, unsigned, unsigned) {
    __shared__ double slab[CHI_SLAB * CHI_LANES];
    d_mono_chiral(slab, a.m, a.N, a.cams, a.X, a.front);
}
SVH_JOB_KERNEL(kd_mono_chiral, , k_mono_chiral, k_mono_chiral_b, MonoChiralJob, CHI_LANES, 1, d_mono_chiral,
               (int)(blockIdx.x * CHI_LANES) < 4 * a.N)

__device__ __forceinline__ void d_mono_pick(const double* __restrict__ X, const uint8_t* __restrict__ front, int32_t N,
                                            double* __restrict__ out_X, int32_t* __restrict__ out_cand) {
    __shared__ int32_t s[4][256];
    int32_t c[4] = {0, 0, 0, 0};
    for (int32_t i = threadIdx.x; i < N; i += 256)
        for (int k = 0; k < 4; k++) c[k] += front[(size_t)k * N + i];
    for (int k = 0; k < 4; k++) s[k][threadIdx.x] = c[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int k = 0; k < 4; k++) s[k][threadIdx.x] += s[k][threadIdx.x + st];
        __syncthreads();
    }
    int best = -1, most = 0;
    for (int k = 0; k < 4; k++)
        if (s[k][0] > most) {   // viso_mono.cpp:350: strictly more than the best so far, starting from 0
            most = s[k][0];
            best = k;
        }
    if (threadIdx.x == 0) {
        out_cand[0] = best;
        for (int k = 0; k < 4; k++) out_cand[1 + k] = s[k][0];
    }
    if (best < 0) return;
    const double* Xc = X + (size_t)best * 4 * N;
    for (int32_t i = threadIdx.x; i < N; i += 256) {
        const double d = Xc[3 * (size_t)N + i];
        for (int r = 0; r < 4; r++) out_X[(size_t)r * N + i] = d != 0 ? Xc[(size_t)r * N + i] / d : 0.0;
    }
}
__device__ __forceinline__ void d_mono_pick(const MonoPickJob& a, unsigned, unsigned) {
    d_mono_pick(a.X, a.front, a.N, a.out_X, a.out_cand);
}
SVH_JOB_KERNEL(kd_mono_pick, , k_mono_pick, k_mono_pick_b, MonoPickJob, 256, 1, d_mono_pick, true)

__device__ __forceinline__ void d_mono_plane(const double* __restrict__ d, int32_t n, double weight, double thr,
                                             double* __restrict__ sums) {
    const int32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double di = d[i];
    double sum = 0;
    if (di > thr)
        for (int32_t j = 0; j < n; j++) {
            const double dist = d[j] - di;
            sum += exp(-dist * dist * weight);
        }
    sums[i] = sum;
}
__device__ __forceinline__ void d_mono_plane(const MonoPlaneJob& a, unsigned, unsigned) {
    d_mono_plane(a.d, a.n, a.weight, a.thr, a.sums);
}
SVH_JOB_KERNEL(kd_mono_plane, , k_mono_plane, k_mono_plane_b, MonoPlaneJob, 64, 1, d_mono_plane,
               (int)(blockIdx.x * 64) < a.n)

}  // namespace

// With a recorder installed on the calling thread (a lockstep call, batch_rec.h) the launchers append their jobs to
// it instead of launching (launch_or_record), exactly as vlaunch_estimate of vo_kernels.hip does.
void mlaunch_ransac(void* stream, const float* q4, int32_t N, const int32_t* samples, int32_t iters, double thr,
                    double* F, int32_t* counts, int32_t* out_sel, uint8_t* out_flags, int32_t* out_counts) {
    const float4* q = reinterpret_cast<const float4*>(q4);
    const MonoHypJob ah = {q, samples, F, N, iters};
    const MonoVoteJob av = {q, F, counts, thr, N, iters};
    const MonoSelectJob as = {counts, F, q, out_sel, out_flags, out_counts, thr, N, iters};
    const unsigned gh = (unsigned)((iters + HYP_LANES - 1) / HYP_LANES);
    if (iters > 0) {
        launch_or_record(stream, kd_mono_hyp, ah, dim3(gh));
        launch_or_record(stream, kd_mono_vote, av, dim3((unsigned)iters));
    }
    launch_or_record(stream, kd_mono_select, as, dim3(1));
}

void mlaunch_chiral(void* stream, const float* m4, int32_t N, const double* cams, double* X, uint8_t* front,
                    double* out_X, int32_t* out_cand) {
    const float4* m = reinterpret_cast<const float4*>(m4);
    const MonoChiralJob ac = {m, cams, X, front, N};
    const MonoPickJob ap = {X, front, out_X, out_cand, N};
    const unsigned gc = (unsigned)((4 * N + CHI_LANES - 1) / CHI_LANES);
    launch_or_record(stream, kd_mono_chiral, ac, dim3(gc));
    launch_or_record(stream, kd_mono_pick, ap, dim3(1));
}

void mlaunch_plane(void* stream, const double* d, int32_t n, double weight, double thr, double* sums) {
    const MonoPlaneJob a = {d, sums, weight, thr, n};
    launch_or_record(stream, kd_mono_plane, a, dim3((unsigned)((n + 63) / 64)));
}

}  // namespace svh

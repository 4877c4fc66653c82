// internal interface between vo_engine.cpp (host) and vo_kernels.hip (device)
#ifndef SVH_VO_INTERNAL_H
#define SVH_VO_INTERNAL_H
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "../../include/svh.h"
#include "svh_config.h"

namespace svh {

struct VoCalib {
    double f, cu, cv, base, inlier_threshold;
    int32_t reweighting;
};

struct VoResult {          // written by k_vo_refine into pinned host memory
    double tr[6];
    int32_t success;       // final Gauss-Newton converged on >= 6 inliers
    int32_t n_inliers;     // size of the winning hypothesis' inlier set (may be < 6)
    int32_t best;          // winning hypothesis, -1 = none
    int32_t pad_;
};

// Where bucketFeatures and getRandomSample draw from.  Default: libc rand(), the process-wide stream the reference
// uses (matcher.cpp:297-343 via std::random_shuffle, viso.cpp:130-153).  An object switched to a PRIVATE stream
// (svh_vo_set_private_rand) draws from its own generator instead, which reproduces glibc's srand(seed) / rand()
// sequence (the additive-feedback TYPE_3 generator, x[i] = x[i-3] + x[i-31], output x >> 1): the object then sees
// exactly the numbers it would see with the process to itself, whatever other objects or threads do, and takes
// no lock (K threads in rand() contend for glibc's lock: ~4x the uncontended cost at K = 16).
struct RandStream {
    bool is_private = false;
    uint32_t r[34];
    int at = 0;   // next output is x[at + 344] of the recurrence, kept in a ring of 34
    void seed(uint32_t s) {
        // glibc srandom_r for TYPE_3: x[0] = seed (0 -> 1), x[i] = 16807 x[i-1] mod (2^31 - 1) by Schrage's
        // method, then 310 outputs are discarded
        uint32_t x[344];
        int32_t w = s == 0 ? 1 : (int32_t)s;
        x[0] = (uint32_t)w;
        for (int i = 1; i < 31; i++) {
            const int32_t hi = w / 127773, lo = w % 127773;
            w = 16807 * lo - 2836 * hi;
            if (w < 0) w += 2147483647;
            x[i] = (uint32_t)w;
        }
        for (int i = 31; i < 34; i++) x[i] = x[i - 31];
        for (int i = 34; i < 344; i++) x[i] = x[i - 31] + x[i - 3];
        for (int i = 0; i < 34; i++) r[i] = x[310 + i];   // ring slot j holds x[j + 310 + 34 k]
        at = 0;
        is_private = true;
    }
    int next() {
        if (!is_private) return rand();
        // ring position of x[n] is (n - 310) % 34; the new element replaces x[n - 34]
        const int i = at, i3 = at >= 3 ? at - 3 : at + 31, i31 = at >= 31 ? at - 31 : at + 3;
        const uint32_t v = r[i3] + r[i31];
        r[i] = v;
        at = at == 33 ? 0 : at + 1;
        return (int)(v >> 1);
    }
};

// bucketFeatures drawing from `rs` (matcher_engine.cpp)
int32_t bucket_features(svh_matcher* m, int32_t max_features, float bw, float bh, RandStream& rs);
// svh_matcher_get_gain of K distinct, non-null Matchers, the device ones in one recorded phase (matcher_engine.cpp)
int32_t matcher_gain_batch(svh_matcher* const* ms, int32_t K, const int32_t* const* inliers, const int32_t* n,
                           float* gain);

void vlaunch_estimate(void* stream, const svh_p_match* pm, int N, const int32_t* samples, int iters,
                      const VoCalib& c, double* hyp_tr, int32_t* hyp_count, uint8_t* hyp_flags, double* Jg,
                      double* resg, VoResult* out, int32_t* out_inliers);

// VisualOdometryMono (vo_mono_engine.cpp, vo_mono_kernels.hip).  Matches go to the device as 4 floats each
// (u1p, v1p, u1c, v1c), 16 bytes per match.
// k_mono_hyp + k_mono_vote + k_mono_select: per-hypothesis counts, the winner {best, count} and its inlier flags
// (out_* in pinned host memory)
void mlaunch_ransac(void* stream, const float* q4, int32_t N, const int32_t* samples, int32_t iters, double thr,
                    double* F, int32_t* counts, int32_t* out_sel, uint8_t* out_flags, int32_t* out_counts);
// k_mono_chiral + k_mono_pick.  cams (device, 60 doubles): triangulateChieral's projection matrices, 3x4 row major
// (viso_mono.cpp:369-375): P1 = K [I | 0], then P2 = K [R | t] of the four candidates of EtoRt, (Ra,t) (Ra,-t) (Rb,t)
// (Rb,-t).  out_cand = {candidate or -1, 4 counts}, out_X = its points / 4th coordinate (4 x N)
void mlaunch_chiral(void* stream, const float* m4, int32_t N, const double* cams, double* X, uint8_t* front,
                    double* out_X, int32_t* out_cand);
// k_mono_plane: sums[i] of the ground-plane vote (0 where d[i] <= thr)
void mlaunch_plane(void* stream, const double* d, int32_t n, double weight, double thr, double* sums);

// the state of a mono estimate behind an svh_vo (vo_mono_engine.cpp)
struct MonoVo;
MonoVo* mono_create(const svh_vo_mono_params& p, int device);
void mono_destroy(MonoVo* M);
// estimateMotion (viso_mono.cpp:40-159): 1 + tr6, 0 for the reference's empty vector, < 0 on error; `inliers` is the
// object's getInlierIndices() state, cleared only where the reference clears it
int mono_estimate(MonoVo* M, const svh_p_match* pm, int32_t N, RandStream& rng, std::vector<int32_t>& inliers,
                  double* tr6);
// The same estimate in steps, for K objects walked through it together (svh_vo_mono_*_batch).  mono_prepare is the host
// part in front of the first device phase and the only step that draws random numbers (1: device work follows, 0: the
// empty vector, < 0: error); mono_enqueue issues the upload and kernels of phase 0 / 1 / 2 (into t_rec when set);
// mono_after is the host side behind the phase's wait (1: go on, or tr6 valid after phase 2; 0: the empty vector).
int mono_prepare(MonoVo* M, const svh_p_match* pm, int32_t N, RandStream& rng, std::vector<int32_t>& inliers);
void mono_enqueue(MonoVo* M, int phase);
int mono_after(MonoVo* M, int phase, std::vector<int32_t>& inliers, double* tr6);
// the three phases of the objects with state[i] > 0 (what mono_prepare returned) in lockstep: per phase one recorded
// pass, one stream wait, the host steps on the helper threads.  On return state[i] is mono_estimate's value for
// object i and tr6[6 i ..] its motion; the function returns SVH_OK or the error.  Same parameters and device.
int mono_run_batch(MonoVo* const* Ms, int32_t K, int* state, std::vector<int32_t>* const* inliers, double* tr6);
bool mono_same_params(const MonoVo* a, const MonoVo* b);
int32_t mono_votes(MonoVo* M, int32_t* out, int32_t cap);
void mono_clear(MonoVo* M);   // forget the last estimate's votes and times
void mono_set_timing(MonoVo* M, bool on);
int32_t mono_timing(MonoVo* M, double* ms3);

// Reconstruction (recon_engine.cpp, recon_kernels.hip).  k_recon_tracks + k_recon_compact over the n_lost tracks
// lost in one update: offs (n_lost + 1) / first (n_lost) / px (2 n_px floats) are the CSR of their pixels and first
// frames, order an optional lane -> track permutation (NULL: identity), frames the per-frame records of recon_core.h
// (FRAME_STRIDE doubles each).  code / xyz (device, n_lost): outcome and point per track; the ACCEPTED points are
// appended in track order to points[3 n_points ...] (room for n_lost more); out_code, out_xyz, out_count = {new
// number of points} are pinned host memory.
namespace recon {
struct Settings;
}
void rlaunch_tracks(void* stream, const int32_t* offs, const int32_t* first, const int32_t* order, const float* px,
                    int32_t n_lost, int32_t n_px, const double* frames, int32_t n_frames, const recon::Settings& s,
                    int32_t* code, float* xyz, float* points, int32_t n_points, int32_t* out_code, float* out_xyz,
                    int32_t* out_count);

}  // namespace svh
#endif

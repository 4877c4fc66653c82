// Reconstruction (libviso2/src/reconstruction.{h,cpp}) behind the svh_recon_* entries of include/svh.h.
//
// Host (this file): what is O(matches) and order-dependent -- the pose chain with Matrix::inv and operator*
// (reconstruction.cpp:59-70; include/matrix.h reproduces both bit for bit), the track_idx table, extend-or-create in
// match order and the active / lost split (:72-126).  Device (recon_kernels.hip): everything that happens to a lost
// track (:131-141), one lane per track, and the append of the accepted points in track order to a resident array.
// One update is: gather the lost tracks as a CSR into pinned memory, two uploads (the new frame record(s), the CSR),
// k_recon_tracks, k_recon_compact, one stream wait.  There is no CPU path for the device part.
//
// An update is a transaction: every buffer it needs is allocated before the tracks are touched, and a HIP failure
// later (launch, wait) undoes the association, so after SVH_ERR_HIP the object is what it was before the call and the
// same update can be given again.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/matrix.h"
#include "../../include/svh.h"
#include "recon_core.h"
#include "vo_internal.h"

namespace svh {
int fail(int code, const std::string& msg);   // elas_engine.cpp: records svh_last_error()
bool fi_armed();                              // elas_engine.cpp: fault injection (svh_internal.h)
bool fi_hit(const char* expr_text);
void report_hip_failure(const char* entry);
}  // namespace svh

using namespace svh;

namespace {

int recon_hip_failed(const char* expr, bool injected, hipError_t e) {
    const int rc = svh::fail(SVH_ERR_HIP, std::string(expr) + ": " +
                                              (injected ? "injected failure (SVH_TEST_FAIL_AT)" : hipGetErrorString(e)));
    svh::report_hip_failure("Reconstruction");
    return rc;
}
#define RECON_TRY(expr)                                                                                  \
    do {                                                                                                 \
        const bool inj_ = svh::fi_armed() && svh::fi_hit(#expr); /* svh_internal.h: fault injection */   \
        hipError_t e_ = inj_ ? hipErrorUnknown : (expr);                                                 \
        if (e_ != hipSuccess) return recon_hip_failed(#expr, inj_, e_);                                  \
    } while (0)

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Track {                  // Reconstruction::track (reconstruction.h:79-84)
    std::vector<float> px;      // u, v per frame
    int32_t first_frame, last_frame, last_idx;
};

}  // namespace

struct svh_recon {
    int device = 0;
    bool calibrated = false;
    Matrix K;
    double cp = 1, sp = 0;                          // cos / sin of Tr_cam_road's pitch (reconstruction.cpp:43-50)
    std::vector<Matrix> Tr_total, Tr_inv_total, P_total;
    std::vector<double> frames;                     // recon::FRAME_STRIDE doubles per frame, what the device holds
    std::vector<Track> tracks;                      // the active tracks
    size_t total_px = 0;                            // pixels (pairs) in `tracks`
    int32_t n_points = 0;
    std::vector<int32_t> codes;                     // last update's lost tracks, in order
    std::vector<float> xyz;
    bool sort_by_length = false;                    // SVH_RECON_SORT=1: lanes of a wave get tracks of similar length
    bool timing = false;
    double ms[3] = {0, 0, 0};
    // device side
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double* d_frames = nullptr;                     // resident per-frame records
    int32_t cap_frames = 0, dev_frames = 0;         // capacity / frames uploaded so far
    float* d_points = nullptr;                      // resident point array, 3 floats per point
    int64_t cap_points = 0;
    uint8_t *h_in = nullptr, *d_in = nullptr;       // [new frame records | offs | first | order | px]
    size_t cap_in = 0;
    int32_t *d_code = nullptr, *h_code = nullptr;   // per lost track
    float *d_xyz = nullptr, *h_xyz = nullptr;
    int32_t cap_lost = -1;
    int32_t* h_count = nullptr;
};

namespace {

// a larger device array with the first `keep` bytes of the old one; the old one stays in place on any failure
template <typename T>
int regrow(svh_recon* r, T** p, size_t keep, size_t bytes) {
    T* q = nullptr;
    RECON_TRY(hipMalloc((void**)&q, bytes + 16));
    if (keep) {
        hipError_t e = hipMemcpyAsync(q, *p, keep, hipMemcpyDeviceToDevice, r->stream);
        if (e == hipSuccess) e = (hipError_t)wait_stream(r->stream);
        if (e != hipSuccess) {
            (void)hipFree(q);
            return recon_hip_failed("hipMemcpyAsync(grow)", false, e);
        }
    }
    (void)hipFree(*p);
    *p = q;
    return SVH_OK;
}

// room for one update that may upload `new_frames` records and lose up to `lost` tracks with `px` pixels in all
int ensure(svh_recon* r, int32_t total_frames, int32_t new_frames, size_t lost, size_t px) {
    RECON_TRY(hipSetDevice(r->device));
    if (!r->stream) {
        hipStream_t s = nullptr;
        RECON_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        r->stream = s;
    }
    for (int i = 0; i < 2; i++)
        if (!r->ev[i]) RECON_TRY(hipEventCreate(&r->ev[i]));
    if (!r->h_count) RECON_TRY(hipHostMalloc((void**)&r->h_count, 64));
    int rc;
    if (total_frames > r->cap_frames) {
        const int32_t cap = std::max(total_frames, std::max(64, 2 * r->cap_frames));
        const size_t rec = recon::FRAME_STRIDE * sizeof(double);
        if ((rc = regrow(r, &r->d_frames, rec * (size_t)r->dev_frames, rec * (size_t)cap))) return rc;
        r->cap_frames = cap;
    }
    if ((int64_t)r->n_points + (int64_t)lost > r->cap_points) {
        const int64_t cap = std::max<int64_t>(r->n_points + (int64_t)lost, std::max<int64_t>(4096, 2 * r->cap_points));
        if ((rc = regrow(r, &r->d_points, 12 * (size_t)r->n_points, 12 * (size_t)cap))) return rc;
        r->cap_points = cap;
    }
    const size_t in = up16(recon::FRAME_STRIDE * sizeof(double) * (size_t)new_frames) + up16(4 * (3 * lost + 1) + 8 * px);
    if (in > r->cap_in) {
        // (capacity goes to 0 before anything is freed and back up only when both buffers exist)
        const size_t cap = std::max(in, 2 * r->cap_in);
        r->cap_in = 0;
        (void)hipHostFree(r->h_in);
        r->h_in = nullptr;
        (void)hipFree(r->d_in);
        r->d_in = nullptr;
        RECON_TRY(hipHostMalloc((void**)&r->h_in, cap + 16));
        RECON_TRY(hipMalloc((void**)&r->d_in, cap + 16));
        r->cap_in = cap;
    }
    if ((int64_t)lost > (int64_t)r->cap_lost) {
        const size_t cap = std::max(lost, (size_t)std::max(1024, 2 * std::max(r->cap_lost, 0)));
        r->cap_lost = -1;
        (void)hipFree(r->d_code); r->d_code = nullptr;
        (void)hipFree(r->d_xyz); r->d_xyz = nullptr;
        (void)hipHostFree(r->h_code); r->h_code = nullptr;
        (void)hipHostFree(r->h_xyz); r->h_xyz = nullptr;
        RECON_TRY(hipMalloc((void**)&r->d_code, 4 * cap + 16));
        RECON_TRY(hipMalloc((void**)&r->d_xyz, 12 * cap + 16));
        RECON_TRY(hipHostMalloc((void**)&r->h_code, 4 * cap + 16));
        RECON_TRY(hipHostMalloc((void**)&r->h_xyz, 12 * cap + 16));
        r->cap_lost = (int32_t)cap;
    }
    return SVH_OK;
}

void frame_record(const Matrix& P, const Matrix& Tr, const Matrix& Tri, double* out) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) out[recon::FRAME_P + 4 * i + j] = P._val[i][j];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            out[recon::FRAME_TR + 4 * i + j] = Tr._val[i][j];
            out[recon::FRAME_TRI + 4 * i + j] = Tri._val[i][j];
        }
}

// the device part of an update for the lost tracks tracks[lost[0]], tracks[lost[1]], ...
int run_lost(svh_recon* r, const std::vector<int32_t>& lost, size_t n_px, const recon::Settings& s, double t_start) {
    const int32_t n_lost = (int32_t)lost.size();
    const int32_t total_frames = (int32_t)r->Tr_total.size(), new_frames = total_frames - r->dev_frames;
    const size_t rec = recon::FRAME_STRIDE * sizeof(double);
    const size_t frames_bytes = up16(rec * (size_t)new_frames);
    uint8_t* h = r->h_in;
    memcpy(h, r->frames.data() + (size_t)recon::FRAME_STRIDE * r->dev_frames, rec * (size_t)new_frames);
    int32_t* offs = reinterpret_cast<int32_t*>(h + frames_bytes);
    int32_t* first = offs + n_lost + 1;
    int32_t* order = first + n_lost;
    float* px = reinterpret_cast<float*>(order + n_lost);
    size_t at = 0;
    for (int32_t i = 0; i < n_lost; i++) {
        const Track& t = r->tracks[lost[i]];
        offs[i] = (int32_t)at;
        first[i] = t.first_frame;
        order[i] = i;
        memcpy(px + 2 * at, t.px.data(), t.px.size() * sizeof(float));
        at += t.px.size() / 2;
    }
    offs[n_lost] = (int32_t)at;
    if (r->sort_by_length)
        std::stable_sort(order, order + n_lost,
                         [&](int32_t a, int32_t b) { return offs[a + 1] - offs[a] > offs[b + 1] - offs[b]; });
    const size_t csr_bytes = up16(4 * (3 * (size_t)n_lost + 1) + 8 * n_px);
    const uint8_t* d = r->d_in + frames_bytes;
    const int32_t* d_offs = reinterpret_cast<const int32_t*>(d);
    const int32_t* d_first = d_offs + n_lost + 1;
    const int32_t* d_order = d_first + n_lost;
    const float* d_px = reinterpret_cast<const float*>(d_order + n_lost);
    const double t_launch = now_ms();
    if (r->timing) (void)hipEventRecord(r->ev[0], r->stream);
    vlaunch_upload(r->stream, h, reinterpret_cast<uint8_t*>(r->d_frames) + rec * (size_t)r->dev_frames,
                   rec * (size_t)new_frames);   // (44 doubles: a multiple of 16 bytes)
    vlaunch_upload(r->stream, h + frames_bytes, r->d_in + frames_bytes, csr_bytes);
    r->h_count[0] = -1;
    rlaunch_tracks(r->stream, d_offs, d_first, r->sort_by_length ? d_order : nullptr, d_px, n_lost, (int32_t)n_px,
                   r->d_frames, total_frames, s, r->d_code, r->d_xyz, r->d_points, r->n_points, r->h_code, r->h_xyz,
                   r->h_count);
    if (r->timing) (void)hipEventRecord(r->ev[1], r->stream);
    RECON_TRY(hipGetLastError());
    RECON_TRY((hipError_t)wait_stream(r->stream));
    RECON_TRY(hipGetLastError());
    const double t_done = now_ms();
    const int32_t count = r->h_count[0];
    if (count < r->n_points || count > r->n_points + n_lost)
        return svh::fail(SVH_ERR_HIP, "Reconstruction: the device returned an impossible point count");
    r->codes.assign(r->h_code, r->h_code + n_lost);
    r->xyz.assign(r->h_xyz, r->h_xyz + 3 * (size_t)n_lost);
    r->n_points = count;
    r->dev_frames = total_frames;
    if (r->timing) {
        float ms = 0;
        r->ms[0] = t_launch - t_start;
        r->ms[1] = hipEventElapsedTime(&ms, r->ev[0], r->ev[1]) == hipSuccess ? ms : 0;
        r->ms[2] = now_ms() - t_done;
    }
    return SVH_OK;
}

}  // namespace

extern "C" {

svh_recon* svh_recon_create(void) {
    svh::ensure_init();
    svh_recon* r = new svh_recon();
    r->K = Matrix::eye(3);
    r->Tr_total.push_back(Matrix::eye(4));       // reconstruction.cpp:27-35
    r->Tr_inv_total.push_back(Matrix::eye(4));
    int nd = 0;
    if (hipGetDeviceCount(&nd) == hipSuccess && nd > 0) (void)hipGetDevice(&r->device);
    const char* e = svh::env("SVH_RECON_SORT");   // (honours svh_config::read_env)
    r->sort_by_length = e && atoi(e) != 0;
    return r;
}

void svh_recon_destroy(svh_recon* r) {
    if (!r) return;
    if (r->stream) {
        (void)hipSetDevice(r->device);
        (void)hipStreamSynchronize(r->stream);
        (void)hipStreamDestroy(r->stream);
    }
    for (int i = 0; i < 2; i++)
        if (r->ev[i]) (void)hipEventDestroy(r->ev[i]);
    (void)hipFree(r->d_frames); (void)hipFree(r->d_points); (void)hipFree(r->d_in); (void)hipFree(r->d_code);
    (void)hipFree(r->d_xyz);
    (void)hipHostFree(r->h_in); (void)hipHostFree(r->h_code); (void)hipHostFree(r->h_xyz); (void)hipHostFree(r->h_count);
    delete r;
}

int32_t svh_recon_set_calibration(svh_recon* r, double f, double cu, double cv) {
    if (!r) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_set_calibration: null object");
    // a second call would push a second P_total[0] in the reference and misalign every later frame
    if (r->calibrated) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_set_calibration: the calibration is already set");
    const FLOAT K_data[9] = {f, 0, cu, 0, f, cv, 0, 0, 1};
    r->K = Matrix(3, 3, K_data);
    const FLOAT cam_pitch = -0.08;
    r->cp = cos(cam_pitch);
    r->sp = sin(cam_pitch);
    r->P_total.push_back(r->K * Matrix::eye(4).getMat(0, 0, 2, 3));
    r->frames.resize(recon::FRAME_STRIDE);
    frame_record(r->P_total[0], r->Tr_total[0], r->Tr_inv_total[0], r->frames.data());
    r->calibrated = true;
    return SVH_OK;
}

int32_t svh_recon_update(svh_recon* r, const svh_p_match* m, int32_t n, const double Tr[16], int32_t point_type,
                         int32_t min_track_length, double max_dist, double min_angle) {
    if (!r || !Tr || n < 0 || (n > 0 && !m)) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update: bad arguments");
    // P_total is empty before setCalibration: the reference reads past its end
    if (!r->calibrated) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update before svh_recon_set_calibration");
    for (int32_t i = 0; i < n; i++)
        if (m[i].i1p < 0 || m[i].i1c < 0)   // (they index track_idx)
            return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update: negative feature index");
    const double t_start = now_ms();
    ActiveCaller active;
    const int32_t total_frames = (int32_t)r->Tr_total.size() + 1;
    int rc = ensure(r, total_frames, total_frames - r->dev_frames, r->tracks.size(), r->total_px);
    if (rc) return rc;

    // ---- pose chain (:61-70)
    const Matrix T(4, 4, Tr);
    const Matrix Tr_total_curr = r->Tr_total.back() * Matrix::inv(T);
    r->Tr_total.push_back(Tr_total_curr);
    r->Tr_inv_total.push_back(Matrix::inv(Tr_total_curr));
    r->P_total.push_back(r->K * Matrix::inv(Tr_total_curr).getMat(0, 0, 2, 3));
    r->frames.resize((size_t)recon::FRAME_STRIDE * total_frames);
    frame_record(r->P_total.back(), r->Tr_total.back(), r->Tr_inv_total.back(),
                 r->frames.data() + (size_t)recon::FRAME_STRIDE * (total_frames - 1));
    const int32_t current_frame = total_frames - 1;

    // ---- index vector (:75-87): a later track overwrites the slot of an earlier one with the same last_idx
    int32_t track_idx_max = 0;
    for (int32_t i = 0; i < n; i++) track_idx_max = std::max(track_idx_max, m[i].i1p);
    for (const Track& t : r->tracks) track_idx_max = std::max(track_idx_max, t.last_idx);
    std::vector<int32_t> track_idx((size_t)track_idx_max + 1, -1);
    const size_t old_tracks = r->tracks.size();
    for (size_t i = 0; i < old_tracks; i++) track_idx[r->tracks[i].last_idx] = (int32_t)i;

    // ---- associate matches to tracks (:89-112), keeping what is needed to take it back
    std::vector<std::pair<int32_t, int32_t>> undo;   // (track, its last_idx before this extension)
    for (int32_t i = 0; i < n; i++) {
        const int32_t idx = track_idx[m[i].i1p];
        if (idx >= 0 && r->tracks[idx].last_frame == current_frame - 1) {
            Track& t = r->tracks[idx];
            undo.emplace_back(idx, t.last_idx);
            t.px.push_back(m[i].u1c);
            t.px.push_back(m[i].v1c);
            t.last_frame = current_frame;
            t.last_idx = m[i].i1c;
        } else {
            Track t;
            t.px = {m[i].u1p, m[i].v1p, m[i].u1c, m[i].v1c};
            t.first_frame = current_frame - 1;
            t.last_frame = current_frame;
            t.last_idx = m[i].i1c;
            r->tracks.push_back(std::move(t));
        }
    }

    // ---- the lost tracks, in order (:118-145), to the device
    std::vector<int32_t> lost;
    size_t lost_px = 0;
    for (size_t i = 0; i < old_tracks; i++)
        if (r->tracks[i].last_frame != current_frame) {
            lost.push_back((int32_t)i);
            lost_px += r->tracks[i].px.size() / 2;
        }
    const recon::Settings s = {point_type, min_track_length, max_dist, min_angle, r->cp, r->sp};
    rc = run_lost(r, lost, lost_px, s, t_start);
    if (rc) {
        // take the update back: the object is what it was before the call
        (void)hipStreamSynchronize(r->stream);
        r->tracks.resize(old_tracks);
        for (size_t k = undo.size(); k-- > 0;) {
            Track& t = r->tracks[undo[k].first];
            t.px.resize(t.px.size() - 2);
            t.last_frame = current_frame - 1;
            t.last_idx = undo[k].second;
        }
        r->Tr_total.pop_back();
        r->Tr_inv_total.pop_back();
        r->P_total.pop_back();
        r->frames.resize((size_t)recon::FRAME_STRIDE * (total_frames - 1));
        return rc;
    }
    // ---- keep the active tracks
    size_t keep = 0, kept_px = 0;
    for (size_t i = 0; i < r->tracks.size(); i++)
        if (r->tracks[i].last_frame == current_frame) {
            kept_px += r->tracks[i].px.size() / 2;
            if (keep != i) r->tracks[keep] = std::move(r->tracks[i]);
            keep++;
        }
    r->tracks.resize(keep);
    r->total_px = kept_px;
    return SVH_OK;
}

int32_t svh_recon_num_points(svh_recon* r) { return r ? r->n_points : 0; }

int32_t svh_recon_get_points(svh_recon* r, float* xyz, int32_t cap) {
    if (!r) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_get_points: null object");
    const int32_t n = std::min(r->n_points, cap);
    if (xyz && n > 0) {
        RECON_TRY(hipSetDevice(r->device));
        RECON_TRY(hipMemcpyAsync(xyz, r->d_points, 12 * (size_t)n, hipMemcpyDeviceToHost, r->stream));
        RECON_TRY((hipError_t)wait_stream(r->stream));
    }
    return r->n_points;
}

int32_t svh_recon_get_points_device(svh_recon* r, const float** xyz) {
    if (!r || !xyz) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_get_points_device: bad arguments");
    *xyz = r->d_points;   // valid until the next update (the array may move when it grows)
    return r->n_points;
}

int32_t svh_recon_num_tracks(svh_recon* r) { return r ? (int32_t)r->tracks.size() : 0; }

int32_t svh_recon_get_outcomes(svh_recon* r, int32_t* code, float* xyz, int32_t cap) {
    if (!r) return 0;
    const int32_t n = (int32_t)r->codes.size(), k = std::min(n, cap);
    if (code && k > 0) memcpy(code, r->codes.data(), 4 * (size_t)k);
    if (xyz && k > 0) memcpy(xyz, r->xyz.data(), 12 * (size_t)k);
    return n;
}

void svh_recon_set_timing(svh_recon* r, int32_t on) {
    if (r) r->timing = on != 0;
}

int32_t svh_recon_get_timing(svh_recon* r, double* ms3) {
    if (!r) return 0;
    for (int i = 0; i < 3 && ms3; i++) ms3[i] = r->ms[i];
    return 3;
}

}  // extern "C"

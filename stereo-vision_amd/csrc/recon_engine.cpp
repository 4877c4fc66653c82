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
#include <numeric>
#include <string>
#include <vector>

#include "../../include/matrix.h"
#include "../../include/svh.h"
#include "batch_rec.h"
#include "hip_guard.h"
#include "matcher_internal.h"
#include "recon_core.h"
#include "recon_internal.h"
#include "vo_internal.h"

using namespace svh;

namespace {

#define RECON_TRY(kind, expr) SVH_HIP_TRY("Reconstruction", kind, expr)
#define RECON_GROW(buf, bytes) SVH_HIP_GROW("Reconstruction", buf, bytes)

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
    // (the cap_* are element counts: what the buffers were last asked to hold, and the base of the doubling)
    HipBuf<double> d_frames;                        // resident per-frame records
    int32_t cap_frames = 0, dev_frames = 0;         // capacity / frames uploaded so far
    HipBuf<float> d_points;                         // resident point array, 3 floats per point
    int64_t cap_points = 0;
    PinnedBuf<uint8_t> h_in;                        // [new frame records | offs | first | order | px]
    HipBuf<uint8_t> d_in;
    size_t cap_in = 0;
    HipBuf<int32_t> d_code;                         // per lost track
    PinnedBuf<int32_t> h_code;
    HipBuf<float> d_xyz;
    PinnedBuf<float> h_xyz;
    size_t cap_lost = 0;
    PinnedBuf<int32_t> h_count;
    // the resident form (svh_recon_create_resident, recon_internal.h): the tracks are a CSR in device memory, tb[cur]
    // holds them and tb[cur ^ 1] is written by an update; `tracks` stays empty
    bool resident = false;
    struct TrackBuf {
        HipBuf<int32_t> first, last, offs;
        HipBuf<float> px;
    } tb[2];
    int cur = 0;
    int32_t n_tracks = 0, cap_tracks = 0;
    int64_t cap_px = 0;
    int32_t idx_bound = 0;                          // every last_idx of the table is below it
    HipBuf<int32_t> d_tidx, d_claim, d_midx, d_src, d_lost, d_hdr;
    int32_t cap_tidx = 0, cap_midx = 0;
    PinnedBuf<ReconJob> h_jobs;                     // job table of the updates this object leads
    HipBuf<ReconJob> d_jobs;
};

namespace {

// a larger device array with the first `keep` bytes of the old one; the old one stays in place on any failure
template <typename T>
int regrow(svh_recon* r, HipBuf<T>& p, size_t keep, size_t bytes) {
    HipBuf<T> q;
    RECON_GROW(q, bytes + 16);
    if (keep) {
        hipError_t e = hipMemcpyAsync(q.p, p.p, keep, hipMemcpyDeviceToDevice, r->stream);
        if (e == hipSuccess) e = (hipError_t)wait_stream(r->stream);
        if (e != hipSuccess) return svh::hip_failed("Reconstruction", "hipMemcpyAsync(grow)", false, e);
    }
    p = std::move(q);
    return SVH_OK;
}

// room for one update that may upload `new_frames` records and lose up to `lost` tracks with `px` pixels in all
int ensure(svh_recon* r, int32_t total_frames, int32_t new_frames, size_t lost, size_t px) {
    RECON_TRY(none, hipSetDevice(r->device));
    if (!r->stream) {
        hipStream_t s = nullptr;
        RECON_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        r->stream = s;
    }
    for (int i = 0; i < 2; i++)
        if (!r->ev[i]) RECON_TRY(none, hipEventCreate(&r->ev[i]));
    RECON_GROW(r->h_count, 64);
    int rc;
    if (total_frames > r->cap_frames) {
        const int32_t cap = std::max(total_frames, std::max(64, 2 * r->cap_frames));
        const size_t rec = recon::FRAME_STRIDE * sizeof(double);
        if ((rc = regrow(r, r->d_frames, rec * (size_t)r->dev_frames, rec * (size_t)cap))) return rc;
        r->cap_frames = cap;
    }
    if ((int64_t)r->n_points + (int64_t)lost > r->cap_points) {
        const int64_t cap = std::max<int64_t>(r->n_points + (int64_t)lost, std::max<int64_t>(4096, 2 * r->cap_points));
        if ((rc = regrow(r, r->d_points, 12 * (size_t)r->n_points, 12 * (size_t)cap))) return rc;
        r->cap_points = cap;
    }
    const size_t in = up16(recon::FRAME_STRIDE * sizeof(double) * (size_t)new_frames) + up16(4 * (3 * lost + 1) + 8 * px);
    // (a buffer that a failed growth left empty is allocated again here: the owners know what they hold)
    if (in > r->cap_in) r->cap_in = std::max(in, 2 * r->cap_in);
    RECON_GROW(r->h_in, r->cap_in + 16);
    RECON_GROW(r->d_in, r->cap_in + 16);
    const size_t want = std::max<size_t>(lost, 1024);   // (the first update allocates even when nothing is lost)
    if (want > r->cap_lost) r->cap_lost = std::max(want, 2 * r->cap_lost);
    RECON_GROW(r->d_code, 4 * r->cap_lost + 16);
    RECON_GROW(r->d_xyz, 12 * r->cap_lost + 16);
    RECON_GROW(r->h_code, 4 * r->cap_lost + 16);
    RECON_GROW(r->h_xyz, 12 * r->cap_lost + 16);
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

// the pose chain of one update (:61-70): one more frame in Tr_total, Tr_inv_total, P_total and `frames`
void push_pose(svh_recon* r, const double* Tr) {
    const Matrix T(4, 4, Tr);
    const Matrix Tr_total_curr = r->Tr_total.back() * Matrix::inv(T);
    r->Tr_total.push_back(Tr_total_curr);
    r->Tr_inv_total.push_back(Matrix::inv(Tr_total_curr));
    r->P_total.push_back(r->K * Matrix::inv(Tr_total_curr).getMat(0, 0, 2, 3));
    const size_t total_frames = r->Tr_total.size();
    r->frames.resize((size_t)recon::FRAME_STRIDE * total_frames);
    frame_record(r->P_total.back(), r->Tr_total.back(), r->Tr_inv_total.back(),
                 r->frames.data() + (size_t)recon::FRAME_STRIDE * (total_frames - 1));
}

// ... and the way back, for an update that failed
void pop_pose(svh_recon* r) {
    r->Tr_total.pop_back();
    r->Tr_inv_total.pop_back();
    r->P_total.pop_back();
    r->frames.resize((size_t)recon::FRAME_STRIDE * r->Tr_total.size());
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
    mlaunch_upload(r->stream, h, reinterpret_cast<uint8_t*>(r->d_frames.p) + rec * (size_t)r->dev_frames,
                   rec * (size_t)new_frames);   // (44 doubles: a multiple of 16 bytes)
    mlaunch_upload(r->stream, h + frames_bytes, r->d_in + frames_bytes, csr_bytes);
    r->h_count[0] = -1;
    rlaunch_tracks(r->stream, d_offs, d_first, r->sort_by_length ? d_order : nullptr, d_px, n_lost, (int32_t)n_px,
                   r->d_frames, total_frames, s, r->d_code, r->d_xyz, r->d_points, r->n_points, r->h_code, r->h_xyz,
                   r->h_count);
    if (r->timing) (void)hipEventRecord(r->ev[1], r->stream);
    RECON_TRY(launch, hipGetLastError());
    RECON_TRY(none, (hipError_t)wait_stream(r->stream));
    RECON_TRY(launch, hipGetLastError());
    const double t_done = now_ms();
    const int32_t count = r->h_count[0];
    if (count < r->n_points || count > r->n_points + n_lost)
        return svh::fail(SVH_ERR_HIP, "Reconstruction: the device returned an impossible point count");
    r->codes.assign(r->h_code.p, r->h_code.p + n_lost);
    r->xyz.assign(r->h_xyz.p, r->h_xyz.p + 3 * (size_t)n_lost);
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

// ------------------------------------------------------------------------------------------------ resident form
// An update of K resident objects (K = 1: svh_recon_update / svh_recon_update_device) is: room for every object,
// the K pose chains, one job per object, one copy of the job table, the seven launches of rlaunch_resident on the
// first object's stream, one wait.  It is a transaction like the host-table update: everything is allocated before
// an object is touched, an update reads buffer A and writes buffer B, appends behind the points that exist and
// uploads its frame record behind the records that are counted, so a failure only has to take the pose chains back.
constexpr int32_t MAX_FEATURE_INDEX = 1 << 26;   // track_idx is an array of max_index entries in device memory

bool have_device() {
    int nd = 0;
    return hipGetDeviceCount(&nd) == hipSuccess && nd > 0;
}

struct ResidentUpdate {
    svh_recon* r;
    const svh_p_match* host;    // matches in host memory, or
    const svh_p_match* dev;     // in device memory
    int32_t n, max_index;
    const double* Tr;
    int32_t slot;               // position in the caller's arrays
};

// room for an update of r with n matches and a feature-index table of tbl entries
int ensure_resident(svh_recon* r, int32_t n, int32_t tbl, bool host_matches) {
    const int32_t total_frames = (int32_t)r->Tr_total.size() + 1;
    // ensure(): stream, events, frame records, a point and an outcome per old track (all of them may be lost), and
    // the staging pair h_in / d_in -- its CSR part carries the matches here, 48 n bytes = 8 bytes x 6 n "pixels"
    int rc = ensure(r, total_frames, total_frames - r->dev_frames, (size_t)r->n_tracks, host_matches ? 6 * (size_t)n : 0);
    if (rc) return rc;
    RECON_GROW(r->d_hdr, 4 * RT_HDR + 16);
    const int64_t need_tracks = (int64_t)r->n_tracks + n, need_px = (int64_t)r->total_px + 2 * (int64_t)n;
    if (need_tracks > INT32_MAX / 4 || need_px > INT32_MAX / 4)
        return svh::fail(SVH_ERR_BAD_ARG, "Reconstruction: the track table would exceed 2^29 entries");
    if (need_tracks > r->cap_tracks || !r->cap_tracks) {   // (an empty first update still writes offs[0] of B)
        const size_t cap = (size_t)std::max<int64_t>(need_tracks, std::max<int64_t>(4096, 2 * (int64_t)r->cap_tracks));
        const size_t keep = 4 * (size_t)r->n_tracks;
        for (int b = 0; b < 2; b++) {
            const bool a = b == r->cur;
            svh_recon::TrackBuf& t = r->tb[b];
            if ((rc = regrow(r, t.first, a ? keep : 0, 4 * cap))) return rc;
            if ((rc = regrow(r, t.last, a ? keep : 0, 4 * cap))) return rc;
            if ((rc = regrow(r, t.offs, a && r->n_tracks ? keep + 4 : 0, 4 * (cap + 1)))) return rc;
        }
        if ((rc = regrow(r, r->d_claim, 0, 4 * cap))) return rc;
        if ((rc = regrow(r, r->d_src, 0, 4 * cap))) return rc;
        if ((rc = regrow(r, r->d_lost, 0, 4 * cap))) return rc;
        r->cap_tracks = (int32_t)cap;
    }
    if (need_px > r->cap_px) {
        const int64_t cap = std::max<int64_t>(need_px, std::max<int64_t>(16384, 2 * r->cap_px));
        for (int b = 0; b < 2; b++)
            if ((rc = regrow(r, r->tb[b].px, b == r->cur ? 8 * r->total_px : 0, 8 * (size_t)cap))) return rc;
        r->cap_px = cap;
    }
    if (tbl > r->cap_tidx) {
        const int32_t cap = std::max(tbl, std::max(4096, 2 * r->cap_tidx));
        if ((rc = regrow(r, r->d_tidx, 0, 4 * (size_t)cap))) return rc;
        r->cap_tidx = cap;
    }
    if (n > r->cap_midx) {
        const int32_t cap = std::max(n, std::max(4096, 2 * r->cap_midx));
        if ((rc = regrow(r, r->d_midx, 0, 4 * (size_t)cap))) return rc;
        r->cap_midx = cap;
    }
    return SVH_OK;
}

int ensure_jobs(svh_recon* lead, int32_t K) {
    const size_t bytes = sizeof(ReconJob) * (size_t)std::max(K, 16);
    RECON_GROW(lead->h_jobs, bytes);
    RECON_GROW(lead->d_jobs, bytes);
    return SVH_OK;
}

// the job of one object; its pose chain already holds the new frame
ReconJob make_job(const ResidentUpdate& u, const recon::Settings& s) {
    svh_recon* r = u.r;
    const int32_t total_frames = (int32_t)r->Tr_total.size(), new_frames = total_frames - r->dev_frames;
    const size_t rec = recon::FRAME_STRIDE * sizeof(double);
    const size_t frames_bytes = up16(rec * (size_t)new_frames);
    memcpy(r->h_in, r->frames.data() + (size_t)recon::FRAME_STRIDE * r->dev_frames, rec * (size_t)new_frames);
    const svh_recon::TrackBuf &A = r->tb[r->cur], &B = r->tb[r->cur ^ 1];
    ReconJob j;
    memset(&j, 0, sizeof(j));
    j.a_first = A.first; j.a_last = A.last; j.a_offs = A.offs; j.a_px = A.px;
    j.b_first = B.first; j.b_last = B.last; j.b_offs = B.offs; j.b_px = B.px;
    j.n = u.n; j.n_old = r->n_tracks; j.old_px = (int32_t)r->total_px;
    j.max_index = u.max_index;
    j.tbl = std::max(u.max_index, r->idx_bound);
    j.cap_tracks = r->cap_tracks; j.cap_px = (int32_t)std::min<int64_t>(r->cap_px, INT32_MAX);
    j.frame_prev = total_frames - 2;
    j.n_frames = total_frames; j.n_points = r->n_points;
    j.track_idx = r->d_tidx; j.claim = r->d_claim; j.midx = r->d_midx; j.src = r->d_src; j.lost = r->d_lost;
    j.hdr = r->d_hdr;
    j.frames = r->d_frames;
    j.s = s;
    j.s.cp = r->cp; j.s.sp = r->sp;
    j.code = r->d_code; j.xyz = r->d_xyz; j.points = r->d_points;
    j.out_hdr = r->h_count; j.out_code = r->h_code; j.out_xyz = r->h_xyz;
    j.up_src[0] = r->h_in;
    j.up_dst[0] = reinterpret_cast<uint8_t*>(r->d_frames.p) + rec * (size_t)r->dev_frames;
    j.up_bytes[0] = (uint32_t)(rec * (size_t)new_frames);   // (44 doubles: a multiple of 16 bytes)
    if (u.host && u.n > 0) {
        memcpy(r->h_in + frames_bytes, u.host, sizeof(svh_p_match) * (size_t)u.n);
        j.up_src[1] = r->h_in + frames_bytes;
        j.up_dst[1] = r->d_in + frames_bytes;
        j.up_bytes[1] = (uint32_t)(sizeof(svh_p_match) * (size_t)u.n);   // (48 bytes each)
        j.m = reinterpret_cast<const svh_p_match*>(r->d_in + frames_bytes);
    } else {
        j.m = u.dev;
    }
    r->h_count[RT_POINTS] = -1;
    r->h_count[RT_ERROR] = 0;
    return j;
}

// job table, launches and the wait, on the first object's stream
int resident_device(svh_recon* lead, int32_t K, bool timing) {
    int32_t max_n = 0, max_old = 0, max_tbl = 0;
    uint32_t max_up = 0;
    for (int32_t i = 0; i < K; i++) {
        const ReconJob& j = lead->h_jobs[i];
        max_n = std::max(max_n, j.n);
        max_old = std::max(max_old, j.n_old);
        max_tbl = std::max(max_tbl, j.tbl);
        max_up = std::max(max_up, std::max(j.up_bytes[0], j.up_bytes[1]));
    }
    if (timing) (void)hipEventRecord(lead->ev[0], lead->stream);
    RECON_TRY(copy, hipMemcpyAsync(lead->d_jobs, lead->h_jobs, sizeof(ReconJob) * (size_t)K, hipMemcpyHostToDevice,
                             lead->stream));
    rlaunch_resident(lead->stream, lead->d_jobs, K, max_n, max_old, max_tbl, max_up);
    if (timing) (void)hipEventRecord(lead->ev[1], lead->stream);
    RECON_TRY(launch, hipGetLastError());
    RECON_TRY(wait, (hipError_t)wait_stream(lead->stream));
    RECON_TRY(launch, hipGetLastError());
    return SVH_OK;
}

// what the device reported for one object: SVH_OK, SVH_ERR_BAD_ARG (its matches: this object alone is refused) or
// SVH_ERR_HIP (a header that cannot be: the whole update is refused)
int resident_verdict(const ResidentUpdate& u, const ReconJob& j) {
    const svh_recon* r = u.r;
    const int32_t* h = r->h_count;
    const int32_t n_lost = h[RT_LOST], count = h[RT_POINTS];
    if (h[RT_ERROR] & RT_BAD_INDEX)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update: a feature index outside [0, max_index)");
    if (h[RT_ERROR] || h[RT_EXTENDED] < 0 || h[RT_EXTENDED] > j.n_old || h[RT_CREATED] < 0 || h[RT_CREATED] > j.n ||
        n_lost != j.n_old - h[RT_EXTENDED] || h[RT_PIXELS] < 0 || h[RT_PIXELS] > j.cap_px || count < r->n_points ||
        count > r->n_points + n_lost)
        return svh::fail(SVH_ERR_HIP, "Reconstruction: the device returned an impossible track or point count");
    return SVH_OK;
}

// the update of one object becomes its state
void resident_commit(const ResidentUpdate& u) {
    svh_recon* r = u.r;
    const int32_t* h = r->h_count;
    const int32_t n_lost = h[RT_LOST];
    r->cur ^= 1;
    r->n_tracks = h[RT_EXTENDED] + h[RT_CREATED];
    r->total_px = (size_t)h[RT_PIXELS];
    r->idx_bound = u.max_index;
    r->codes.assign(r->h_code.p, r->h_code.p + n_lost);
    r->xyz.assign(r->h_xyz.p, r->h_xyz.p + 3 * (size_t)n_lost);
    r->n_points = h[RT_POINTS];
    r->dev_frames = (int32_t)r->Tr_total.size();
}

// K objects of one device in lockstep.  status (may be NULL): per caller slot.  Returns SVH_OK when the device part
// ran (each object's own outcome is in status), or the error that left every object as it was.
int resident_run(std::vector<ResidentUpdate>& us, const recon::Settings& s, int32_t* status, double t_start) {
    const int32_t K = (int32_t)us.size();
    if (K == 0) return SVH_OK;
    svh_recon* lead = us[0].r;
    int rc;
    for (const ResidentUpdate& u : us)
        if ((rc = ensure_resident(u.r, u.n, std::max(u.max_index, u.r->idx_bound), u.host != nullptr))) return rc;
    if ((rc = ensure_jobs(lead, K))) return rc;
    bool timing = false;
    for (int32_t i = 0; i < K; i++) {
        push_pose(us[i].r, us[i].Tr);
        lead->h_jobs[i] = make_job(us[i], s);
        timing = timing || us[i].r->timing;
    }
    const double t_launch = now_ms();
    rc = resident_device(lead, K, timing);
    if (rc) {
        (void)hipStreamSynchronize(lead->stream);   // whatever was launched has written only what is not counted yet
        for (const ResidentUpdate& u : us) pop_pose(u.r);
        return rc;
    }
    const double t_done = now_ms();
    // every header is looked at before any object is committed: an impossible one refuses the whole update
    std::vector<int> verdict(K);
    for (int32_t i = 0; i < K; i++)
        if ((verdict[i] = resident_verdict(us[i], lead->h_jobs[i])) == SVH_ERR_HIP) {
            for (const ResidentUpdate& u : us) pop_pose(u.r);
            return SVH_ERR_HIP;
        }
    for (int32_t i = 0; i < K; i++) {
        if (verdict[i] == SVH_OK) resident_commit(us[i]);
        else pop_pose(us[i].r);
        if (status) status[us[i].slot] = verdict[i];
    }
    if (timing) {
        float ms = 0;
        const double dev = hipEventElapsedTime(&ms, lead->ev[0], lead->ev[1]) == hipSuccess ? ms : 0;
        const double t_end = now_ms();
        for (const ResidentUpdate& u : us)
            if (u.r->timing) {
                u.r->ms[0] = t_launch - t_start;
                u.r->ms[1] = dev;
                u.r->ms[2] = t_end - t_done;
            }
    }
    return SVH_OK;
}

// the host's look at matches in host memory: SVH_OK and the bound of their feature indices, or SVH_ERR_BAD_ARG
int scan_matches(const svh_p_match* m, int32_t n, int32_t* max_index) {
    int32_t top = -1;
    for (int32_t i = 0; i < n; i++) {
        if (m[i].i1p < 0 || m[i].i1c < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update: negative feature index");
        top = std::max(top, std::max(m[i].i1p, m[i].i1c));
    }
    if (top >= MAX_FEATURE_INDEX)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update: a feature index of 2^26 or more on a resident object");
    *max_index = top + 1;
    return SVH_OK;
}

int resident_update_one(svh_recon* r, const svh_p_match* host, const svh_p_match* dev, int32_t n, int32_t max_index,
                        const double* Tr, const recon::Settings& s) {
    const double t_start = now_ms();
    ActiveCaller active;
    std::vector<ResidentUpdate> us(1, ResidentUpdate{r, host, dev, n, max_index, Tr, 0});
    int32_t status = SVH_OK;
    const int rc = resident_run(us, s, &status, t_start);
    return rc ? rc : status;
}

}  // namespace

extern "C" {

static svh_recon* recon_create(bool resident);
svh_recon* svh_recon_create(void) { return recon_create(false); }
svh_recon* svh_recon_create_resident(void) { return recon_create(true); }

static svh_recon* recon_create(bool resident) {
    svh::ensure_init();
    svh_recon* r = new svh_recon();
    r->K = Matrix::eye(3);
    r->Tr_total.push_back(Matrix::eye(4));       // reconstruction.cpp:27-35
    r->Tr_inv_total.push_back(Matrix::eye(4));
    int nd = 0;
    if (hipGetDeviceCount(&nd) == hipSuccess && nd > 0) (void)hipGetDevice(&r->device);
    const char* e = svh::env("SVH_RECON_SORT");   // (honours svh_config::read_env)
    r->sort_by_length = e && atoi(e) != 0;
    r->resident = resident;
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
    delete r;   // the buffers free themselves, on the device selected above
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
    if (r->resident) {
        int32_t max_index = 0;
        const int rc = scan_matches(m, n, &max_index);
        if (rc) return rc;
        if (!have_device()) return svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
        const recon::Settings s = {point_type, min_track_length, max_dist, min_angle, r->cp, r->sp};
        return resident_update_one(r, m, nullptr, n, max_index, Tr, s);
    }
    for (int32_t i = 0; i < n; i++)
        if (m[i].i1p < 0 || m[i].i1c < 0)   // (they index track_idx)
            return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update: negative feature index");
    const double t_start = now_ms();
    ActiveCaller active;
    const int32_t total_frames = (int32_t)r->Tr_total.size() + 1;
    int rc = ensure(r, total_frames, total_frames - r->dev_frames, r->tracks.size(), r->total_px);
    if (rc) return rc;

    push_pose(r, Tr);
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
        pop_pose(r);
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

int32_t svh_recon_update_device(svh_recon* r, const svh_p_match* d_matches, int32_t n, int32_t max_index,
                                const double Tr[16], int32_t point_type, int32_t min_track_length, double max_dist,
                                double min_angle) {
    if (!r || !Tr || n < 0 || (n > 0 && !d_matches) || max_index < 0 || max_index > MAX_FEATURE_INDEX)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update_device: bad arguments");
    if (!r->resident)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update_device needs an object of svh_recon_create_resident");
    if (!r->calibrated) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update_device before svh_recon_set_calibration");
    if (!have_device()) return svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
    const recon::Settings s = {point_type, min_track_length, max_dist, min_angle, r->cp, r->sp};
    return resident_update_one(r, nullptr, d_matches, n, max_index, Tr, s);
}

int32_t svh_recon_update_batch(svh_recon* const* rs, const svh_p_match* const* m, const int32_t* n, const double* Tr,
                               int32_t K, int32_t point_type, int32_t min_track_length, double max_dist,
                               double min_angle, int32_t* status) {
    if (K < 0 || (K > 0 && (!rs || !m || !n || !Tr)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update_batch: bad arguments");
    bool one_device = true;
    const int32_t bad = check_batch(rs, K, "object", &one_device, [](int) { return true; });
    if (bad) return bad;
    if (!one_device) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update_batch: objects of different devices");
    for (int32_t i = 0; i < K; i++) {
        if (!rs[i]->resident)
            return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update_batch: a host-table object in the batch (svh_recon_create)");
        if (!rs[i]->calibrated)
            return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update_batch before svh_recon_set_calibration");
        if (m[i] && n[i] < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_update_batch: negative match count");
    }
    if (K > 0 && !have_device())
        return svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
    const double t_start = now_ms();
    ActiveCaller active;
    std::vector<ResidentUpdate> us;
    for (int32_t i = 0; i < K; i++) {
        if (status) status[i] = SVH_OK;
        if (!m[i]) continue;   // sits this update out
        int32_t max_index = 0;
        const int rc = scan_matches(m[i], n[i], &max_index);
        if (rc) {              // this object's own refusal: it sits out as well
            if (status) status[i] = rc;
            continue;
        }
        us.push_back(ResidentUpdate{rs[i], m[i], nullptr, n[i], max_index, Tr + 16 * (size_t)i, i});
    }
    const recon::Settings s = {point_type, min_track_length, max_dist, min_angle, 1.0, 0.0};   // (cp, sp: per object)
    return resident_run(us, s, status, t_start);
}

int32_t svh_recon_num_points(svh_recon* r) { return r ? r->n_points : 0; }

int32_t svh_recon_get_points(svh_recon* r, float* xyz, int32_t cap) {
    if (!r) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_get_points: null object");
    const int32_t n = std::min(r->n_points, cap);
    if (xyz && n > 0) {
        RECON_TRY(none, hipSetDevice(r->device));
        RECON_TRY(copy, hipMemcpyAsync(xyz, r->d_points, 12 * (size_t)n, hipMemcpyDeviceToHost, r->stream));
        RECON_TRY(none, (hipError_t)wait_stream(r->stream));
    }
    return r->n_points;
}

int32_t svh_recon_get_points_device(svh_recon* r, const float** xyz) {
    if (!r || !xyz) return svh::fail(SVH_ERR_BAD_ARG, "svh_recon_get_points_device: bad arguments");
    *xyz = r->d_points;   // valid until the next update (the array may move when it grows)
    return r->n_points;
}

int32_t svh_recon_num_tracks(svh_recon* r) {
    return !r ? 0 : (r->resident ? r->n_tracks : (int32_t)r->tracks.size());
}

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

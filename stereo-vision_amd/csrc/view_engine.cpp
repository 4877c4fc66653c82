// The map view behind the svh_view_* entries of include/svh_view.h: stereomapper's View3D (view3d.cpp) without Qt.
//
// Host (this file): the sequence of point lists in ONE growing device buffer (addPoints' list semantics, :174-254),
// the cameras (addCamera in double, :127-166), the matrices and the segment list of a render, playPoses' pose loop.
// Device (view_kernels.hip): the render; (view_thin_kernels.hip): the voxel-grid thinning, whose survivors go to a second
// store that changes places with the first after the last wait.  The object has its own stream; every entry returns when
// it is complete.
//
// Draw index of a point = 162 + its position in the store, so the store holds the lists back to back in sequence
// order and dropping the newest list is forgetting the tail.  A growth allocates the new store first and moves the
// content device to device, so a failed growth leaves the object as it was.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/svh_view.h"
#include "hip_guard.h"
#include "map_internal.h"
#include "svh_config.h"
#include "view_core.h"
#include "view_internal.h"
#include "view_thin_core.h"

using namespace svh;

namespace {

#define VIEW_TRY(kind, expr) SVH_HIP_TRY("View", kind, expr)
#define VIEW_GROW(buf, bytes) SVH_HIP_GROW("View", buf, bytes)

constexpr int32_t kMaxSide = 16384;
constexpr int64_t kMaxPoints = ((int64_t)1 << 31) - 4096;
constexpr int64_t kFirstCapacity = 4096;     // points
constexpr size_t kMaxCameras = (size_t)1 << 24;

bool side_ok(int32_t v) { return v >= 1 && v <= kMaxSide; }

}  // namespace

struct svh_view {
    int device = 0;
    hipStream_t stream = nullptr;
    int32_t W = 0, H = 0;
    view::Pose pose{};
    svh_view_flags flags{1, 1, 0};
    // the sequence of lists: lengths in sequence order; the store holds them back to back
    std::vector<int64_t> lens;
    int64_t total = 0;
    HipBuf<float4> store;
    std::vector<view::Cam> cams;
    // a render's buffers
    HipBuf<unsigned long long> key;
    HipBuf<uint32_t> ovl;
    HipBuf<view::Seg> d_segs;
    PinnedBuf<view::Seg> h_segs;
    HipBuf<uint8_t> d_rgb;
    PinnedBuf<uint8_t> h_rgb;
    PinnedBuf<float4> h_pts;     // host lists on their way to the store
    std::vector<view::Seg> segs;
    // a thinning's table and scratch (they grow, nothing is allocated per call) and the store the survivors go to
    HipBuf<unsigned long long> t_keys;
    HipBuf<uint32_t> t_win, t_slot;
    HipBuf<uint8_t> t_keep;
    HipBuf<int32_t> t_blk;
    HipBuf<int64_t> t_dev;       // the list boundaries, then ThinJob::out
    PinnedBuf<int64_t> t_host;   // the same layout
    HipBuf<float4> store2;

    int64_t capacity() const { return (int64_t)(store.cap / sizeof(float4)); }
};

namespace {

// room for `need` points, content kept
int reserve(svh_view* v, int64_t need) {
    if (need <= v->capacity()) return SVH_OK;
    int64_t cap = std::max(v->capacity(), kFirstCapacity);
    while (cap < need) cap *= 2;
    HipBuf<float4> bigger;
    VIEW_GROW(bigger, (size_t)cap * sizeof(float4));
    if (v->total > 0) {
        VIEW_TRY(copy, hipMemcpyAsync(bigger, v->store, (size_t)v->total * sizeof(float4), hipMemcpyDeviceToDevice, v->stream));
        VIEW_TRY(wait, hipStreamSynchronize(v->stream));
    }
    v->store = std::move(bigger);
    return SVH_OK;
}

// addPoints with arguments that have been checked: src[i] (host or device) holds n[i] points
int add_lists(svh_view* v, const float* const* src, const int64_t* n, int32_t lists, bool on_device) {
    const bool drop = lists > 1 && !v->lens.empty();
    const int32_t first = std::max(lists - 2, 0);
    const int64_t kept = v->total - (drop ? v->lens.back() : 0);
    int64_t added = 0;
    for (int32_t i = first; i < lists; i++) {
        if (n[i] > kMaxPoints) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_view_add_points: more than 2^31 - 4096 points");
        added += n[i];
    }
    if (kept + added > kMaxPoints) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_view_add_points: more than 2^31 - 4096 points");
    if (lists == 0) return SVH_OK;
    VIEW_TRY(none, hipSetDevice(v->device));
    int rc = reserve(v, kept + added);
    if (rc) return rc;
    if (!on_device && added > 0) VIEW_GROW(v->h_pts, (size_t)added * sizeof(float4));
    // from here on the dropped list's place is written to
    if (drop) {
        v->total = kept;
        v->lens.pop_back();
    }
    int64_t at = kept, staged = 0;
    for (int32_t i = first; i < lists; i++) {
        if (n[i] == 0) continue;
        const size_t bytes = (size_t)n[i] * sizeof(float4);
        if (on_device) {
            VIEW_TRY(copy, hipMemcpyAsync(v->store + at, src[i], bytes, hipMemcpyDeviceToDevice, v->stream));
        } else {
            memcpy(v->h_pts + staged, src[i], bytes);
            VIEW_TRY(copy, hipMemcpyAsync(v->store + at, v->h_pts + staged, bytes, hipMemcpyHostToDevice, v->stream));
            staged += n[i];
        }
        at += n[i];
    }
    VIEW_TRY(wait, hipStreamSynchronize(v->stream));
    for (int32_t i = first; i < lists; i++) v->lens.push_back(n[i]);
    v->total = at;
    return SVH_OK;
}

int render(svh_view* v, uint8_t* rgb, bool rgb_dev) {
    VIEW_TRY(none, hipSetDevice(v->device));
    const size_t npix = (size_t)v->W * (size_t)v->H;
    view::RenderJob j;
    view::make_frame(v->pose, v->W, v->H, &j.frame);
    view::build_segments(v->cams.data(), v->cams.size(), v->flags.show_grid != 0, v->flags.show_cams != 0, &v->segs);
    const size_t nseg = v->segs.size();
    VIEW_GROW(v->key, npix * 8);
    VIEW_GROW(v->ovl, npix * 4);
    VIEW_GROW(v->d_segs, std::max(nseg, (size_t)1) * sizeof(view::Seg));
    VIEW_GROW(v->h_segs, std::max(nseg, (size_t)1) * sizeof(view::Seg));
    if (!rgb_dev) {
        VIEW_GROW(v->d_rgb, npix * 3);
        VIEW_GROW(v->h_rgb, npix * 3);
    }
    hipStream_t s = v->stream;
    if (nseg > 0) {
        memcpy(v->h_segs, v->segs.data(), nseg * sizeof(view::Seg));
        VIEW_TRY(copy, hipMemcpyAsync(v->d_segs, v->h_segs, nseg * sizeof(view::Seg), hipMemcpyHostToDevice, s));
    }
    VIEW_TRY(copy, hipMemsetAsync(v->key, 0xFF, npix * 8, s));
    VIEW_TRY(copy, hipMemsetAsync(v->ovl, 0, npix * 4, s));
    j.pts = v->store;
    j.npts = (uint32_t)v->total;
    j.segs = v->d_segs;
    j.nseg = (uint32_t)nseg;
    j.anchor_index = v->flags.show_cams ? view::GRID_SEGS + (uint32_t)v->total : view::NO_ANCHOR;
    j.anchor[0] = -v->pose.tx, j.anchor[1] = -v->pose.ty, j.anchor[2] = -v->pose.tz;
    j.white = v->flags.white != 0;
    j.key = v->key;
    j.ovl = v->ovl;
    j.rgb = rgb_dev ? rgb : v->d_rgb.p;
    VIEW_TRY(launch, (view::launch_render(s, j), hipGetLastError()));
    if (!rgb_dev) VIEW_TRY(copy, hipMemcpyAsync(v->h_rgb, v->d_rgb, npix * 3, hipMemcpyDeviceToHost, s));
    VIEW_TRY(wait, hipStreamSynchronize(s));
    if (!rgb_dev) memcpy(rgb, v->h_rgb, npix * 3);
    return SVH_OK;
}

// svh_view_thin with arguments that have been checked and a store that is not empty
int thin_store(svh_view* v, float voxel, svh_view_thin_stats* st) {
    VIEW_TRY(none, hipSetDevice(v->device));
    const int64_t n = v->total, room = v->capacity();
    const size_t nl = v->lens.size(), nbounds = nl + 1, words = nbounds + 2 + nbounds;
    const uint64_t cap = thin::capacity_for(n);
    // every allocation before anything is written; the scratch follows the store's capacity, so it grows when that does
    VIEW_GROW(v->t_keys, (size_t)cap * 8);
    VIEW_GROW(v->t_win, (size_t)cap * 4);
    VIEW_GROW(v->t_slot, (size_t)room * 4);
    VIEW_GROW(v->t_keep, (size_t)room);
    VIEW_GROW(v->t_blk, (size_t)((room + view::THIN_BLOCK - 1) / view::THIN_BLOCK) * 4);
    VIEW_GROW(v->t_dev, words * 8);
    VIEW_GROW(v->t_host, words * 8);
    VIEW_GROW(v->store2, v->store.cap);
    hipStream_t s = v->stream;
    int64_t* const hb = v->t_host;
    hb[0] = 0;
    for (size_t k = 0; k < nl; k++) hb[k + 1] = hb[k] + v->lens[k];
    VIEW_TRY(copy, hipMemsetAsync(v->t_keys, 0xFF, (size_t)cap * 8, s));
    VIEW_TRY(copy, hipMemsetAsync(v->t_win, 0xFF, (size_t)cap * 4, s));
    VIEW_TRY(copy, hipMemsetAsync(v->t_dev + nbounds, 0, (2 + nbounds) * 8, s));
    VIEW_TRY(copy, hipMemcpyAsync(v->t_dev, hb, nbounds * 8, hipMemcpyHostToDevice, s));
    view::ThinJob j;
    j.pts = v->store;
    j.n = (uint32_t)n;
    j.voxel = voxel;
    j.keys = v->t_keys;
    j.win = v->t_win;
    j.capacity = cap;
    j.slot = v->t_slot;
    j.keep = v->t_keep;
    j.blockcnt = v->t_blk;
    j.bounds = v->t_dev;
    j.nbounds = (int32_t)nbounds;
    j.out = v->t_dev + nbounds;
    j.dst = v->store2;
    VIEW_TRY(launch, (view::launch_thin(s, j), hipGetLastError()));
    VIEW_TRY(copy, hipMemcpyAsync(hb + nbounds, j.out, (2 + nbounds) * 8, hipMemcpyDeviceToHost, s));
    VIEW_TRY(wait, hipStreamSynchronize(s));
    // from here on nothing can fail: the survivors become the store
    const int64_t* out = hb + nbounds;
    std::swap(v->store, v->store2);
    for (size_t k = 0; k < nl; k++) v->lens[k] = out[2 + k + 1] - out[2 + k];
    v->total = out[0];
    if (st) st->before = n, st->after = out[0], st->unplaced = out[1];
    return SVH_OK;
}

// the place of a list in the store (list -1: all of it); false for an index out of range
bool list_range(const svh_view* v, int32_t list, int64_t* at, int64_t* n) {
    if (list == -1) return *at = 0, *n = v->total, true;
    if (list < 0 || (size_t)list >= v->lens.size()) return false;
    int64_t a = 0;
    for (int32_t i = 0; i < list; i++) a += v->lens[i];
    return *at = a, *n = v->lens[list], true;
}

int get_points(svh_view* v, int64_t at, int64_t n, float* xyzv, bool on_device) {
    VIEW_TRY(none, hipSetDevice(v->device));
    VIEW_TRY(copy, hipMemcpyAsync(xyzv, v->store + at, (size_t)n * sizeof(float4), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, v->stream));
    VIEW_TRY(wait, hipStreamSynchronize(v->stream));
    return SVH_OK;
}

// nothing of a failed call is in flight when the caller goes on
int drained(svh_view* v, int rc) {
    if (rc == SVH_ERR_HIP && v->stream) {
        (void)hipSetDevice(v->device);
        (void)hipStreamSynchronize(v->stream);
    }
    return rc;
}

view::Pose to_pose(const svh_view_pose& p) { return view::Pose{p.zoom, p.rotx, p.roty, p.tx, p.ty, p.tz}; }

}  // namespace

svh::view::StoreRef svh::view::store_of(const svh_view* v) { return StoreRef{v->store.p, v->total, v->device, v->stream}; }

bool svh::view::list_range(const svh_view* v, int32_t first, int32_t n_lists, int64_t* at, int64_t* n) {
    if (first < 0 || n_lists < 0 || (int64_t)first + n_lists > (int64_t)v->lens.size()) return false;
    int64_t before = 0, in = 0;
    for (int32_t i = 0; i < first; i++) before += v->lens[(size_t)i];
    for (int32_t i = first; i < first + n_lists; i++) in += v->lens[(size_t)i];
    *at = before, *n = in;
    return true;
}

extern "C" {

void svh_view_pose_default(svh_view_pose* p) {
    if (!p) return;
    p->zoom = -1.5f, p->rotx = 180.f, p->roty = 0.f, p->tx = 0.f, p->ty = 0.f, p->tz = -1.5f;
}

svh_view* svh_view_create(int32_t width, int32_t height) {
    svh::ensure_init();
    if (!side_ok(width) || !side_ok(height)) {
        svh::fail(SVH_ERR_BAD_ARG, "svh_view_create: width and height must be 1..16384");
        return nullptr;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
        return nullptr;
    }
    svh_view* v = new svh_view();
    v->W = width, v->H = height;
    svh_view_pose p;
    svh_view_pose_default(&p);
    v->pose = to_pose(p);
    (void)hipGetDevice(&v->device);
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) {
        delete v;
        svh::fail(SVH_ERR_HIP, "svh_view_create: hipStreamCreateWithFlags failed");
        return nullptr;
    }
    return v;
}

void svh_view_destroy(svh_view* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    const hipStream_t s = v->stream;
    if (s) (void)hipStreamSynchronize(s);
    delete v;   // the buffers free themselves, on the device selected above
    if (s) (void)hipStreamDestroy(s);
}

void svh_view_clear(svh_view* v) {
    if (!v) return;
    v->lens.clear();
    v->total = 0;
    v->cams.clear();
}

int32_t svh_view_resize(svh_view* v, int32_t width, int32_t height) {
    if (!v || !side_ok(width) || !side_ok(height)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_resize: bad arguments");
    v->W = width, v->H = height;
    return SVH_OK;
}

int32_t svh_view_set_pose(svh_view* v, const svh_view_pose* p) {
    if (!v || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_set_pose: null argument");
    v->pose = to_pose(*p);
    return SVH_OK;
}

int32_t svh_view_set_flags(svh_view* v, const svh_view_flags* f) {
    if (!v || !f) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_set_flags: null argument");
    v->flags = *f;
    return SVH_OK;
}

int32_t svh_view_add_points(svh_view* v, const float* const* xyzv, const int64_t* n, int32_t lists, int32_t on_device) {
    if (!v || lists < 0 || (lists > 0 && (!xyzv || !n))) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_add_points: bad arguments");
    for (int32_t i = 0; i < lists; i++)
        if (n[i] < 0 || (n[i] > 0 && !xyzv[i])) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_add_points: bad list");
    return drained(v, add_lists(v, xyzv, n, lists, on_device != 0));
}

int32_t svh_view_add_map(svh_view* v, svh_map* m) {
    if (!v || !m) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_add_map: null argument");
    if (!m->have_prev) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_add_map: the map has no frame yet");
    if (m->device != v->device) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_add_map: the map lives on another device");
    const float* src[2] = {(const float*)m->b.pts[0].p, (const float*)m->b.pts[1].p};
    const int64_t n[2] = {m->npts[0], m->npts[1]};
    if (m->last_fused) return drained(v, add_lists(v, src, n, 2, true));
    return drained(v, add_lists(v, src + 1, n + 1, 1, true));
}

int32_t svh_view_add_camera(svh_view* v, const double* H_total, float s, int32_t keyframe) {
    if (!v || !H_total) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_add_camera: null argument");
    if (v->cams.size() >= kMaxCameras) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_view_add_camera: more than 2^24 cameras");
    view::Cam c;
    view::make_camera(H_total, s, keyframe, &c);
    v->cams.push_back(c);
    return SVH_OK;
}

int64_t svh_view_count(svh_view* v, int32_t what) {
    if (!v) return 0;
    switch (what) {
    case 0: return (int64_t)v->lens.size();
    case 1: return v->total;
    case 2: return (int64_t)v->cams.size();
    case 3: return v->capacity();
    default: return 0;
    }
}

int32_t svh_view_thin(svh_view* v, float voxel, svh_view_thin_stats* stats) {
    if (!v || !(voxel > 0.f) || !thin::finite_f(voxel)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_thin: a view and a finite voxel size > 0 are needed");
    if (v->total == 0) {
        if (stats) stats->before = stats->after = stats->unplaced = 0;
        return SVH_OK;
    }
    return drained(v, thin_store(v, voxel, stats));
}

int64_t svh_view_list_len(svh_view* v, int32_t list) {
    int64_t at, n;
    if (!v || list < 0 || !list_range(v, list, &at, &n)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_list_len: no such list");
    return n;
}

int64_t svh_view_get_points(svh_view* v, int32_t list, float* xyzv, int64_t cap, int32_t on_device) {
    int64_t at, n;
    if (!v || cap < 0 || (cap > 0 && !xyzv)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_get_points: bad arguments");
    if (!list_range(v, list, &at, &n)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_get_points: no such list");
    const int64_t m = std::min(n, cap);
    if (m > 0) {
        const int rc = drained(v, get_points(v, at, m, xyzv, on_device != 0));
        if (rc) return rc;
    }
    return n;
}

int32_t svh_test_thin_keys(const float* xyzv, int64_t n, float voxel, uint64_t* key, uint32_t* home, uint64_t* capacity) {
    if (n < 0 || (n > 0 && !xyzv) || !(voxel > 0.f) || !thin::finite_f(voxel)) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_thin_keys: bad arguments");
    const uint64_t cap = thin::capacity_for(n);
    if (capacity) *capacity = cap;
    for (int64_t i = 0; i < n; i++) {
        const uint64_t k = thin::key_of(xyzv[4 * i], xyzv[4 * i + 1], xyzv[4 * i + 2], voxel);
        if (key) key[i] = k;
        if (home) home[i] = k == thin::EMPTY_KEY ? thin::NO_HOME : thin::home_of(k, cap);
    }
    return SVH_OK;
}

int32_t svh_view_render(svh_view* v, uint8_t* rgb, int32_t rgb_on_device) {
    if (!v || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_render: null argument");
    return drained(v, render(v, rgb, rgb_on_device != 0));
}

int64_t svh_view_play_sequence(const svh_view_pose* poses, int32_t n, svh_view_pose* out, int64_t cap) {
    if (n < 0 || cap < 0 || (n > 0 && !poses) || (cap > 0 && !out)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_play_sequence: bad arguments");
    std::vector<view::Pose> in((size_t)n), seq;
    for (int32_t i = 0; i < n; i++) in[i] = to_pose(poses[i]);
    view::play_sequence(in.data(), n, &seq);
    for (size_t k = 0; k < seq.size() && (int64_t)k < cap; k++) {
        const view::Pose& q = seq[k];
        out[k] = svh_view_pose{q.zoom, q.rotx, q.roty, q.tx, q.ty, q.tz};
    }
    return (int64_t)seq.size();
}

int64_t svh_view_play_poses(svh_view* v, const svh_view_pose* poses, int32_t n, uint8_t* rgb, int64_t cap, int32_t rgb_on_device) {
    if (!v || n < 0 || cap < 0 || (n > 0 && !poses) || (cap > 0 && !rgb)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view_play_poses: bad arguments");
    std::vector<view::Pose> in((size_t)n), seq;
    for (int32_t i = 0; i < n; i++) in[i] = to_pose(poses[i]);
    view::play_sequence(in.data(), n, &seq);
    const size_t bytes = (size_t)v->W * (size_t)v->H * 3;
    const bool dev = rgb_on_device != 0;
    HipBuf<uint8_t> sink;   // frames beyond cap are rendered, as updateGL() does, and not kept
    for (size_t k = 0; k < seq.size(); k++) {
        v->pose = seq[k];
        int rc;
        if ((int64_t)k < cap) {
            rc = render(v, rgb + k * bytes, dev);
        } else {
            rc = [&]() -> int {
                VIEW_TRY(none, hipSetDevice(v->device));
                VIEW_GROW(sink, bytes);
                return render(v, sink, true);
            }();
        }
        if (rc) return drained(v, rc);
    }
    return (int64_t)seq.size();
}

}  // extern "C"

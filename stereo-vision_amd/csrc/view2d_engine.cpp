// The 2-D panes behind the svh_view2d_* entries of include/svh_view2d.h: stereomapper's View2D (view2d.cpp) without Qt.
//
// Host (this file): what the object holds -- the texels of one image and one list of matches with their inlier flags,
// both in device memory -- and the order of the copies.  Device (view2d_kernels.hip): the conversion of a source into
// texels and the render.  The object has its own stream; every entry returns when it is complete.
//
// An image and a match list are each kept twice: a call fills the set that is NOT shown and makes it the shown one
// only when everything has succeeded, so a failed call leaves the object as it was.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/svh_view2d.h"
#include "hip_guard.h"
#include "svh_config.h"
#include "view2d_core.h"
#include "view2d_internal.h"

using namespace svh;

static_assert(sizeof(view2d::Match) == sizeof(svh_p_match), "view2d::Match is svh_p_match");

namespace {

#define V2_TRY(kind, expr) SVH_HIP_TRY("View2D", kind, expr)
#define V2_GROW(buf, bytes) SVH_HIP_GROW("View2D", buf, bytes)

constexpr int32_t kMaxSide = 16384;

bool side_ok(int32_t v) { return v >= 1 && v <= kMaxSide; }

struct Texels {
    HipBuf<uint8_t> px;
    int32_t w = 1, h = 1, ch = 0;   // View2D starts with a 1 x 1 image: nothing is drawn
    uint32_t pitch = 0;
};

struct MatchList {
    HipBuf<view2d::Match> m;
    HipBuf<uint8_t> inlier;
};

}  // namespace

struct svh_view2d {
    int device = 0;
    hipStream_t stream = nullptr;
    int32_t W = 0, H = 0;
    Texels tex[2];
    int shown = 0;
    MatchList matches[2];
    int listed = 0;
    int32_t n = 0, left = 1;
    // a source or a match list on its way from the host
    PinnedBuf<uint8_t> h_src;
    HipBuf<uint8_t> d_src;
    // a render's buffers
    HipBuf<uint32_t> ovl;
    HipBuf<uint8_t> d_rgb;
    PinnedBuf<uint8_t> h_rgb;
};

namespace {

// glTexImage2D: the source (checked) into the set of texels that is not shown, then that set is shown
int set_texels(svh_view2d* v, int32_t kind, const void* src, int32_t w, int32_t h, uint32_t src_pitch, bool on_device) {
    V2_TRY(none, hipSetDevice(v->device));
    Texels& next = v->tex[v->shown ^ 1];
    const size_t n = (size_t)w * (size_t)h;
    const bool grey = kind == view2d::SRC_GREY;
    const uint32_t dst_pitch = grey ? (uint32_t)up16((size_t)w) : 3u * (uint32_t)w;
    V2_GROW(next.px, grey ? (size_t)dst_pitch * (size_t)h : (n + 3) / 4 * 12);
    hipStream_t s = v->stream;
    const void* dsrc = src;
    if (!on_device) {
        const size_t row = grey ? (size_t)w : (kind == view2d::SRC_RGB_F32 ? 12 : 4) * (size_t)w;
        V2_GROW(v->h_src, row * (size_t)h);
        V2_GROW(v->d_src, row * (size_t)h);
        const size_t from = grey ? (size_t)src_pitch : row;
        for (int32_t y = 0; y < h; y++) memcpy(v->h_src + (size_t)y * row, (const uint8_t*)src + (size_t)y * from, row);
        V2_TRY(copy, hipMemcpyAsync(v->d_src, v->h_src, row * (size_t)h, hipMemcpyHostToDevice, s));
        dsrc = v->d_src;
        src_pitch = (uint32_t)w;
    }
    const view2d::TexelJob j{kind, dsrc, w, h, src_pitch, dst_pitch, next.px.p};
    V2_TRY(launch, (view2d::launch_texels(s, j), hipGetLastError()));
    V2_TRY(wait, hipStreamSynchronize(s));
    next.w = w, next.h = h, next.ch = grey ? 1 : 3, next.pitch = dst_pitch;
    v->shown ^= 1;
    return SVH_OK;
}

// setMatches with arguments that have been checked, n > 0
int set_matches(svh_view2d* v, const svh_p_match* m, int32_t n, const uint8_t* inlier, int32_t left, bool on_device) {
    V2_TRY(none, hipSetDevice(v->device));
    MatchList& next = v->matches[v->listed ^ 1];
    const size_t mb = (size_t)n * sizeof(svh_p_match);
    V2_GROW(next.m, mb);
    V2_GROW(next.inlier, (size_t)n);
    hipStream_t s = v->stream;
    if (on_device) {
        V2_TRY(copy, hipMemcpyAsync(next.m, m, mb, hipMemcpyDeviceToDevice, s));
        V2_TRY(copy, hipMemcpyAsync(next.inlier, inlier, (size_t)n, hipMemcpyDeviceToDevice, s));
    } else {
        V2_GROW(v->h_src, mb + (size_t)n);
        memcpy(v->h_src, m, mb);
        memcpy(v->h_src + mb, inlier, (size_t)n);
        V2_TRY(copy, hipMemcpyAsync(next.m, v->h_src, mb, hipMemcpyHostToDevice, s));
        V2_TRY(copy, hipMemcpyAsync(next.inlier, v->h_src + mb, (size_t)n, hipMemcpyHostToDevice, s));
    }
    V2_TRY(wait, hipStreamSynchronize(s));
    v->listed ^= 1;
    v->n = n, v->left = left != 0;
    return SVH_OK;
}

int render(svh_view2d* v, uint8_t* rgb, bool rgb_dev) {
    V2_TRY(none, hipSetDevice(v->device));
    const size_t npix = (size_t)v->W * (size_t)v->H;
    if (v->n > 0) V2_GROW(v->ovl, (npix + 3) / 4 * 16);
    if (!rgb_dev) {
        V2_GROW(v->d_rgb, npix * 3);
        V2_GROW(v->h_rgb, npix * 3);
    }
    hipStream_t s = v->stream;
    const Texels& t = v->tex[v->shown];
    const MatchList& l = v->matches[v->listed];
    if (v->n > 0) V2_TRY(copy, hipMemsetAsync(v->ovl, 0, npix * 4, s));
    view2d::RenderJob j;
    j.pane = view2d::Pane{v->W, v->H, t.w, t.h, t.ch, t.pitch};
    j.tex = t.px;
    j.matches = l.m;
    j.inlier = l.inlier;
    j.n = v->n, j.left = v->left;
    j.ovl = v->ovl;
    j.rgb = rgb_dev ? rgb : v->d_rgb.p;
    V2_TRY(launch, (view2d::launch_render(s, j), hipGetLastError()));
    if (!rgb_dev) V2_TRY(copy, hipMemcpyAsync(v->h_rgb, v->d_rgb, npix * 3, hipMemcpyDeviceToHost, s));
    V2_TRY(wait, hipStreamSynchronize(s));
    if (!rgb_dev) memcpy(rgb, v->h_rgb, npix * 3);
    return SVH_OK;
}

// nothing of a failed call is in flight when the caller goes on
int drained(svh_view2d* v, int rc) {
    if (rc == SVH_ERR_HIP && v->stream) {
        (void)hipSetDevice(v->device);
        (void)hipStreamSynchronize(v->stream);
    }
    return rc;
}

}  // namespace

extern "C" {

svh_view2d* svh_view2d_create(int32_t width, int32_t height) {
    svh::ensure_init();
    if (!side_ok(width) || !side_ok(height)) {
        svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_create: width and height must be 1..16384");
        return nullptr;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
        return nullptr;
    }
    svh_view2d* v = new svh_view2d();
    v->W = width, v->H = height;
    (void)hipGetDevice(&v->device);
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) {
        delete v;
        svh::fail(SVH_ERR_HIP, "svh_view2d_create: hipStreamCreateWithFlags failed");
        return nullptr;
    }
    return v;
}

void svh_view2d_destroy(svh_view2d* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    const hipStream_t s = v->stream;
    if (s) (void)hipStreamSynchronize(s);
    delete v;   // the buffers free themselves, on the device selected above
    if (s) (void)hipStreamDestroy(s);
}

int32_t svh_view2d_resize(svh_view2d* v, int32_t width, int32_t height) {
    if (!v || !side_ok(width) || !side_ok(height)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_resize: bad arguments");
    v->W = width, v->H = height;
    return SVH_OK;
}

int32_t svh_view2d_set_image(svh_view2d* v, const uint8_t* I, const int32_t* dims, int32_t on_device) {
    if (!v || !I || !dims || !side_ok(dims[0]) || !side_ok(dims[1]) || dims[2] < dims[0])
        return svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_set_image: bad arguments");
    const int rc = drained(v, set_texels(v, view2d::SRC_GREY, I, dims[0], dims[1], (uint32_t)dims[2], on_device != 0));
    if (rc == SVH_OK) v->n = 0;   // setImage: clearMatches()
    return rc;
}

int32_t svh_view2d_set_color_image(svh_view2d* v, const float* rgb, int32_t w, int32_t h, int32_t on_device) {
    if (!v || !rgb || !side_ok(w) || !side_ok(h)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_set_color_image: bad arguments");
    return drained(v, set_texels(v, view2d::SRC_RGB_F32, rgb, w, h, 0, on_device != 0));
}

int32_t svh_view2d_set_disparity(svh_view2d* v, const float* D, int32_t w, int32_t h, int32_t on_device) {
    if (!v || !D || !side_ok(w) || !side_ok(h)) return svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_set_disparity: bad arguments");
    return drained(v, set_texels(v, view2d::SRC_DISPARITY, D, w, h, 0, on_device != 0));
}

int32_t svh_view2d_set_matches(svh_view2d* v, const svh_p_match* m, int32_t n, const uint8_t* inlier, int32_t left,
                               int32_t on_device) {
    if (!v || n < 0 || (n > 0 && (!m || !inlier))) return svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_set_matches: bad arguments");
    if (n == 0) {
        v->n = 0, v->left = left != 0;
        return SVH_OK;
    }
    return drained(v, set_matches(v, m, n, inlier, left, on_device != 0));
}

int32_t svh_view2d_set_matches_indexed(svh_view2d* v, const svh_p_match* m, int32_t n, const int32_t* inlier_idx,
                                       int32_t n_inliers, int32_t left) {
    if (!v || n < 0 || n_inliers < 0 || (n > 0 && !m) || (n_inliers > 0 && !inlier_idx))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_set_matches_indexed: bad arguments");
    for (int32_t k = 0; k < n_inliers; k++)
        if (inlier_idx[k] < 0 || inlier_idx[k] >= n)
            return svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_set_matches_indexed: inlier index outside the match list");
    if (n == 0) {
        v->n = 0, v->left = left != 0;
        return SVH_OK;
    }
    std::vector<uint8_t> flags((size_t)n, 0);
    for (int32_t k = 0; k < n_inliers; k++) flags[(size_t)inlier_idx[k]] = 1;
    return drained(v, set_matches(v, m, n, flags.data(), left, false));
}

void svh_view2d_clear_matches(svh_view2d* v) {
    if (v) v->n = 0;
}

int32_t svh_view2d_render(svh_view2d* v, uint8_t* rgb, int32_t rgb_on_device) {
    if (!v || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_view2d_render: null argument");
    return drained(v, render(v, rgb, rgb_on_device != 0));
}

}  // extern "C"

// The rectification in front of the stereo pipeline (stereomapper/framecapturethread.cpp:100-131, 328-349) behind the
// svh_rectify_* entries of include/svh_rectify.h.
//
// Host (this file): the parameters, the inverse of P R per camera (create fails on a singular one), the maps of an
// object that has no device to ask, and the staging of host images.  Device (rectify_kernels.hip): k_rect_maps once per
// object, k_rect_remap per call.  Every object has its own stream; nothing synchronises the default stream.
//
// A compute call is a transaction.  Everything that can fail before the remap kernel -- the object's stream and events,
// its buffers, the maps, the upload of a host source -- comes first, and the launch with its check is ONE guarded
// expression, so a failure up to and including the launch check leaves a device destination untouched.  A host
// destination is written from the pinned copy after the final wait, so it is untouched after any failure.  The object
// itself changes only by what the next call would redo: its maps count as built once the call that built them has waited.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../include/svh_rectify.h"
#include "batch_rec.h"
#include "hip_guard.h"
#include "rectify_internal.h"
#include "svh_config.h"
#include "vo_internal.h"

using namespace svh;

namespace {

#define RECT_TRY(kind, expr) SVH_HIP_TRY("Rectify", kind, expr)
#define RECT_GROW(buf, bytes) SVH_HIP_GROW("Rectify", buf, bytes)

bool have_device() {
    int nd = 0;
    return hipGetDeviceCount(&nd) == hipSuccess && nd > 0;
}

int no_device() { return svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback"); }

}  // namespace

struct svh_rectify {
    svh_rectify_params prm;
    rect::Cam cam[2];
    int device = 0;
    bool timing = false;
    double ms[2] = {0, 0};
    // device side
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool maps_ready = false;
    HipBuf<float> d_maps;      // [cameras][2][dh * dw]: mx, my
    HipBuf<int32_t> d_tab;     // [cameras][dh * dw][2]: sx, sy
    HipBuf<uint8_t> d_src, d_dst;       // a host image on its way to / from the device
    PinnedBuf<uint8_t> h_src, h_dst;
    size_t pixels() const { return (size_t)prm.dst_width * (size_t)prm.dst_height; }
};

namespace {

bool side_ok(int32_t v) { return v >= 1 && v <= SVH_RECTIFY_MAX_SIDE; }

// bytes an image of h rows of w bytes spans at this row stride
size_t span(int32_t w, int32_t h, int32_t stride) { return (size_t)(h - 1) * (size_t)stride + (size_t)w; }

// stream, events, maps and table: what every compute call needs first
int ensure(svh_rectify* r, bool* built) {
    RECT_TRY(none, hipSetDevice(r->device));
    if (!r->stream) {
        hipStream_t s = nullptr;
        RECT_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        r->stream = s;
    }
    for (int i = 0; i < 4; i++)
        if (!r->ev[i]) RECT_TRY(none, hipEventCreate(&r->ev[i]));
    const size_t px = r->pixels(), nc = (size_t)r->prm.cameras;
    if (r->d_maps.cap < 8 * px * nc || r->d_tab.cap < 8 * px * nc) r->maps_ready = false;
    RECT_GROW(r->d_maps, 8 * px * nc);
    RECT_GROW(r->d_tab, 8 * px * nc);
    *built = false;
    if (!r->maps_ready) {
        if (r->timing) (void)hipEventRecord(r->ev[2], r->stream);
        for (size_t c = 0; c < nc; c++)
            RECT_TRY(launch, (rectlaunch_maps(r->stream, r->cam[c], r->prm.src_width, r->prm.src_height, r->prm.dst_width,
                                              r->prm.dst_height, r->prm.border, r->d_maps + 2 * px * c,
                                              r->d_maps + 2 * px * c + px, r->d_tab + 2 * px * c),
                              hipGetLastError()));
        if (r->timing) (void)hipEventRecord(r->ev[3], r->stream);
        *built = true;   // ready once the caller has waited for the stream
    }
    return SVH_OK;
}

// the wait that ends a call; the maps count as built after it
int finish(svh_rectify* r, bool built, bool timed) {
    RECT_TRY(wait, (hipError_t)wait_stream(r->stream));
    if (built) r->maps_ready = true;
    if (r->timing) {
        float a = 0, b = 0;
        r->ms[0] = timed && hipEventElapsedTime(&a, r->ev[0], r->ev[1]) == hipSuccess ? a : 0;
        r->ms[1] = built && hipEventElapsedTime(&b, r->ev[2], r->ev[3]) == hipSuccess ? b : 0;
    }
    return SVH_OK;
}

int remap_one(svh_rectify* r, int32_t cam, const uint8_t* src, bool src_dev, int32_t src_stride, uint8_t* dst,
              bool dst_dev, int32_t dst_stride) {
    const svh_rectify_params& p = r->prm;
    ActiveCaller active;
    bool built = false;
    int rc = ensure(r, &built);
    if (rc) return rc;
    const size_t src_bytes = span(p.src_width, p.src_height, src_stride);
    const size_t dst_bytes = span(p.dst_width, p.dst_height, dst_stride);
    if (!src_dev) {
        RECT_GROW(r->d_src, src_bytes);
        RECT_GROW(r->h_src, src_bytes);
    }
    if (!dst_dev) {
        RECT_GROW(r->d_dst, dst_bytes);
        RECT_GROW(r->h_dst, dst_bytes);
    }
    const size_t px = r->pixels();
    RectRemap a;
    a.src[0] = a.src[1] = src_dev ? src : r->d_src.p;
    a.dst[0] = a.dst[1] = dst_dev ? dst : r->d_dst.p;
    a.tab[0] = a.tab[1] = r->d_tab + 2 * px * (size_t)cam;
    a.src_image_stride = a.dst_image_stride = 0;
    a.src_row_stride = src_stride;
    a.dst_row_stride = dst_stride;
    a.sw = p.src_width, a.sh = p.src_height, a.dw = p.dst_width, a.dh = p.dst_height;
    a.ncam = 1, a.images = 1, a.border = p.border;
    if (r->timing) (void)hipEventRecord(r->ev[0], r->stream);
    if (!src_dev) {
        memcpy(r->h_src, src, src_bytes);
        RECT_TRY(copy, hipMemcpyAsync(r->d_src, r->h_src, src_bytes, hipMemcpyHostToDevice, r->stream));
    }
    RECT_TRY(launch, (rectlaunch_remap(r->stream, a), hipGetLastError()));
    if (!dst_dev) RECT_TRY(copy, hipMemcpyAsync(r->h_dst, r->d_dst, dst_bytes, hipMemcpyDeviceToHost, r->stream));
    if (r->timing) (void)hipEventRecord(r->ev[1], r->stream);
    rc = finish(r, built, true);
    if (rc) return rc;
    if (!dst_dev)   // only the pixels: what lies between the rows of the caller's image stays
        for (int32_t y = 0; y < p.dst_height; y++)
            memcpy(dst + (size_t)y * (size_t)dst_stride, r->h_dst + (size_t)y * (size_t)dst_stride, (size_t)p.dst_width);
    return SVH_OK;
}

int remap_pairs(svh_rectify* r, int32_t n, const uint8_t* dS1, const uint8_t* dS2, int32_t src_stride,
                size_t src_image_stride, uint8_t* dI1, uint8_t* dI2, int32_t dst_stride, size_t dst_image_stride) {
    const svh_rectify_params& p = r->prm;
    ActiveCaller active;
    bool built = false;
    int rc = ensure(r, &built);
    if (rc) return rc;
    const size_t px = r->pixels();
    RectRemap a;
    a.src[0] = dS1, a.src[1] = dS2;
    a.dst[0] = dI1, a.dst[1] = dI2;
    a.tab[0] = r->d_tab;
    a.tab[1] = r->d_tab + 2 * px;
    a.src_image_stride = src_image_stride;
    a.dst_image_stride = dst_image_stride;
    a.src_row_stride = src_stride;
    a.dst_row_stride = dst_stride;
    a.sw = p.src_width, a.sh = p.src_height, a.dw = p.dst_width, a.dh = p.dst_height;
    a.ncam = 2, a.images = 2 * n, a.border = p.border;
    if (r->timing) (void)hipEventRecord(r->ev[0], r->stream);
    RECT_TRY(launch, (rectlaunch_remap(r->stream, a), hipGetLastError()));
    if (r->timing) (void)hipEventRecord(r->ev[1], r->stream);
    return finish(r, built, true);
}

// nothing of a failed call is in flight when the caller goes on
int drained(svh_rectify* r, int rc) {
    if (rc == SVH_ERR_HIP && r->stream) {
        (void)hipSetDevice(r->device);
        (void)hipStreamSynchronize(r->stream);
    }
    return rc;
}

}  // namespace

extern "C" {

void svh_rectify_params_default(svh_rectify_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->border = SVH_RECTIFY_WRAP;
    p->cameras = 2;
    for (int c = 0; c < 2; c++) {
        svh_rectify_camera& k = p->cam[c];
        k.K[0] = k.K[4] = k.K[8] = 1.0;
        k.R[0] = k.R[4] = k.R[8] = 1.0;
        k.P[0] = k.P[5] = k.P[10] = 1.0;
    }
}

int32_t svh_rectify_from_kitti(const svh_kitti_calib* calib, int32_t cam_left, int32_t cam_right, int32_t border,
                               svh_rectify_params* out) {
    if (!calib || !out || cam_left < 0 || cam_left >= SVH_KITTI_CAMERAS || cam_right < -1 ||
        cam_right >= SVH_KITTI_CAMERAS || (border != SVH_RECTIFY_WRAP && border != SVH_RECTIFY_ZERO))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_from_kitti: bad arguments");
    const int32_t cams[2] = {cam_left, cam_right};
    const int32_t nc = cam_right < 0 ? 1 : 2;
    auto whole = [](double v, int32_t* o) {
        if (!(v >= 1.0 && v <= (double)SVH_RECTIFY_MAX_SIDE) || v != floor(v)) return false;
        *o = (int32_t)v;
        return true;
    };
    svh_rectify_params p;
    svh_rectify_params_default(&p);
    p.border = border;
    p.cameras = nc;
    for (int32_t c = 0; c < nc; c++) {
        const int32_t k = cams[c];
        int32_t sz[4];
        if (!whole(calib->S[k][0], &sz[0]) || !whole(calib->S[k][1], &sz[1]) || !whole(calib->S_rect[k][0], &sz[2]) ||
            !whole(calib->S_rect[k][1], &sz[3]))
            return svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_from_kitti: S / S_rect is not an image size");
        if (c == 0) {
            p.src_width = sz[0], p.src_height = sz[1], p.dst_width = sz[2], p.dst_height = sz[3];
        } else if (p.src_width != sz[0] || p.src_height != sz[1] || p.dst_width != sz[2] || p.dst_height != sz[3]) {
            return svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_from_kitti: the two cameras differ in size");
        }
        memcpy(p.cam[c].K, calib->K[k], sizeof(p.cam[c].K));
        memcpy(p.cam[c].D, calib->D[k], sizeof(p.cam[c].D));
        memcpy(p.cam[c].R, calib->R_rect[k], sizeof(p.cam[c].R));
        memcpy(p.cam[c].P, calib->P_rect[k], sizeof(p.cam[c].P));
    }
    *out = p;
    return SVH_OK;
}

svh_rectify* svh_rectify_create(const svh_rectify_params* prm) {
    svh::ensure_init();
    if (!prm || !side_ok(prm->src_width) || !side_ok(prm->src_height) || !side_ok(prm->dst_width) ||
        !side_ok(prm->dst_height) || (prm->cameras != 1 && prm->cameras != 2) ||
        (prm->border != SVH_RECTIFY_WRAP && prm->border != SVH_RECTIFY_ZERO)) {
        svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_create: bad sizes, camera count or border mode");
        return nullptr;
    }
    rect::Cam cam[2];
    for (int32_t c = 0; c < prm->cameras; c++)
        if (!rect::make_cam(prm->cam[c].K, prm->cam[c].D, prm->cam[c].R, prm->cam[c].P, &cam[c])) {
            svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_create: P[:3,:3] R of camera " + std::to_string(c) + " is singular");
            return nullptr;
        }
    svh_rectify* r = new svh_rectify();
    r->prm = *prm;
    for (int32_t c = 0; c < prm->cameras; c++) r->cam[c] = cam[c];
    if (have_device()) (void)hipGetDevice(&r->device);
    return r;
}

void svh_rectify_destroy(svh_rectify* r) {
    if (!r) return;
    if (r->stream) {
        (void)hipSetDevice(r->device);
        (void)hipStreamSynchronize(r->stream);
        (void)hipStreamDestroy(r->stream);
    }
    for (int i = 0; i < 4; i++)
        if (r->ev[i]) (void)hipEventDestroy(r->ev[i]);
    delete r;
}

int64_t svh_rectify_release(svh_rectify* r) {
    if (!r) return 0;
    const int64_t bytes = (int64_t)(r->d_maps.cap + r->d_tab.cap + r->d_src.cap + r->d_dst.cap + r->h_src.cap + r->h_dst.cap);
    if (r->stream) {
        (void)hipSetDevice(r->device);
        (void)hipStreamSynchronize(r->stream);
    }
    r->d_maps.release();
    r->d_tab.release();
    r->d_src.release();
    r->d_dst.release();
    r->h_src.release();
    r->h_dst.release();
    r->maps_ready = false;
    return bytes;
}

int64_t svh_rectify_get_maps(svh_rectify* r, int32_t cam, float* mx, float* my, size_t cap) {
    if (!r || cam < 0 || cam >= r->prm.cameras) return svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_get_maps: bad arguments");
    const size_t px = r->pixels();
    if (!mx || !my || cap < px) return (int64_t)px;
    if (!have_device()) {
        const int32_t dw = r->prm.dst_width, dh = r->prm.dst_height;
        for (int32_t i = 0; i < dh; i++)
            for (int32_t j = 0; j < dw; j++)
                rect::map_entry(r->cam[cam], i, j, mx + (size_t)i * dw + j, my + (size_t)i * dw + j);
        return (int64_t)px;
    }
    auto run = [&]() -> int {
        ActiveCaller active;
        bool built = false;
        int rc = ensure(r, &built);
        if (rc) return rc;
        RECT_GROW(r->h_dst, 8 * px);
        RECT_TRY(copy, hipMemcpyAsync(r->h_dst, r->d_maps + 2 * px * (size_t)cam, 8 * px, hipMemcpyDeviceToHost, r->stream));
        return finish(r, built, false);
    };
    const int rc = drained(r, run());
    if (rc) return rc;
    memcpy(mx, r->h_dst, 4 * px);
    memcpy(my, r->h_dst + 4 * px, 4 * px);
    return (int64_t)px;
}

int32_t svh_rectify_remap(svh_rectify* r, int32_t cam, const uint8_t* src, int32_t src_on_device, int32_t src_row_stride,
                          uint8_t* dst, int32_t dst_on_device, int32_t dst_row_stride) {
    if (!r || !src || !dst || cam < 0 || cam >= r->prm.cameras || src_row_stride < r->prm.src_width ||
        dst_row_stride < r->prm.dst_width)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_remap: bad arguments");
    if (!have_device()) return no_device();
    return drained(r, remap_one(r, cam, src, src_on_device != 0, src_row_stride, dst, dst_on_device != 0, dst_row_stride));
}

int32_t svh_rectify_pairs_device(svh_rectify* r, int32_t n, const uint8_t* dS1, const uint8_t* dS2,
                                 int32_t src_row_stride, size_t src_image_stride, uint8_t* dI1, uint8_t* dI2,
                                 int32_t dst_row_stride, size_t dst_image_stride) {
    if (!r || r->prm.cameras != 2 || n < 1 || n > 4096 || !dS1 || !dS2 || !dI1 || !dI2 ||
        src_row_stride < r->prm.src_width || dst_row_stride < r->prm.dst_width)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_pairs_device: bad arguments");
    if (n > 1 && (src_image_stride < span(r->prm.src_width, r->prm.src_height, src_row_stride) ||
                  dst_image_stride < span(r->prm.dst_width, r->prm.dst_height, dst_row_stride)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_rectify_pairs_device: an image stride is shorter than an image");
    if (!have_device()) return no_device();
    return drained(r, remap_pairs(r, n, dS1, dS2, src_row_stride, src_image_stride, dI1, dI2, dst_row_stride,
                                  dst_image_stride));
}

void svh_rectify_set_timing(svh_rectify* r, int32_t on) {
    if (r) r->timing = on != 0;
}

int32_t svh_rectify_get_timing(svh_rectify* r, double* ms2) {
    if (!r) return 0;
    for (int i = 0; i < 2 && ms2; i++) ms2[i] = r->ms[i];
    return 2;
}

}  // extern "C"

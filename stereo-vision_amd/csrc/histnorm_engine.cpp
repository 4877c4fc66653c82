// StereoImage::histogramNormalization (stereomapper/stereoimage.cpp:94-134) behind the svh_histnorm_* entries of
// include/svh_histnorm.h.
//
// Host (this file): the segment table of f for the object's image size (histnorm_core.h, built in create: a few
// operations per binade), the host form of the table, and the staging of a host image.  Device
// (histnorm_kernels.hip): k_hist_count, k_hist_table, k_hist_apply, one launch each over all images of a call.  Every
// object has its own stream; nothing synchronises the default stream.
//
// A compute call is a transaction.  Everything that can fail before the image changes -- the object's stream and
// events, its buffers, the upload of the segment table and of a host image, the clearing of the counters, k_hist_count
// and k_hist_table -- comes first; each launch with its check is ONE guarded expression, so a failure up to and
// including the launch check of k_hist_apply leaves a device image untouched.  A host image is written from the pinned
// copy after the final wait, so it is untouched after any failure.  The object itself changes only by what the next
// call would redo: its segment table counts as uploaded, and the tables of the parity tap as those of `images` images,
// once the call has waited.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>

#include "../../include/svh_histnorm.h"
#include "batch_rec.h"
#include "hip_guard.h"
#include "histnorm_internal.h"
#include "svh_config.h"

using namespace svh;

static_assert(SVH_HISTNORM_MAX_SIDE == hn::MAX_SIDE && SVH_HISTNORM_MAX_SEGMENTS == hn::MAX_SEG, "header and core differ");

namespace {

#define HN_TRY(kind, expr) SVH_HIP_TRY("HistNorm", kind, expr)
#define HN_GROW(buf, bytes) SVH_HIP_GROW("HistNorm", buf, bytes)

bool have_device() {
    int nd = 0;
    return hipGetDeviceCount(&nd) == hipSuccess && nd > 0;
}

int no_device() { return svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback"); }

bool side_ok(int32_t v) { return v >= 1 && v <= SVH_HISTNORM_MAX_SIDE; }

// bytes an image of h rows of w bytes spans at this row stride
size_t span(int32_t w, int32_t h, int32_t stride) { return (size_t)(h - 1) * (size_t)stride + (size_t)w; }

constexpr size_t TAB_BYTES = 256 * (sizeof(int32_t) + sizeof(float) + sizeof(uint8_t));   // per image

// the host form: p, the chain and the map from the table
void table_from_counts(const hn::Seg* seg, int ns, const int32_t* counts, float* cdf, uint8_t* map) {
    float p[256], s[256];
    for (int g = 0; g < 256; g++) p[g] = hn::eval(seg, ns, counts[g]);
    hn::cdf_chain(p, s);
    for (int g = 0; g < 256; g++) {
        if (cdf) cdf[g] = s[g];
        if (map) map[g] = hn::map_entry(s[g]);
    }
}

}  // namespace

struct svh_histnorm {
    int32_t w = 0, h = 0;
    hn::Seg seg[hn::MAX_SEG];
    int32_t nseg = 0;
    int device = 0;
    bool timing = false;
    double ms[3] = {0, 0, 0};
    // device side
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool seg_ready = false;
    int32_t images = 0;                 // of the last successful call: what d_tab holds
    HipBuf<hn::Seg> d_seg;
    PinnedBuf<hn::Seg> h_seg;
    HipBuf<uint8_t> d_tab;              // counts [n][256] int32, cdf [n][256] float, map [n][256] uint8
    PinnedBuf<uint8_t> h_tab;
    HipBuf<uint8_t> d_img;              // a host image on its way to the device and back
    PinnedBuf<uint8_t> h_img;
};

namespace {

// stream, events, the segment table on the device and room for the tables of n images
int ensure(svh_histnorm* o, int32_t n, bool* uploaded) {
    HN_TRY(none, hipSetDevice(o->device));
    if (!o->stream) {
        hipStream_t s = nullptr;
        HN_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        o->stream = s;
    }
    for (int i = 0; i < 4; i++)
        if (!o->ev[i]) HN_TRY(none, hipEventCreate(&o->ev[i]));
    const size_t seg_bytes = sizeof(hn::Seg) * hn::MAX_SEG;
    if (o->d_seg.cap < seg_bytes || o->h_seg.cap < seg_bytes) o->seg_ready = false;
    HN_GROW(o->d_seg, seg_bytes);
    HN_GROW(o->h_seg, seg_bytes);
    if (o->d_tab.cap < TAB_BYTES * (size_t)n) o->images = 0;   // growing discards the last call's tables
    HN_GROW(o->d_tab, TAB_BYTES * (size_t)n);
    *uploaded = false;
    if (!o->seg_ready) {
        memcpy(o->h_seg.p, o->seg, seg_bytes);
        HN_TRY(copy, hipMemcpyAsync(o->d_seg, o->h_seg, seg_bytes, hipMemcpyHostToDevice, o->stream));
        *uploaded = true;   // ready once the caller has waited for the stream
    }
    return SVH_OK;
}

HistJob job_of(svh_histnorm* o, uint8_t* i0, uint8_t* i1, int32_t slots, int32_t images, int32_t row_stride,
               size_t image_stride) {
    HistJob a;
    a.img0 = i0, a.img1 = i1;
    a.image_stride = image_stride;
    a.row_stride = row_stride, a.w = o->w, a.h = o->h;
    a.slots = slots, a.images = images;
    a.counts = reinterpret_cast<int32_t*>(o->d_tab.p);
    a.cdf = reinterpret_cast<float*>(o->d_tab.p + 1024 * (size_t)images);
    a.map = o->d_tab.p + 2048 * (size_t)images;
    a.seg = o->d_seg;
    a.nseg = o->nseg;
    return a;
}

// counters cleared, then the three kernels; the image changes in the last one only
int enqueue(svh_histnorm* o, const HistJob& a) {
    HN_TRY(copy, hipMemsetAsync(a.counts, 0, 1024 * (size_t)a.images, o->stream));
    HN_TRY(launch, (histlaunch_count(o->stream, a), hipGetLastError()));
    HN_TRY(launch, (histlaunch_table(o->stream, a), hipGetLastError()));
    if (o->timing) (void)hipEventRecord(o->ev[1], o->stream);
    HN_TRY(launch, (histlaunch_apply(o->stream, a), hipGetLastError()));
    if (o->timing) (void)hipEventRecord(o->ev[2], o->stream);
    return SVH_OK;
}

// the wait that ends a call
int finish(svh_histnorm* o, bool uploaded, int32_t images) {
    HN_TRY(wait, (hipError_t)wait_stream(o->stream));
    if (uploaded) o->seg_ready = true;
    o->images = images;
    if (o->timing) {
        float t[3] = {0, 0, 0};
        const bool ok = hipEventElapsedTime(&t[0], o->ev[0], o->ev[3]) == hipSuccess &&
                        hipEventElapsedTime(&t[1], o->ev[0], o->ev[1]) == hipSuccess &&
                        hipEventElapsedTime(&t[2], o->ev[1], o->ev[2]) == hipSuccess;
        for (int i = 0; i < 3; i++) o->ms[i] = ok ? t[i] : 0;
    }
    return SVH_OK;
}

int run_device(svh_histnorm* o, uint8_t* i0, uint8_t* i1, int32_t slots, int32_t images, int32_t row_stride,
               size_t image_stride) {
    ActiveCaller active;
    bool uploaded = false;
    o->images = 0;   // the tables are overwritten from here on
    int rc = ensure(o, images, &uploaded);
    if (rc) return rc;
    const HistJob a = job_of(o, i0, i1, slots, images, row_stride, image_stride);
    if (o->timing) (void)hipEventRecord(o->ev[0], o->stream);
    if ((rc = enqueue(o, a))) return rc;
    if (o->timing) (void)hipEventRecord(o->ev[3], o->stream);
    return finish(o, uploaded, images);
}

int run_host(svh_histnorm* o, uint8_t* I, int32_t row_stride) {
    ActiveCaller active;
    bool uploaded = false;
    o->images = 0;
    int rc = ensure(o, 1, &uploaded);
    if (rc) return rc;
    const size_t bytes = span(o->w, o->h, row_stride);
    HN_GROW(o->d_img, bytes);
    HN_GROW(o->h_img, bytes);
    const HistJob a = job_of(o, o->d_img, o->d_img, 1, 1, row_stride, 0);
    if (o->timing) (void)hipEventRecord(o->ev[0], o->stream);
    for (int32_t y = 0; y < o->h; y++)   // only the pixels: the caller's padding may not even be readable
        memcpy(o->h_img + (size_t)y * (size_t)row_stride, I + (size_t)y * (size_t)row_stride, (size_t)o->w);
    HN_TRY(copy, hipMemcpyAsync(o->d_img, o->h_img, bytes, hipMemcpyHostToDevice, o->stream));
    if ((rc = enqueue(o, a))) return rc;
    HN_TRY(copy, hipMemcpyAsync(o->h_img, o->d_img, bytes, hipMemcpyDeviceToHost, o->stream));
    if (o->timing) (void)hipEventRecord(o->ev[3], o->stream);
    if ((rc = finish(o, uploaded, 1))) return rc;
    for (int32_t y = 0; y < o->h; y++)
        memcpy(I + (size_t)y * (size_t)row_stride, o->h_img + (size_t)y * (size_t)row_stride, (size_t)o->w);
    return SVH_OK;
}

// nothing of a failed call is in flight when the caller goes on
int drained(svh_histnorm* o, int rc) {
    if (rc == SVH_ERR_HIP && o->stream) {
        (void)hipSetDevice(o->device);
        (void)hipStreamSynchronize(o->stream);
    }
    return rc;
}

// the table of a size without an object
int segments_of(int32_t width, int32_t height, hn::Seg* seg, const char* who) {
    if (!side_ok(width) || !side_ok(height))
        return svh::fail(SVH_ERR_BAD_ARG, std::string(who) + ": a side is outside 1.." + std::to_string(SVH_HISTNORM_MAX_SIDE));
    const int ns = hn::build_segments(hn::fraction(width, height), width * height, seg);
    if (ns < 0) return svh::fail(SVH_ERR_UNSUPPORTED, std::string(who) + ": the segment table overflows");
    return ns;
}

}  // namespace

extern "C" {

svh_histnorm* svh_histnorm_create(int32_t width, int32_t height) {
    svh::ensure_init();
    svh_histnorm* o = new svh_histnorm();
    const int ns = segments_of(width, height, o->seg, "svh_histnorm_create");
    if (ns < 0) {
        delete o;
        return nullptr;
    }
    for (int i = ns; i < hn::MAX_SEG; i++) o->seg[i] = o->seg[ns - 1];
    o->w = width, o->h = height, o->nseg = ns;
    if (have_device()) (void)hipGetDevice(&o->device);
    return o;
}

void svh_histnorm_destroy(svh_histnorm* o) {
    if (!o) return;
    if (o->stream) {
        (void)hipSetDevice(o->device);
        (void)hipStreamSynchronize(o->stream);
        (void)hipStreamDestroy(o->stream);
    }
    for (int i = 0; i < 4; i++)
        if (o->ev[i]) (void)hipEventDestroy(o->ev[i]);
    delete o;
}

int64_t svh_histnorm_release(svh_histnorm* o) {
    if (!o) return 0;
    const int64_t bytes =
        (int64_t)(o->d_seg.cap + o->h_seg.cap + o->d_tab.cap + o->h_tab.cap + o->d_img.cap + o->h_img.cap);
    if (o->stream) {
        (void)hipSetDevice(o->device);
        (void)hipStreamSynchronize(o->stream);
    }
    o->d_seg.release();
    o->h_seg.release();
    o->d_tab.release();
    o->h_tab.release();
    o->d_img.release();
    o->h_img.release();
    o->seg_ready = false;
    o->images = 0;
    return bytes;
}

int32_t svh_histnorm_apply(svh_histnorm* o, uint8_t* I, int32_t on_device, int32_t row_stride) {
    if (!o || !I || row_stride < o->w) return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_apply: bad arguments");
    if (!have_device()) return no_device();
    return drained(o, on_device ? run_device(o, I, I, 1, 1, row_stride, 0) : run_host(o, I, row_stride));
}

int32_t svh_histnorm_images_device(svh_histnorm* o, int32_t n, uint8_t* dI, int32_t row_stride, size_t image_stride) {
    if (!o || n < 1 || n > 4096 || !dI || row_stride < o->w)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_images_device: bad arguments");
    if (n > 1 && image_stride < span(o->w, o->h, row_stride))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_images_device: the image stride is shorter than an image");
    if (!have_device()) return no_device();
    return drained(o, run_device(o, dI, dI, 1, n, row_stride, image_stride));
}

int32_t svh_histnorm_pairs_device(svh_histnorm* o, int32_t n, uint8_t* dI1, uint8_t* dI2, int32_t row_stride,
                                  size_t image_stride) {
    if (!o || n < 1 || n > 4096 || !dI1 || !dI2 || row_stride < o->w)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_pairs_device: bad arguments");
    if (n > 1 && image_stride < span(o->w, o->h, row_stride))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_pairs_device: the image stride is shorter than an image");
    if (!have_device()) return no_device();
    return drained(o, run_device(o, dI1, dI2, 2, 2 * n, row_stride, image_stride));
}

int32_t svh_histnorm_get_tables(svh_histnorm* o, int32_t* counts, float* cdf, uint8_t* map, int32_t cap_images) {
    if (!o || cap_images < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_get_tables: bad arguments");
    const int32_t n = o->images;
    if (n == 0 || cap_images < n) return n;
    auto run = [&]() -> int {
        ActiveCaller active;
        HN_TRY(none, hipSetDevice(o->device));
        HN_GROW(o->h_tab, TAB_BYTES * (size_t)n);
        HN_TRY(copy, hipMemcpyAsync(o->h_tab, o->d_tab, TAB_BYTES * (size_t)n, hipMemcpyDeviceToHost, o->stream));
        HN_TRY(wait, (hipError_t)wait_stream(o->stream));
        return SVH_OK;
    };
    const int rc = drained(o, run());
    if (rc) return rc;
    if (counts) memcpy(counts, o->h_tab.p, 1024 * (size_t)n);
    if (cdf) memcpy(cdf, o->h_tab.p + 1024 * (size_t)n, 1024 * (size_t)n);
    if (map) memcpy(map, o->h_tab.p + 2048 * (size_t)n, 256 * (size_t)n);
    return n;
}

int32_t svh_histnorm_table_host(int32_t width, int32_t height, const int32_t* counts256, float* cdf256,
                                uint8_t* map256) {
    hn::Seg seg[hn::MAX_SEG];
    const int ns = segments_of(width, height, seg, "svh_histnorm_table_host");
    if (ns < 0) return ns;
    if (!counts256) return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_table_host: no counts");
    for (int g = 0; g < 256; g++)
        if (counts256[g] < 0 || counts256[g] > width * height)
            return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_table_host: a count is outside 0..width*height");
    table_from_counts(seg, ns, counts256, cdf256, map256);
    return SVH_OK;
}

int32_t svh_histnorm_segments(int32_t width, int32_t height, int32_t* n0, float* f, float* inc, int32_t cap) {
    hn::Seg seg[hn::MAX_SEG];
    const int ns = segments_of(width, height, seg, "svh_histnorm_segments");
    if (ns < 0 || !n0 || !f || !inc || cap < ns) return ns;
    for (int i = 0; i < ns; i++) n0[i] = seg[i].n0, f[i] = seg[i].f, inc[i] = seg[i].inc;
    return ns;
}

int32_t svh_histnorm_chain(int32_t width, int32_t height, const int32_t* n, int64_t count, float* out) {
    hn::Seg seg[hn::MAX_SEG];
    const int ns = segments_of(width, height, seg, "svh_histnorm_chain");
    if (ns < 0) return ns;
    if (!n || !out || count < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_chain: bad arguments");
    for (int64_t i = 0; i < count; i++)
        if (n[i] < 0 || n[i] > width * height)
            return svh::fail(SVH_ERR_BAD_ARG, "svh_histnorm_chain: an n is outside 0..width*height");
    for (int64_t i = 0; i < count; i++) out[i] = hn::eval(seg, ns, n[i]);
    return SVH_OK;
}

void svh_histnorm_set_timing(svh_histnorm* o, int32_t on) {
    if (o) o->timing = on != 0;
}

int32_t svh_histnorm_get_timing(svh_histnorm* o, double* ms3) {
    if (!o) return 0;
    for (int i = 0; i < 3 && ms3; i++) ms3[i] = o->ms[i];
    return 3;
}

}  // extern "C"

/* C-ABI of the histogram normalisation of 8-bit frames (reference: StereoImage::histogramNormalization,
 * stereomapper/stereoimage.cpp:94-134): the photometric equalisation of a frame in place, on the device, so that a
 * frame which rectification left in device memory reaches the matchers without a round trip.  Exported by libsvhip.so.
 *
 * THE CONTRACT is the reference's arithmetic as its x86-64 build performs it (stereo-vision_amd/csrc/histnorm_core.h),
 * with N = width * height and count[g] the number of pixels of grey level g:
 *     c      = (float)(1.0 / (double)(float)N)
 *     p[g]   = f(count[g]),  f(0) = 0,  f(n) = fl32(f(n-1) + c)      -- the reference adds c once per pixel, in float
 *     cdf[0] = p[0],  cdf[g] = fl32(cdf[g-1] + p[g])                  -- in the order of g
 *     map[g] = (uint8_t)(int32_t)((double)cdf[g] * 255.0)             -- THE WRAP: see below
 *     I[v][u] = map[I[v][u]]
 * The float chain does not end at 1: a flat 1392x512 frame ends at 1.009, the product is 257.3, the conversion to a
 * 32-bit integer keeps 257 and the byte is 1.  Every pixel of that frame becomes 1, in the reference and here.  A flat
 * 1242x375 frame becomes 254.  This is stated behaviour, not repaired.
 * f is evaluated from a table of its linear segments (a few dozen per image size, built on the host once per object),
 * never by N additions; the result is bit for bit the chain's.                                                     */
#ifndef SVH_HISTNORM_H
#define SVH_HISTNORM_H
#include <stddef.h>
#include <stdint.h>

#include "svh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVH_HISTNORM_MAX_SIDE 16384
#define SVH_HISTNORM_MAX_SEGMENTS 192

typedef struct svh_histnorm svh_histnorm;
/* An object for images of width x height pixels.  Needs no device.  NULL with svh_last_error() for a side outside
 * 1..SVH_HISTNORM_MAX_SIDE.                                                                                        */
svh_histnorm* svh_histnorm_create(int32_t width, int32_t height);
void          svh_histnorm_destroy(svh_histnorm*);
/* gives back the device and pinned buffers; the next call builds them again.  Returns the bytes released.         */
int64_t       svh_histnorm_release(svh_histnorm*);

/* The reference's call: one image of height rows of width bytes, row_stride bytes apart, equalised IN PLACE; host
 * memory, or device memory with on_device != 0.  Synchronous, on the object's own stream.  Returns SVH_OK,
 * SVH_ERR_BAD_ARG, SVH_ERR_NO_DEVICE or SVH_ERR_HIP (svh_last_error() names the failing call; the stream is drained
 * and the object usable).  A host image is untouched after any failure.  A device image is untouched after a failure
 * up to and including the launch check of the last kernel (k_hist_apply); only a failure of the final wait can leave
 * it mapped.  Bytes between the rows are never written.                                                            */
int32_t svh_histnorm_apply(svh_histnorm*, uint8_t* I, int32_t on_device, int32_t row_stride);

/* n images resident in device memory, image k at dI + k * image_stride, each equalised with its own table: three
 * launches whatever n is.  1 <= n <= 4096; image_stride must hold an image when n > 1.  Errors as for a device image
 * above.                                                                                                           */
int32_t svh_histnorm_images_device(svh_histnorm*, int32_t n, uint8_t* dI, int32_t row_stride, size_t image_stride);
/* n stereo pairs as svh_rectify_pairs_device leaves them and svh_elas_process_batch_device takes them: left / right
 * image k at dI1 / dI2 + k * image_stride.  Every one of the 2 n images gets its own table, as two calls of the
 * reference do.  Image order of the parity tap: left 0, right 0, left 1, ...                                       */
int32_t svh_histnorm_pairs_device(svh_histnorm*, int32_t n, uint8_t* dI1, uint8_t* dI2, int32_t row_stride,
                                  size_t image_stride);

/* Parity tap of the last successful call: counts int32 [images][256], cdf float [images][256], map uint8
 * [images][256] (any may be NULL).  Returns the number of images of that call (nothing is copied when cap_images is
 * smaller; 0 before the first call or after a release) or a negative SVH_ERR_*.                                    */
int32_t svh_histnorm_get_tables(svh_histnorm*, int32_t* counts, float* cdf, uint8_t* map, int32_t cap_images);

/* The host form of the same core, usable without a device: cdf and map of an image of width x height pixels with the
 * given counts (each in 0..width*height; their sum is not checked).  cdf256 or map256 may be NULL.                  */
int32_t svh_histnorm_table_host(int32_t width, int32_t height, const int32_t* counts256, float* cdf256,
                                uint8_t* map256);
/* The segment table of f for this image size: f(n) = f[k] + (n - n0[k]) * inc[k] for n0[k] <= n < n0[k+1], the last
 * segment reaching to N.  Returns the number of segments (at most SVH_HISTNORM_MAX_SEGMENTS; nothing is copied when
 * cap is smaller) or SVH_ERR_BAD_ARG.                                                                              */
int32_t svh_histnorm_segments(int32_t width, int32_t height, int32_t* n0, float* f, float* inc, int32_t cap);
/* f(n[i]) for i < count from that table (each n in 0..width*height): what p[g] is for a count.                     */
int32_t svh_histnorm_chain(int32_t width, int32_t height, const int32_t* n, int64_t count, float* out);

/* device ms of the last successful call from HIP events, recorded only after svh_histnorm_set_timing(h, 1): ms3[0]
 * the whole call (uploads and copy-back of a host image included), ms3[1] k_hist_count and k_hist_table, ms3[2]
 * k_hist_apply.  Returns 3.                                                                                        */
void    svh_histnorm_set_timing(svh_histnorm*, int32_t on);
int32_t svh_histnorm_get_timing(svh_histnorm*, double* ms3);

#ifdef __cplusplus
}
#endif
#endif /* SVH_HISTNORM_H */

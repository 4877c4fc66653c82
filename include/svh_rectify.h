/* C-ABI of the rectification in front of the stereo pipeline (reference: stereomapper/framecapturethread.cpp:100-131,
 * 328-349): the undistort-and-rectify maps of a calibrated camera, built once per object, and the bilinear remap of every
 * raw 8-bit frame through them, on the device.  Exported by libsvhip.so.
 *
 * The reference calls cv::initUndistortRectifyMap(K, D, R, P, size, CV_32FC1, Mx, My) and cv::remap(I, I_rect, Mx, My,
 * INTER_LINEAR, BORDER_WRAP).  OpenCV is not part of this project; the arithmetic is written out in
 * stereo-vision_amd/csrc/rectify_core.h as OpenCV's documentation publishes it, and THAT arithmetic is the contract.
 * Equality with an OpenCV build has not been verified.  Stated deviations: the maps are evaluated per
 * pixel in the direct form, not with running sums along a row; a map entry that is not finite or has |m| >= 2^20 yields 0;
 * the reference's cv::Size(roi->height, roi->width) swap is not reproduced.
 *
 * Maps (all double): A = P[:3,:3] R, ir = A^-1; for output pixel (row i, column j)
 *     X = j ir[0] + i ir[1] + ir[2],  Y = j ir[3] + i ir[4] + ir[5],  W = j ir[6] + i ir[7] + ir[8]
 *     x = X / W, y = Y / W (as products with 1 / W), r2 = x x + y y, kr = 1 + ((k3 r2 + k2) r2 + k1) r2
 *     u = fx (x kr + p1 2xy + p2 (r2 + 2 x x)) + cx,  v = fy (y kr + p1 (r2 + 2 y y) + p2 2xy) + cy,  map = (float)(u, v)
 * Sample: sx = rint(32 mx), sy = rint(32 my) (ties to even); x0 = sx >> 5, a = sx & 31, y0 = sy >> 5, b = sy & 31;
 *     out = ((32-a)(32-b) S(y0,x0) + a (32-b) S(y0,x0+1) + (32-a) b S(y0+1,x0) + a b S(y0+1,x0+1) + 512) >> 10
 * with every tap coordinate taken modulo the source size (SVH_RECTIFY_WRAP) or a tap outside the image read as 0
 * (SVH_RECTIFY_ZERO).                                                                                                */
#ifndef SVH_RECTIFY_H
#define SVH_RECTIFY_H
#include <stddef.h>
#include <stdint.h>

#include "svh.h"
#include "svh_kitti.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVH_RECTIFY_WRAP 0   /* the reference's call (BORDER_WRAP) and the default                                 */
#define SVH_RECTIFY_ZERO 1   /* the reference's commented-out cvRemap(... CV_WARP_FILL_OUTLIERS, 0)                */
#define SVH_RECTIFY_MAX_SIDE 16384

typedef struct svh_rectify_camera {
    double K[9];    /* camera matrix, row major: fx = K[0], fy = K[4], cx = K[2], cy = K[5]                     */
    double D[5];    /* k1 k2 p1 p2 k3                                                                           */
    double R[9];    /* rectifying rotation, row major                                                           */
    double P[12];   /* new projection, 3x4 row major; only its left 3x3 is used                                 */
} svh_rectify_camera;

typedef struct svh_rectify_params {
    int32_t src_width, src_height;   /* the raw frame                                                           */
    int32_t dst_width, dst_height;   /* the rectified frame                                                     */
    int32_t border;                  /* SVH_RECTIFY_WRAP / SVH_RECTIFY_ZERO                                     */
    int32_t cameras;                 /* 1 or 2                                                                  */
    svh_rectify_camera cam[2];
} svh_rectify_params;
/* sizes 0 (to be set), WRAP, two cameras, K = R = I, P = [I | 0], D = 0 */
void svh_rectify_params_default(svh_rectify_params* p);

/* The parameters of a KITTI calibration file (svh_kitti_read_cam_to_cam): source size S_xx, destination size S_rect_xx,
 * K_xx, D_xx, R_rect_xx and P_rect_xx of cam_left (0..3) and cam_right (0..3, or -1 for one camera).  Both cameras
 * must agree in both sizes.  Host only.  Returns SVH_OK or SVH_ERR_BAD_ARG.                                       */
int32_t svh_rectify_from_kitti(const svh_kitti_calib* calib, int32_t cam_left, int32_t cam_right, int32_t border,
                               svh_rectify_params* out);

typedef struct svh_rectify svh_rectify;
/* Needs no device.  NULL with svh_last_error() for a size <= 0 or > SVH_RECTIFY_MAX_SIDE, cameras other than 1 or 2,
 * an unknown border mode, or a camera whose P[:3,:3] R is singular (determinant 0 or not finite).                 */
svh_rectify* svh_rectify_create(const svh_rectify_params* p);
void         svh_rectify_destroy(svh_rectify*);
/* gives back the device and pinned buffers (maps, table, staging); the next call builds them again.  Returns the
 * bytes released.                                                                                                 */
int64_t      svh_rectify_release(svh_rectify*);

/* Parity tap: the float maps of camera `cam`, dst_height x dst_width each, packed; cap = floats available in each of
 * mx and my.  With a device they are what k_rect_maps wrote; without one the host form of the same arithmetic
 * answers.  Returns the number of entries of one map (nothing is copied when cap is smaller) or a negative SVH_ERR_*. */
int64_t svh_rectify_get_maps(svh_rectify*, int32_t cam, float* mx, float* my, size_t cap);

/* The reference's per-frame call for one image of camera `cam`: src is src_height rows of src_width bytes,
 * src_row_stride bytes apart, dst likewise with the destination size; either may be host memory or, with its
 * *_on_device != 0, device memory.  Synchronous.  Returns SVH_OK, SVH_ERR_BAD_ARG, SVH_ERR_NO_DEVICE or SVH_ERR_HIP.
 * After SVH_ERR_BAD_ARG or SVH_ERR_HIP the object is what it was before the call; a host destination is untouched,
 * and so is a device destination unless the failure is the final stream wait (the kernel may have run then).      */
int32_t svh_rectify_remap(svh_rectify*, int32_t cam, const uint8_t* src, int32_t src_on_device, int32_t src_row_stride,
                          uint8_t* dst, int32_t dst_on_device, int32_t dst_row_stride);

/* n stereo pairs resident in device memory in ONE launch (an object with two cameras): raw image k of the left / right
 * camera starts at dS1 / dS2 + k * src_image_stride, its rectified image at dI1 / dI2 + k * dst_image_stride.  The
 * output is what svh_elas_process_batch_device and svh_elas_stream_push_device_n take: dims = {dst_width, dst_height,
 * dst_row_stride}, in_stride = dst_image_stride.  Synchronous (complete on return), on the object's own stream.
 * 1 <= n <= 4096.  Errors as svh_rectify_remap with a device destination.                                          */
int32_t svh_rectify_pairs_device(svh_rectify*, int32_t n, const uint8_t* dS1, const uint8_t* dS2,
                                 int32_t src_row_stride, size_t src_image_stride, uint8_t* dI1, uint8_t* dI2,
                                 int32_t dst_row_stride, size_t dst_image_stride);

/* device ms of the last successful compute call from HIP events, recorded only after svh_rectify_set_timing(r, 1):
 * ms2[0] the remap (its uploads and copy-back included), ms2[1] the map kernel when that call built the maps, else 0.
 * Returns 2.                                                                                                       */
void    svh_rectify_set_timing(svh_rectify*, int32_t on);
int32_t svh_rectify_get_timing(svh_rectify*, double* ms2);

#ifdef __cplusplus
}
#endif
#endif /* SVH_RECTIFY_H */

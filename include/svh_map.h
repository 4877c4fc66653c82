/*
 * svh_map.h -- the consumer of D1 after the hot path: stereomapper's 3-D
 * reprojection and frame-to-frame map fusion on the device.
 *
 * Reference interfaces (paths relative to the reference checkout):
 *   stereomapper/stereothread.cpp:180-255   StereoThread::createCurrentMap
 *   stereomapper/stereothread.cpp:290-437   StereoThread::addDisparityMapToReconstruction
 *   stereomapper/stereothread.cpp:441-456   getIntrinsics (f, cu, cv, base, K)
 *   stereomapper/stereothread.cpp:460-470   clearReconstruction
 *
 * The reference keeps `_previous_map3d` pointing at buffers it has just freed (:432-433); this
 * library implements the intended behaviour -- the previous map is the current map of the frame
 * before, as the fusion left it -- see DESIGN.md.  Plain C like svh.h; device work runs on the
 * object's own stream and every call returns when it is complete.
 */
#ifndef SVH_MAP_H
#define SVH_MAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the float members StereoThread reads its geometry from (stereothread.h:192-196) */
typedef struct svh_map_params {
    float f, cu, cv, base;
    float max_dist;              /* StereoThread::_max_dist, 20 in the constructor (:14) */
} svh_map_params;

typedef struct svh_map svh_map;

svh_map* svh_map_create(const svh_map_params* p);   /* NULL without a HIP device */
void     svh_map_destroy(svh_map* m);
/* clearReconstruction(): forget the previous map and the point lists */
void     svh_map_clear(svh_map* m);

/* One frame = pushBack(simage, H_total, gain) + the "reconstruction" step of run()
 * (stereothread.cpp:30-41, 166-170).
 *   D1        left disparity map, dims[0] x dims[1] floats, rows packed: a host pointer, or -- with
 *             d1_on_device -- the device pointer Elas::process wrote to (no copy of the map then)
 *   I1        left image on the host, dims[2] bytes per row
 *   H_total   4x4 camera pose, row major (StereoThread::_H_total)
 *   gain      VisualOdometryStereo::getGain of the frame (0: no gain correction)
 * A frame of another size than the one before starts a new reconstruction, exactly as if
 * svh_map_clear had been called before it: the previous map cannot be addressed with the new
 * dimensions, list 0 is empty after that frame and the next frame of the same size fuses again.
 * Returns SVH_OK or a negative SVH_ERR_*.  SVH_ERR_BAD_ARG (a null pointer, w or h < 1, step < w,
 * w * h > 2^28) is decided before anything is read and leaves the object as it was.            */
int32_t svh_map_add(svh_map* m, const float* D1, int32_t d1_on_device, const uint8_t* I1,
                    const int32_t* dims, const double* H_total, float gain);

/* svh_map_add with BOTH inputs in device memory: dD1 as with d1_on_device, dI1 = dims[1] rows of dims[0] bytes,
 * dims[2] bytes apart, any alignment and any pitch >= width.  The image is read where it lies (no host staging, no
 * copy); both must be complete when the call is made and are not read after it returns.  Checks, errors and results
 * (point lists, planes) are those of svh_map_add given the same pixels. */
int32_t svh_map_add_device(svh_map* m, const float* dD1, const uint8_t* dI1, const int32_t* dims,
                           const double* H_total, float gain);

/* One frame of K maps in lockstep, every input in device memory: object i fuses (dD1[i], dI1[i]) with pose H_total[i]
 * and gain[i], as svh_map_add_device(ms[i], dD1[i], dI1[i], dims, H_total[i], gain[i]) would -- point lists and planes
 * are bit for bit those of K such calls, and svh_map_points, svh_map_planes and svh_view_add_map work per object
 * afterwards.  `dims` (width, height, pitch of the images) is shared; the svh_map_params of the objects may differ.
 * The maps that fuse with a previous map run as one recorded phase (one launch per kernel over all of them, one
 * wait), the maps that start a reconstruction (first frame, after svh_map_clear, another geometry) as a second one;
 * no object runs one by one because of its state.  Objects on different devices, or K = 1, run one after the other
 * through svh_map_add_device.
 * SVH_ERR_BAD_ARG, decided before anything is touched: a null table or a null entry of one, the same map twice,
 * K < 0, bad dims.  K = 0: SVH_OK.  After SVH_ERR_HIP nothing is in flight and NO object has taken the frame: adding
 * the same frames again gives the right result.  Host inputs have no batch form. */
int32_t svh_map_add_batch_device(svh_map* const* ms, int32_t K, const float* const* dD1, const uint8_t* const* dI1,
                                 const int32_t* dims, const double* const* H_total, const float* gain);

/* The two point lists StereoThread::_points holds after a frame, as (x, y, z, val) floats in the
 * reference's push_back order (columns left to right, each top to bottom):
 *   which 0   points of the previous map that were not merged into the current one
 *   which 1   points of the current map (after the fusion)
 * Copies min(number, cap) points to `xyzv` (may be NULL) and returns the number of points;
 * any `which` other than 0 means 1.                                                            */
int64_t svh_map_points(svh_map* m, int32_t which, float* xyzv, int64_t cap);

/* The colour-coded disparity map StereoThread shows next to the image (stereothread.cpp:117-147):
 * hue from red (near, d >= 200) over green to magenta (far), black where D <= 0.  D: n floats on the
 * host or (d_on_device) on the device; rgb receives 3*n floats on the host, interleaved.           */
int32_t svh_disparity_colormap(const float* D, int32_t d_on_device, int64_t n, float* rgb);

/* Test access: the current map's planes I, D, X, Y, Z (5 x width*height floats) after the frame.
 * SVH_ERR_BAD_ARG, nothing written: before the first frame, after svh_map_clear, cap_floats too small. */
int32_t svh_map_planes(svh_map* m, float* out5, size_t cap_floats);

#ifdef __cplusplus
}
#endif
#endif

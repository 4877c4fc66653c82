/*
 * svh_view2d.h -- the 2-D panes of the stereomapper window, rendered on the device: the left and the right image with
 * the matches over them, and the colour-coded disparity map.  A headless stand-in for the reference's OpenGL widget
 * View2D; the frame, the matches and D1 are read where the chain left them in device memory.
 *
 * Reference interfaces (paths relative to the reference checkout):
 *   stereomapper/view2d.cpp:18-27           View2D::setImage (grey texture; clears the matches)
 *   stereomapper/view2d.cpp:31-39           View2D::setColorImage (float RGB texture; the matches stay)
 *   stereomapper/view2d.cpp:43-49           View2D::setMatches
 *   stereomapper/view2d.cpp:69-154          View2D::paintGL
 *   stereomapper/view2d.cpp:158-163         View2D::resizeGL
 *   stereomapper/stereothread.cpp:117-147   the colour map of a disparity map
 *   stereomapper/visualodometrythread.cpp:109-119   the inlier flags from getInlierIndices
 *   stereomapper/maindialog.cpp:451-452, 506-511, 588-598   what MainDialog feeds the three panes
 *
 * View2D is a QGLWidget, and OpenGL leaves the rasterisation of textured quads, lines and points partly to the
 * implementation.  The contract of this library is the arithmetic of stereo-vision_amd/csrc/view2d_core.h (restated in
 * tests/view2d_ref.py and summarised in DESIGN.md): the image sampled GL_NEAREST at pixel centres in exact integers, a
 * 2-pixel line and a 5 x 5 point per match in list order, later over earlier, opaque, RGB8 out.  Equality with any
 * OpenGL implementation is NOT verified.  Out of scope: multisampling (the widget asks for QGL::SampleBuffers; every
 * pixel is one sample), blending (no colour of the widget has an alpha below 1), a window (render returns the image).
 *
 * Plain C like svh_view.h.  An object has its own stream and every call returns when it is complete; the caller's
 * image, map and match array are copied by the call (GL texture semantics) and never read after it returns.  Sources
 * may have any pitch >= w and start at any byte.  Calls return SVH_OK or a negative SVH_ERR_*; svh_last_error() has the
 * text.  SVH_ERR_BAD_ARG -- a null object or array, a pane side outside 1..16384, an image side outside 1..16384, a
 * pitch < w, n < 0, n > 0 with a null array, an inlier index outside 0..n-1 -- is decided before anything is read or
 * changed.  After SVH_ERR_HIP the object renders what it held before the call.
 */
#ifndef SVH_VIEW2D_H
#define SVH_VIEW2D_H

#include <stddef.h>
#include <stdint.h>

#include "svh.h"       /* SVH_OK, SVH_ERR_*, svh_last_error, svh_p_match */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svh_view2d svh_view2d;

svh_view2d* svh_view2d_create(int32_t width, int32_t height);   /* pane size; NULL without a HIP device */
void        svh_view2d_destroy(svh_view2d* v);
int32_t     svh_view2d_resize(svh_view2d* v, int32_t width, int32_t height);   /* resizeGL */

/* setImage: a grey image, dims = {w, h, pitch in bytes}; also clears the matches */
int32_t     svh_view2d_set_image(svh_view2d* v, const uint8_t* I, const int32_t* dims, int32_t on_device);
/* setColorImage: w * h * 3 floats, stored as byte_of of each; the matches stay */
int32_t     svh_view2d_set_color_image(svh_view2d* v, const float* rgb, int32_t w, int32_t h, int32_t on_device);
/* the colour map of stereothread.cpp:117-147 and setColorImage in one pass over a w * h disparity map (D1 where
 * svh_elas_process_batch_device wrote it): byte_of of what svh_disparity_colormap gives; the matches stay */
int32_t     svh_view2d_set_disparity(svh_view2d* v, const float* D, int32_t w, int32_t h, int32_t on_device);

/* setMatches: n matches and n inlier flags (0 = outlier), both on the host or both on the device; left != 0 draws
 * (u1p, v1p) -> (u1c, v1c), else (u2p, v2p) -> (u2c, v2c) */
int32_t     svh_view2d_set_matches(svh_view2d* v, const svh_p_match* m, int32_t n, const uint8_t* inlier, int32_t left,
                                   int32_t on_device);
/* the same with the inliers as getInlierIndices gives them (host arrays): flags as visualodometrythread.cpp:109-119
 * sets them */
int32_t     svh_view2d_set_matches_indexed(svh_view2d* v, const svh_p_match* m, int32_t n, const int32_t* inlier_idx,
                                           int32_t n_inliers, int32_t left);
void        svh_view2d_clear_matches(svh_view2d* v);

/* paintGL + grabFrameBuffer: width * height * 3 bytes, row 0 = top, to the host or (rgb_on_device) a device pointer
 * of any byte alignment */
int32_t     svh_view2d_render(svh_view2d* v, uint8_t* rgb, int32_t rgb_on_device);

#ifdef __cplusplus
}
#endif
#endif

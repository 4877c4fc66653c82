/*
 * svh_grid.h -- the ground grid: a 2.5-D bird's-eye grid over the road plane, binned on the device from the
 * accumulated map (svh_view.h) or from any list of (x, y, z, val) points.  Per cell: how many points, how high, how
 * bright, and whether the cell is drivable.  It is the consumer of the road plane of svh_plane.h, which the reference
 * computes and never applies (stereomapper/stereothread.cpp:152-164, under `if (0)`); the reference has no such grid.
 *
 * The contract is the arithmetic of stereo-vision_amd/csrc/grid_core.h (restated in tests/grid_ref.py and summarised in
 * DESIGN.md, "Ground grid").  Per point: a = T0.(x,y,z,1) lateral, b = T1.(x,y,z,1) forward, h = T2.(x,y,z,1) height,
 * in fp32; the cell is (floorf((a - x0) / cell), floorf((b - z0) / cell)).  A point is
 *   unplaced  if a coordinate or one of a, b, h is not finite,
 *   outside   if its cell is not in the window or not |h| < 2^20,
 *   overhead  if h > clearance (bridges, branches): only the cell's overhead count grows,
 *   low       otherwise: the cell's count, lowest and highest height, height sum (in 1/1024) and intensity sum grow.
 * Everything a cell accumulates is an integer under a commutative, associative update, so the grid depends only on
 * the multiset of points added since the last clear: never on their order, the launch shape or the scheduling.
 * The class of a cell (bits 0-1 of the class byte), tested in this order: 0 unknown (fewer than min_points low
 * points), 2 obstacle (HMAX > step), 3 drop (HMIN < -drop), 1 free.  Bit 7 (overhang): overhead >= min_points.
 * Not done: slope or neighbour-cell tests, ray-traced free space, a window that scrolls without clearing.
 *
 * Plain C like svh_view.h.  An object has its own stream and every call returns when it is complete.  Calls return
 * SVH_OK or a negative SVH_ERR_*; svh_last_error() has the text.  SVH_ERR_BAD_ARG -- a null pointer, parameters out of
 * the ranges below, n < 0, n > 0 with a null array, a device array that is not 16-byte aligned, an unknown plane or
 * mode -- is decided before anything is read or changed.  svh_grid_create returns NULL without a HIP device.
 * SVH_ERR_UNSUPPORTED, nothing changed: the object would have been given more than 2^31 - 1 points since the last
 * clear (counts are 32 bits).  After SVH_ERR_HIP inside svh_grid_add_* the grid is EMPTY (accumulation is in place, a
 * half-added call cannot be taken back): all statistics are zero and the next add starts afresh.  After SVH_ERR_HIP
 * inside svh_grid_get or svh_grid_render the accumulated grid is untouched.
 */
#ifndef SVH_GRID_H
#define SVH_GRID_H

#include <stddef.h>
#include <stdint.h>

#include "svh.h"       /* SVH_OK, SVH_ERR_*, svh_last_error */
#include "svh_view.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svh_grid svh_grid;

typedef struct svh_grid_params {
    int32_t nx, nz;            /* cells across (lateral) and along (forward); each 1..8192 */
    float   cell;              /* side of a cell, finite, > 0 */
    float   x0, z0;            /* ground coordinates of the low corner of cell (0, 0), finite */
    double  T[12];             /* 3x4 row major, camera/map frame -> ground frame; rounded to float once at create
                                  (the rounded values must be finite): rows a lateral, b forward, h height, road h = 0 */
    int32_t min_points;        /* 3: fewer low points than this -> the cell is unknown; >= 1 */
    float   step;              /* 0.2: a cell whose highest low point is above this is an obstacle; finite, >= 0 */
    float   drop;              /* 0.3: a cell whose lowest point is below -drop is a drop; finite, >= 0 */
    float   clearance;         /* 2.0: points above this are overhead, not obstacles; finite, > step */
    float   render_h_lo, render_h_hi;   /* 0, 2: range of the height colouring; finite, lo < hi */
} svh_grid_params;

typedef struct svh_grid_stats { int64_t added, binned, overhead, outside, unplaced; } svh_grid_stats;

/* planes of svh_grid_get, row major, index = ib * nx + ia (ia lateral, ib forward) */
#define SVH_GRID_COUNT      0   /* int32: low points */
#define SVH_GRID_OVERHEAD   1   /* int32: overhead points */
#define SVH_GRID_HMIN       2   /* float: lowest low point, NaN where COUNT is 0 */
#define SVH_GRID_HMAX       3   /* float: highest low point, NaN where COUNT is 0 */
#define SVH_GRID_HMEAN      4   /* float: (float)((double)sum of rintf(h * 1024) / (1024.0 * COUNT)), NaN where COUNT is 0 */
#define SVH_GRID_INTENSITY  5   /* uint8: mean of (uint8)rintf(clamp(val, 0, 1) * 255), rounded half up; 0 where COUNT is 0 */
#define SVH_GRID_CLASS      6   /* uint8: class in bits 0-1, overhang in bit 7 */
/* modes of svh_grid_render */
#define SVH_GRID_RENDER_CLASS      0   /* unknown (32,32,32), free (0, 64 + 3 I / 4, 0), obstacle (255,0,0), drop (0,0,160);
                                          with the overhang bit the blue byte is 255 */
#define SVH_GRID_RENDER_HEIGHT     1   /* HMAX over render_h_lo..render_h_hi through the disparity colour map; black where
                                          COUNT is 0 and at or below render_h_lo */
#define SVH_GRID_RENDER_INTENSITY  2   /* grey; black where COUNT is 0 */

/* 256 x 256 cells of 0.2 m, x0 = -25.6, z0 = 0, T = svh_grid_frame_camera(1.65), the thresholds above */
void      svh_grid_params_default(svh_grid_params* p);
/* a level camera cam_height above the road, x right, y down, z forward: rows (1,0,0,0), (0,0,1,0), (0,-1,0,cam_height) */
int32_t   svh_grid_frame_camera(double cam_height, double T[12]);
/* from svh_plane_get_plane_euclidean (the road is e.X = 1) and svh_plane_get_transformation (columns r1 right, r2 down,
 * r3 forward): rows a = r1.X, b = r3.X, h = 1/|e| - (e/|e|).X.  SVH_ERR_BAD_ARG for |e| == 0 -- what the estimate leaves
 * after SVH_PLANE_NO_POINTS or SVH_PLANE_FEW_INLIERS -- or an input that is not finite.  Needs no device.           */
int32_t   svh_grid_frame_plane(const double plane_e[3], const double H[16], double T[12]);

svh_grid* svh_grid_create(const svh_grid_params* p);   /* NULL: bad parameters, or no HIP device */
void      svh_grid_destroy(svh_grid* g);
int32_t   svh_grid_clear(svh_grid* g);
int32_t   svh_grid_set_window(svh_grid* g, float x0, float z0);   /* moves the window with the vehicle; clears */

/* n points (x, y, z, val), on the host or (on_device) in device memory, 16-byte aligned there */
int32_t   svh_grid_add_points(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device);
/* the view's whole store, device to device, no host copy; an empty view: SVH_OK, nothing changes */
int32_t   svh_grid_add_view(svh_grid* g, svh_view* v);
/* totals since the last clear; added = binned + overhead + outside + unplaced */
int32_t   svh_grid_get_stats(svh_grid* g, svh_grid_stats* stats);

/* one plane, nx * nz elements of its type, to the host or (on_device) a device pointer */
int32_t   svh_grid_get(svh_grid* g, int32_t plane, void* out, int32_t on_device);
/* nx x nz RGB8; row 0 is the farthest row (ib = nz - 1): forward is up */
int32_t   svh_grid_render(svh_grid* g, int32_t mode, uint8_t* rgb, int32_t on_device);

#ifdef __cplusplus
}
#endif
#endif

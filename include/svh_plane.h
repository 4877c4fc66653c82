/* C-ABI of the ground-plane estimation (reference: stereomapper/planeestimation.{h,cpp}, class PlaneEstimation):
 * the road plane in disparity space, the same plane in camera coordinates, the camera pitch and the 4x4 levelling
 * transform StereoThread uses as _H_init, found by RANSAC over a lattice of the left disparity map.  Exported by
 * libsvhip.so; the drop-in C++ class is include/planeestimation.h.
 *
 * Two deliberate deviations from the reference: an empty list returns SVH_PLANE_NO_POINTS (the
 * reference divides by zero), and the draws come from a private generator that reproduces glibc's srand(seed) /
 * rand() sequence instead of reseeding the process-wide rand().                                                   */
#ifndef SVH_PLANE_H
#define SVH_PLANE_H
#include <stdint.h>

#include "svh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* positive statuses of svh_plane_estimate: the outputs are what the reference leaves in these cases */
#define SVH_PLANE_NO_POINTS    2  /* no lattice point with d >= 1: _plane_d, _plane_e zero, _H identity, _pitch kept  */
#define SVH_PLANE_FEW_INLIERS  3  /* the best hypothesis has <= 3 inliers: _plane_d is the LAST hypothesis' plane,
                                   * _plane_e zero, _H identity, _pitch kept                                        */

typedef struct svh_plane_params {
    int32_t num_samples;   /* 5000 */
    int32_t step_size;     /* 5: lattice step, pixels */
    int32_t max_draws;     /* 1000: draws one hypothesis may consume */
    int32_t roi[4];        /* u0, v0, u1, v1 inclusive; all -1: the reference's {0, height/3, width-1, height-1} */
    float   min_dist;      /* 50: second point from the first / third point from the line through both, pixels */
    double  d_threshold;   /* 5: inlier bound on |a u + b v + c - d| */
} svh_plane_params;
void svh_plane_params_default(svh_plane_params* p);

typedef struct svh_plane svh_plane;
svh_plane* svh_plane_create(const svh_plane_params* p);   /* NULL parameters: the defaults; NULL on bad parameters */
void       svh_plane_destroy(svh_plane*);
/* gives back what the object caches between calls (device and pinned buffers, the raw draws of the last seed); the
 * results stay, the next call allocates again.  Returns the bytes released.                                        */
int64_t    svh_plane_release(svh_plane*);

/* computeTransformationFromDisparityMap(D, width, height, step, f, cu, cv, base) with the draws of srand(seed).
 * D: host memory, or with d_on_device != 0 a device pointer (what svh_elas_process_batch_device and svh_map_add use);
 * the map is not copied then.  Returns SVH_OK, SVH_PLANE_NO_POINTS, SVH_PLANE_FEW_INLIERS or a negative SVH_ERR_*.
 * After SVH_ERR_HIP or SVH_ERR_BAD_ARG the object, _pitch included, is what it was before the call.                */
int32_t svh_plane_estimate(svh_plane*, const float* D, int32_t d_on_device, int32_t width, int32_t height,
                           int32_t step, float f, float cu, float cv, float base, uint32_t seed);
/* n objects (distinct, created with equal parameters), n device-resident maps of equal size, one launch per kernel
 * over all maps.  Object i gets the result of the single call on D[i] with seeds[i]; status[i] (may be NULL) its
 * status.  Returns SVH_OK or a negative SVH_ERR_*, after which no object has changed.                             */
int32_t svh_plane_estimate_batch(svh_plane* const* p, const float* const* D, int32_t n, int32_t width,
                                 int32_t height, int32_t step, float f, float cu, float cv, float base,
                                 const uint32_t* seeds, int32_t* status);

void  svh_plane_get_plane_dsi(svh_plane*, double abc[3]);         /* getPlaneDsi() */
void  svh_plane_get_plane_euclidean(svh_plane*, double abc[3]);   /* getPlaneEuclidean() */
void  svh_plane_get_transformation(svh_plane*, double H[16]);     /* getTransformation(), row major */
float svh_plane_get_pitch(svh_plane*);                            /* getPitch() */

/* Parity taps of the last successful call (as svh_vo_mono_get_votes).  Each returns the full count and copies at
 * most `cap` entries.
 *   list        the lattice list, 3 floats (u, v, d) per entry, in the reference's order
 *   hypotheses  per hypothesis: plane (3 doubles), draws consumed, votes
 *   best        *best = index of the winning hypothesis (-1: none); its inlier indices into the list           */
int32_t svh_plane_get_list(svh_plane*, float* uvd, int32_t cap);
int32_t svh_plane_get_hypotheses(svh_plane*, double* planes, int32_t* draws, int32_t* votes, int32_t cap);
int32_t svh_plane_get_best(svh_plane*, int32_t* best, int32_t* inliers, int32_t cap);

/* ms of the last call by phase, recorded only after svh_plane_set_timing(p, 1).  ms7: [0] host, start to the first
 * sync (upload of a host map, lattice kernel, list copy-back), [1] the draw walk on the host, [2] host, sample upload
 * to the second sync (fit, vote, select, copy-back), [3] final refit and planeDsiTo3d on the host, [4] the whole
 * call, [5] / [6] the device time of phase [0] / [2] between HIP events.  A batch records on its first object.   */
void    svh_plane_set_timing(svh_plane*, int32_t on);
int32_t svh_plane_get_timing(svh_plane*, double* ms7);

#ifdef __cplusplus
}
#endif
#endif /* SVH_PLANE_H */

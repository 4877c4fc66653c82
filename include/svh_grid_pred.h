/* PREDICTION: the tracks of the ground grid's objects (svh_grid_obj.h) carried ahead at constant velocity, and the rollouts
 * (svh_grid.h, "ROLLOUT") scored against where the objects will be.  Included by svh_grid.h; the entries are declared here, in a
 * header of their own, with the cache contract of this layer stated below.  The arithmetic is
 * stereo-vision_amd/csrc/grid_pred_core.h (restated in tests/grid_pred_ref.py): integers throughout; PRED is an OR, the statistics
 * integer sums, the cut a first index, so no byte depends on launch shape or scheduling.
 *
 * Time is cut into `slots` SLOTS, one bit each of a 32-bit word: slot s stands for the time s * stride steps after the last
 * svh_grid_objects_step.  The PREDICTING tracks are those of the table as the last step left it that have a label and, if only_moving,
 * the MOVING flag.  Track i is displaced at slot s by D_i(s) = rdiv(v16 s stride, 16) per axis (to the nearest cell, halves towards
 * +infinity), and its cells are inflated by a square of radius m(s) = min(16, margin + ((s grow16) >> 4)).
 * PRED has one uint32 per cell of the ID FRAME -- the ID plane of the last step, under the offsets it was written under, not under
 * the window's: bit s of cell p is set iff a cell q of the frame holds the id of a predicting track i, q + D_i(s) lies inside the
 * frame and p is within m(s) cells (Chebyshev) of it.  Shifted cells outside the frame are dropped before the inflation, which does
 * not leave the frame either.  Bits at or above `slots` are 0; before the first step and after anything that empties the tracks
 * PRED is all 0.  PRED is addressed by GLOBAL cell, like the tracks: a scroll between the step and a query needs no hook, and a
 * global cell outside the ID frame reads 0.
 * Pose t of a candidate is at slot s_t = min(slots - 1, rdiv(t + 1, poses_per_step stride)).
 *
 * CACHE.  PRED and its statistics are a cached function of the track state (the table and the ID plane) and the parameters of this
 * layer, not of the accumulators: they are computed by the first entry that asks and kept until svh_grid_objects_step (a failed one
 * included), svh_grid_objects_reset, svh_grid_set_objects, svh_grid_set_window or svh_grid_set_predict.  Nothing else invalidates
 * them -- no add, observation, scroll, follow or clear, and no other layer's parameters, goals or candidates.  After SVH_ERR_HIP in
 * an entry of this layer the accumulated grid, the tracks and every other layer are untouched; PRED is invalid and computed again by
 * the next call.  svh_grid_render_roll keeps drawing the last svh_grid_roll_score only.
 * A moving object's present cells stay lethal in COST: this layer does not release them (svh_grid_time.h does, in a cost map of its own).
 */
#ifndef SVH_GRID_PRED_H
#define SVH_GRID_PRED_H

#include "svh_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svh_grid_pred_params {
    int32_t slots;             /* 8: time slots; 1..32 */
    int32_t stride;            /* 1: track steps per slot; 1..64 */
    int32_t poses_per_step;    /* 1: candidate poses per track step; 1..1024 */
    int32_t margin;            /* 1: cells of square inflation at slot 0; 0..16 */
    int32_t grow16;            /* 0: sixteenths of a cell the inflation grows per slot; 0..256 */
    int32_t only_moving;       /* 1: only tracks with the MOVING flag predict; 0 or 1 */
} svh_grid_pred_params;

void      svh_grid_pred_params_default(svh_grid_pred_params* p);
/* SVH_ERR_BAD_ARG, nothing changed: a value out of its range.  Otherwise PRED is computed again by the next read */
int32_t   svh_grid_set_predict(svh_grid* g, const svh_grid_pred_params* p);
int32_t   svh_grid_get_predict(svh_grid* g, svh_grid_pred_params* p);
/* PRED, uint32 laid out as the plane of svh_grid_get_track_plane, under the offsets off[0], off[1] of the ID frame (off may be NULL);
 * all 0 before the first step.  A device array is 4-byte aligned */
int32_t   svh_grid_get_pred_plane(svh_grid* g, uint32_t* out, int32_t on_device, int32_t off[2]);
/* out[0] predicting tracks, out[1] source cells (the ID cells of predicting tracks), out[2] PRED cells with any bit set, out[3] kernel
 * launches of the computation that produced them, a constant of the build: 4, 2 when every radius is 0 (the inflation is skipped),
 * 0 while the table is empty (PRED is a fill) */
int32_t   svh_grid_get_pred_stats(svh_grid* g, int64_t out[4]);
/* per pose (ga, gb, k) of n poses the OR of PRED over the footprint cells of heading k: the slots at which the vehicle, standing
 * there, overlaps a predicted object.  A footprint cell outside the ID frame contributes 0; neither the window nor COST is looked
 * at.  The roll parameters must be set.  A heading outside 0..8 m - 1: SVH_ERR_BAD_ARG for host arrays, mask 0 for device arrays */
int32_t   svh_grid_footprint_pred(svh_grid* g, const int32_t* poses, int64_t n, int32_t on_device, uint32_t* out);
#define SVH_GRID_ROLL_CUT_OBJECT  4   /* status: the footprint met a predicted object at the pose's slot */
#define SVH_GRID_ROLL_PRED_RECORD 6   /* int32 per record: the five fields of SVH_GRID_ROLL_RECORD, then slot: the slot of the cut pose
                                         when the status is 4, -1 otherwise */
/* svh_grid_roll_score with one more cut: at pose t, after the window (status 2) and the cost (status 1), bit s_t of the pose's
 * footprint prediction cuts with status 4.  recs (6 K int32) and scores (K int64) may be NULL.  Preconditions and refusals are those
 * of svh_grid_roll_score; one host wait.  With PRED all 0 the first five fields, the scores and the best are svh_grid_roll_score's */
int32_t   svh_grid_roll_score_pred(svh_grid* g, const double anchor_xyz[3], int32_t set, int32_t* recs, int64_t* scores, int32_t on_device,
                                   int32_t* best);
/* svh_grid_render(mode) with every window cell whose PRED word is non-zero drawn (255, 8 s, 255 - 8 s), s the lowest set slot */
int32_t   svh_grid_render_pred(svh_grid* g, int32_t mode, uint8_t* rgb, int32_t on_device);

#ifdef __cplusplus
}
#endif
#endif

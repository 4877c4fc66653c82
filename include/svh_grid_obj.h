/* OBJECTS: the obstacles of the ground grid (svh_grid.h) as things, and their tracks from frame to frame.  Included by svh_grid.h;
 * the entries are declared here, in a header of their own, with the cache contract of this layer stated below (the table in
 * DESIGN.md, "Caches: who invalidates what", speaks of the entries of svh_grid.h proper).  The arithmetic is
 * stereo-vision_amd/csrc/grid_obj_core.h (restated in tests/grid_obj_ref.py): integers throughout, every accumulator a commutative
 * update and every choice the minimum or maximum of unique keys, so no byte depends on launch shape or scheduling.
 *
 * A cell is an OBJECT cell when its class (bits 0-1 of STATE) is obstacle.  Components are the 8-connected sets of object cells.
 * LABEL is -1 elsewhere and the LOWEST window index ib * nx + ia of the cell's component on them.  A component is KEPT when
 * min_size <= size <= max_size and the largest HMAX over its cells is at least min_height (compared on the float; equal is kept);
 * LARGE when size > max_size: structure such as walls and hedges, labelled, flagged and counted, not in the table; LOW when only
 * the height fails.  Each kept component has one record of SVH_GRID_OBJ_RECORD int32, the records in ascending order of label; the
 * RANK of an object is its position in the table.  c16 is the centroid in sixteenths of a global cell, a cell's centre at 16 i + 8:
 * per axis floor(16 (2 sum + size) / (2 size)) + 16 offset.  hmax_bits are the float bits of the largest HMAX (HMAX of an obstacle
 * cell is positive, so the bits order as integers), points the sum of COUNT saturated at INT32_MAX.
 * The planes, the table and the statistics are a cached function of the accumulators, the window's offsets and the parameters of
 * this layer: they are computed by the first entry that asks and kept until one of the three changes.  Nothing else invalidates
 * them -- not the traversability, plan, frontier, roll, explore or align parameters, not the goals or candidates -- and the
 * layer needs no traversability.  After SVH_ERR_HIP in an entry of this layer the accumulated grid and every other layer are
 * untouched; the objects are invalid and computed again by the next call, and after a failed step the tracks are EMPTY.
 *
 * TRACKS are state that only svh_grid_objects_step advances.  The object keeps the track table, the ID plane of the last step (per
 * window cell the id of the track of the kept component that covered it, or -1) and the offsets the plane was written under.
 * Cells are compared as GLOBAL cells, so scrolling the window between steps keeps the tracks; a global cell outside the previous
 * window has no track.  svh_grid_clear leaves the tracks alone (a caller who rebuilds the grid per frame can track);
 * svh_grid_set_window, svh_grid_set_objects and svh_grid_objects_reset empty them and restart the ids at 0.  A step is a pure
 * function of the object table, the LABEL plane, the previous ID plane with its offsets and the previous track table:
 *   OVERLAP  O[i, t] is the number of cells of kept object i whose global cell held track t.  Pairs with O >= min_overlap count.
 *            Object i claims the track with the largest O, ties to the lowest id; track t claims the object with the largest O,
 *            ties to the lowest rank; mutual claims match (BY_OVERLAP).  An object with two or more counting tracks sets MERGED
 *            on the track it ends up with; a track with two or more counting objects has SPLIT.
 *   GATE     when gate > 0, one round over the objects and tracks left unmatched: a track's prediction is c16 + v16 (missed + 1),
 *            d2 the squared distance in sixteenths from it to the object's c16; pairs with d2 <= (16 gate)^2 count.  An object
 *            picks the least d2, ties to the lowest id; a track the least d2, ties to the lowest rank; mutual picks match (BY_GATE).
 *   UPDATE   matched: age++, raw = rdiv(c16_now - c16_before, missed + 1) per axis (rounded to nearest, halves up); at the first
 *            match v16 = raw, afterwards v16 += rdiv(raw - v16, 1 << smooth_shift); missed = 0.  Unmatched: missed++, label -1,
 *            MISSED; dropped once missed > max_missed; size, c16, v16 stay.  An unmatched object becomes a NEW track with the next
 *            id, in ascending rank, v16 = 0, birth = c16, while the table has room; otherwise its assign is -2 and it is counted
 *            as untracked.  MOVING: age >= min_age and the squared distance from the birth position >= (16 move_cells)^2.
 * The flags of a record are those of the last step.  The track table is in ascending order of id.
 */
#ifndef SVH_GRID_OBJ_H
#define SVH_GRID_OBJ_H

#include "svh_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svh_grid_obj_params {
    int32_t min_size;          /* 4: the smallest component that is kept; 1..2^26 */
    int32_t max_size;          /* 4096: larger components are structure; min_size..2^26 */
    float   min_height;        /* 0.3: a kept component has a cell with HMAX >= this; finite, >= 0 */
    int32_t max_tracks;        /* 1024: capacity of the track table; 1..4096 */
    int32_t min_overlap;       /* 1: cells of overlap that count as evidence; >= 1 */
    int32_t gate;              /* 4: cells; the reach of the centroid fallback, 0..64, 0 = off */
    int32_t max_missed;        /* 2: consecutive steps a track may go unmatched; 0..255 */
    int32_t min_age;           /* 3: matches before a track can be MOVING; 0..2^30 */
    int32_t move_cells;        /* 2: cells from the birth position that make a track MOVING; 1..8192 */
    int32_t smooth_shift;      /* 1: the velocity follows by 1 / 2^shift of the difference per match; 0..4 */
} svh_grid_obj_params;

void      svh_grid_obj_params_default(svh_grid_obj_params* p);
/* SVH_ERR_BAD_ARG, nothing changed: a value out of its range.  Otherwise the objects are computed again by the next read and the
 * tracks are emptied */
int32_t   svh_grid_set_objects(svh_grid* g, const svh_grid_obj_params* p);
int32_t   svh_grid_get_objects_params(svh_grid* g, svh_grid_obj_params* p);
/* planes of svh_grid_get_obj_plane, laid out as those of svh_grid_get */
#define SVH_GRID_OBJ_FLAGS 0    /* uint8: bit 0 object cell, bit 1 in a kept component, bit 2 in a component above max_size */
#define SVH_GRID_OBJ_LABEL 1    /* int32: -1 off the objects, else the lowest index of the component; a device array is 4-byte aligned */
int32_t   svh_grid_get_obj_plane(svh_grid* g, int32_t plane, void* out, int32_t on_device);
#define SVH_GRID_OBJ_RECORD 10  /* int32 per record: label, size, ga_min, gb_min, ga_max, gb_max, c16_a, c16_b, hmax_bits, points */
/* *n = the kept components; the first min(*n, cap) records, in ascending order of label, to recs (host memory) */
int32_t   svh_grid_get_objects(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n);
/* out[0] object cells, out[1] components, out[2] kept, out[3] cells in kept components, out[4] too large, out[5] too low, out[6] kernel
 * launches of the computation that produced them (a constant of the build) */
int32_t   svh_grid_get_object_stats(svh_grid* g, int64_t out[7]);

/* one step of the tracks on the objects as they are (computed first if they are not current).  *n_obj = the kept objects;
 * assign[i], for the first min(*n_obj, cap) of them by rank, is the id of the object's track or -2 (the table was full).  assign
 * may be NULL with cap 0.  One host wait after the objects are current.  SVH_ERR_UNSUPPORTED, nothing changed: 2^31 - 1 steps */
int32_t   svh_grid_objects_step(svh_grid* g, int32_t* assign, int64_t cap, int64_t* n_obj);
/* empties the tracks and restarts the ids at 0 */
int32_t   svh_grid_objects_reset(svh_grid* g);
#define SVH_GRID_TRACK_RECORD 14 /* int32 per record: id, flags, age, missed, label (-1 when missed), size, c16_a, c16_b, v16_a, v16_b,
                                    birth c16_a, birth c16_b, the winning overlap, hmax_bits */
#define SVH_GRID_TRACK_NEW        1
#define SVH_GRID_TRACK_BY_OVERLAP 2
#define SVH_GRID_TRACK_BY_GATE    4
#define SVH_GRID_TRACK_MISSED     8
#define SVH_GRID_TRACK_MOVING     16
#define SVH_GRID_TRACK_MERGED     32
#define SVH_GRID_TRACK_SPLIT      64
/* *n = the tracks; the first min(*n, cap) records, in ascending order of id, to recs (host memory) */
int32_t   svh_grid_get_tracks(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n);
/* the ID plane of the last step, int32 laid out as the planes of svh_grid_get under the offsets off[0], off[1] it was written under
 * (off may be NULL); all -1 before the first step.  A device array is 4-byte aligned */
int32_t   svh_grid_get_track_plane(svh_grid* g, int32_t* out, int32_t on_device, int32_t off[2]);
/* out[0] steps since the tracks were last emptied, out[1] tracks in the table; of the last step: out[2] matched by overlap, out[3]
 * matched by the gate, out[4] new, out[5] missed and kept, out[6] dropped, out[7] objects left untracked */
int32_t   svh_grid_get_track_stats(svh_grid* g, int64_t out[8]);
/* svh_grid_render (class colours) with the objects over it: the cells of a kept component in the colour of the track that the ID
 * plane of the last step holds at the cell's global cell -- a fixed function of the id, at full brightness when the track is
 * MOVING, at half otherwise; (128, 0, 0) where it holds none -- the cells of a large component (128, 128, 128); then, per track
 * with a label, the cell of c16 + 8 v16 (255, 255, 0), then the cell of c16 (255, 255, 255) */
int32_t   svh_grid_render_objects(svh_grid* g, uint8_t* rgb, int32_t on_device);

#ifdef __cplusplus
}
#endif
#endif

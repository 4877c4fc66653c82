// Between csrc/grid_engine.cpp (host) and csrc/grid_kernels.hip / csrc/grid_trav_kernels.hip / csrc/grid_plan_kernels.hip /
// csrc/grid_front_kernels.hip / csrc/grid_obj_kernels.hip / csrc/grid_roll_kernels.hip / csrc/grid_pred_kernels.hip /
// csrc/grid_explore_kernels.hip / csrc/grid_align_kernels.hip / csrc/grid_dyn_kernels.hip / csrc/grid_pose_kernels.hip /
// csrc/grid_archive_kernels.hip / csrc/grid_time_kernels.hip: the launches of the
// ground grid (include/svh_grid.h).
#ifndef SVH_GRID_INTERNAL_H
#define SVH_GRID_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include "grid_align_core.h"
#include "grid_archive_core.h"
#include "grid_core.h"
#include "grid_dyn_core.h"
#include "grid_explore_core.h"
#include "grid_front_core.h"
#include "grid_obj_core.h"
#include "grid_plan_core.h"
#include "grid_pose_core.h"
#include "grid_pred_core.h"
#include "grid_roll_core.h"
#include "grid_time_core.h"

namespace svh {
namespace grid {

// The accumulators of the cells, structure of arrays, nx * nz elements each: the empty grid is kmin all ones and every
// other plane zero, so clearing is two byte fills.  A cell's accumulators lie at its SLOT (grid_core.h, slot_at).
struct Cells {
    uint32_t* kmin;
    uint32_t* kmax;
    int32_t* count;
    int32_t* overhead;
    unsigned long long* hsum;   // int64 in two's complement
    unsigned long long* vsum;
    int32_t* pass;              // rays that passed the cell (svh_grid_add_*_from)
};
// bytes of the seven accumulators of one cell; the engine lays the planes out kmin first, then those that clear to zero
constexpr size_t CELL_BYTES = 36;

constexpr uint32_t BIN_BLOCK = 256;          // k_grid_bin: one lane per point
constexpr uint32_t BIN_MAX_BLOCKS = 2048;    // the launch is capped here; beyond 2048 * 256 points the lanes stride
constexpr uint32_t FIN_BLOCK = 256;          // k_grid_finalise, k_grid_render, k_grid_enter: one lane per cell
constexpr uint32_t RAY_BLOCK = 256;          // k_grid_rays: four waves
constexpr int STAT_RAY_CELLS = 4;            // stats[4]: the sum of pass increments; stats[0..3] are per grid::Fate
constexpr int STAT_WORDS = 5;
constexpr int STAT_DYN = 5;                  // stats[5..7]: cells cleared, aged and confirmed by the observations (grid_dyn_core.h)
constexpr int STAT_ALL = 8;                  // the words the engine allocates and clears

struct BinJob {
    Params prm;
    const float4* pts;          // n points (x, y, z, val), 16-byte aligned
    int64_t n;
    Cells cells;
    unsigned long long* stats;  // [fate]: points of each grid::Fate, added to
    int32_t* ends = nullptr;    // svh_grid_add_*_from: nx * nz counts in logical order, this call's low points per cell,
                                // added to; nullptr: the plain add, which touches no such plane
};
void launch_bin(hipStream_t s, const BinJob& j);

// the rays of one svh_grid_add_*_from: one line per cell with ends != 0, from the origin's cell, weighted by ends
struct RayJob {
    Params prm;
    uint32_t origin;            // the logical index of the origin's cell
    int32_t* ends;              // read, and left all zero
    int32_t* pass;              // by slot, added to
    unsigned long long* ray_cells;   // the sum of pass increments, added to
};
void launch_rays(hipStream_t s, const RayJob& j);

// svh_grid_scroll: the cells of the strips that enter the window become the empty cell.  `prm` has the NEW offsets; the
// window moved by (da, db) with |da| < nx and |db| < nz, not both zero.
struct EnterJob {
    Params prm;
    int32_t da, db;
    Cells cells;
};
void launch_enter(hipStream_t s, const EnterJob& j);

// accumulators by slot -> finished planes in logical order
struct FinalJob {
    Params prm;
    Cells cells;
    int32_t* count;
    int32_t* overhead;
    int32_t* pass;
    float* hmin;
    float* hmax;
    float* hmean;
    uint8_t* intensity;
    uint8_t* cls;
    uint8_t* state;
};
void launch_finalise(hipStream_t s, const FinalJob& j);

struct RenderJob {
    Params prm;
    int32_t mode;               // a grid::Mode, M_LOCAL included
    const int32_t* count;       // the finished planes, logical order
    const int32_t* pass;
    const float* hmin;
    const float* hmax;
    const float* hmean;
    const uint8_t* intensity;
    const uint8_t* cls;
    uint8_t* rgb;               // nx * nz * 3 bytes, row 0 = ib nz - 1
};
void launch_render(hipStream_t s, const RenderJob& j);

// The traversability layer (csrc/grid_trav_kernels.hip): finished planes in logical order -> FLAGS, DIST2, COST.
constexpr uint32_t TRAV_BLOCK = 256;         // k_grid_trav_mask, k_grid_render_cost: one lane per cell; k_grid_dist_rows:
                                             // one workgroup per 256 cells of a row
constexpr uint32_t COLS_BLOCK = 64;          // k_grid_dist_cols: one lane per column and chunk of rows
constexpr int32_t COLS_CHUNK = 32;           // ... of this many rows
constexpr uint32_t ROWS_TILE = TRAV_BLOCK + 2 * (uint32_t)MAX_REACH;   // the tile of g and its halo, uint16 each

struct TravJob {
    TravParams trv;
    int32_t nx, nz;
    const uint8_t* cls;         // the finished planes
    const float* hmean;
    const uint8_t* state;
    const uint8_t* table;       // reach^2 + 1 cost bytes
    uint8_t* flags;             // nx * nz each
    uint16_t* g;                // the column distances, scratch
    int32_t* dist2;
    uint8_t* cost;
};
// the three launches: mask, columns, rows
void launch_trav(hipStream_t s, const TravJob& j);
// the last two of them on the FLAGS plane the job names: of the job they read trv.reach, nx, nz, cls, table, flags, g, dist2 and cost
void launch_trav_dist(hipStream_t s, const TravJob& j);

struct RenderCostJob {
    int32_t nx, nz;
    const uint8_t* cost;
    const uint8_t* flags;
    uint8_t* rgb;               // nx * nz * 3 bytes, row 0 = ib nz - 1
};
void launch_render_cost(hipStream_t s, const RenderCostJob& j);

// The planner (csrc/grid_plan_kernels.hip): the finished COST plane and the goals -> POT, DIR, a path.
#ifndef SVH_PLAN_TILE
#define SVH_PLAN_TILE 16
#endif
constexpr int32_t PLAN_TILE = SVH_PLAN_TILE;     // k_grid_plan_relax: one workgroup per active tile of this side; 16, 32 and 64
                                                 // were measured (grid_plan_kernels.hip)
constexpr uint32_t PLAN_BLOCK = 256;
static_assert(PLAN_TILE == 16 || PLAN_TILE == 32 || PLAN_TILE == 64, "a tile is whole passes of 256 lanes");
// the control words on the device: the lengths of the tile lists of rounds r, r + 1, r + 2 at [r % 3], the rounds whose list
// was not empty, the goals that counted, and (64 bits at word 6) the cells whose POT is not FAR
enum PlanCtl { CTL_LEN = 0, CTL_ROUNDS = 3, CTL_COUNTED = 4, CTL_REACHED = 6, CTL_WORDS = 8 };

struct PlanJob {
    PlanParams pln;
    int32_t nx, nz, oa, ob;
    const uint8_t* cost;        // the finished COST plane
    uint16_t* price;            // nx * nz each, logical order
    int32_t* pot;
    uint8_t* dir;
    const int32_t* goals;       // n_goals global cells (ga, gb)
    int32_t n_goals;
    uint32_t* lists;            // 2 * tiles: the tiles of this round and of the next
    uint32_t* flags;            // 2 * tiles: a tile is in that list
    uint32_t* ctl;              // CTL_WORDS
};
inline uint32_t plan_tiles_x(const PlanJob& j) { return ((uint32_t)j.nx + (uint32_t)PLAN_TILE - 1) / (uint32_t)PLAN_TILE; }
inline uint32_t plan_tiles_y(const PlanJob& j) { return ((uint32_t)j.nz + (uint32_t)PLAN_TILE - 1) / (uint32_t)PLAN_TILE; }
// the price plane and POT all FAR, then the goals: POT 0 where one counts, its tile and those it touches on list 0.  `flags`
// and `ctl` are all zero before
void launch_plan_seed(hipStream_t s, const PlanJob& j);
// round `round` over the first `blocks` entries of its list (the kernel reads the list's true length; blocks >= 1)
void launch_plan_relax(hipStream_t s, const PlanJob& j, uint32_t round, uint32_t blocks);
void launch_plan_dir(hipStream_t s, const PlanJob& j);
// the walk from the window cell (a, b): out[0] a PathStatus, out[1] the cells of the path, out[2] POT of the start; the first
// min(out[1], cap) cells to `cells`
void launch_plan_walk(hipStream_t s, const PlanJob& j, int32_t a, int32_t b, int32_t* cells, int64_t cap, int64_t* out);
// n global cells drawn into an image of svh_grid_render_cost's layout: a path, or (goals) only those that count
void launch_plan_overlay(hipStream_t s, const PlanJob& j, const int32_t* cells, int64_t n, bool goals, uint8_t* rgb);

// The pose planner (csrc/grid_pose_kernels.hip): the finished COST plane, the footprint table and the goal states -> CF, PPOT, PDIR,
// a pose path.  The tile lists, their flags and the control words are the planner's (PlanCtl), over tiles of POSE_TILE x POSE_TILE
// cells x 8 headings.
constexpr int32_t POSE_TILE = 16;                // k_grid_pose_relax: one workgroup per active tile, one lane per cell, 8 states each
constexpr uint32_t POSE_BLOCK = 256;
static_assert(POSE_TILE * POSE_TILE == (int32_t)POSE_BLOCK, "a tile is one pass of 256 lanes");
constexpr int32_t FOOT_TILE = 16;                // k_grid_pose_foot: one workgroup per tile of cells and heading, one lane per cell
constexpr uint32_t FOOT_LDS = 32 * 1024;         // ... the bytes of r(COST) it stages at most (grid_pose_kernels.hip)

struct PoseJob {
    PoseParams pp;
    int32_t stop_cost, unknown_cost, m;   // of the rollouts
    int32_t nx, nz, oa, ob;
    const uint8_t* cost;        // the finished COST plane
    const int2* offs;           // the footprint table on the device
    const int32_t* start;
    int32_t box[POSE_HEADINGS][4];   // per planning heading the bounding box of its list: min da, max da, min db, max db
    uint8_t* cf;                // 8 * nx * nz each, heading-major
    uint16_t* price;
    int32_t* pot;
    uint8_t* dir;
    const int32_t* goals;       // n_goals triples (ga, gb, d)
    int32_t n_goals;
    uint32_t* lists;            // 2 * tiles
    uint32_t* flags;            // 2 * tiles
    uint32_t* ctl;              // CTL_WORDS
};
inline uint32_t pose_tiles_x(const PoseJob& j) { return ((uint32_t)j.nx + (uint32_t)POSE_TILE - 1) / (uint32_t)POSE_TILE; }
inline uint32_t pose_tiles_y(const PoseJob& j) { return ((uint32_t)j.nz + (uint32_t)POSE_TILE - 1) / (uint32_t)POSE_TILE; }
// the eight CF planes: one launch
void launch_pose_foot(hipStream_t s, const PoseJob& j);
// the price planes from CF and PPOT all FAR, then the goals: PPOT 0 where one counts, its tile and those it touches on list 0.
// `flags` and `ctl` are all zero before
void launch_pose_seed(hipStream_t s, const PoseJob& j);
// round `round` over the first `blocks` entries of its list (the kernel reads the list's true length; blocks >= 1)
void launch_pose_relax(hipStream_t s, const PoseJob& j, uint32_t round, uint32_t blocks);
void launch_pose_dir(hipStream_t s, const PoseJob& j);
// the walk from the window state (a, b, d): out[0] a PathStatus, out[1] the poses of the path, out[2] PPOT of the start; the first
// min(out[1], cap) poses to `poses`
void launch_pose_walk(hipStream_t s, const PoseJob& j, int32_t a, int32_t b, int32_t d, int32_t* poses, int64_t cap, int64_t* out);
// n triples drawn into an image of svh_grid_render_cost's layout by their cells: a path, or (goals) only the goals that count
void launch_pose_overlay(hipStream_t s, const PoseJob& j, const int32_t* triples, int64_t n, bool goals, uint8_t* rgb);

// The frontiers (csrc/grid_front_kernels.hip): the finished STATE and COST planes -> FRONT, LABEL and the table of components.
#ifndef SVH_FRONT_TILE
#define SVH_FRONT_TILE 16
#endif
constexpr int32_t FRONT_TILE = SVH_FRONT_TILE;   // k_grid_front_tile: one workgroup per tile of this side, one lane per cell
constexpr uint32_t FRONT_BLOCK = 256;
static_assert(FRONT_TILE * FRONT_TILE == (int32_t)FRONT_BLOCK, "a tile is one pass of 256 lanes");
constexpr uint32_t FRONT_SCAN_BLOCK = 1024;      // the ordered compactions count and scatter in blocks of this many
constexpr uint32_t FRONT_UNION_TRIES = 1024;     // a union gives up after this many lost atomics (each lost to another union's link)
// the launches of one computation, a constant of the build: mask; tile, merge, flatten; roots counted, scanned | scattered;
// accumulate, centroids, representatives; kept counted, scanned, records; flags
constexpr int32_t FRONT_LABEL_LAUNCHES = 3, FRONT_LAUNCHES = 14;
// the control words on the device, 64 bits each
enum FrontCtl { FC_CELLS = 0, FC_COMPONENTS, FC_KEPT, FC_KEPT_CELLS, FC_UNSETTLED, FC_WORDS = 8 };
// bytes per component of the accumulators: sum (2 x 64 bits), rep (64 bits), size, box max (2), box min (2), centroid (2)
constexpr size_t FRONT_COMP_BYTES = 52;

struct FrontJob {
    FrontParams frp;
    int32_t nx, nz, oa, ob;
    const uint8_t* state;       // the finished planes
    const uint8_t* cost;
    uint8_t* flags;             // nx * nz each, logical order
    int32_t* label;             // ... the parent plane of the union-find until it is flattened
    int32_t* blockcnt;          // ceil(nx * nz / FRONT_SCAN_BLOCK) counts, then offsets; used again for the components
    unsigned long long* ctl;    // FC_WORDS, all zero before
    // what exists once the number of components is known (front_table)
    int32_t n_comp = 0;
    int32_t* roots = nullptr;   // n_comp labels, ascending
    uint8_t* acc = nullptr;     // FRONT_COMP_BYTES per component, laid out by front_acc below
    int32_t* recs = nullptr;    // FRONT_REC per kept component
};
inline uint32_t front_tiles_x(const FrontJob& j) { return ((uint32_t)j.nx + (uint32_t)FRONT_TILE - 1) / (uint32_t)FRONT_TILE; }
inline uint32_t front_tiles_y(const FrontJob& j) { return ((uint32_t)j.nz + (uint32_t)FRONT_TILE - 1) / (uint32_t)FRONT_TILE; }
inline size_t front_blocks(const FrontJob& j) { return ((size_t)j.nx * (size_t)j.nz + FRONT_SCAN_BLOCK - 1) / FRONT_SCAN_BLOCK; }
struct FrontAcc {
    unsigned long long* sum;    // 2 per component: ia, ib
    unsigned long long* rep;    // the least front_key
    int32_t* size;
    int32_t* bmax;              // 2 per component
    int32_t* bmin;
    int32_t* cen;               // the centroid in window cells
};
inline FrontAcc front_acc(uint8_t* p, size_t n) {
    return FrontAcc{(unsigned long long*)p, (unsigned long long*)(p + 16 * n), (int32_t*)(p + 24 * n), (int32_t*)(p + 28 * n),
                    (int32_t*)(p + 36 * n), (int32_t*)(p + 44 * n)};
}
// Each returns the kernels it launched.  mask: the frontier bit, LABEL = own index or -1, the count of frontier cells.
int32_t launch_front_mask(hipStream_t s, const FrontJob& j);
// LABEL holding own index or -1 -> the lowest index of the component: tile, merge, flatten
int32_t launch_front_label(hipStream_t s, const FrontJob& j);
// the roots counted per block and scanned: ctl[FC_COMPONENTS]
int32_t launch_front_count(hipStream_t s, const FrontJob& j);
// with n_comp, roots, acc (sum, size and box max zero, rep all ones, box min 0x7F bytes) and recs: everything else
int32_t launch_front_table(hipStream_t s, const FrontJob& j);
// the frontier cells drawn over an image of svh_grid_render_cost's layout
void launch_front_overlay(hipStream_t s, int32_t nx, int32_t nz, const uint8_t* flags, uint8_t* rgb);
// The labelling and the ordered compaction serve any plane of the form "own index or -1" (the objects use them too): of a job
// they read nx, nz, label, blockcnt, ctl, n_comp and roots alone.  The roots scattered in ascending order, after
// launch_front_count; one launch
int32_t launch_front_roots(hipStream_t s, const FrontJob& j);
// slot[i] = the position of element i among those of n with mark[i] != 0, -1 for the others; *total = how many are marked.
// blockcnt has room for ceil(n / FRONT_SCAN_BLOCK) counts.  Three launches
int32_t launch_front_rank(hipStream_t s, uint32_t n, const int32_t* mark, int32_t* blockcnt, unsigned long long* total, int32_t* slot);

// The objects and their tracks (csrc/grid_obj_kernels.hip): the finished STATE, HMAX and COUNT planes -> FLAGS, LABEL and the table
// of kept components; then, per step, the overlap of the components with the ID plane of the step before -> the track table.
constexpr uint32_t OBJ_BLOCK = 256;
constexpr unsigned OBJ_MASK_BLOCKS = 2048;       // k_grid_obj_mask: the launch is capped here; beyond 2048 * 256 cells the lanes stride
constexpr uint32_t OBJ_UPDATE_BLOCK = 1024;      // k_grid_obj_update: one workgroup
// the launches of one computation of the objects, a constant of the build: mask; tile, merge, flatten; roots counted, scanned |
// scattered; accumulate, verdicts; kept counted, scanned, ranked; records; flags
constexpr int32_t OBJ_LAUNCHES = 14;
// the control words beside those of FrontCtl, which the shared kernels write
enum ObjCtl { OC_LARGE = 5, OC_LOW = 6 };
// bytes per component of the accumulators: sum (2 x 64 bits), points (64 bits), size, box max (2), box min (2), biased HMAX bits, mark
constexpr size_t OBJ_COMP_BYTES = 52;
struct ObjAcc {
    unsigned long long* sum;    // 2 per component: ia, ib
    unsigned long long* pts;    // the sum of COUNT
    int32_t* size;
    int32_t* bmax;              // 2 per component
    int32_t* bmin;
    uint32_t* hbits;            // the greatest bits of HMAX ^ 0x80000000: int32 order as unsigned, all zero is below every value
    int32_t* mark;              // 1: kept
};
inline ObjAcc obj_acc(uint8_t* p, size_t n) {
    return ObjAcc{(unsigned long long*)p, (unsigned long long*)(p + 16 * n), (int32_t*)(p + 24 * n), (int32_t*)(p + 28 * n),
                  (int32_t*)(p + 36 * n), (uint32_t*)(p + 44 * n), (int32_t*)(p + 48 * n)};
}
struct ObjJob {
    ObjParams op;
    int32_t nx, nz, oa, ob;
    const uint8_t* state;       // the finished planes
    const float* hmax;
    const int32_t* count;
    uint8_t* flags;             // nx * nz each, logical order
    int32_t* label;
    int32_t* blockcnt;          // ceil(nx * nz / FRONT_SCAN_BLOCK) counts, as FrontJob's
    unsigned long long* ctl;    // FC_WORDS, all zero before
    // what exists once the number of components is known
    int32_t n_comp = 0;
    int32_t* roots = nullptr;   // n_comp labels, ascending
    uint8_t* acc = nullptr;     // OBJ_COMP_BYTES per component: all zero but box min, 0x7F bytes
    int32_t* slot = nullptr;    // n_comp: the rank of a kept component, -1 for the others
    int32_t* recs = nullptr;    // OBJ_REC per kept component
};
// Each returns the kernels it launched.  mask: FLAGS bit 0, LABEL = own index or -1, the object cells counted
int32_t launch_obj_mask(hipStream_t s, const ObjJob& j);
// the frontier layer's labelling and root count on LABEL: ctl[FC_COMPONENTS]
int32_t launch_obj_label(hipStream_t s, const ObjJob& j);
// with n_comp, roots, acc, slot and recs: everything else
int32_t launch_obj_table(hipStream_t s, const ObjJob& j);

// the control words of a step, 64 bits each
enum ObjStepCtl { SC_TRACKS = 0, SC_BY_OVERLAP, SC_BY_GATE, SC_NEW, SC_MISSED, SC_DROPPED, SC_UNTRACKED, SC_UNSETTLED, SC_WORDS };
// bytes of scratch per object and per track: claim (64 bits), counting pairs | gate pick (64 bits), match; a track has its `how` too
constexpr size_t OBJ_STEP_ZERO_OBJ = 12, OBJ_STEP_ONES_OBJ = 12, OBJ_STEP_ZERO_TRK = 16, OBJ_STEP_ONES_TRK = 12;
struct ObjStepJob {
    ObjParams op;
    int32_t nx, nz, oa, ob, poa, pob;
    const uint8_t* flags;       // of the objects that are current
    const int32_t* label;
    const int32_t* roots;
    const int32_t* slot;
    int32_t n_comp;
    const int32_t* recs;
    int32_t n_obj;
    const int32_t* prev_id;     // the ID plane of the step before
    const int32_t* prev;        // its n_prev track records
    int32_t n_prev, next_id;
    unsigned long long* keys;   // the table of pairs: `capacity` slots (a power of two), all ones before
    int32_t* counts;            // ... all zero before
    uint32_t capacity;
    uint8_t* zero;              // OBJ_STEP_ZERO_OBJ * n_obj + OBJ_STEP_ZERO_TRK * n_prev bytes, all zero before (obj_step_scratch)
    uint8_t* ones;              // OBJ_STEP_ONES_OBJ * n_obj + OBJ_STEP_ONES_TRK * n_prev bytes, all ones before
    int32_t* tracks;            // the new table: room for max_tracks records
    int32_t* assign;            // n_obj
    int32_t* id;                // the new ID plane, nx * nz
    unsigned long long* ctl;    // SC_WORDS, all zero before
};
struct ObjStepScratch {
    unsigned long long *claim_obj, *claim_trk, *pick_obj, *pick_trk;
    int32_t *cnt_obj, *cnt_trk, *how, *obj_trk, *trk_obj;
};
inline ObjStepScratch obj_step_scratch(const ObjStepJob& j) {
    const size_t no = (size_t)j.n_obj, nt = (size_t)j.n_prev;
    uint8_t *z = j.zero, *o = j.ones;
    return ObjStepScratch{(unsigned long long*)z, (unsigned long long*)(z + 8 * no), (unsigned long long*)o, (unsigned long long*)(o + 8 * no),
                          (int32_t*)(z + 8 * (no + nt)), (int32_t*)(z + 8 * (no + nt) + 4 * no), (int32_t*)(z + 8 * (no + nt) + 4 * (no + nt)),
                          (int32_t*)(o + 8 * (no + nt)), (int32_t*)(o + 8 * (no + nt) + 4 * no)};
}
// the slots of the table of pairs for a step: a power of two, at least twice the pairs that can occur
uint32_t obj_step_capacity(int64_t kept_cells, int64_t n_obj, int64_t n_prev);
// the whole step; returns the kernels it launched: 5, and 2 more when the gate is on
int32_t launch_obj_step(hipStream_t s, const ObjStepJob& j);
// the objects and tracks drawn over an image of svh_grid_render's layout: the cells by colour_obj, then the two marks per
// track with a label
void launch_obj_overlay(hipStream_t s, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* flags, const int32_t* id, int32_t id_oa,
                        int32_t id_ob, const int32_t* tracks, int32_t n_tracks, uint8_t* rgb);

// The rollouts (csrc/grid_roll_kernels.hip): the finished COST and POT planes, the footprint table and the candidates of one set ->
// F of poses, the records, the scores and the best.
constexpr uint32_t ROLL_BLOCK = 256;             // k_grid_roll_score: one workgroup per candidate, in groups of `group` lanes per pose
constexpr uint32_t ROLL_BEST_BLOCK = 1024;       // k_grid_roll_best: one workgroup

struct RollJob {
    RollParams rp;
    int32_t nx, nz, oa, ob;
    const uint8_t* cost;        // the finished COST plane
    const int32_t* pot;         // the finished POT plane; not read when w_pot == 0
    const int2* offs;           // the footprint table: the lists of (da, db), one after the other
    const int32_t* start;       // 8 m + 1: where the list of a heading begins
    int32_t group;              // roll_group(the longest list)
    const int32_t* cands = nullptr;   // the candidates of ONE set, K * T * 3
    const int32_t* lens = nullptr;    // their lengths, K
    int32_t K = 0, T = 0, ga0 = 0, gb0 = 0;   // the anchor, a global cell
    int32_t* recs = nullptr;    // ROLL_REC per candidate
    long long* scores = nullptr;
    int32_t* best = nullptr;
};
// the lanes that share a pose: the smallest power of two that holds the longest list, at most 64
int32_t roll_group(int64_t longest);
// records and scores of the K candidates, then the best: two launches whatever the scene
void launch_roll_score(hipStream_t s, const RollJob& j);
// F of n free poses (ga, gb, k), global cells
void launch_footprint_cost(hipStream_t s, const RollJob& j, const int32_t* poses, int64_t n, int32_t* out);
// the reference cells of the poses before the cut of every candidate, then of `best` (>= 0) over them, drawn into an image of
// svh_grid_render_cost's layout from the records in j.recs
void launch_roll_overlay(hipStream_t s, const RollJob& j, int32_t best, uint8_t* rgb);

// The prediction (csrc/grid_pred_kernels.hip): the track table and the ID plane of the last step -> PRED; PRED, the finished COST and
// POT planes, the footprint table and the candidates of one set -> the records with the object cut, the scores and the best.
constexpr uint32_t PRED_BLOCK = 256;             // every kernel of the layer but the column pass
constexpr unsigned PRED_MAX_BLOCKS = 2048;       // k_grid_pred_scatter: the lanes stride over the ID frame beyond 2048 * 256 cells
constexpr int32_t PRED_ROWS_TILE = (int32_t)PRED_BLOCK + 2 * PRED_MAX_RADIUS;   // k_grid_pred_rows: 256 cells of a row and their halo
constexpr int32_t PRED_COLS_X = 64, PRED_COLS_Y = 32;   // k_grid_pred_cols: the cells a workgroup of 64 x 4 lanes writes
// the launches of one computation, a constant of the build: displacements, scatter, rows, columns; without the last two when every
// radius is 0
constexpr int32_t PRED_LAUNCHES = 4, PRED_LAUNCHES_FLAT = 2;
// the control words on the device, 64 bits each: a grid::PredStat without the launches
constexpr int32_t PRED_CTL_WORDS = 4;

struct PredJob {
    PredParams pp;
    int32_t nx, nz;             // the ID frame
    const int32_t* id;          // the ID plane of the last step
    const int32_t* tracks;      // its n_tracks records, ascending by id; 1..4096
    int32_t n_tracks;
    int2* disp;                 // n_tracks * 32: D_i(s)
    int32_t* predicts;          // n_tracks: the track predicts
    uint32_t* pred;             // nx * nz, all zero before
    uint32_t* rows;             // nx * nz, scratch of the inflation; not touched when the largest radius is 0
    unsigned long long* ctl;    // PRED_CTL_WORDS, all zero before
    uint32_t ge[PRED_MAX_RADIUS + 1];   // pred_ge(pp, r)
    int32_t max_r;              // the radius of the last slot, the largest
};
// the whole computation; returns the kernels it launched
int32_t launch_pred(hipStream_t s, const PredJob& j);

// a RollJob with PRED: the frame has the window's size and its own offsets
struct RollPredJob {
    RollJob r;                  // recs: ROLL_PRED_REC per candidate
    PredParams pp;
    int32_t poa, pob;
    const uint32_t* pred;
};
// records and scores of the K candidates, then the best: two launches whatever the scene
void launch_roll_score_pred(hipStream_t s, const RollPredJob& j);
// the footprint predictions of n free poses (ga, gb, k), global cells
void launch_footprint_pred(hipStream_t s, const RollPredJob& j, const int32_t* poses, int64_t n, uint32_t* out);
// the window cells whose PRED word is not zero, drawn over an image of svh_grid_render's layout
void launch_pred_overlay(hipStream_t s, int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t poa, int32_t pob, const uint32_t* pred, uint8_t* rgb);
// k_grid_roll_best of csrc/grid_roll_kernels.hip
void launch_roll_best(hipStream_t s, const long long* scores, int32_t K, int32_t* best);

// The time layer (csrc/grid_time_kernels.hip): FLAGS and the tracks -> FLAGS'; the static planes RPRICE, RPOT, RDIR and PRED -> TPOT and
// TDIR over cell x layer, a path through them.
constexpr uint32_t TIME_BLOCK = 256;             // every kernel of the layer but the walk: one lane per cell
// the control words on the device, 64 bits each: the released cells, then a grid::TimeStat's REACHED, BLOCKED and WAITS
enum TimeCtl { TC_RELEASED = 0, TC_REACHED, TC_BLOCKED, TC_WAITS, TC_WORDS };

struct TimeReleaseJob {
    PredParams pp;
    int32_t nx, nz, oa, ob, poa, pob;   // the window and the offsets of the ID frame
    const int32_t* id;          // the ID plane of the last step
    const int32_t* tracks;      // its n_tracks records, ascending by id; 1..4096
    int32_t n_tracks;
    const uint8_t* flags;       // FLAGS
    uint8_t* out;               // FLAGS'
    unsigned long long* ctl;    // [TC_RELEASED] added to
};
void launch_time_release(hipStream_t s, const TimeReleaseJob& j);

struct TimeJob {
    PlanParams pln;
    TimeParams tp;
    PredParams pp;
    int32_t nx, nz, oa, ob, poa, pob;
    const uint16_t* price;      // RPRICE, RPOT, RDIR: nx * nz each, logical order
    const int32_t* rpot;
    const uint8_t* rdir;
    const uint32_t* pred;       // PRED of the frame of nx x nz cells under (poa, pob)
    int32_t* tpot;              // layers * nx * nz each, layer-major
    uint8_t* tdir;
    unsigned long long* ctl;    // TC_WORDS: [TC_REACHED ..] all zero before the sweep, added to
};
// k_grid_time_sweep: a workgroup owns TIME_TILE x TIME_TILE cells and TIME_K layers; it stages a box with a halo of TIME_K cells
#ifndef SVH_TIME_TILE
#define SVH_TIME_TILE 32
#endif
#ifndef SVH_TIME_K
#define SVH_TIME_K 8
#endif
constexpr int32_t TIME_TILE = SVH_TIME_TILE, TIME_K = SVH_TIME_K, TIME_BOX = TIME_TILE + 2 * TIME_K;
static_assert(TIME_K >= 1 && (size_t)TIME_BOX * TIME_BOX * 14 <= 64 * 1024, "the box of k_grid_time_sweep is static LDS: 14 bytes per cell");
// the whole sweep, layer L - 1 first: 1 + ceil((L - 1) / TIME_K) launches; returns the kernels it launched
int32_t launch_time_sweep(hipStream_t s, const TimeJob& j);
// the walk from the window cell (a, b) at layer 0: out[0] a PathStatus, out[1] the entries of the path, out[2] TPOT of the start; the
// first min(out[1], cap) triples to `triples`
void launch_time_walk(hipStream_t s, const TimeJob& j, int32_t a, int32_t b, int32_t* triples, int64_t cap, int64_t* out);
// over an image of svh_grid_render_cost's layout: the cells with BLOCK at layer t, then (two more launches) the goals that count and the
// cells of n triples
void launch_time_overlay(hipStream_t s, const TimeJob& j, int32_t t, const int32_t* goals, int32_t n_goals, const int32_t* triples, int64_t n,
                         uint8_t* rgb);

// The exploration layer (csrc/grid_explore_kernels.hip): the finished STATE plane, the frontier table and the reach field -> GAIN of
// viewpoints, the VIEW plane of one, the records, the scores and the best.
constexpr uint32_t VIEW_BLOCK = 256;             // k_grid_view_gain: one workgroup per viewpoint, its rays dealt to the lanes
constexpr int64_t VIEW_MAX_BLOCKS = 16384;       // ... the workgroups stride over the viewpoints beyond this many
constexpr uint32_t EXPLORE_BEST_BLOCK = 1024;    // k_grid_explore_best: one workgroup

struct ExploreJob {
    ExploreParams exp;
    FrontParams frp;            // what counts as unexplored
    int32_t R;                  // explore_range(exp.range, cell), 1..128
    int32_t nx, nz, oa, ob;
    const uint8_t* state;       // the finished STATE plane
    // a ranking
    const int32_t* front_recs = nullptr;   // the frontier table, FRONT_REC per kept component
    int32_t n = 0;              // its first min(kept, EXPLORE_MAX_RECORDS) records
    const int32_t* pot = nullptr;   // the reach field: POT with the start as the only goal
    int32_t* gain = nullptr;    // n
    int32_t* recs = nullptr;    // EXPLORE_REC per record
    long long* scores = nullptr;
    int32_t* out = nullptr;     // [0] the best, [1] the feasible records
};
// GAIN of n viewpoints, global cells at cells[i * stride], cells[i * stride + 1]; returns the kernels it launched
int32_t launch_view_gain(hipStream_t s, const ExploreJob& j, const int32_t* cells, int32_t stride, int64_t n, int32_t* out);
// the VIEW plane of the window viewpoint (va, vb), inside the window, into a plane that is all zero
void launch_view_mask(hipStream_t s, const ExploreJob& j, int32_t va, int32_t vb, uint8_t* view);
// gains of the representatives, records and scores, the best: three launches (one when n == 0); returns those of the gains
int32_t launch_explore_rank(hipStream_t s, const ExploreJob& j);
// a VIEW plane and its viewpoint drawn over an image of svh_grid_render_cost's layout
void launch_view_overlay(hipStream_t s, int32_t nx, int32_t nz, const uint8_t* view, int32_t va, int32_t vb, uint8_t* rgb);

// The alignment layer (csrc/grid_align_kernels.hip): the finished STATE plane and the obstacle points of a frame -> the field F, the
// scan, the volume of scores, the record of the best.
constexpr uint32_t ALIGN_BLOCK = 256;            // every kernel of the layer but the best
constexpr uint32_t ALIGN_MAX_BLOCKS = 2048;      // k_grid_align_mark: the lanes stride beyond 2048 * 256 points
constexpr int32_t ALIGN_CHUNK = 1024;            // k_grid_align_score: scan subs a workgroup places at a time
constexpr uint32_t ALIGN_MAX_SLICES = 64;        // ... the slices of the scan a launch has at most; a slice strides over its chunks
constexpr uint32_t ALIGN_BEST_BLOCK = 1024;      // k_grid_align_best: one workgroup
constexpr int32_t ALIGN_TILED_RUN = (2 * ALIGN_MAX_W) / 4 + 1;   // k_grid_align_score_tiled: translations a lane owns at most, 17
constexpr uint32_t ALIGN_TILED_LDS = 160 * 1024;   // ... the LDS of a workgroup: the chunk and the staged cells of F
constexpr uint32_t ALIGN_TILED_SLICES = 4;       // ... the slices of the scan a launch has at most
enum AlignForm : int32_t { ALIGN_FORM_CHUNK = 0, ALIGN_FORM_PLAIN = 1, ALIGN_FORM_TILED = 2, ALIGN_FORMS = 3,   // of the score kernel
                           ALIGN_FORM_MASK = 4 };   // added to one of them: the field in three launches, the mask first
enum AlignCtl { AC_SCAN = 0, AC_POINTS = 1, AC_WORDS = 2 };   // the control words on the device

struct AlignJob {
    Params prm;                 // where a point goes; nx, nz, oa, ob of the window
    AlignParams alp;
    int32_t Pa, Pb;             // the pivot's global sub
    int32_t rot[2 * ALIGN_MAX_ROTS];   // align_rot_table
    const uint8_t* state;       // the finished STATE plane
    uint16_t* g;                // the column distances, scratch, nx * nz
    uint8_t* field;             // F, nx * nz
    uint32_t* bitmap;           // ceil(side^2 / 32) words, all zero before the marks
    uint32_t* blockcnt;         // one count per ALIGN_BLOCK words of the bitmap
    int32_t* scan;              // pairs (ua, ub); room for min(points, side^2)
    int64_t scan_room;          // ... that many: the bound of every loop over the scan
    uint32_t* ctl;              // AC_WORDS, all zero before the marks
    int32_t* volume;            // align_volume_size(K, W), all zero before the scores
    int32_t* rec;               // ALIGN_REC
};
inline uint32_t align_words(const AlignJob& j) {
    const uint64_t side = (uint64_t)align_side(j.alp.Rg);
    return (uint32_t)((side * side + 31) / 32);
}
inline uint32_t align_count_blocks(const AlignJob& j) { return (align_words(j) + ALIGN_BLOCK - 1) / ALIGN_BLOCK; }
// F from STATE: the column sweep and the row pass
void launch_align_field(hipStream_t s, const AlignJob& j, bool mask);
// the kept points of n points (x, y, z, val), or (subs) of n pairs (ua, ub), marked in the bitmap and counted into ctl[AC_POINTS]
void launch_align_mark(hipStream_t s, const AlignJob& j, const float4* pts, const int32_t* subs, int64_t n);
// the set bits in ascending order to `scan`, their number to ctl[AC_SCAN]: two launches
void launch_align_compact(hipStream_t s, const AlignJob& j);
// the volume (all zero before) and the record.  Every loop over the scan is bounded by scan_room; with fewer than min_scan subs
// the volume is not written
void launch_align_score(hipStream_t s, const AlignJob& j, int32_t form);
// the cells of the scan at the identity, those of the scan placed at (k, ta, tb), the pivot's cell, drawn in that order over an
// image of svh_grid_render_local's layout: three launches
void launch_align_overlay(hipStream_t s, const AlignJob& j, int32_t n_scan, int32_t k, int32_t ta, int32_t tb, uint8_t* rgb);

// The dynamics (csrc/grid_dyn_kernels.hip): the phases 2 and 3 of an observation; phase 1 is launch_bin on the frame record.
// The layer's planes, nx * nz elements each, at the cell's SLOT: they travel with the torus.  All zero is the empty state.
struct DynPlanes {
    int2* body;                 // (q_lo, q_hi + 1) of the stored cell, (0, 0) where it is not tall: what a line step loads.  Kept by
                                // k_grid_settle for the cells it writes; a plain add makes it stale and k_grid_body writes it anew
    int32_t* contra;            // contradicting frames in a row
    int32_t* last;              // the stamp of the last observation with a point in the cell, 0 = never
    int32_t* kept;              // THROUGH of the last observation
    int32_t* through;           // THROUGH of the observation in flight: scratch, all zero between observations
    uint8_t* event;             // the DynEvent flags of the last observation
};
// bytes of the six planes of one cell; the engine lays them out in the order above
constexpr size_t DYN_BYTES = 25;
// bytes of the frame record of one cell: the accumulators of Cells without pass, kmin first
constexpr size_t FRAME_BYTES = 32;

struct SightJob {
    Params prm;
    DynParams dyn;
    uint32_t origin;            // the logical index of the origin's cell
    int32_t q_o;                // place(origin).q
    int32_t* ends;              // this frame's low points per cell, logical order: read, and left all zero
    Cells cells;                // the stored accumulators: count, kmin, kmax read where the bodies are stale, pass added to
    Cells frame;                // the frame record, by slot (pass is null): kmin read
    bool write_body;            // the bodies are stale: k_grid_body first
    DynPlanes planes;           // body read, through added to
    unsigned long long* ray_cells;   // the sum of pass increments, added to
};
// the bodies where they are stale, then the sight lines: one or two launches
void launch_sight(hipStream_t s, const SightJob& j);

struct SettleJob {
    Params prm;
    DynParams dyn;
    int32_t stamp;
    Cells cells, frame;         // the frame record is left empty
    DynPlanes planes;
    unsigned long long* stats;  // [DS_CLEARED], [DS_AGED], [DS_CONFIRMED] added to; [0] is not touched
};
void launch_settle(hipStream_t s, const SettleJob& j);
// svh_grid_scroll with the layer set: the planes of the entering strips become empty; the arguments of launch_enter
void launch_dyn_enter(hipStream_t s, const Params& prm, int32_t da, int32_t db, const DynPlanes& d);
// a grid::DynPlane in logical order
void launch_dyn_get(hipStream_t s, const Params& prm, int32_t plane, int32_t stamp, const DynPlanes& d, int32_t* out);
// svh_grid_render_dyn: a RenderJob (its mode is not read) with the layer's planes
void launch_render_dyn(hipStream_t s, const RenderJob& j, const DynPlanes& d);

// The archive (csrc/grid_archive_kernels.hip): the cells a scroll takes out of the window stored in pages by tile, the cells it brings
// in restored from them, and the finished planes over any box of global cells from the window and the pages together.
constexpr uint32_t ARCH_BLOCK = 256;             // every kernel of the layer; k_grid_arch_assign: one workgroup per claim, one lane per record
static_assert(ARCH_BLOCK == (uint32_t)TILE_CELLS, "a workgroup initialises one page");
// the control words on the device, 64 bits each: the tiles claimed by the leaving pass in flight (zero between calls), a claim that
// found the table full (zero between calls), the unused pages, and the four counts of grid::ArchiveStat
enum ArchCtl { AR_CLAIMS = 0, AR_OVERFLOW, AR_FREE, AR_SAVED, AR_RESTORED, AR_LOST, AR_REFUSED, AR_WORDS = 8 };
// the pool: max_tiles * 256 elements per plane, the record of cell i of page p at p * 256 + i
struct Pages {
    uint32_t* kmin;
    uint32_t* kmax;
    int32_t* count;
    int32_t* overhead;
    unsigned long long* hsum;
    unsigned long long* vsum;
    int32_t* pass;
    int32_t* contra;
    int32_t* last;
};
struct Archive {
    unsigned long long* keys = nullptr;   // `table` slots: a tile_key or TILE_NONE
    int32_t* page = nullptr;              // ... the tile's page, -1 while a claim is pending and in every empty slot
    uint32_t table = 0;                   // a power of two; 0: there is no archive, every lookup finds nothing
    int32_t max_tiles = 0;
    int32_t* stack = nullptr;             // max_tiles: the unused pages at [0, ctl[AR_FREE])
    int32_t* claims = nullptr;            // `table`: the slots claimed by the leaving pass in flight
    unsigned long long* ctl = nullptr;    // AR_WORDS
    Pages pages{};
};
// keys and page are all ones before: the stack holds every page, the control words are zero but AR_FREE
void launch_archive_reset(hipStream_t s, const Archive& ar);
// One scroll by (da, db), not both zero.  leave: `prm` has the OLD offsets; three launches -- claim, assign or withdraw, store.
// enter: `prm` has the NEW offsets; one launch, which replaces launch_enter and launch_dyn_enter.  dyn: the planes exist
struct ArchScrollJob {
    Params prm;
    int32_t da, db;
    Cells cells;
    bool dyn;
    DynPlanes planes;
    Archive ar;
};
void launch_archive_leave(hipStream_t s, const ArchScrollJob& j);
void launch_archive_enter(hipStream_t s, const ArchScrollJob& j);
// a plane of svh_grid_get (kind RK_GRID) or svh_grid_get_local (RK_LOCAL) over the box of w x h global cells from (ga0, gb0), row major
struct RegionJob {
    Params prm;
    Cells cells;
    Archive ar;
    int32_t kind, plane, ga0, gb0, w, h;
};
void launch_archive_region(hipStream_t s, const RegionJob& j, void* out);
// the image of a grid::Mode (M_LOCAL included) over the box, row 0 = gb0 + h - 1
void launch_archive_render_region(hipStream_t s, const RegionJob& j, int32_t mode, uint8_t* rgb);
// svh_grid_archive_trim in two halves, keys and page filled with ones between them: the tiles that meet the box to (skeys, spages),
// room for max_tiles, their number to ctl[AR_CLAIMS]; the pages of the others back on the stack.  Then the kept tiles inserted again
void launch_archive_trim_collect(hipStream_t s, const Archive& ar, int32_t ga0, int32_t gb0, int32_t ga1, int32_t gb1, unsigned long long* skeys,
                                 int32_t* spages);
void launch_archive_trim_insert(hipStream_t s, const Archive& ar, const unsigned long long* skeys, const int32_t* spages);

}  // namespace grid
}  // namespace svh
#endif

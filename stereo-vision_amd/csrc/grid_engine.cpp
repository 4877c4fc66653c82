// The ground grid behind the svh_grid_* entries of include/svh_grid.h: a 2.5-D bird's-eye grid over the road plane, binned
// on the device from the map view's store or from a list of points.
//
// Host (this file): the parameters (T rounded to float once), the two frames, the window's offsets, the statistics, the
// lazy clear and the lazy finalise.  Device (grid_kernels.hip): the binning, the rays, the strips of a scroll, the
// finalise, the render; (grid_trav_kernels.hip): the traversability layer -- flags, obstacle distance, cost, its render;
// (grid_plan_kernels.hip): the planner -- the relaxation over active tiles, whose round loop is plan_rounds() here;
// (grid_front_kernels.hip): the frontiers -- mask, union-find labelling, the table of components, run by front_run() here;
// (grid_roll_kernels.hip): the rollouts -- footprint costs, the scoring of a set of candidates and its best;
// (grid_obj_kernels.hip): the objects and their tracks -- obstacle components labelled by the frontier layer's kernels, the table of
// kept ones, and the step that associates them with the tracks of the step before, run by obj_run() and objects_step() here;
// (grid_pred_kernels.hip): the prediction -- the tracks carried ahead into the slots of PRED, run by predict() here, and the
// footprint masks and the scoring of a set of candidates against it;
// (grid_explore_kernels.hip): the exploration layer -- the gain of viewpoints, the ranking of the frontiers, run by explore_rank() here;
// (grid_align_kernels.hip): the alignment layer -- the field, the scan of a frame's obstacle points, the volume of scores, run by align() here;
// (grid_dyn_kernels.hip): the dynamics -- the sight lines and the settle of an observation, run by observe() here;
// (grid_archive_kernels.hip): the archive -- the leaving and entering passes of a scroll, run by scroll() here, and the region reader;
// (grid_time_kernels.hip): the time layer -- the release of the predicting tracks' cells, the sweep over cell x layer, run by
// time_static() and time_field() here.
// The arithmetic is csrc/grid_core.h.  The object has its own stream; every entry returns when it is complete.
//
// The accumulators are cleared lazily: svh_grid_clear, svh_grid_set_window and an add that failed only mark the grid
// empty, and the next entry that touches the device fills the planes with the empty values first.  That is what makes
// "after SVH_ERR_HIP inside an add the grid is empty" hold even when the failure was a lost device queue: no HIP call is
// needed to get there.  The accumulators lie at their slots (the torus of grid_core.h); everything derived from them is in
// logical order, and every plane that leaves the object is a derived one.  A scroll moves no data: it changes the offsets
// and resets the strips that enter; on an empty grid it changes the offsets alone.
// Everything derived is computed lazily, by the first entry that needs it, and kept.  What is kept, what each kept layer is
// computed from and what each change makes stale is one table, below beside the struct (Kept, kNeeds, kDrops): a setter says
// what it changed (touch), a function that launches a layer says so (pending), and the entry that has waited for the launches
// makes them count (settle); a failed entry makes nothing count (failed).  The reach field has a key beside its bit: the start
// cell of the ranking it was computed for.  Gains and VIEW planes are computed per call.  PRED has a bit of its own outside the
// derived layers: it is computed from the tracks, which are state, and from its parameters, never from the accumulators.
// The dynamics keep CONTRA, LAST, the THROUGH and the events of the last observation and the bodies of the cells at the cells' slots
// (they travel with the torus and are cleared as lazily as the accumulators, dyn_need_clear); the body plane is kept by the settle
// kernel and written anew (body_valid) after anything else wrote the accumulators.  The frame record and `ends` are scratch, empty
// between observations (frame_clean, ends_clean).  These describe the accumulators' side and are not part of the table.
// The archive (svh_grid_set_archive) is state beside the accumulators too: the cells outside the window.  It is emptied as lazily as
// they are (arch_need_clear), by everything that empties them; nothing cached is computed from it, so its mutators touch no source of
// the table, and a scroll, which restores from it, drops ACC as it always did.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/svh_grid.h"
#include "grid_align_core.h"
#include "grid_archive_core.h"
#include "grid_core.h"
#include "grid_explore_core.h"
#include "grid_internal.h"
#include "hip_guard.h"
#include "svh_config.h"
#include "view_internal.h"

using namespace svh;

namespace {

#define GRID_TRY(kind, expr) SVH_HIP_TRY("Grid", kind, expr)
#define GRID_GROW(buf, bytes) SVH_HIP_GROW("Grid", buf, bytes)
#define GRID_GROW_N(buf, count) SVH_HIP_GROW_N("Grid", buf, count)

constexpr int64_t kMaxPoints = ((int64_t)1 << 31) - 1;
constexpr int64_t kHostChunk = (int64_t)1 << 22;   // points of a host array staged per copy
constexpr size_t kFinalBytes = 27;                 // per cell: COUNT, OVERHEAD, PASS, HMIN, HMAX, HMEAN; INTENSITY, CLASS, STATE
enum FinPlane { F_COUNT = 0, F_OVERHEAD, F_PASS, F_HMIN, F_HMAX, F_HMEAN, F_WORDS };   // the 4-byte planes of `fin`
enum FinByte { B_INTENSITY = 0, B_CLASS, B_STATE };                                    // its byte planes
constexpr size_t kTravBytes = 8;                   // per cell: DIST2; g (uint16); FLAGS, COST
constexpr size_t kPlanBytes = 7;                   // per cell: POT; price (uint16); DIR
constexpr size_t kFrontBytes = 5;                  // per cell: LABEL; FRONT
constexpr size_t kPoseBytes = 8;                   // per state: PPOT; price (uint16); PDIR; CF
constexpr size_t kTimeStaticBytes = 11;            // per cell: RPOT; price (uint16); g (uint16); RDIR, RCOST, FLAGS'
constexpr size_t kTimeBytes = 5;                   // per state: TPOT; TDIR
// rounds of the relaxation enqueued per wait: a round whose list is empty costs one empty launch, a wait costs a round trip,
// and the bound on the workgroups of a round grows with its distance from the last known length.  Measured alternating in one
// process at 1, 2, 4, 8 and 16 (profiles/grid_plan_times.jsonl; ms on an open field of 256^2 / 1024^2 / 8192^2 cells):
// 0.52 / 2.08 / 29.7 at 1, 0.37 / 1.48 / 27.8 at 4, 0.32 / 1.32 / 37.3 at 16 -- at 8192^2 the later rounds of a long batch launch
// a workgroup for every tile.  4 is kept.  1..64; svh_test_grid_plan_rounds_per_wait changes it for that measurement
// (tools/gpu_grid_plan.py)
int g_rounds_per_wait = 4;
// the form of the alignment's score kernel (grid::AlignForm); svh_test_grid_align_form changes it for the paired measurement
// (tools/gpu_grid_align.py) and the tests
int g_align_form = grid::ALIGN_FORM_CHUNK;

bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }

// svh_grid_params -> grid::Params; false: out of range
bool convert(const svh_grid_params* p, grid::Params* q) {
    if (!p) return false;
    q->nx = p->nx, q->nz = p->nz;
    q->cell = p->cell, q->x0 = p->x0, q->z0 = p->z0;
    for (int k = 0; k < 12; k++) {
        if (!finite_d(p->T[k])) return false;
        q->T[k] = (float)p->T[k];
    }
    q->min_points = p->min_points;
    q->step = p->step, q->drop = p->drop, q->clearance = p->clearance;
    q->h_lo = p->render_h_lo, q->h_hi = p->render_h_hi;
    return grid::params_ok(*q);
}

// what a frontier computation needs beside the two planes: the block counts of the ordered compactions, the control words and
// their pinned copy, and what is sized by the components once their number is known
struct FrontBufs {
    HipBuf<int32_t> blocks, roots, recs;
    HipBuf<uint8_t> acc;
    HipBuf<unsigned long long> ctl;
    PinnedBuf<unsigned long long> h_ctl;
};

// the same for the objects: the ranks of the kept components (`slot`) stay with the roots, for the steps of the tracks
struct ObjBufs {
    HipBuf<int32_t> blocks, roots, slot, recs;
    HipBuf<uint8_t> acc;
    HipBuf<unsigned long long> ctl;
    PinnedBuf<unsigned long long> h_ctl;
};

// the tracks: two track tables and two ID planes (a step reads one and writes the other), the scratch of a step, and the control
// words with the first records of ASSIGN on their way to the host
struct TrackBufs {
    HipBuf<int32_t> table[2], id[2], assign, counts;
    HipBuf<unsigned long long> keys, ctl;
    HipBuf<uint8_t> zero, ones;
    PinnedBuf<uint8_t> h_out;
};

// the rollout parameters with what is derived from them for a cell side: the reach and the footprint table (grid_roll_core.h)
struct RollTable {
    grid::RollParams p{3.5f, 1.0f, 0.9f, 8, 253, 254, 1, 1, 0};
    int32_t R = 0;
    std::vector<int32_t> offs;      // pairs (da, db)
    std::vector<int64_t> start;     // 8 m + 1
    std::vector<int32_t> start32;   // the same for the device: at most 256 lists of at most 257^2 cells
    int64_t longest = 0;
    bool derive(float cell) {
        R = grid::roll_table(p, cell, &offs, &start);
        longest = 0;
        for (size_t k = 0; R && k + 1 < start.size(); k++) longest = std::max(longest, start[k + 1] - start[k]);
        start32.assign(start.begin(), start.end());
        return R != 0;
    }
};

// what the rollout kernels need on the device beside the planes: the footprint table, and the records, scores and best of a scoring
struct RollBufs {
    HipBuf<int32_t> offs, start, recs, best;
    HipBuf<long long> scores;
};

// the prediction: PRED and the scratch of its inflation, the displacements and flags of the tracks, the control words with their pinned
// copy (the statistics of the PRED that is valid are read there), and the outputs of a scoring with prediction, which leave those of
// svh_grid_roll_score alone
struct PredBufs {
    HipBuf<uint32_t> plane, rows, d_mask;
    HipBuf<int2> disp;
    HipBuf<int32_t> predicts, recs, best, d_poses;
    HipBuf<long long> scores;
    HipBuf<unsigned long long> ctl;
    PinnedBuf<unsigned long long> h_ctl;
    PinnedBuf<uint8_t> h_roll;
};

// what a ranking needs on the device beside the planes: the gains of the representatives, the records, the scores, and the best
// with the count of feasible records
struct ExploreBufs {
    HipBuf<int32_t> gain, recs, out;
    HipBuf<long long> scores;
};

// what an alignment needs on the device beside STATE: the field and its column distances, the bitmap of the box with the counts of
// its blocks, the list of the scan, the control words, the volume and the record
struct AlignBufs {
    HipBuf<uint8_t> field;
    HipBuf<uint16_t> g;
    HipBuf<uint32_t> bitmap, blockcnt, ctl;
    HipBuf<int32_t> scan, volume, rec;
};

// ---- what the object keeps, and what makes it stale ---------------------------------------------------------------------------
// One bit each in svh_grid::valid.  A derived layer's bit: its planes are those of the state as it is.  An upload's: the device
// holds the host's table.  A last result's: the buffers hold the records of the last scoring or alignment, for the getters and images
enum Kept : uint32_t {
    FINAL = 1u << 0,      // `fin`, from the accumulators and the offsets
    TRAV = 1u << 1,       // `trav`, from `fin` and the traversability parameters
    PLAN = 1u << 2,       // `plan`, from COST, the plan parameters and the goals
    FRONT = 1u << 3,      // `front` and the table, from STATE, COST and the frontier parameters
    REACH = 1u << 4,      // `reach`, from COST and the plan parameters, for the start (reach_ga, reach_gb)
    AFIELD = 1u << 5,     // al.field, from STATE and the align parameters
    OBJ = 1u << 6,        // `obj`, the object table and its statistics, from STATE, HMAX, COUNT and the object parameters
    POSE_CF = 1u << 7,    // the CF planes of `pose`, from COST and the footprint table: a bit of its own, so that new goals or pose
                          // parameters do not run k_grid_pose_foot again
    POSE = 1u << 8,       // PPOT, the prices and PDIR of `pose` and their statistics, from CF, the pose parameters and the pose goals
    TIME_STATIC = 1u << 9,// RCOST, RPOT, RDIR of `tstat` and the released count, from FLAGS and COST and the planner's field (whatever makes
                          // PLAN stale makes them stale) and, only when release = 1, from the tracks and the prediction parameters
                          // (kDropsReleased below)
    TIME = 1u << 10,      // TPOT, TDIR of `tfield` and their statistics, from the static planes, PRED and the time parameters
    UP_TABLE = 1u << 11,  // d_table holds `table`
    UP_GOALS = 1u << 12,  // d_goals holds `goals`
    UP_ROLL = 1u << 13,   // roll_bufs.offs and .start hold the footprint table
    UP_CANDS = 1u << 14,  // d_cands and d_cand_lens hold the candidates
    ROLL_LAST = 1u << 15, // roll_bufs.recs holds the records of the last svh_grid_roll_score
    ALIGN_LAST = 1u << 16,// al.scan and al.volume hold the scan and (unless FEW) the volume of the last alignment
    PRED = 1u << 17,      // pred.plane and its statistics, from the track state and the prediction parameters: not a derived layer, the
                          // accumulators do not reach it
    UP_POSE_GOALS = 1u << 18   // d_pose_goals holds `pose_goals`
};
constexpr int kLayers = 11;
constexpr uint32_t kAllLayers = (1u << kLayers) - 1;
// the layers each derived layer is computed from, by the layer's bit number
constexpr uint32_t kNeeds[kLayers] = {0, FINAL, TRAV, TRAV, TRAV, FINAL, FINAL, TRAV, POSE_CF, TRAV | PLAN, TIME_STATIC};
// what changes, and what it makes stale directly; the layers computed from a stale layer follow by closure()
enum Source { ACC, TRAV_PARAMS, PLAN_PARAMS, GOALS, FRONT_PARAMS, ROLL_PARAMS, CANDS, ALIGN_PARAMS, OBJ_PARAMS, TRACKS, PRED_PARAMS, POSE_PARAMS, POSE_GOALS, TIME_PARAMS, SOURCES };
constexpr uint32_t kDrops[SOURCES] = {
    FINAL,                    // ACC: the accumulators or the window's offsets
    TRAV | UP_TABLE,          // TRAV_PARAMS
    PLAN | REACH,             // PLAN_PARAMS
    PLAN | UP_GOALS,          // GOALS
    FRONT,                    // FRONT_PARAMS
    UP_ROLL | ROLL_LAST | POSE_CF,   // ROLL_PARAMS: the footprint table, stop_cost and unknown_cost reach CF and the prices
    UP_CANDS | ROLL_LAST,     // CANDS: the candidate table
    AFIELD | ALIGN_LAST,      // ALIGN_PARAMS
    OBJ,                      // OBJ_PARAMS
    PRED | TIME,              // TRACKS: the track table or the ID plane: a step, or anything that empties the tracks
    PRED | TIME,              // PRED_PARAMS
    POSE,                     // POSE_PARAMS
    POSE | UP_POSE_GOALS,     // POSE_GOALS
    TIME,                     // TIME_PARAMS; a new `release` drops kDropsNewRelease too (svh_grid_set_time)
};
// what a source makes stale beside that while the time layer's release = 1: the released cells are those of the predicting tracks
constexpr uint32_t kDropsReleased[SOURCES] = {0, 0, 0, 0, 0, 0, 0, 0, 0, TIME_STATIC, TIME_STATIC, 0, 0, 0};
// what svh_grid_set_time drops beside kDrops[TIME_PARAMS] when `release` itself changes
constexpr uint32_t kDropsNewRelease = TIME_STATIC;
constexpr uint32_t closure(uint32_t m) {
    for (int pass = 0; pass < kLayers; pass++)
        for (int k = 0; k < kLayers; k++)
            if (kNeeds[k] & m) m |= 1u << k;
    return m;
}
struct StaleTable {
    uint32_t of[SOURCES];
};
constexpr StaleTable stale_table() {
    StaleTable t{};
    for (int s = 0; s < SOURCES; s++) t.of[s] = closure(kDrops[s]);
    return t;
}
constexpr StaleTable kStale = stale_table();
static_assert((kStale.of[ACC] & kAllLayers) == kAllLayers, "a derived layer without a path to FINAL in kNeeds would survive a change of the accumulators");
static_assert(kStale.of[TRAV_PARAMS] == (TRAV | PLAN | FRONT | REACH | POSE_CF | POSE | TIME_STATIC | TIME | UP_TABLE), "the closure of kNeeds");
static_assert(kStale.of[ROLL_PARAMS] == (UP_ROLL | ROLL_LAST | POSE_CF | POSE) && kStale.of[POSE_PARAMS] == POSE && kStale.of[POSE_GOALS] == (POSE | UP_POSE_GOALS),
              "the pose field follows the vehicle, its own parameters and its own goals");
static_assert(!((kStale.of[PLAN_PARAMS] | kStale.of[GOALS] | kStale.of[FRONT_PARAMS] | kStale.of[CANDS] | kStale.of[ALIGN_PARAMS] | kStale.of[OBJ_PARAMS] |
                 kStale.of[TRACKS] | kStale.of[PRED_PARAMS]) & (POSE | POSE_CF)), "the planner, the candidates, the objects and the prediction leave the pose field alone");
static_assert(kStale.of[OBJ_PARAMS] == OBJ && (kStale.of[ACC] & OBJ), "the objects follow the accumulators and their own parameters");
static_assert(!((kStale.of[TRAV_PARAMS] | kStale.of[PLAN_PARAMS] | kStale.of[GOALS] | kStale.of[FRONT_PARAMS] | kStale.of[ROLL_PARAMS] |
                 kStale.of[CANDS] | kStale.of[ALIGN_PARAMS] | kStale.of[POSE_PARAMS] | kStale.of[POSE_GOALS]) & OBJ), "no other layer's source makes the objects stale");
static_assert(kStale.of[TRACKS] == (PRED | TIME) && kStale.of[PRED_PARAMS] == (PRED | TIME), "the prediction follows the tracks and its own parameters, and TIME follows it");
static_assert(kStale.of[PLAN_PARAMS] == (PLAN | REACH | TIME_STATIC | TIME) && kStale.of[GOALS] == (PLAN | UP_GOALS | TIME_STATIC | TIME) && kStale.of[TIME_PARAMS] == TIME,
              "the time layer follows the planner's field and its own parameters; its setter makes no other layer stale");
static_assert(!((kStale.of[FRONT_PARAMS] | kStale.of[ROLL_PARAMS] | kStale.of[CANDS] | kStale.of[ALIGN_PARAMS] | kStale.of[OBJ_PARAMS] | kStale.of[POSE_PARAMS] |
                 kStale.of[POSE_GOALS]) & (TIME | TIME_STATIC)), "the frontiers, the rollouts, the candidates, the alignment, the object parameters and the pose planner leave TIME alone");
static_assert(!((kStale.of[TRACKS] | kStale.of[PRED_PARAMS]) & TIME_STATIC) && kDropsReleased[TRACKS] == TIME_STATIC && kDropsReleased[PRED_PARAMS] == TIME_STATIC,
              "with release = 0 a step keeps the static planes; with release = 1 it drops them");
static_assert(kDropsReleased[TIME_PARAMS] == 0 && closure(kDropsNewRelease) == (TIME_STATIC | TIME), "a new wait or L keeps the static planes; a new release drops them and the field, nothing else");
static_assert(!((kStale.of[ACC] | kStale.of[TRAV_PARAMS] | kStale.of[PLAN_PARAMS] | kStale.of[GOALS] | kStale.of[FRONT_PARAMS] | kStale.of[ROLL_PARAMS] |
                 kStale.of[CANDS] | kStale.of[ALIGN_PARAMS] | kStale.of[OBJ_PARAMS] | kStale.of[POSE_PARAMS] | kStale.of[POSE_GOALS] | kStale.of[TIME_PARAMS]) & PRED), "nothing else makes the prediction stale");

}  // namespace

struct svh_grid {
    int device = 0;
    hipStream_t stream = nullptr;
    grid::Params prm{};
    size_t ncells = 0;
    HipBuf<uint8_t> acc;        // CELL_BYTES per cell: kmin | kmax | count | overhead | hsum | vsum | pass, a plane each
    HipBuf<uint8_t> fin;        // kFinalBytes per cell: the FinPlane planes, then the FinByte planes, logical order
    HipBuf<int32_t> ends;       // svh_grid_add_*_from: the call's low points per cell; all zero between calls
    bool ends_clean = false;    // ... and it is
    HipBuf<unsigned long long> d_stats;
    PinnedBuf<unsigned long long> h_stats;
    HipBuf<float4> d_pts;       // a host array on its way to the kernel
    PinnedBuf<float4> h_pts;
    HipBuf<uint8_t> d_rgb;      // a render bound for the host
    PinnedBuf<uint8_t> h_out;
    bool need_clear = true;     // the accumulators do not hold the empty grid yet
    uint32_t valid = 0;         // Kept bits: what is current
    uint32_t pending = 0;       // layers launched by this entry and not waited for yet: settle() makes them valid
    grid::TravParams trv{};     // the traversability layer: parameters and what is derived from them; reach 0: the
    bool trav_ok = false;       // defaults do not fit this grid's cell, and svh_grid_set_traversability has not succeeded
    std::vector<uint8_t> table; // cost by DIST2, reach^2 + 1 bytes
    HipBuf<uint8_t> d_table;
    PinnedBuf<uint8_t> h_table;
    HipBuf<uint8_t> trav;       // kTravBytes per cell: DIST2 | g | FLAGS | COST, logical order
    grid::PlanParams pln{50, -1, 0x7FFFFFFE};   // the planner: parameters, the goals as global cells
    std::vector<int32_t> goals;
    HipBuf<int32_t> d_goals;
    PinnedBuf<int32_t> h_cells; // goals or a path on their way to the device
    HipBuf<uint8_t> plan;       // kPlanBytes per cell: POT | price | DIR, logical order
    HipBuf<uint32_t> plan_tiles;   // 4 per tile: the two lists, the two flags
    HipBuf<uint32_t> plan_ctl;  // grid::CTL_WORDS
    PinnedBuf<uint32_t> h_ctl;
    int64_t plan_counted = 0, plan_reached = 0, plan_rounds = 0;   // of the field that is valid
    HipBuf<int32_t> d_path;     // the cells a walk writes, or a caller's path for the plan image
    HipBuf<int64_t> d_walk;     // status, length, cost
    PinnedBuf<int64_t> h_walk;
    grid::FrontParams frp{252, 8, grid::LETHAL_UNSEEN, 0};   // the frontiers: parameters, planes, table
    HipBuf<uint8_t> front;      // kFrontBytes per cell: LABEL | FRONT, logical order
    FrontBufs front_bufs;
    int64_t front_stats[grid::FS_WORDS] = {0, 0, 0, 0, 0};   // of the result that is valid
    RollTable rol;              // the rollouts: parameters and the footprint table; R 0: the defaults do not fit this grid's cell
    RollBufs roll_bufs;
    std::vector<int32_t> cands, cand_lens;   // the candidate table (S * K * T * 3) and the lengths of its S * K candidates
    int32_t cand_S = 0, cand_K = 0, cand_T = 0;
    HipBuf<int32_t> d_cands, d_cand_lens;
    HipBuf<int32_t> d_poses, d_fcost;   // free poses of a host caller and their F
    PinnedBuf<uint8_t> h_roll;  // records, scores and the best on their way to the host
    int32_t roll_last_set = 0, roll_last_ga = 0, roll_last_gb = 0, roll_last_best = -1;   // ROLL_LAST: the set, anchor and best of that scoring
    grid::ExploreParams exp{10.f, 1, 500, 1};   // the exploration layer: parameters and their R; 0: the defaults do not fit this grid's cell
    int32_t exp_R = 0;
    HipBuf<uint8_t> reach;      // kPlanBytes per cell: POT | price | DIR of the reach field, logical order
    HipBuf<uint32_t> reach_tiles, reach_ctl;   // as plan_tiles and plan_ctl
    PinnedBuf<uint32_t> h_reach_ctl;
    HipBuf<int32_t> d_start;    // the start cell: the one goal of the reach field
    PinnedBuf<int32_t> h_start;
    int32_t reach_ga = 0, reach_gb = 0;   // REACH: the start the field was computed from, a global cell
    ExploreBufs ex_bufs;
    PinnedBuf<uint8_t> h_explore;   // scores, records, best and feasible count of the last ranking on their way to the host
    HipBuf<int32_t> d_vcells, d_vgain;   // viewpoints of a host caller and their GAIN
    HipBuf<uint8_t> d_view;     // the VIEW plane of one viewpoint
    int64_t ex_stats[grid::ES_WORDS] = {0, 0, 0, 0};
    grid::AlignParams alp{};    // the alignment layer: parameters with what is derived from them and the rotation table;
    bool align_ok = false;      // false until svh_grid_set_align succeeds
    int32_t align_rot[2 * grid::ALIGN_MAX_ROTS] = {0};
    AlignBufs al;
    PinnedBuf<int32_t> h_arec;
    int32_t align_rec[grid::ALIGN_REC] = {0}, align_Pa = 0, align_Pb = 0;   // ALIGN_LAST: the record and pivot sub of that alignment
    svh_grid_stats st{0, 0, 0, 0, 0};
    int64_t rays = 0, ray_cells = 0;
    bool dyn_on = false;        // the dynamics: svh_grid_set_dynamics has succeeded and the layer has not been dropped
    grid::DynParams dyn{};
    HipBuf<uint8_t> dynp;       // DYN_BYTES per cell: body | CONTRA | LAST | kept THROUGH | THROUGH in flight | event, by slot
    HipBuf<uint8_t> frame;      // FRAME_BYTES per cell: the frame record, kmin | kmax | count | overhead | hsum | vsum, by slot
    bool body_valid = false;    // the body plane is that of the accumulators as they are, under the parameters in force
    HipBuf<int32_t> d_dyn;      // a plane of svh_grid_get_dyn bound for the host
    bool dyn_need_clear = true; // dynp does not hold the empty state yet
    bool frame_clean = false;   // the frame record is empty and `ends` all zero: true between observations that succeeded
    int32_t stamp = 0;          // of the last observation; 0 after a clear
    int64_t dyn_stats[grid::DS_WORDS] = {0, 0, 0, 0};
    grid::ObjParams obp{4, 4096, 0.3f, 1024, 1, 4, 2, 3, 2, 1};   // the objects: parameters, planes, table
    HipBuf<uint8_t> obj;        // kFrontBytes per cell: LABEL | FLAGS, logical order
    ObjBufs obj_bufs;
    int64_t obj_stats[grid::OS_WORDS] = {0, 0, 0, 0, 0, 0, 0};   // of the result that is valid
    TrackBufs trk;              // the tracks: state that only svh_grid_objects_step advances
    int trk_cur = 0;            // which of the two tables and ID planes is current
    bool trk_plane = false;     // a step has written the current ID plane; false: it counts as all -1
    int32_t trk_n = 0, trk_next = 0, trk_oa = 0, trk_ob = 0;   // the tracks, the next id, the offsets of the ID plane
    int64_t trk_stats[grid::TS_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    grid::PredParams prp{8, 1, 1, 1, 0, 1};   // the prediction: parameters, PRED
    PredBufs pred;
    int32_t pred_launches = 0;  // PRED: the launches of the computation that produced it
    grid::PoseParams pose_prm{50, 0x7FFFFFFE, 100, -1, -1};   // the pose planner: parameters, the goal triples as global cells
    std::vector<int32_t> pose_goals;
    HipBuf<int32_t> d_pose_goals;
    HipBuf<uint8_t> pose;       // kPoseBytes per state, 8 states per cell: PPOT | price | PDIR | CF, heading-major planes; first use
    HipBuf<uint32_t> pose_tiles, pose_ctl;   // as plan_tiles and plan_ctl
    PinnedBuf<uint32_t> h_pose_ctl;
    int64_t pose_counted = 0, pose_reached = 0, pose_rounds = 0;   // of the field that is valid
    HipBuf<int32_t> d_pose_path;   // the poses a walk writes, or a caller's for the pose image
    bool time_on = false;       // the time layer: svh_grid_set_time has succeeded
    grid::TimeParams tmp{32, 100, 1};
    HipBuf<uint8_t> tstat;      // kTimeStaticBytes per cell: RPOT | price | g | RDIR | RCOST | FLAGS', logical order; written only when cells are released
    HipBuf<uint32_t> tstat_tiles, tstat_ctl;   // as plan_tiles and plan_ctl
    PinnedBuf<uint32_t> h_tstat_ctl;
    HipBuf<uint8_t> tfield;     // kTimeBytes per state: TPOT | TDIR, layer-major planes.  While TIME is stale the first plane of TPOT is also the
                                // DIST2 scratch of time_static's distance pass: TIME is stale whenever TIME_STATIC is (kNeeds)
    HipBuf<unsigned long long> time_ctl;   // grid::TC_WORDS
    PinnedBuf<unsigned long long> h_time_ctl;
    bool time_own = false;      // TIME_STATIC: the static planes are those of `tstat`; false: the planner's
    int64_t time_released = 0, time_rounds = 0;   // TIME_STATIC: the released cells, the rounds of RPOT
    int64_t time_stats[grid::TM_WORDS] = {0, 0, 0, 0, 0, 0};   // TIME
    HipBuf<int32_t> d_time_path;   // the triples a walk writes, or a caller's for the time image
    int32_t arch_tiles = 0;     // the archive: max_tiles, 0 = off
    HipBuf<uint8_t> arch_pool;  // PAGE_BYTES per tile: kmin | kmax | count | overhead | hsum | vsum | pass | CONTRA | LAST, a plane each; first use
    HipBuf<unsigned long long> arch_keys, arch_ctl, arch_skeys;   // the table's keys, the control words, the kept keys of a trim
    HipBuf<int32_t> arch_page, arch_stack, arch_claims, arch_spages;
    PinnedBuf<unsigned long long> h_arch_ctl;
    HipBuf<uint8_t> d_region;   // a region bound for the host
    bool arch_need_clear = true;   // the table and the stack do not hold the empty archive yet
    int64_t arch_stats[grid::AS_WORDS] = {0, 0, 0, 0, 0, 0};   // since the archive was last emptied

    grid::Cells cells() const {
        uint8_t* b = acc.p;
        const size_t n = ncells;
        return grid::Cells{(uint32_t*)b, (uint32_t*)(b + 4 * n), (int32_t*)(b + 8 * n), (int32_t*)(b + 12 * n),
                           (unsigned long long*)(b + 16 * n), (unsigned long long*)(b + 24 * n), (int32_t*)(b + 32 * n)};
    }
    float* fplane(int k) const { return (float*)(fin.p + 4 * ncells * (size_t)k); }
    int32_t* iplane(int k) const { return (int32_t*)(fin.p + 4 * ncells * (size_t)k); }
    uint8_t* bplane(int k) const { return fin.p + 4 * F_WORDS * ncells + ncells * (size_t)k; }
    int32_t* t_dist2() const { return (int32_t*)trav.p; }
    uint16_t* t_g() const { return (uint16_t*)(trav.p + 4 * ncells); }
    uint8_t* t_flags() const { return trav.p + 6 * ncells; }
    uint8_t* t_cost() const { return trav.p + 7 * ncells; }
    int32_t* p_pot() const { return (int32_t*)plan.p; }
    uint16_t* p_price() const { return (uint16_t*)(plan.p + 4 * ncells); }
    uint8_t* p_dir() const { return plan.p + 6 * ncells; }
    int32_t* r_pot() const { return (int32_t*)reach.p; }
    int32_t* f_label() const { return (int32_t*)front.p; }
    uint8_t* f_flags() const { return front.p + 4 * ncells; }
    int32_t* q_pot() const { return (int32_t*)pose.p; }
    uint16_t* q_price() const { return (uint16_t*)(pose.p + 32 * ncells); }
    uint8_t* q_dir() const { return pose.p + 48 * ncells; }
    uint8_t* q_cf() const { return pose.p + 56 * ncells; }
    int32_t* s_pot() const { return (int32_t*)tstat.p; }
    uint16_t* s_price() const { return (uint16_t*)(tstat.p + 4 * ncells); }
    uint16_t* s_g() const { return (uint16_t*)(tstat.p + 6 * ncells); }
    uint8_t* s_dir() const { return tstat.p + 8 * ncells; }
    uint8_t* s_cost() const { return tstat.p + 9 * ncells; }
    uint8_t* s_flags() const { return tstat.p + 10 * ncells; }
    int32_t* t_pot() const { return (int32_t*)tfield.p; }
    uint8_t* t_dir() const { return tfield.p + 4 * ncells * (size_t)tmp.layers; }
    int32_t* o_label() const { return (int32_t*)obj.p; }
    uint8_t* o_flags() const { return obj.p + 4 * ncells; }
    grid::DynPlanes dplanes() const {
        uint8_t* b = dynp.p;
        const size_t n = ncells;
        return grid::DynPlanes{(int2*)b, (int32_t*)(b + 8 * n), (int32_t*)(b + 12 * n), (int32_t*)(b + 16 * n), (int32_t*)(b + 20 * n), b + 24 * n};
    }
    // the archive as the kernels see it; without buffers that hold it, one in which every lookup finds nothing
    grid::Archive archive() const {
        grid::Archive a;
        if (arch_tiles <= 0 || arch_need_clear || !arch_pool.p) return a;
        const size_t n = (size_t)arch_tiles * (size_t)grid::TILE_CELLS;
        uint8_t* b = arch_pool.p;
        a.keys = arch_keys.p, a.page = arch_page.p, a.stack = arch_stack.p, a.claims = arch_claims.p, a.ctl = arch_ctl.p;
        a.table = grid::archive_table_size(arch_tiles), a.max_tiles = arch_tiles;
        a.pages = grid::Pages{(uint32_t*)b, (uint32_t*)(b + 4 * n), (int32_t*)(b + 8 * n), (int32_t*)(b + 12 * n), (unsigned long long*)(b + 16 * n),
                              (unsigned long long*)(b + 24 * n), (int32_t*)(b + 32 * n), (int32_t*)(b + 36 * n), (int32_t*)(b + 40 * n)};
        return a;
    }
    grid::Cells fcells() const {
        uint8_t* b = frame.p;
        const size_t n = ncells;
        return grid::Cells{(uint32_t*)b, (uint32_t*)(b + 4 * n), (int32_t*)(b + 8 * n), (int32_t*)(b + 12 * n),
                           (unsigned long long*)(b + 16 * n), (unsigned long long*)(b + 24 * n), nullptr};
    }
};

namespace {

bool has(const svh_grid* g, uint32_t kept) { return (g->valid & kept) == kept; }

// `kept` is not current any more, whatever was launched
void drop(svh_grid* g, uint32_t kept) { g->valid &= ~kept, g->pending &= ~kept; }

// `s` changes: what the table derives from it is stale
// while the time layer is on with release = 1, what kDropsReleased adds (TIME_STATIC is never set while the layer is off)
void touch(svh_grid* g, Source s) { drop(g, kStale.of[s] | ((g->time_on && g->tmp.release) ? closure(kDropsReleased[s]) : 0u)); }

// the entry has waited for everything it launched: the layers among it count
void settle(svh_grid* g) {
    g->valid |= g->pending;
    g->pending = 0;
}

// The one exit of an entry that may have failed: whatever was launched and not settled does not count, and after SVH_ERR_HIP nothing
// of the call is in flight when the caller goes on and `kept`, what the entry's family computes, is computed again by the next call
int failed(svh_grid* g, int rc, uint32_t kept = 0) {
    g->pending = 0;
    if (rc == SVH_ERR_HIP) {
        drop(g, kept);
        if (g->stream) {
            (void)hipSetDevice(g->device);
            (void)hipStreamSynchronize(g->stream);
        }
    }
    return rc;
}
// what each family of entries drops there
constexpr uint32_t kPlanner = PLAN, kFrontier = FRONT, kRollouts = ROLL_LAST, kExploration = REACH, kAlign = AFIELD | ALIGN_LAST, kObjects = OBJ, kPrediction = PRED, kPose = POSE | POSE_CF, kTime = TIME | TIME_STATIC;

// the tracks are empty and the ids start again at 0
void forget_tracks(svh_grid* g) {
    touch(g, TRACKS);
    g->trk_plane = false;
    g->trk_n = g->trk_next = 0;
    for (int k = 0; k < grid::TS_WORDS; k++) g->trk_stats[k] = 0;
}

// the archive holds no tile, and its counts start again
void forget_archive(svh_grid* g) {
    g->arch_need_clear = true;
    for (int k = 0; k < grid::AS_WORDS; k++) g->arch_stats[k] = 0;
}

void mark_empty(svh_grid* g) {
    forget_archive(g);   // the stamp restarts, and a new corner renumbers the global cells
    g->need_clear = true;
    touch(g, ACC);
    g->st = svh_grid_stats{0, 0, 0, 0, 0};
    g->rays = g->ray_cells = 0;
    g->dyn_need_clear = true;
    g->frame_clean = g->body_valid = false;
    g->stamp = 0;
    for (int k = 0; k < grid::DS_WORDS; k++) g->dyn_stats[k] = 0;
}

// the accumulators become those of the empty grid; the statistics are not touched
int fill_empty(svh_grid* g) {
    GRID_TRY(copy, hipMemsetAsync(g->acc, 0xFF, 4 * g->ncells, g->stream));
    GRID_TRY(copy, hipMemsetAsync(g->acc + 4 * g->ncells, 0, (grid::CELL_BYTES - 4) * g->ncells, g->stream));
    return SVH_OK;
}

// the buffers exist and the accumulators hold what the object says they hold
int ready(svh_grid* g) {
    GRID_TRY(none, hipSetDevice(g->device));
    if (g->acc.cap < g->ncells * grid::CELL_BYTES) g->need_clear = true;
    GRID_GROW(g->acc, g->ncells * grid::CELL_BYTES);
    GRID_GROW(g->fin, g->ncells * kFinalBytes);
    GRID_GROW(g->d_stats, grid::STAT_ALL * sizeof(unsigned long long));
    GRID_GROW(g->h_stats, grid::STAT_ALL * sizeof(unsigned long long));
    if (g->need_clear) {
        const int rc = fill_empty(g);
        if (rc) return rc;
        GRID_TRY(copy, hipMemsetAsync(g->d_stats, 0, grid::STAT_ALL * sizeof(unsigned long long), g->stream));
        g->need_clear = false;   // in stream order before whatever the entry does next; every entry ends with a wait
    }
    return SVH_OK;
}

// the binning of n > 0 points, host or device, by a job that is complete but for the points: a host array goes through the
// staging buffers in chunks
int bin_points(svh_grid* g, grid::BinJob& j, const float* xyzv, int64_t n, bool on_device) {
    hipStream_t s = g->stream;
    if (on_device) {
        j.pts = (const float4*)xyzv;
        j.n = n;
        GRID_TRY(launch, (grid::launch_bin(s, j), hipGetLastError()));
        return SVH_OK;
    }
    const int64_t room = std::min(n, kHostChunk);
    GRID_GROW(g->h_pts, (size_t)room * sizeof(float4));
    GRID_GROW(g->d_pts, (size_t)room * sizeof(float4));
    for (int64_t at = 0; at < n; at += room) {
        const int64_t m = std::min(room, n - at);
        if (at > 0) GRID_TRY(wait, hipStreamSynchronize(s));   // the staging buffer is read until here
        memcpy(g->h_pts, xyzv + 4 * at, (size_t)m * sizeof(float4));
        GRID_TRY(copy, hipMemcpyAsync(g->d_pts, g->h_pts, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, s));
        j.pts = g->d_pts;
        j.n = m;
        GRID_TRY(launch, (grid::launch_bin(s, j), hipGetLastError()));
    }
    return SVH_OK;
}

// `ends` exists and is all zero; it counts as dirty until the rays of the call have zeroed what its binning counts
int zero_ends(svh_grid* g) {
    const size_t bytes = g->ncells * sizeof(int32_t);
    if (g->ends.cap < bytes) g->ends_clean = false;
    GRID_GROW(g->ends, bytes);
    if (!g->ends_clean) GRID_TRY(copy, hipMemsetAsync(g->ends, 0, bytes, g->stream));
    g->ends_clean = false;
    return SVH_OK;
}

// the statistics of a call of n points that is complete, from h_stats; rays: the call cast them, and `ends` is zero again
void read_stats(svh_grid* g, int64_t n, bool rays) {
    const unsigned long long* h = g->h_stats;
    if (rays) {
        g->ends_clean = true;
        g->rays += (int64_t)h[grid::LOW] - g->st.binned;
        g->ray_cells = (int64_t)h[grid::STAT_RAY_CELLS];
    }
    g->st.added += n;
    g->st.binned = (int64_t)h[grid::LOW], g->st.overhead = (int64_t)h[grid::OVERHEAD];
    g->st.outside = (int64_t)h[grid::OUTSIDE], g->st.unplaced = (int64_t)h[grid::UNPLACED];
}

// n > 0 points, host or device, with arguments that have been checked; origin >= 0: the logical index of the cell the
// low points cast their rays from
int add(svh_grid* g, const float* xyzv, int64_t n, bool on_device, int64_t origin = -1) {
    int rc = ready(g);
    if (rc) return rc;
    touch(g, ACC);
    g->body_valid = false;   // the dynamics: the accumulators change behind the layer
    grid::BinJob j;
    j.prm = g->prm;
    j.cells = g->cells();
    j.stats = g->d_stats;
    hipStream_t s = g->stream;
    if (origin >= 0) {
        if ((rc = zero_ends(g))) return rc;
        j.ends = g->ends;
    }
    if ((rc = bin_points(g, j, xyzv, n, on_device))) return rc;
    if (origin >= 0) {
        grid::RayJob r;
        r.prm = g->prm;
        r.origin = (uint32_t)origin;
        r.ends = g->ends;
        r.pass = j.cells.pass;
        r.ray_cells = g->d_stats + grid::STAT_RAY_CELLS;
        GRID_TRY(launch, (grid::launch_rays(s, r), hipGetLastError()));
    }
    GRID_TRY(copy, hipMemcpyAsync(g->h_stats, g->d_stats, grid::STAT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    read_stats(g, n, origin >= 0);
    return SVH_OK;
}

// ---- the dynamics ---------------------------------------------------------------------------------------------------------
// the layer's planes exist and hold what the object says they hold; after ready()
int dyn_ready(svh_grid* g) {
    if (g->dynp.cap < g->ncells * grid::DYN_BYTES) g->dyn_need_clear = true;
    GRID_GROW(g->dynp, g->ncells * grid::DYN_BYTES);
    if (g->dyn_need_clear) {
        g->body_valid = false;   // all zero is the body plane of the empty grid, which this one may not be
        GRID_TRY(copy, hipMemsetAsync(g->dynp, 0, g->ncells * grid::DYN_BYTES, g->stream));
        g->dyn_need_clear = false;   // in stream order before whatever the entry does next; every entry ends with a wait
    }
    return SVH_OK;
}

// One observation: n >= 0 points, host or device, with arguments that have been checked, from the origin's logical cell `origin`
// at the height q_o.  Phase 1 bins into the frame record, phase 2 casts the sight lines, phase 3 settles; one wait at the end (a
// host array of more than kHostChunk points waits once more per further chunk).  A frame without points still ages the cells.
int observe(svh_grid* g, const float* xyzv, int64_t n, bool on_device, int64_t origin, int32_t q_o) {
    int rc = ready(g);
    if (rc || (rc = dyn_ready(g))) return rc;
    touch(g, ACC);
    hipStream_t s = g->stream;
    const size_t nc = g->ncells;
    if ((rc = zero_ends(g))) return rc;
    if (g->frame.cap < nc * grid::FRAME_BYTES) g->frame_clean = false;
    GRID_GROW(g->frame, nc * grid::FRAME_BYTES);
    if (!g->frame_clean) {
        GRID_TRY(copy, hipMemsetAsync(g->frame, 0xFF, 4 * nc, s));
        GRID_TRY(copy, hipMemsetAsync(g->frame + 4 * nc, 0, (grid::FRAME_BYTES - 4) * nc, s));
        GRID_TRY(copy, hipMemsetAsync(g->dplanes().through, 0, 4 * nc, s));
    }
    g->frame_clean = false;   // as `ends`: until this observation has settled
    const int32_t stamp = g->stamp + 1;
    if (n > 0) {
        grid::BinJob j;
        j.prm = g->prm;
        j.cells = g->fcells();
        j.stats = g->d_stats;
        j.ends = g->ends;
        if ((rc = bin_points(g, j, xyzv, n, on_device))) return rc;
        grid::SightJob v;
        v.prm = g->prm, v.dyn = g->dyn;
        v.origin = (uint32_t)origin, v.q_o = q_o;
        v.ends = g->ends;
        v.cells = g->cells(), v.frame = g->fcells();
        v.write_body = !g->body_valid;
        v.planes = g->dplanes();
        v.ray_cells = g->d_stats + grid::STAT_RAY_CELLS;
        GRID_TRY(launch, (grid::launch_sight(s, v), hipGetLastError()));
    }
    grid::SettleJob t;
    t.prm = g->prm, t.dyn = g->dyn;
    t.stamp = stamp;
    t.cells = g->cells(), t.frame = g->fcells();
    t.planes = g->dplanes();
    t.stats = g->d_stats + grid::STAT_DYN - grid::DS_CLEARED;
    GRID_TRY(launch, (grid::launch_settle(s, t), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(g->h_stats, g->d_stats, grid::STAT_ALL * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    const unsigned long long* h = g->h_stats;
    read_stats(g, n, true);
    g->frame_clean = true;
    if (n > 0) g->body_valid = true;   // k_grid_body wrote it or it was valid, and k_grid_settle kept it
    g->stamp = stamp;
    g->dyn_stats[grid::DS_OBSERVATIONS] = stamp;
    for (int k = grid::DS_CLEARED; k < grid::DS_WORDS; k++) g->dyn_stats[k] = (int64_t)h[grid::STAT_DYN + k - grid::DS_CLEARED];
    return SVH_OK;
}

// the finished planes, launched on the stream and pending until the caller has waited and settles
int finalise(svh_grid* g) {
    if (has(g, FINAL)) return SVH_OK;
    grid::FinalJob j;
    j.prm = g->prm;
    j.cells = g->cells();
    j.count = g->iplane(F_COUNT), j.overhead = g->iplane(F_OVERHEAD), j.pass = g->iplane(F_PASS);
    j.hmin = g->fplane(F_HMIN), j.hmax = g->fplane(F_HMAX), j.hmean = g->fplane(F_HMEAN);
    j.intensity = g->bplane(B_INTENSITY), j.cls = g->bplane(B_CLASS), j.state = g->bplane(B_STATE);
    GRID_TRY(launch, (grid::launch_finalise(g->stream, j), hipGetLastError()));
    g->pending |= FINAL;
    return SVH_OK;
}

// `bytes` from device memory `src` to `out` (host or device) and the wait
int deliver(svh_grid* g, const void* src, size_t bytes, void* out, bool on_device) {
    hipStream_t s = g->stream;
    if (on_device) {
        GRID_TRY(copy, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
    } else {
        GRID_GROW(g->h_out, bytes);
        GRID_TRY(copy, hipMemcpyAsync(g->h_out, src, bytes, hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        memcpy(out, g->h_out, bytes);
    }
    return SVH_OK;
}

// a finished plane: a 4-byte plane FinPlane k, or (bytes) the byte plane FinByte k
int get(svh_grid* g, bool bytes, int k, void* out, bool on_device) {
    int rc = ready(g);
    if (rc) return rc;
    const void* src = bytes ? (const void*)g->bplane(k) : (const void*)g->iplane(k);
    if ((rc = finalise(g))) return rc;
    if ((rc = deliver(g, src, g->ncells * (bytes ? 1 : 4), out, on_device))) return rc;
    settle(g);
    return SVH_OK;
}

// The end of an entry whose kernels wrote `bytes` to the caller's device array, or to the scratch `src` on their way to the host
// array `out`: the wait, or the copy and the wait; then what the entry launched counts
int finish(svh_grid* g, const void* src, size_t bytes, void* out, bool on_device) {
    if (on_device) {
        GRID_TRY(wait, hipStreamSynchronize(g->stream));
    } else {
        const int rc = deliver(g, src, bytes, out, false);
        if (rc) return rc;
    }
    settle(g);
    return SVH_OK;
}

// Every image: the buffers, room for an image bound for the host, then draw(dst), which makes the layers it reads current and
// enqueues its launches into `dst` (their one check follows here), then finish().  dyn: the image reads the planes of the dynamics
template <typename Draw>
int render_with(svh_grid* g, uint8_t* rgb, bool on_device, bool dyn, Draw draw) {
    int rc = ready(g);
    if (rc || (dyn && (rc = dyn_ready(g)))) return rc;
    const size_t bytes = g->ncells * 3;
    if (!on_device) {
        GRID_GROW(g->d_rgb, bytes);
        GRID_GROW(g->h_out, bytes);
    }
    if ((rc = draw(on_device ? rgb : g->d_rgb.p))) return rc;
    GRID_TRY(launch, hipGetLastError());
    return finish(g, g->d_rgb, bytes, rgb, on_device);
}

// the job of an image of the finished planes in `mode` (a grid::Mode, M_LOCAL included)
grid::RenderJob render_job(const svh_grid* g, int32_t mode, uint8_t* dst) {
    grid::RenderJob j;
    j.prm = g->prm;
    j.mode = mode;
    j.count = g->iplane(F_COUNT), j.pass = g->iplane(F_PASS);
    j.hmin = g->fplane(F_HMIN), j.hmax = g->fplane(F_HMAX), j.hmean = g->fplane(F_HMEAN);
    j.intensity = g->bplane(B_INTENSITY), j.cls = g->bplane(B_CLASS);
    j.rgb = dst;
    return j;
}

int render(svh_grid* g, int32_t mode, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        const int rc = finalise(g);
        if (!rc) grid::launch_render(g->stream, render_job(g, mode, dst));
        return rc;
    });
}

// a plane of the layer in logical order
int get_dyn(svh_grid* g, int32_t plane, int32_t* out, bool on_device) {
    int rc = ready(g);
    if (rc || (rc = dyn_ready(g))) return rc;
    const size_t bytes = g->ncells * sizeof(int32_t);
    if (!on_device) GRID_GROW(g->d_dyn, bytes);
    int32_t* dst = on_device ? out : g->d_dyn.p;
    GRID_TRY(launch, (grid::launch_dyn_get(g->stream, g->prm, plane, g->stamp, g->dplanes(), dst), hipGetLastError()));
    return finish(g, g->d_dyn, bytes, out, on_device);
}

int render_dyn(svh_grid* g, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, true, [&](uint8_t* dst) {
        const int rc = finalise(g);
        if (!rc) grid::launch_render_dyn(g->stream, render_job(g, grid::M_LOCAL, dst), g->dplanes());
        return rc;
    });
}

// svh_grid_trav_params -> grid::TravParams with the derived values and the cost table for a cell side; false: out of range
bool convert_trav(const svh_grid_trav_params* t, float cell, grid::TravParams* q, std::vector<uint8_t>* table) {
    if (!t) return false;
    q->max_slope = t->max_slope, q->inscribed = t->inscribed, q->inflate = t->inflate, q->lethal = t->lethal;
    if (!grid::trav_derive(*q, cell)) return false;
    if (table) {
        table->resize((size_t)q->reach * (size_t)q->reach + 1);
        for (size_t d2 = 0; d2 < table->size(); d2++) (*table)[d2] = grid::cost_of((int32_t)d2, cell, q->inscribed, q->inflate);
    }
    return true;
}

// the cost table lies on the device
int send_table(svh_grid* g) {
    if (has(g, UP_TABLE)) return SVH_OK;
    GRID_TRY(none, hipSetDevice(g->device));
    const size_t bytes = g->table.size();
    GRID_GROW(g->d_table, bytes);
    GRID_GROW(g->h_table, bytes);
    memcpy(g->h_table, g->table.data(), bytes);
    GRID_TRY(copy, hipMemcpyAsync(g->d_table, g->h_table, bytes, hipMemcpyHostToDevice, g->stream));
    GRID_TRY(wait, hipStreamSynchronize(g->stream));   // the staging buffer is free again
    g->valid |= UP_TABLE;
    return SVH_OK;
}

// the finished planes and the three traversability planes, launched on the stream and pending until the caller has waited and settles
int traverse(svh_grid* g) {
    if (has(g, TRAV)) return SVH_OK;
    GRID_GROW(g->trav, g->ncells * kTravBytes);
    int rc = send_table(g);
    if (rc) return rc;
    if ((rc = finalise(g))) return rc;
    grid::TravJob j;
    j.trv = g->trv;
    j.nx = g->prm.nx, j.nz = g->prm.nz;
    j.cls = g->bplane(B_CLASS), j.hmean = g->fplane(F_HMEAN), j.state = g->bplane(B_STATE);
    j.table = g->d_table.p;
    j.flags = g->t_flags(), j.g = g->t_g(), j.dist2 = g->t_dist2(), j.cost = g->t_cost();
    GRID_TRY(launch, (grid::launch_trav(g->stream, j), hipGetLastError()));
    g->pending |= TRAV;
    return SVH_OK;
}

int get_trav(svh_grid* g, int32_t plane, void* out, bool on_device) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = traverse(g))) return rc;
    const void* src = plane == grid::TV_FLAGS ? (const void*)g->t_flags() : plane == grid::TV_DIST2 ? (const void*)g->t_dist2()
                                                                                                   : (const void*)g->t_cost();
    if ((rc = deliver(g, src, g->ncells * (plane == grid::TV_DIST2 ? 4 : 1), out, on_device))) return rc;
    settle(g);
    return SVH_OK;
}

// the job of the image of COST, which the images of the layers above it draw over
grid::RenderCostJob cost_job(const svh_grid* g, uint8_t* dst) {
    grid::RenderCostJob j;
    j.nx = g->prm.nx, j.nz = g->prm.nz;
    j.cost = g->t_cost(), j.flags = g->t_flags();
    j.rgb = dst;
    return j;
}

int render_cost(svh_grid* g, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        const int rc = traverse(g);
        if (!rc) grid::launch_render_cost(g->stream, cost_job(g, dst));
        return rc;
    });
}

// ---- the planner ----------------------------------------------------------------------------------------------------------
void forget_goals(svh_grid* g) {
    g->goals.clear();
    touch(g, GOALS);
    g->pose_goals.clear();   // the pose planner's too: svh_grid_clear and svh_grid_set_window end a scene for both
    touch(g, POSE_GOALS);
}

size_t plan_tiles(const grid::Params& p) {
    return ((size_t)(p.nx + grid::PLAN_TILE - 1) / grid::PLAN_TILE) * ((size_t)(p.nz + grid::PLAN_TILE - 1) / grid::PLAN_TILE);
}

// The rounds of the relaxation on a seeded job, until a round finds its list empty: g_rounds_per_wait launches, then the control
// words come back through `h_ctl` (pinned) and the host waits.  The kernel strides over its list, so the number of workgroups
// is a matter of speed alone: a tile of round r + k lies within k tiles of one of round r, so (2 k + 1)^2 times the known
// length bounds the list.  Three bounds keep a bug from hanging: the sweeps of a tile, these rounds, the walk.
// The loop serves the planner and the pose planner alike: `relax(round, blocks)` launches one round of whichever, over `tiles`
// tiles seeded by `n_goals` goals, with the control words `ctl` (PlanCtl) and at most `limit` rounds; `unsettled` is what it says of a
// relaxation that goes beyond them.
template <typename Relax>
int relax_rounds(hipStream_t s, uint64_t tiles, uint64_t limit, uint64_t n_goals, const uint32_t* ctl, uint32_t* h_ctl, const char* unsettled, Relax relax) {
    uint64_t known = std::min<uint64_t>(tiles, 4 * n_goals);   // a goal's 3 x 3 cells touch at most four tiles
    for (uint64_t round = 0; known > 0;) {
        if (round >= limit) return svh::fail(SVH_ERR_HIP, unsettled);
        for (int k = 0, per_wait = g_rounds_per_wait; k < per_wait; k++, round++) {
            const uint64_t reach = (uint64_t)(2 * k + 1) * (uint64_t)(2 * k + 1);
            relax((uint32_t)round, (uint32_t)std::min(tiles, known * reach));
        }
        GRID_TRY(launch, hipGetLastError());
        GRID_TRY(copy, hipMemcpyAsync(h_ctl, ctl, grid::CTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        known = h_ctl[grid::CTL_LEN + round % 3];   // the list of the round to come
    }
    return SVH_OK;
}

int plan_rounds(hipStream_t s, const grid::PlanJob& j, uint32_t* h_ctl) {
    return relax_rounds(s, (uint64_t)grid::plan_tiles_x(j) * grid::plan_tiles_y(j), (uint64_t)j.nx * (uint64_t)j.nz + 2, (uint64_t)j.n_goals, j.ctl, h_ctl,
                        "Grid: the relaxation of the plan did not settle within nx * nz + 2 rounds",
                        [&](uint32_t round, uint32_t blocks) { grid::launch_plan_relax(s, j, round, blocks); });
}

// seed, rounds, DIR on buffers that exist; the control words of the finished field are in h_ctl when it returns
int plan_run(hipStream_t s, const grid::PlanJob& j, uint32_t* h_ctl) {
    const size_t tiles = (size_t)grid::plan_tiles_x(j) * grid::plan_tiles_y(j);
    GRID_TRY(copy, hipMemsetAsync(j.flags, 0, 2 * tiles * sizeof(uint32_t), s));
    GRID_TRY(copy, hipMemsetAsync(j.ctl, 0, grid::CTL_WORDS * sizeof(uint32_t), s));
    GRID_TRY(launch, (grid::launch_plan_seed(s, j), hipGetLastError()));
    const int rc = plan_rounds(s, j, h_ctl);
    if (rc) return rc;
    GRID_TRY(launch, (grid::launch_plan_dir(s, j), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(h_ctl, j.ctl, grid::CTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    return SVH_OK;
}

// `n` cells (pairs) from the host to `dst` through the pinned staging buffer, and the wait
int send_cells(svh_grid* g, const int32_t* cells, int64_t n, HipBuf<int32_t>& dst) {
    const size_t bytes = (size_t)n * 2 * sizeof(int32_t);
    GRID_GROW(dst, bytes);
    GRID_GROW(g->h_cells, bytes);
    memcpy(g->h_cells, cells, bytes);
    GRID_TRY(copy, hipMemcpyAsync(dst, g->h_cells, bytes, hipMemcpyHostToDevice, g->stream));
    GRID_TRY(wait, hipStreamSynchronize(g->stream));   // the staging buffer is free again
    return SVH_OK;
}

grid::PlanJob plan_job(const svh_grid* g) {
    grid::PlanJob j;
    const size_t tiles = plan_tiles(g->prm);
    j.pln = g->pln;
    j.nx = g->prm.nx, j.nz = g->prm.nz, j.oa = g->prm.oa, j.ob = g->prm.ob;
    j.cost = g->t_cost();
    j.price = g->p_price(), j.pot = g->p_pot(), j.dir = g->p_dir();
    j.goals = g->d_goals.p, j.n_goals = (int32_t)(g->goals.size() / 2);
    j.lists = g->plan_tiles.p, j.flags = g->plan_tiles.p + 2 * tiles;
    j.ctl = g->plan_ctl.p;
    return j;
}

// the field is valid: the cost planes, then seed, rounds and DIR; complete when it returns
int plan_field(svh_grid* g) {
    if (has(g, PLAN)) return SVH_OK;
    const size_t tiles = plan_tiles(g->prm);
    GRID_GROW(g->plan, g->ncells * kPlanBytes);
    GRID_GROW(g->plan_tiles, 4 * tiles * sizeof(uint32_t));
    GRID_GROW(g->plan_ctl, grid::CTL_WORDS * sizeof(uint32_t));
    GRID_GROW(g->h_ctl, grid::CTL_WORDS * sizeof(uint32_t));
    int rc;
    if (!has(g, UP_GOALS) && !g->goals.empty() && (rc = send_cells(g, g->goals.data(), (int64_t)(g->goals.size() / 2), g->d_goals))) return rc;
    g->valid |= UP_GOALS;
    if ((rc = traverse(g))) return rc;
    if ((rc = plan_run(g->stream, plan_job(g), g->h_ctl))) return rc;
    const uint32_t* h = g->h_ctl;
    g->plan_counted = h[grid::CTL_COUNTED], g->plan_rounds = h[grid::CTL_ROUNDS];
    g->plan_reached = (int64_t)((uint64_t)h[grid::CTL_REACHED] | ((uint64_t)h[grid::CTL_REACHED + 1] << 32));
    g->pending |= PLAN;
    settle(g);
    return SVH_OK;
}

int get_plan(svh_grid* g, int32_t plane, void* out, bool on_device) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = plan_field(g))) return rc;
    return plane == grid::PL_POT ? deliver(g, g->p_pot(), g->ncells * 4, out, on_device) : deliver(g, g->p_dir(), g->ncells, out, on_device);
}

// the walk from the window cell (a, b)
int plan_path(svh_grid* g, int32_t a, int32_t b, int32_t* cells, int64_t cap, int64_t* len, int32_t* cost, int32_t* status) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = plan_field(g))) return rc;
    const int64_t room = std::min<int64_t>(cap, (int64_t)g->ncells);   // a path has at most nx * nz cells
    GRID_GROW_N(g->d_path, 2 * room);
    GRID_GROW(g->d_walk, 3 * sizeof(int64_t));
    GRID_GROW(g->h_walk, 3 * sizeof(int64_t));
    GRID_TRY(launch, (grid::launch_plan_walk(g->stream, plan_job(g), a, b, g->d_path, room, g->d_walk), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(g->h_walk, g->d_walk, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    GRID_TRY(wait, hipStreamSynchronize(g->stream));
    const int64_t n = g->h_walk[1], m = std::min(n, room);
    if (m > 0 && (rc = deliver(g, g->d_path, (size_t)m * 2 * sizeof(int32_t), cells, false))) return rc;
    *status = (int32_t)g->h_walk[0], *len = n, *cost = (int32_t)g->h_walk[2];
    return SVH_OK;
}

int render_plan(svh_grid* g, const int32_t* cells, int64_t n, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        int rc = plan_field(g);
        if (rc || (n > 0 && (rc = send_cells(g, cells, n, g->d_path)))) return rc;
        const grid::PlanJob pj = plan_job(g);
        grid::launch_render_cost(g->stream, cost_job(g, dst));
        grid::launch_plan_overlay(g->stream, pj, pj.goals, pj.n_goals, true, dst);
        grid::launch_plan_overlay(g->stream, pj, g->d_path, n, false, dst);
        return rc;
    });
}

// ---- the frontiers --------------------------------------------------------------------------------------------------------
const char* const kUnsettled = "Grid: the labelling of the frontiers did not settle within its bounds";

// The whole computation on a job whose planes exist (state, cost, flags, label): FRONT_LAUNCHES launches whatever the scene, and
// two waits -- the number of components sizes the accumulators, so it comes back through pinned memory before they are made;
// the kept count comes back the same way at the end.  The table stays on the device.  Complete when it returns.
int front_run(hipStream_t s, grid::FrontJob& j, FrontBufs& b, int64_t stats[grid::FS_WORDS]) {
    const size_t ctl_bytes = grid::FC_WORDS * sizeof(unsigned long long);
    GRID_GROW_N(b.blocks, grid::front_blocks(j));
    GRID_GROW(b.ctl, ctl_bytes);
    GRID_GROW(b.h_ctl, ctl_bytes);
    j.blockcnt = b.blocks, j.ctl = b.ctl;
    GRID_TRY(copy, hipMemsetAsync(j.ctl, 0, ctl_bytes, s));
    int64_t launches = grid::launch_front_mask(s, j);
    launches += grid::launch_front_label(s, j);
    launches += grid::launch_front_count(s, j);
    GRID_TRY(launch, hipGetLastError());
    GRID_TRY(copy, hipMemcpyAsync(b.h_ctl, j.ctl, ctl_bytes, hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    const unsigned long long* h = b.h_ctl;
    if (h[grid::FC_UNSETTLED]) return svh::fail(SVH_ERR_HIP, kUnsettled);
    const size_t n = (size_t)h[grid::FC_COMPONENTS], room = n ? n : 1;
    const size_t kept_cap = std::min<size_t>(n, (size_t)h[grid::FC_CELLS] / (size_t)j.frp.min_size);   // a kept component has min_size cells
    GRID_GROW_N(b.roots, n);
    GRID_GROW(b.acc, grid::FRONT_COMP_BYTES * room);
    GRID_GROW_N(b.recs, (size_t)grid::FRONT_REC * kept_cap);
    j.n_comp = (int32_t)n, j.roots = b.roots, j.acc = b.acc, j.recs = b.recs;
    const grid::FrontAcc acc = grid::front_acc(j.acc, room);
    GRID_TRY(copy, hipMemsetAsync(j.acc, 0, grid::FRONT_COMP_BYTES * room, s));
    GRID_TRY(copy, hipMemsetAsync(acc.rep, 0xFF, 8 * room, s));
    GRID_TRY(copy, hipMemsetAsync(acc.bmin, 0x7F, 8 * room, s));
    launches += grid::launch_front_table(s, j);
    GRID_TRY(launch, hipGetLastError());
    GRID_TRY(copy, hipMemcpyAsync(b.h_ctl, j.ctl, ctl_bytes, hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    if (h[grid::FC_UNSETTLED]) return svh::fail(SVH_ERR_HIP, kUnsettled);
    stats[grid::FS_CELLS] = (int64_t)h[grid::FC_CELLS], stats[grid::FS_COMPONENTS] = (int64_t)h[grid::FC_COMPONENTS];
    stats[grid::FS_KEPT] = (int64_t)h[grid::FC_KEPT], stats[grid::FS_KEPT_CELLS] = (int64_t)h[grid::FC_KEPT_CELLS];
    stats[grid::FS_LAUNCHES] = launches;
    return SVH_OK;
}

// the frontier result is valid: the cost planes, then front_run
int frontiers(svh_grid* g) {
    if (has(g, FRONT)) return SVH_OK;
    GRID_GROW(g->front, g->ncells * kFrontBytes);
    int rc = traverse(g);
    if (rc) return rc;
    grid::FrontJob j;
    j.frp = g->frp;
    j.nx = g->prm.nx, j.nz = g->prm.nz, j.oa = g->prm.oa, j.ob = g->prm.ob;
    j.state = g->bplane(B_STATE), j.cost = g->t_cost();
    j.flags = g->f_flags(), j.label = g->f_label();
    int64_t stats[grid::FS_WORDS];
    if ((rc = front_run(g->stream, j, g->front_bufs, stats))) return rc;
    memcpy(g->front_stats, stats, sizeof(stats));
    g->pending |= FRONT;
    settle(g);
    return SVH_OK;
}

int get_front(svh_grid* g, int32_t plane, void* out, bool on_device) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = frontiers(g))) return rc;
    return plane == grid::FP_LABEL ? deliver(g, g->f_label(), g->ncells * 4, out, on_device) : deliver(g, g->f_flags(), g->ncells, out, on_device);
}

// *n = the kept components, the first min(*n, cap) records to the host
int get_frontiers(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = frontiers(g))) return rc;
    const int64_t kept = g->front_stats[grid::FS_KEPT], m = std::min(kept, cap);
    if (m > 0 && (rc = deliver(g, g->front_bufs.recs, (size_t)m * grid::FRONT_REC * sizeof(int32_t), recs, false))) return rc;
    *n = kept;
    return SVH_OK;
}

int render_frontiers(svh_grid* g, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        const int rc = frontiers(g);
        if (rc) return rc;
        grid::launch_render_cost(g->stream, cost_job(g, dst));
        grid::launch_front_overlay(g->stream, g->prm.nx, g->prm.nz, g->f_flags(), dst);
        return rc;
    });
}

bool convert_front(const svh_grid_front_params* p, grid::FrontParams* q) {
    if (!p) return false;
    *q = grid::FrontParams{p->max_cell_cost, p->min_size, p->unexplored, p->border};
    return grid::front_ok(*q);
}

// ---- the objects and their tracks -------------------------------------------------------------------------------------------
const char* const kObjUnsettled = "Grid: the labelling of the objects did not settle within its bounds";
const char* const kStepUnsettled = "Grid: the table of overlap pairs of a step overflowed its probe bound";

bool convert_obj(const svh_grid_obj_params* p, grid::ObjParams* q) {
    if (!p) return false;
    *q = grid::ObjParams{p->min_size,   p->max_size, p->min_height, p->max_tracks, p->min_overlap,
                         p->gate,       p->max_missed, p->min_age,  p->move_cells, p->smooth_shift};
    return grid::obj_ok(*q);
}

// The whole computation on a job whose planes exist (state, hmax, count, flags, label): OBJ_LAUNCHES launches whatever the scene
// and two waits, as front_run.  The table, the roots and the ranks stay on the device.  Complete when it returns.
int obj_run(hipStream_t s, grid::ObjJob& j, ObjBufs& b, int64_t stats[grid::OS_WORDS]) {
    const size_t ctl_bytes = grid::FC_WORDS * sizeof(unsigned long long);
    GRID_GROW_N(b.blocks, ((size_t)j.nx * (size_t)j.nz + grid::FRONT_SCAN_BLOCK - 1) / grid::FRONT_SCAN_BLOCK);
    GRID_GROW(b.ctl, ctl_bytes);
    GRID_GROW(b.h_ctl, ctl_bytes);
    j.blockcnt = b.blocks, j.ctl = b.ctl;
    GRID_TRY(copy, hipMemsetAsync(j.ctl, 0, ctl_bytes, s));
    int64_t launches = grid::launch_obj_mask(s, j);
    launches += grid::launch_obj_label(s, j);
    GRID_TRY(launch, hipGetLastError());
    GRID_TRY(copy, hipMemcpyAsync(b.h_ctl, j.ctl, ctl_bytes, hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    const unsigned long long* h = b.h_ctl;
    if (h[grid::FC_UNSETTLED]) return svh::fail(SVH_ERR_HIP, kObjUnsettled);
    const size_t n = (size_t)h[grid::FC_COMPONENTS], room = n ? n : 1;
    const size_t kept_cap = std::min<size_t>(n, (size_t)h[grid::FC_CELLS] / (size_t)j.op.min_size);   // a kept component has min_size cells
    GRID_GROW_N(b.roots, n);
    GRID_GROW_N(b.slot, n);
    GRID_GROW(b.acc, grid::OBJ_COMP_BYTES * room);
    GRID_GROW_N(b.recs, (size_t)grid::OBJ_REC * kept_cap);
    j.n_comp = (int32_t)n, j.roots = b.roots, j.slot = b.slot, j.acc = b.acc, j.recs = b.recs;
    const grid::ObjAcc acc = grid::obj_acc(j.acc, room);
    GRID_TRY(copy, hipMemsetAsync(j.acc, 0, grid::OBJ_COMP_BYTES * room, s));
    GRID_TRY(copy, hipMemsetAsync(acc.bmin, 0x7F, 8 * room, s));
    launches += grid::launch_obj_table(s, j);
    GRID_TRY(launch, hipGetLastError());
    GRID_TRY(copy, hipMemcpyAsync(b.h_ctl, j.ctl, ctl_bytes, hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    if (h[grid::FC_UNSETTLED]) return svh::fail(SVH_ERR_HIP, kObjUnsettled);
    stats[grid::OS_CELLS] = (int64_t)h[grid::FC_CELLS], stats[grid::OS_COMPONENTS] = (int64_t)h[grid::FC_COMPONENTS];
    stats[grid::OS_KEPT] = (int64_t)h[grid::FC_KEPT], stats[grid::OS_KEPT_CELLS] = (int64_t)h[grid::FC_KEPT_CELLS];
    stats[grid::OS_LARGE] = (int64_t)h[grid::OC_LARGE], stats[grid::OS_LOW] = (int64_t)h[grid::OC_LOW];
    stats[grid::OS_LAUNCHES] = launches;
    return SVH_OK;
}

// the objects are valid: the finished planes, then obj_run
int objects(svh_grid* g) {
    if (has(g, OBJ)) return SVH_OK;
    GRID_GROW(g->obj, g->ncells * kFrontBytes);
    int rc = finalise(g);
    if (rc) return rc;
    grid::ObjJob j;
    j.op = g->obp;
    j.nx = g->prm.nx, j.nz = g->prm.nz, j.oa = g->prm.oa, j.ob = g->prm.ob;
    j.state = g->bplane(B_STATE), j.hmax = g->fplane(F_HMAX), j.count = g->iplane(F_COUNT);
    j.flags = g->o_flags(), j.label = g->o_label();
    int64_t stats[grid::OS_WORDS];
    if ((rc = obj_run(g->stream, j, g->obj_bufs, stats))) return rc;
    memcpy(g->obj_stats, stats, sizeof(stats));
    g->pending |= OBJ;
    settle(g);
    return SVH_OK;
}

int get_obj(svh_grid* g, int32_t plane, void* out, bool on_device) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = objects(g))) return rc;
    return plane == grid::OP_LABEL ? deliver(g, g->o_label(), g->ncells * 4, out, on_device) : deliver(g, g->o_flags(), g->ncells, out, on_device);
}

// *n = the kept components, the first min(*n, cap) records to the host
int get_objects(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = objects(g))) return rc;
    const int64_t kept = g->obj_stats[grid::OS_KEPT], m = std::min(kept, cap);
    if (m > 0 && (rc = deliver(g, g->obj_bufs.recs, (size_t)m * grid::OBJ_REC * sizeof(int32_t), recs, false))) return rc;
    *n = kept;
    return SVH_OK;
}

// The scratch of a step on a job that is complete but for it: the table of pairs all ones, its counts and the claims zero, the
// picks and matches all ones, the control words zero
int step_scratch(hipStream_t s, grid::ObjStepJob& j, TrackBufs& b, int64_t kept_cells) {
    const size_t no = (size_t)j.n_obj, nt = (size_t)j.n_prev;
    j.capacity = grid::obj_step_capacity(kept_cells, j.n_obj, j.n_prev);
    const size_t zero = grid::OBJ_STEP_ZERO_OBJ * no + grid::OBJ_STEP_ZERO_TRK * nt, ones = grid::OBJ_STEP_ONES_OBJ * no + grid::OBJ_STEP_ONES_TRK * nt;
    GRID_GROW_N(b.keys, j.capacity);
    GRID_GROW_N(b.counts, j.capacity);
    GRID_GROW(b.zero, zero ? zero : 8);
    GRID_GROW(b.ones, ones ? ones : 8);
    GRID_GROW_N(b.assign, no);
    GRID_GROW(b.ctl, grid::SC_WORDS * sizeof(unsigned long long));
    j.keys = b.keys, j.counts = b.counts, j.zero = b.zero, j.ones = b.ones, j.assign = b.assign, j.ctl = b.ctl;
    GRID_TRY(copy, hipMemsetAsync(j.keys, 0xFF, (size_t)j.capacity * sizeof(unsigned long long), s));
    GRID_TRY(copy, hipMemsetAsync(j.counts, 0, (size_t)j.capacity * sizeof(int32_t), s));
    if (zero) GRID_TRY(copy, hipMemsetAsync(j.zero, 0, zero, s));
    if (ones) GRID_TRY(copy, hipMemsetAsync(j.ones, 0xFF, ones, s));
    GRID_TRY(copy, hipMemsetAsync(j.ctl, 0, grid::SC_WORDS * sizeof(unsigned long long), s));
    return SVH_OK;
}

// One step: the objects made current, then the overlap, the claims, the gate, the update and the new ID plane in 5 or 7 launches
// and one wait, with the control words and the first min(kept, cap) of ASSIGN coming back through pinned memory
int objects_step(svh_grid* g, int32_t* assign, int64_t cap, int64_t* n_obj) {
    int rc = ready(g);
    if (rc || (rc = objects(g))) return rc;
    hipStream_t s = g->stream;
    TrackBufs& b = g->trk;
    const int cur = g->trk_cur, nxt = 1 - cur;
    for (int k = 0; k < 2; k++) {
        GRID_GROW_N(b.table[k], (size_t)g->obp.max_tracks * grid::TRACK_REC);
        GRID_GROW_N(b.id[k], g->ncells);
    }
    grid::ObjStepJob j;
    j.op = g->obp;
    j.nx = g->prm.nx, j.nz = g->prm.nz, j.oa = g->prm.oa, j.ob = g->prm.ob, j.poa = g->trk_oa, j.pob = g->trk_ob;
    j.flags = g->o_flags(), j.label = g->o_label();
    j.roots = g->obj_bufs.roots, j.slot = g->obj_bufs.slot, j.n_comp = (int32_t)g->obj_stats[grid::OS_COMPONENTS];
    j.recs = g->obj_bufs.recs, j.n_obj = (int32_t)g->obj_stats[grid::OS_KEPT];
    j.prev_id = b.id[cur], j.prev = b.table[cur];
    j.n_prev = g->trk_plane ? g->trk_n : 0, j.next_id = g->trk_next;
    j.tracks = b.table[nxt], j.id = b.id[nxt];
    if ((rc = step_scratch(s, j, b, g->obj_stats[grid::OS_KEPT_CELLS]))) return rc;
    const size_t ctl_bytes = grid::SC_WORDS * sizeof(unsigned long long);
    const size_t m = (size_t)std::min<int64_t>(j.n_obj, cap);
    GRID_GROW(b.h_out, ctl_bytes + m * sizeof(int32_t));
    GRID_TRY(launch, (grid::launch_obj_step(s, j), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(b.h_out, j.ctl, ctl_bytes, hipMemcpyDeviceToHost, s));
    if (m > 0) GRID_TRY(copy, hipMemcpyAsync(b.h_out + ctl_bytes, j.assign, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    const unsigned long long* h = (const unsigned long long*)b.h_out.p;
    if (h[grid::SC_UNSETTLED]) return svh::fail(SVH_ERR_HIP, kStepUnsettled);
    if (m > 0) memcpy(assign, b.h_out + ctl_bytes, m * sizeof(int32_t));
    touch(g, TRACKS);
    g->trk_cur = nxt, g->trk_plane = true;
    g->trk_n = (int32_t)h[grid::SC_TRACKS], g->trk_next += (int32_t)h[grid::SC_NEW];
    g->trk_oa = j.oa, g->trk_ob = j.ob;
    g->trk_stats[grid::TS_STEPS]++;
    g->trk_stats[grid::TS_TRACKS] = g->trk_n;
    g->trk_stats[grid::TS_BY_OVERLAP] = (int64_t)h[grid::SC_BY_OVERLAP], g->trk_stats[grid::TS_BY_GATE] = (int64_t)h[grid::SC_BY_GATE];
    g->trk_stats[grid::TS_NEW] = (int64_t)h[grid::SC_NEW], g->trk_stats[grid::TS_MISSED] = (int64_t)h[grid::SC_MISSED];
    g->trk_stats[grid::TS_DROPPED] = (int64_t)h[grid::SC_DROPPED], g->trk_stats[grid::TS_UNTRACKED] = (int64_t)h[grid::SC_UNTRACKED];
    *n_obj = j.n_obj;
    return SVH_OK;
}

int get_tracks(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n) {
    const int64_t m = std::min<int64_t>(g->trk_n, cap);
    if (m > 0) {
        GRID_TRY(none, hipSetDevice(g->device));
        const int rc = deliver(g, g->trk.table[g->trk_cur], (size_t)m * grid::TRACK_REC * sizeof(int32_t), recs, false);
        if (rc) return rc;
    }
    *n = g->trk_n;
    return SVH_OK;
}

int get_track_plane(svh_grid* g, int32_t* out, bool on_device) {
    GRID_TRY(none, hipSetDevice(g->device));
    const size_t bytes = g->ncells * sizeof(int32_t);
    GRID_GROW_N(g->trk.id[g->trk_cur], g->ncells);
    if (!g->trk_plane) GRID_TRY(copy, hipMemsetAsync(g->trk.id[g->trk_cur], 0xFF, bytes, g->stream));
    return deliver(g, g->trk.id[g->trk_cur], bytes, out, on_device);
}

int render_objects(svh_grid* g, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        const int rc = objects(g);
        if (rc) return rc;
        const TrackBufs& b = g->trk;
        grid::launch_render(g->stream, render_job(g, grid::M_CLASS, dst));
        grid::launch_obj_overlay(g->stream, g->prm.nx, g->prm.nz, g->prm.oa, g->prm.ob, g->o_flags(), g->trk_plane ? b.id[g->trk_cur].p : nullptr,
                                 g->trk_oa, g->trk_ob, b.table[g->trk_cur].p, g->trk_plane ? g->trk_n : 0, dst);
        return rc;
    });
}

// ---- the rollouts ---------------------------------------------------------------------------------------------------------
bool convert_roll(const svh_grid_roll_params* p, grid::RollParams* q) {
    if (!p) return false;
    *q = grid::RollParams{p->front, p->rear, p->half_width, p->headings_m, p->stop_cost, p->unknown_cost, p->w_pot, p->w_cost, p->w_cut};
    return grid::roll_ok(*q);
}

// the footprint table lies on the device; complete when it returns SVH_OK.  Both sources belong to `t`: they outlive a copy that
// a failed call leaves in flight until its caller has drained the stream
int send_roll_table(hipStream_t s, const RollTable& t, RollBufs& b) {
    GRID_GROW_N(b.offs, t.offs.size());
    GRID_GROW_N(b.start, t.start32.size());
    GRID_TRY(copy, hipMemcpyAsync(b.offs, t.offs.data(), t.offs.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    GRID_TRY(copy, hipMemcpyAsync(b.start, t.start32.data(), t.start32.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    return SVH_OK;
}

// a job on planes and a table that lie on the device; the candidates and the outputs are the caller's to fill in
grid::RollJob roll_job(const RollTable& t, const RollBufs& b, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost,
                       const int32_t* pot) {
    grid::RollJob j;
    j.rp = t.p;
    j.nx = nx, j.nz = nz, j.oa = oa, j.ob = ob;
    j.cost = cost, j.pot = pot;
    j.offs = (const int2*)b.offs.p, j.start = b.start.p;
    j.group = grid::roll_group(t.longest);
    return j;
}

// set `set` of a table of K x T on the device, anchored at the global cell (ga, gb), with the outputs of `b`, which exist
void roll_candidates(grid::RollJob& j, const RollBufs& b, const int32_t* d_cands, const int32_t* d_lens, int32_t set, int32_t K, int32_t T,
                     int32_t ga, int32_t gb) {
    j.cands = d_cands + (size_t)set * (size_t)K * (size_t)T * 3, j.lens = d_lens + (size_t)set * (size_t)K;
    j.K = K, j.T = T, j.ga0 = ga, j.gb0 = gb;
    j.recs = b.recs.p, j.scores = b.scores.p, j.best = b.best.p;
}

int roll_outputs(RollBufs& b, int32_t K) {
    GRID_GROW_N(b.recs, (size_t)grid::ROLL_REC * (size_t)K);
    GRID_GROW_N(b.scores, K);
    GRID_GROW_N(b.best, 1);
    return SVH_OK;
}

// both tables lie on the device
int roll_tables(svh_grid* g, bool candidates) {
    GRID_TRY(none, hipSetDevice(g->device));
    if (!has(g, UP_ROLL)) {
        const int rc = send_roll_table(g->stream, g->rol, g->roll_bufs);
        if (rc) return rc;
        g->valid |= UP_ROLL;
    }
    if (candidates && !has(g, UP_CANDS)) {
        GRID_GROW_N(g->d_cands, g->cands.size());
        GRID_GROW_N(g->d_cand_lens, g->cand_lens.size());
        GRID_TRY(copy, hipMemcpyAsync(g->d_cands, g->cands.data(), g->cands.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
        GRID_TRY(copy, hipMemcpyAsync(g->d_cand_lens, g->cand_lens.data(), g->cand_lens.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
        GRID_TRY(wait, hipStreamSynchronize(g->stream));
        g->valid |= UP_CANDS;
    }
    return SVH_OK;
}

grid::RollJob roll_job(const svh_grid* g) {
    return roll_job(g->rol, g->roll_bufs, g->prm.nx, g->prm.nz, g->prm.oa, g->prm.ob, g->t_cost(), g->rol.p.w_pot != 0 ? g->p_pot() : nullptr);
}

// F of n > 0 poses with arguments that have been checked
int footprint_cost(svh_grid* g, const int32_t* poses, int64_t n, bool on_device, int32_t* out) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = roll_tables(g, false))) return rc;
    if (!on_device) {
        GRID_GROW_N(g->d_poses, 3 * n);
        GRID_GROW_N(g->d_fcost, n);
        GRID_GROW(g->h_out, (size_t)n * sizeof(int32_t));
        GRID_TRY(copy, hipMemcpyAsync(g->d_poses, poses, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    }
    if ((rc = traverse(g))) return rc;
    grid::launch_footprint_cost(g->stream, roll_job(g), on_device ? poses : g->d_poses.p, n, on_device ? out : g->d_fcost.p);
    GRID_TRY(launch, hipGetLastError());
    return finish(g, g->d_fcost, (size_t)n * sizeof(int32_t), out, on_device);
}

// set `set` scored at the global cell (ga, gb); recs and scores may be null
int roll_score(svh_grid* g, int32_t ga, int32_t gb, int32_t set, int32_t* recs, int64_t* scores, bool on_device, int32_t* best) {
    int rc = ready(g);
    if (rc) return rc;
    const int32_t K = g->cand_K;
    const size_t rec_bytes = (size_t)K * grid::ROLL_REC * sizeof(int32_t), score_bytes = (size_t)K * sizeof(int64_t);
    drop(g, ROLL_LAST);
    if ((rc = roll_outputs(g->roll_bufs, K))) return rc;
    GRID_GROW(g->h_roll, score_bytes + rec_bytes + sizeof(int32_t));   // the scores first: they are the widest
    if ((rc = roll_tables(g, true))) return rc;
    if ((rc = g->rol.p.w_pot != 0 ? plan_field(g) : traverse(g))) return rc;
    grid::RollJob j = roll_job(g);
    roll_candidates(j, g->roll_bufs, g->d_cands, g->d_cand_lens, set, K, g->cand_T, ga, gb);
    hipStream_t s = g->stream;
    GRID_TRY(launch, (grid::launch_roll_score(s, j), hipGetLastError()));
    uint8_t* h = g->h_roll;
    if (scores) GRID_TRY(copy, hipMemcpyAsync(on_device ? (void*)scores : (void*)h, j.scores, score_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (recs) GRID_TRY(copy, hipMemcpyAsync(on_device ? (void*)recs : (void*)(h + score_bytes), j.recs, rec_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    GRID_TRY(copy, hipMemcpyAsync(h + score_bytes + rec_bytes, j.best, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    settle(g);
    if (scores && !on_device) memcpy(scores, h, score_bytes);
    if (recs && !on_device) memcpy(recs, h + score_bytes, rec_bytes);
    memcpy(best, h + score_bytes + rec_bytes, sizeof(int32_t));
    g->valid |= ROLL_LAST;
    g->roll_last_set = set, g->roll_last_ga = ga, g->roll_last_gb = gb, g->roll_last_best = *best;
    return SVH_OK;
}

int render_roll(svh_grid* g, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        const int rc = traverse(g);
        if (rc) return rc;
        grid::RollJob j = roll_job(g);
        roll_candidates(j, g->roll_bufs, g->d_cands, g->d_cand_lens, g->roll_last_set, g->cand_K, g->cand_T, g->roll_last_ga, g->roll_last_gb);
        grid::launch_render_cost(g->stream, cost_job(g, dst));
        grid::launch_roll_overlay(g->stream, j, g->roll_last_best, dst);
        return rc;
    });
}

// ---- the pose planner -------------------------------------------------------------------------------------------------------
size_t pose_tiles(int32_t nx, int32_t nz) {
    return ((size_t)(nx + grid::POSE_TILE - 1) / grid::POSE_TILE) * ((size_t)(nz + grid::POSE_TILE - 1) / grid::POSE_TILE);
}

// a job on a footprint table that lies on the device, with the bounding boxes of the eight lists a planning heading has; the planes,
// the goals and the lists are the caller's to fill in
grid::PoseJob pose_job(const grid::PoseParams& pp, const RollTable& t, const RollBufs& b, int32_t nx, int32_t nz, int32_t oa, int32_t ob) {
    grid::PoseJob j{};
    j.pp = pp;
    j.stop_cost = t.p.stop_cost, j.unknown_cost = t.p.unknown_cost, j.m = t.p.m;
    j.nx = nx, j.nz = nz, j.oa = oa, j.ob = ob;
    j.offs = (const int2*)b.offs.p, j.start = b.start.p;
    for (int32_t d = 0; d < grid::POSE_HEADINGS; d++) {
        int32_t* box = j.box[d];
        box[0] = box[1] = box[2] = box[3] = 0;      // (0, 0) is in every list
        for (int64_t i = t.start[(size_t)d * t.p.m]; i < t.start[(size_t)d * t.p.m + 1]; i++) {
            const int32_t da = t.offs[2 * i], db = t.offs[2 * i + 1];
            box[0] = std::min(box[0], da), box[1] = std::max(box[1], da), box[2] = std::min(box[2], db), box[3] = std::max(box[3], db);
        }
    }
    return j;
}

// the planes of a job in one buffer of kPoseBytes per state, and the tile lists
void pose_planes(grid::PoseJob& j, uint8_t* field, uint32_t* tiles, uint32_t* ctl) {
    const size_t cells = (size_t)j.nx * (size_t)j.nz, n_tiles = pose_tiles(j.nx, j.nz);
    j.pot = (int32_t*)field, j.price = (uint16_t*)(field + 32 * cells), j.dir = field + 48 * cells, j.cf = field + 56 * cells;
    j.lists = tiles, j.flags = tiles + 2 * n_tiles;
    j.ctl = ctl;
}

// seed, rounds, PDIR on a job whose CF planes are written (in stream order); the control words of the finished field are in h_ctl
// when it returns
int pose_run(hipStream_t s, const grid::PoseJob& j, uint32_t* h_ctl) {
    const size_t tiles = pose_tiles(j.nx, j.nz);
    GRID_TRY(copy, hipMemsetAsync(j.flags, 0, 2 * tiles * sizeof(uint32_t), s));
    GRID_TRY(copy, hipMemsetAsync(j.ctl, 0, grid::CTL_WORDS * sizeof(uint32_t), s));
    GRID_TRY(launch, (grid::launch_pose_seed(s, j), hipGetLastError()));
    const int rc = relax_rounds(s, tiles, (uint64_t)grid::POSE_HEADINGS * (uint64_t)j.nx * (uint64_t)j.nz + 2, (uint64_t)j.n_goals, j.ctl, h_ctl,
                                "Grid: the relaxation of the pose field did not settle within 8 * nx * nz + 2 rounds",
                                [&](uint32_t round, uint32_t blocks) { grid::launch_pose_relax(s, j, round, blocks); });
    if (rc) return rc;
    GRID_TRY(launch, (grid::launch_pose_dir(s, j), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(h_ctl, j.ctl, grid::CTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    return SVH_OK;
}

grid::PoseJob pose_job(const svh_grid* g) {
    grid::PoseJob j = pose_job(g->pose_prm, g->rol, g->roll_bufs, g->prm.nx, g->prm.nz, g->prm.oa, g->prm.ob);
    j.cost = g->t_cost();
    pose_planes(j, g->pose.p, g->pose_tiles.p, g->pose_ctl.p);
    j.goals = g->d_pose_goals.p, j.n_goals = (int32_t)(g->pose_goals.size() / 3);
    return j;
}

// the buffers of the layer exist
int pose_ready(svh_grid* g) {
    GRID_GROW(g->pose, g->ncells * grid::POSE_HEADINGS * kPoseBytes);
    GRID_GROW(g->pose_tiles, 4 * pose_tiles(g->prm.nx, g->prm.nz) * sizeof(uint32_t));
    GRID_GROW(g->pose_ctl, grid::CTL_WORDS * sizeof(uint32_t));
    GRID_GROW(g->h_pose_ctl, grid::CTL_WORDS * sizeof(uint32_t));
    return SVH_OK;
}

// CF is valid or launched: the cost planes and the footprint table, then one launch, pending until the caller has waited and settles
int pose_foot(svh_grid* g) {
    if (has(g, POSE_CF) || (g->pending & POSE_CF)) return SVH_OK;
    int rc = pose_ready(g);
    if (rc || (rc = roll_tables(g, false)) || (rc = traverse(g))) return rc;
    GRID_TRY(launch, (grid::launch_pose_foot(g->stream, pose_job(g)), hipGetLastError()));
    g->pending |= POSE_CF;
    return SVH_OK;
}

// the field is valid: CF, then seed, rounds and PDIR; complete when it returns
int pose_field(svh_grid* g) {
    if (has(g, POSE)) return SVH_OK;
    int rc = pose_foot(g);
    if (rc) return rc;
    const size_t n = g->pose_goals.size();
    if (!has(g, UP_POSE_GOALS) && n > 0) {
        GRID_GROW_N(g->d_pose_goals, n);
        GRID_GROW(g->h_cells, n * sizeof(int32_t));
        memcpy(g->h_cells, g->pose_goals.data(), n * sizeof(int32_t));
        GRID_TRY(copy, hipMemcpyAsync(g->d_pose_goals, g->h_cells, n * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
        GRID_TRY(wait, hipStreamSynchronize(g->stream));   // the staging buffer is free again
    }
    g->valid |= UP_POSE_GOALS;
    if ((rc = pose_run(g->stream, pose_job(g), g->h_pose_ctl))) return rc;
    const uint32_t* h = g->h_pose_ctl;
    g->pose_counted = h[grid::CTL_COUNTED], g->pose_rounds = h[grid::CTL_ROUNDS];
    g->pose_reached = (int64_t)((uint64_t)h[grid::CTL_REACHED] | ((uint64_t)h[grid::CTL_REACHED + 1] << 32));
    g->pending |= POSE;
    settle(g);
    return SVH_OK;
}

int get_pose_plane(svh_grid* g, int32_t plane, void* out, bool on_device) {
    int rc = ready(g);
    if (rc) return rc;
    const size_t states = g->ncells * grid::POSE_HEADINGS;
    if (plane == grid::PP_CF) {
        if ((rc = pose_foot(g)) || (rc = deliver(g, g->q_cf(), states, out, on_device))) return rc;
        settle(g);
        return SVH_OK;
    }
    if ((rc = pose_field(g))) return rc;
    return plane == grid::PP_POT ? deliver(g, g->q_pot(), states * 4, out, on_device) : deliver(g, g->q_dir(), states, out, on_device);
}

// the walk from the window state (a, b, d)
int pose_path(svh_grid* g, int32_t a, int32_t b, int32_t d, int32_t* poses, int64_t cap, int64_t* len, int32_t* cost, int32_t* status) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = pose_field(g))) return rc;
    const int64_t room = std::min<int64_t>(cap, (int64_t)g->ncells * grid::POSE_HEADINGS);   // a path has at most 8 nx nz poses
    GRID_GROW_N(g->d_pose_path, 3 * room);
    GRID_GROW(g->d_walk, 3 * sizeof(int64_t));
    GRID_GROW(g->h_walk, 3 * sizeof(int64_t));
    GRID_TRY(launch, (grid::launch_pose_walk(g->stream, pose_job(g), a, b, d, g->d_pose_path, room, g->d_walk), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(g->h_walk, g->d_walk, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    GRID_TRY(wait, hipStreamSynchronize(g->stream));
    const int64_t n = g->h_walk[1], m = std::min(n, room);
    if (m > 0 && (rc = deliver(g, g->d_pose_path, (size_t)m * 3 * sizeof(int32_t), poses, false))) return rc;
    *status = (int32_t)g->h_walk[0], *len = n, *cost = (int32_t)g->h_walk[2];
    return SVH_OK;
}

int render_pose(svh_grid* g, const int32_t* poses, int64_t n, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        int rc = pose_field(g);
        if (rc) return rc;
        if (n > 0) {
            const size_t bytes = (size_t)n * 3 * sizeof(int32_t);
            GRID_GROW(g->d_pose_path, bytes);
            GRID_GROW(g->h_cells, bytes);
            memcpy(g->h_cells, poses, bytes);
            GRID_TRY(copy, hipMemcpyAsync(g->d_pose_path, g->h_cells, bytes, hipMemcpyHostToDevice, g->stream));
            GRID_TRY(wait, hipStreamSynchronize(g->stream));   // the staging buffer is free again
        }
        const grid::PoseJob pj = pose_job(g);
        grid::launch_render_cost(g->stream, cost_job(g, dst));
        grid::launch_pose_overlay(g->stream, pj, pj.goals, pj.n_goals, true, dst);
        grid::launch_pose_overlay(g->stream, pj, g->d_pose_path, n, false, dst);
        return rc;
    });
}

// the planes of a test entry on the device and the kernels on them: CF, PPOT and PDIR to the host, out as svh_grid_get_pose_stats
// without the goals given
int pose_device(const grid::PoseParams& pp, const RollTable& t, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost, const int32_t* goals,
                int32_t n, uint8_t* cf, int32_t* pot, uint8_t* dir, int64_t out[3]) {
    const size_t cells = (size_t)nx * (size_t)nz, states = cells * grid::POSE_HEADINGS, tiles = pose_tiles(nx, nz);
    HipBuf<uint8_t> d_cost, field;
    HipBuf<int32_t> d_goals;
    HipBuf<uint32_t> d_tiles, d_ctl;
    PinnedBuf<uint32_t> h_ctl;
    RollBufs b;
    hipStream_t s = nullptr;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(d_cost, cells);
        GRID_GROW(field, states * kPoseBytes);
        GRID_GROW_N(d_goals, 3 * (size_t)n);
        GRID_GROW(d_tiles, 4 * tiles * sizeof(uint32_t));
        GRID_GROW(d_ctl, grid::CTL_WORDS * sizeof(uint32_t));
        GRID_GROW(h_ctl, grid::CTL_WORDS * sizeof(uint32_t));
        GRID_TRY(copy, hipMemcpyAsync(d_cost, cost, cells, hipMemcpyHostToDevice, s));
        if (n > 0) GRID_TRY(copy, hipMemcpyAsync(d_goals, goals, 3 * (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        int r = send_roll_table(s, t, b);
        if (r) return r;
        grid::PoseJob j = pose_job(pp, t, b, nx, nz, oa, ob);
        j.cost = d_cost.p;
        pose_planes(j, field.p, d_tiles.p, d_ctl.p);
        j.goals = d_goals.p, j.n_goals = n;
        GRID_TRY(launch, (grid::launch_pose_foot(s, j), hipGetLastError()));
        if ((r = pose_run(s, j, h_ctl))) return r;
        GRID_TRY(copy, hipMemcpyAsync(cf, j.cf, states, hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(pot, j.pot, states * 4, hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(dir, j.dir, states, hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    out[0] = h_ctl.p[grid::CTL_COUNTED];
    out[1] = (int64_t)((uint64_t)h_ctl.p[grid::CTL_REACHED] | ((uint64_t)h_ctl.p[grid::CTL_REACHED + 1] << 32));
    out[2] = h_ctl.p[grid::CTL_ROUNDS];
    return SVH_OK;
}

// ---- the prediction ---------------------------------------------------------------------------------------------------------
bool convert_pred(const svh_grid_pred_params* p, grid::PredParams* q) {
    if (!p) return false;
    *q = grid::PredParams{p->slots, p->stride, p->poses_per_step, p->margin, p->grow16, p->only_moving};
    return grid::pred_ok(*q);
}

// the offsets PRED lies under: those of the ID plane, the window's while no step has written one (PRED is all 0 then)
int32_t pred_oa(const svh_grid* g) { return g->trk_plane ? g->trk_oa : g->prm.oa; }
int32_t pred_ob(const svh_grid* g) { return g->trk_plane ? g->trk_ob : g->prm.ob; }

// a job on a track table and an ID plane that lie on the device, with the buffers of `b`, which this grows; PRED and the control
// words are cleared on the stream
int pred_job(hipStream_t s, const grid::PredParams& pp, int32_t nx, int32_t nz, const int32_t* id, const int32_t* tracks, int32_t n_tracks, PredBufs& b,
             grid::PredJob* j) {
    const size_t cells = (size_t)nx * (size_t)nz, ctl_bytes = grid::PRED_CTL_WORDS * sizeof(unsigned long long);
    j->pp = pp;
    j->nx = nx, j->nz = nz;
    j->id = id, j->tracks = tracks, j->n_tracks = n_tracks;
    for (int32_t r = 0; r <= grid::PRED_MAX_RADIUS; r++) j->ge[r] = grid::pred_ge(pp, r);
    j->max_r = grid::pred_radius(pp, pp.slots - 1);
    GRID_GROW_N(b.plane, cells);
    GRID_GROW(b.ctl, ctl_bytes);
    GRID_GROW(b.h_ctl, ctl_bytes);
    if (n_tracks > 0) {
        GRID_GROW_N(b.disp, (size_t)n_tracks * grid::PRED_MAX_SLOTS);
        GRID_GROW_N(b.predicts, n_tracks);
        if (j->max_r > 0) GRID_GROW_N(b.rows, cells);
    }
    j->disp = b.disp, j->predicts = b.predicts, j->pred = b.plane, j->rows = b.rows, j->ctl = b.ctl;
    GRID_TRY(copy, hipMemsetAsync(b.plane, 0, cells * sizeof(uint32_t), s));
    GRID_TRY(copy, hipMemsetAsync(b.ctl, 0, ctl_bytes, s));
    return SVH_OK;
}

// PRED is valid or launched: from the track state as it is, pending until the caller has waited and settles.  The control words
// follow to pinned memory on the stream, where the statistics are read once PRED counts.  An empty table is a fill
int predict(svh_grid* g) {
    if (has(g, PRED) || (g->pending & PRED)) return SVH_OK;
    hipStream_t s = g->stream;
    PredBufs& b = g->pred;
    const int32_t n = g->trk_plane ? g->trk_n : 0;
    grid::PredJob j;
    const int rc = pred_job(s, g->prp, g->prm.nx, g->prm.nz, n ? g->trk.id[g->trk_cur].p : nullptr, n ? g->trk.table[g->trk_cur].p : nullptr, n, b, &j);
    if (rc) return rc;
    g->pred_launches = 0;
    if (n > 0) GRID_TRY(launch, (g->pred_launches = grid::launch_pred(s, j), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(b.h_ctl, b.ctl, grid::PRED_CTL_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    g->pending |= PRED;
    return SVH_OK;
}

int get_pred_plane(svh_grid* g, uint32_t* out, bool on_device) {
    int rc = ready(g);
    if (rc || (rc = predict(g))) return rc;
    if ((rc = deliver(g, g->pred.plane, g->ncells * sizeof(uint32_t), out, on_device))) return rc;
    settle(g);
    return SVH_OK;
}

int get_pred_stats(svh_grid* g, int64_t out[4]) {
    int rc = ready(g);
    if (rc || (rc = predict(g))) return rc;
    if (g->pending) {
        GRID_TRY(wait, hipStreamSynchronize(g->stream));
        settle(g);
    }
    const unsigned long long* h = g->pred.h_ctl;
    out[grid::PS_TRACKS] = (int64_t)h[grid::PS_TRACKS], out[grid::PS_SOURCES] = (int64_t)h[grid::PS_SOURCES];
    out[grid::PS_CELLS] = (int64_t)h[grid::PS_CELLS], out[grid::PS_LAUNCHES] = g->pred_launches;
    return SVH_OK;
}

grid::RollPredJob roll_pred_job(const svh_grid* g) {
    grid::RollPredJob j;
    j.r = roll_job(g);
    j.pp = g->prp;
    j.poa = pred_oa(g), j.pob = pred_ob(g);
    j.pred = g->pred.plane;
    return j;
}

// the footprint predictions of n > 0 poses with arguments that have been checked
int footprint_pred(svh_grid* g, const int32_t* poses, int64_t n, bool on_device, uint32_t* out) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = roll_tables(g, false))) return rc;
    PredBufs& b = g->pred;
    if (!on_device) {
        GRID_GROW_N(b.d_poses, 3 * n);
        GRID_GROW_N(b.d_mask, n);
        GRID_GROW(g->h_out, (size_t)n * sizeof(uint32_t));
        GRID_TRY(copy, hipMemcpyAsync(b.d_poses, poses, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    }
    if ((rc = predict(g))) return rc;
    grid::launch_footprint_pred(g->stream, roll_pred_job(g), on_device ? poses : b.d_poses.p, n, on_device ? out : b.d_mask.p);
    GRID_TRY(launch, hipGetLastError());
    return finish(g, b.d_mask, (size_t)n * sizeof(uint32_t), out, on_device);
}

// set `set` scored at the global cell (ga, gb) with the prediction; recs and scores may be null.  The outputs are the layer's own:
// those of the last svh_grid_roll_score stay
int roll_score_pred(svh_grid* g, int32_t ga, int32_t gb, int32_t set, int32_t* recs, int64_t* scores, bool on_device, int32_t* best) {
    int rc = ready(g);
    if (rc) return rc;
    PredBufs& b = g->pred;
    const int32_t K = g->cand_K;
    const size_t rec_bytes = (size_t)K * grid::ROLL_PRED_REC * sizeof(int32_t), score_bytes = (size_t)K * sizeof(int64_t);
    GRID_GROW_N(b.recs, (size_t)grid::ROLL_PRED_REC * (size_t)K);
    GRID_GROW_N(b.scores, K);
    GRID_GROW_N(b.best, 1);
    GRID_GROW(b.h_roll, score_bytes + rec_bytes + sizeof(int32_t));   // the scores first: they are the widest
    if ((rc = roll_tables(g, true))) return rc;
    if ((rc = g->rol.p.w_pot != 0 ? plan_field(g) : traverse(g))) return rc;
    if ((rc = predict(g))) return rc;
    grid::RollPredJob j = roll_pred_job(g);
    j.r.cands = g->d_cands + (size_t)set * (size_t)K * (size_t)g->cand_T * 3, j.r.lens = g->d_cand_lens + (size_t)set * (size_t)K;
    j.r.K = K, j.r.T = g->cand_T, j.r.ga0 = ga, j.r.gb0 = gb;
    j.r.recs = b.recs, j.r.scores = b.scores, j.r.best = b.best;
    hipStream_t s = g->stream;
    GRID_TRY(launch, (grid::launch_roll_score_pred(s, j), hipGetLastError()));
    uint8_t* h = b.h_roll;
    if (scores) GRID_TRY(copy, hipMemcpyAsync(on_device ? (void*)scores : (void*)h, j.r.scores, score_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (recs) GRID_TRY(copy, hipMemcpyAsync(on_device ? (void*)recs : (void*)(h + score_bytes), j.r.recs, rec_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    GRID_TRY(copy, hipMemcpyAsync(h + score_bytes + rec_bytes, j.r.best, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    settle(g);
    if (scores && !on_device) memcpy(scores, h, score_bytes);
    if (recs && !on_device) memcpy(recs, h + score_bytes, rec_bytes);
    memcpy(best, h + score_bytes + rec_bytes, sizeof(int32_t));
    return SVH_OK;
}

int render_pred(svh_grid* g, int32_t mode, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        int rc = finalise(g);
        if (rc || (rc = predict(g))) return rc;
        grid::launch_render(g->stream, render_job(g, mode, dst));
        grid::launch_pred_overlay(g->stream, g->prm.nx, g->prm.nz, g->prm.oa, g->prm.ob, pred_oa(g), pred_ob(g), g->pred.plane, dst);
        return rc;
    });
}

const char* const kNoRoll =": the default vehicle does not fit this grid's cell; set one (svh_grid_set_roll)";

// the planes and the tables of a test entry on the device, and the kernels on them; the outputs as those of svh_test_grid_roll
int roll_device(const grid::RollParams& q, const RollTable& t, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost, const int32_t* pot, const int32_t* table,
                int32_t S, int32_t K, int32_t T, int32_t set, int32_t ga0, int32_t gb0, const int32_t* poses, int64_t n_poses, int32_t* fout,
                int32_t* recs, int64_t* scores, int32_t* best) {
    const size_t cells = (size_t)nx * (size_t)nz;
    HipBuf<uint8_t> d_cost;
    HipBuf<int32_t> d_pot, d_cands, d_lens, d_poses, d_f;
    RollBufs b;
    std::vector<int32_t> lens((size_t)S * (size_t)K);
    for (size_t c = 0; c < lens.size(); c++) lens[c] = grid::roll_len(table + c * (size_t)T * 3, T);
    hipStream_t s = nullptr;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(d_cost, cells);
        GRID_TRY(copy, hipMemcpyAsync(d_cost, cost, cells, hipMemcpyHostToDevice, s));
        if (q.w_pot != 0) {
            GRID_GROW_N(d_pot, cells);
            GRID_TRY(copy, hipMemcpyAsync(d_pot, pot, cells * sizeof(int32_t), hipMemcpyHostToDevice, s));
        }
        int r = send_roll_table(s, t, b);
        if (r) return r;
        grid::RollJob j = roll_job(t, b, nx, nz, oa, ob, d_cost, q.w_pot != 0 ? d_pot.p : nullptr);
        j.rp = q;   // the table is that of the vehicle; the costs and the weights are this call's
        if (n_poses > 0) {
            GRID_GROW_N(d_poses, 3 * n_poses);
            GRID_GROW_N(d_f, n_poses);
            GRID_TRY(copy, hipMemcpyAsync(d_poses, poses, (size_t)n_poses * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
            GRID_TRY(launch, (grid::launch_footprint_cost(s, j, d_poses, n_poses, d_f), hipGetLastError()));
            GRID_TRY(copy, hipMemcpyAsync(fout, d_f, (size_t)n_poses * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        if (S > 0) {
            const size_t words = (size_t)S * (size_t)K * (size_t)T * 3;
            GRID_GROW_N(d_cands, words);
            GRID_GROW_N(d_lens, lens.size());
            if ((r = roll_outputs(b, K))) return r;
            GRID_TRY(copy, hipMemcpyAsync(d_cands, table, words * sizeof(int32_t), hipMemcpyHostToDevice, s));
            GRID_TRY(copy, hipMemcpyAsync(d_lens, lens.data(), lens.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            roll_candidates(j, b, d_cands, d_lens, set, K, T, ga0, gb0);
            GRID_TRY(launch, (grid::launch_roll_score(s, j), hipGetLastError()));
            if (recs) GRID_TRY(copy, hipMemcpyAsync(recs, j.recs, (size_t)K * grid::ROLL_REC * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (scores) GRID_TRY(copy, hipMemcpyAsync(scores, j.scores, (size_t)K * sizeof(int64_t), hipMemcpyDeviceToHost, s));
            GRID_TRY(copy, hipMemcpyAsync(best, j.best, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    return rc;
}

// The footprint table of a test entry.  A caller fills its table once, not per call, so the table of the last vehicle and cell
// side asked for is kept: a call with the same front, rear, half_width, headings_m and cell gets it back without building it.
// The weights and the two costs of the parameters play no part in it; nullptr: the reach is outside 1..128
std::shared_ptr<const RollTable> roll_table_for(const grid::RollParams& q, float cell) {
    static std::mutex mu;
    static std::shared_ptr<const RollTable> last;
    static float last_cell = 0.f;
    std::lock_guard<std::mutex> lock(mu);
    if (last && last_cell == cell && last->p.front == q.front && last->p.rear == q.rear && last->p.half_width == q.half_width && last->p.m == q.m)
        return last;
    std::shared_ptr<RollTable> t = std::make_shared<RollTable>();
    t->p = q;
    if (!t->derive(cell)) return nullptr;
    last = t, last_cell = cell;
    return last;
}

// the checks that svh_test_grid_roll and svh_test_grid_roll_device share; the parameters to `q`, their table to `t`
bool roll_test_args(const svh_grid_roll_params* p, float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost,
                    const int32_t* pot, const int32_t* table, int32_t S, int32_t K, int32_t T, int32_t set, int32_t ga0, int32_t gb0,
                    const int32_t* poses, int64_t n_poses, const int32_t* fout, const int32_t* best, grid::RollParams* q,
                    std::shared_ptr<const RollTable>* t) {
    if (!convert_roll(p, q) || !(grid::finite_f(cell) && cell > 0.f) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE ||
        !grid::offsets_ok(oa, ob) || !cost || (q->w_pot != 0 && !pot) || n_poses < 0 || n_poses > ((int64_t)1 << 26) ||
        (n_poses > 0 && (!poses || !fout)))
        return false;
    if (table || S != 0) {
        if (!grid::roll_table_ok(table, S, K, T, 8 * q->m) || set < 0 || set >= S || !best || ga0 <= -grid::PLAN_GOAL_LIMIT ||
            ga0 >= grid::PLAN_GOAL_LIMIT || gb0 <= -grid::PLAN_GOAL_LIMIT || gb0 >= grid::PLAN_GOAL_LIMIT)
            return false;
    }
    *t = roll_table_for(*q, cell);
    return *t != nullptr;
}

const char* const kNoTrav =": the default traversability does not fit this grid's cell; set one (svh_grid_set_traversability)";

// what every entry that computes the pose planner's layer refuses; nullptr: nothing
const char* pose_refusal(const svh_grid* g) {
    if (!g->trav_ok) return kNoTrav;
    if (!g->rol.R) return kNoRoll;
    if ((int64_t)g->ncells > grid::POSE_MAX_CELLS) return ": the window has more than 2^24 cells, PPOT would exceed 512 MiB";
    return nullptr;
}

// the checks that svh_test_grid_pose and svh_test_grid_pose_device share; the parameters to `q` and `pp`, the vehicle's table to `t`
bool pose_test_args(const svh_grid_roll_params* r, const svh_grid_pose_params* p, float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                    const uint8_t* cost, const int32_t* goals, int32_t n, const void* cf, const void* pot, const void* dir, grid::RollParams* q,
                    grid::PoseParams* pp, std::shared_ptr<const RollTable>* t) {
    if (!p || !convert_roll(r, q) || !(grid::finite_f(cell) && cell > 0.f) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE ||
        (int64_t)nx * nz > grid::POSE_MAX_CELLS || !grid::offsets_ok(oa, ob) || !cost || n < 0 || n > grid::POSE_MAX_GOALS || (n > 0 && !goals) || !cf ||
        !pot || !dir)
        return false;
    *pp = grid::PoseParams{p->neutral, p->max_cost, p->turn, p->reverse, p->spin};
    if (!grid::pose_ok(*pp)) return false;
    for (int32_t k = 0; k < n; k++)
        if (!grid::pose_goal_ok(goals + 3 * k)) return false;
    *t = roll_table_for(*q, cell);
    return *t != nullptr;
}

// ---- the time layer -----------------------------------------------------------------------------------------------------------
bool convert_time(const svh_grid_time_params* p, grid::TimeParams* q) {
    if (!p) return false;
    *q = grid::TimeParams{p->layers, p->wait, p->release};
    return grid::time_ok(*q);
}

const char* time_refusal(const svh_grid* g) {
    if (!g->time_on) return ": the time layer is off; switch it on (svh_grid_set_time)";
    if (!g->trav_ok) return kNoTrav;
    if (!grid::time_fits(g->tmp, g->prm.nx, g->prm.nz)) return ": layers * nx * nz exceeds 2^28";
    return nullptr;
}

// FLAGS' and the released cells on buffers that exist: one launch and one wait, the count through `h_ctl` (pinned)
int time_release_run(hipStream_t s, const grid::TimeReleaseJob& j, unsigned long long* h_ctl, int64_t* released) {
    GRID_TRY(copy, hipMemsetAsync(j.ctl, 0, grid::TC_WORDS * sizeof(unsigned long long), s));
    GRID_TRY(launch, (grid::launch_time_release(s, j), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(h_ctl, j.ctl, grid::TC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    *released = (int64_t)h_ctl[grid::TC_RELEASED];
    return SVH_OK;
}

// RCOST over FLAGS' by the two distance launches, then the planner on it, a job with buffers of its own; complete when it returns
int time_static_run(hipStream_t s, const grid::TravJob& tj, const grid::PlanJob& pj, uint32_t* h_ctl) {
    GRID_TRY(launch, (grid::launch_trav_dist(s, tj), hipGetLastError()));
    return plan_run(s, pj, h_ctl);
}

// the sweep on static planes and a PRED plane that are written in stream order; the control words of the statistics are in `h_ctl`
// (pinned) when it returns
int time_sweep_run(hipStream_t s, const grid::TimeJob& j, unsigned long long* h_ctl) {
    GRID_TRY(copy, hipMemsetAsync(j.ctl + grid::TC_REACHED, 0, (grid::TC_WORDS - grid::TC_REACHED) * sizeof(unsigned long long), s));
    GRID_TRY(launch, ((void)grid::launch_time_sweep(s, j), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(h_ctl, j.ctl, grid::TC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    return SVH_OK;
}

// the buffers of the layer exist
int time_ready(svh_grid* g) {
    GRID_GROW(g->tfield, g->ncells * (size_t)g->tmp.layers * kTimeBytes);
    GRID_GROW(g->time_ctl, grid::TC_WORDS * sizeof(unsigned long long));
    GRID_GROW(g->h_time_ctl, grid::TC_WORDS * sizeof(unsigned long long));
    return SVH_OK;
}

// The static planes are valid; complete when it returns.  The planner's field comes first, always: while no cell is released it IS
// RPOT and RDIR and nothing is computed twice, and it must be current whenever they are read.  With cells to release: FLAGS', the two
// distance launches on it, and the planner's seed, rounds and DIR on a job of the layer's own, as the reach field's.  DIST2 of that
// pass is scratch and goes where TPOT will be written.
int time_static(svh_grid* g) {
    int rc = plan_field(g);
    if (rc || has(g, TIME_STATIC)) return rc;
    bool own = false;
    int64_t released = 0, rounds = g->plan_rounds;
    const int32_t n = (g->tmp.release && g->trk_plane) ? g->trk_n : 0;
    if (n > 0) {
        if ((rc = time_ready(g))) return rc;
        GRID_GROW(g->tstat, g->ncells * kTimeStaticBytes);
        grid::TimeReleaseJob rj;
        rj.pp = g->prp;
        rj.nx = g->prm.nx, rj.nz = g->prm.nz, rj.oa = g->prm.oa, rj.ob = g->prm.ob, rj.poa = pred_oa(g), rj.pob = pred_ob(g);
        rj.id = g->trk.id[g->trk_cur].p, rj.tracks = g->trk.table[g->trk_cur].p, rj.n_tracks = n;
        rj.flags = g->t_flags(), rj.out = g->s_flags(), rj.ctl = g->time_ctl.p;
        if ((rc = time_release_run(g->stream, rj, g->h_time_ctl, &released))) return rc;
    }
    if (released > 0) {
        const size_t tiles = plan_tiles(g->prm);
        GRID_GROW(g->tstat_tiles, 4 * tiles * sizeof(uint32_t));
        GRID_GROW(g->tstat_ctl, grid::CTL_WORDS * sizeof(uint32_t));
        GRID_GROW(g->h_tstat_ctl, grid::CTL_WORDS * sizeof(uint32_t));
        grid::TravJob tj;
        tj.trv = g->trv;
        tj.nx = g->prm.nx, tj.nz = g->prm.nz;
        tj.cls = g->bplane(B_CLASS), tj.hmean = nullptr, tj.state = nullptr;
        tj.table = g->d_table.p;
        static_assert(kTimeBytes >= sizeof(int32_t) && (kNeeds[10] & TIME_STATIC), "DIST2 of this pass is scratch in TPOT: the field has room for it and is stale with the static planes");
        drop(g, TIME);   // ... and says so itself: what is written below overwrites layer 0 of TPOT
        tj.flags = g->s_flags(), tj.g = g->s_g(), tj.dist2 = g->t_pot(), tj.cost = g->s_cost();
        grid::PlanJob pj = plan_job(g);
        pj.cost = g->s_cost();
        pj.price = g->s_price(), pj.pot = g->s_pot(), pj.dir = g->s_dir();
        pj.lists = g->tstat_tiles.p, pj.flags = g->tstat_tiles.p + 2 * tiles;
        pj.ctl = g->tstat_ctl.p;
        if ((rc = time_static_run(g->stream, tj, pj, g->h_tstat_ctl))) return rc;
        own = true, rounds = g->h_tstat_ctl[grid::CTL_ROUNDS];
    }
    g->time_own = own, g->time_released = released, g->time_rounds = rounds;
    g->pending |= TIME_STATIC;
    settle(g);
    return SVH_OK;
}

grid::TimeJob time_job(const svh_grid* g) {
    grid::TimeJob j;
    j.pln = g->pln, j.tp = g->tmp, j.pp = g->prp;
    j.nx = g->prm.nx, j.nz = g->prm.nz, j.oa = g->prm.oa, j.ob = g->prm.ob, j.poa = pred_oa(g), j.pob = pred_ob(g);
    j.price = g->time_own ? g->s_price() : g->p_price(), j.rpot = g->time_own ? g->s_pot() : g->p_pot(), j.rdir = g->time_own ? g->s_dir() : g->p_dir();
    j.pred = g->pred.plane;
    j.tpot = g->t_pot(), j.tdir = g->t_dir();
    j.ctl = g->time_ctl.p;
    return j;
}

// the field is valid: the static planes, PRED, then the sweep; complete when it returns
int time_field(svh_grid* g) {
    int rc = time_static(g);
    if (rc || has(g, TIME)) return rc;
    if ((rc = time_ready(g)) || (rc = predict(g))) return rc;
    if ((rc = time_sweep_run(g->stream, time_job(g), g->h_time_ctl))) return rc;
    const unsigned long long* h = g->h_time_ctl;
    g->time_stats[grid::TM_LAYERS] = g->tmp.layers, g->time_stats[grid::TM_REACHED] = (int64_t)h[grid::TC_REACHED];
    g->time_stats[grid::TM_BLOCKED] = (int64_t)h[grid::TC_BLOCKED], g->time_stats[grid::TM_WAITS] = (int64_t)h[grid::TC_WAITS];
    g->pending |= TIME;
    settle(g);
    return SVH_OK;
}

int get_time_plane(svh_grid* g, int32_t plane, int32_t t0, int32_t count, void* out, bool on_device) {
    int rc = ready(g);
    if (rc) return rc;
    if (plane == grid::TP_RCOST || plane == grid::TP_RPOT) {
        if ((rc = time_static(g))) return rc;
        return plane == grid::TP_RCOST ? deliver(g, g->time_own ? g->s_cost() : g->t_cost(), g->ncells, out, on_device)
                                       : deliver(g, g->time_own ? g->s_pot() : g->p_pot(), g->ncells * 4, out, on_device);
    }
    if ((rc = time_field(g))) return rc;
    return plane == grid::TP_TPOT ? deliver(g, g->t_pot() + (size_t)t0 * g->ncells, (size_t)count * g->ncells * 4, out, on_device)
                                  : deliver(g, g->t_dir() + (size_t)t0 * g->ncells, (size_t)count * g->ncells, out, on_device);
}

// `n` triples from the host to d_time_path through the pinned staging buffer, and the wait
int send_triples(svh_grid* g, const int32_t* triples, int64_t n) {
    const size_t bytes = (size_t)n * 3 * sizeof(int32_t);
    GRID_GROW(g->d_time_path, bytes);
    GRID_GROW(g->h_cells, bytes);
    memcpy(g->h_cells, triples, bytes);
    GRID_TRY(copy, hipMemcpyAsync(g->d_time_path, g->h_cells, bytes, hipMemcpyHostToDevice, g->stream));
    GRID_TRY(wait, hipStreamSynchronize(g->stream));   // the staging buffer is free again
    return SVH_OK;
}

// the walk from the window cell (a, b) at layer 0
int time_path(svh_grid* g, int32_t a, int32_t b, int32_t* triples, int64_t cap, int64_t* len, int32_t* cost, int32_t* status) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = time_field(g))) return rc;
    const int64_t room = std::min<int64_t>(cap, (int64_t)g->ncells + g->tmp.layers);   // a path has at most L + nx * nz entries
    GRID_GROW_N(g->d_time_path, 3 * room);
    GRID_GROW(g->d_walk, 3 * sizeof(int64_t));
    GRID_GROW(g->h_walk, 3 * sizeof(int64_t));
    GRID_TRY(launch, (grid::launch_time_walk(g->stream, time_job(g), a, b, g->d_time_path, room, g->d_walk), hipGetLastError()));
    GRID_TRY(copy, hipMemcpyAsync(g->h_walk, g->d_walk, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    GRID_TRY(wait, hipStreamSynchronize(g->stream));
    const int64_t n = g->h_walk[1], m = std::min(n, room);
    if (m > 0 && (rc = deliver(g, g->d_time_path, (size_t)m * 3 * sizeof(int32_t), triples, false))) return rc;
    *status = (int32_t)g->h_walk[0], *len = n, *cost = (int32_t)g->h_walk[2];
    return SVH_OK;
}

int render_time(svh_grid* g, int32_t t, const int32_t* triples, int64_t n, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        int rc = time_field(g);
        if (rc || (n > 0 && (rc = send_triples(g, triples, n)))) return rc;
        const grid::TimeJob tj = time_job(g);
        grid::RenderCostJob cj = cost_job(g, dst);
        if (g->time_own) cj.cost = g->s_cost(), cj.flags = g->s_flags();
        grid::launch_render_cost(g->stream, cj);
        grid::launch_time_overlay(g->stream, tj, t, g->d_goals.p, (int32_t)(g->goals.size() / 2), g->d_time_path, n, dst);
        return rc;
    });
}

// the arguments of the two test entries of the layer, checked and converted
struct TimeTestArgs {
    grid::PlanParams pln;
    grid::PredParams pp;
    grid::TimeParams tp;
    grid::TravParams trv;       // reach 0: nothing can be released
    std::vector<uint8_t> table;
    int32_t n_tracks;           // 0 unless release = 1 and an ID plane and tracks are given
};

// the static planes of a test entry on the host: RCOST, RPOT, RDIR and the released cells
void time_static_host(const TimeTestArgs& q, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost, const uint8_t* flags, const uint8_t* cls,
                      const int32_t* goals, int32_t n_goals, int32_t poa, int32_t pob, const int32_t* id, const int32_t* tracks, uint8_t* rcost, int32_t* rpot,
                      uint8_t* rdir, int64_t* released) {
    const size_t cells = (size_t)nx * (size_t)nz;
    std::vector<uint8_t> f2(cells);
    *released = q.n_tracks > 0 ? grid::time_release_window(q.pp, nx, nz, oa, ob, poa, pob, id, tracks, q.n_tracks, flags, f2.data()) : 0;
    if (*released > 0) {
        std::vector<uint16_t> gcol(cells);
        grid::dist_window(q.trv.reach, nx, nz, cls, q.table.data(), f2.data(), gcol.data(), nullptr, rcost);
    } else {
        memcpy(rcost, cost, cells);
    }
    (void)grid::plan_window(q.pln, nx, nz, oa, ob, rcost, goals, n_goals, rpot, rdir);
}

// the same on the device, and the sweep and the walk there: the planes to the host, stats as svh_grid_get_time_stats, walk[3] the
// status, the entries and the cost of the path from the window cell (a, b) (a < 0: no walk)
int time_device(const TimeTestArgs& q, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost, const uint8_t* flags, const uint8_t* cls,
                const int32_t* goals, int32_t n_goals, const uint32_t* pred, int32_t poa, int32_t pob, const int32_t* id, const int32_t* tracks, int32_t* tpot,
                uint8_t* tdir, uint8_t* rcost, int32_t* rpot, uint8_t* rdir, int64_t* stats, int32_t a, int32_t b, int32_t* triples, int64_t cap, int64_t* walk) {
    const size_t cells = (size_t)nx * (size_t)nz, states = cells * (size_t)q.tp.layers, tiles = ((size_t)(nx + grid::PLAN_TILE - 1) / grid::PLAN_TILE) * ((size_t)(nz + grid::PLAN_TILE - 1) / grid::PLAN_TILE);
    HipBuf<uint8_t> d_cost, d_flags, d_cls, d_table, stat, field;
    HipBuf<int32_t> d_goals, d_id, d_tracks, d_path;
    HipBuf<uint32_t> d_pred, d_tiles, d_ctl;
    HipBuf<unsigned long long> t_ctl;
    HipBuf<int64_t> d_walk;
    PinnedBuf<uint32_t> h_ctl;
    PinnedBuf<unsigned long long> h_tctl;
    PinnedBuf<int64_t> h_walk;
    hipStream_t s = nullptr;
    int64_t released = 0;
    const int64_t room = std::min<int64_t>(cap, (int64_t)cells + q.tp.layers);
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(d_cost, cells);
        GRID_GROW(d_flags, cells);
        GRID_GROW(stat, cells * kTimeStaticBytes);
        GRID_GROW(field, states * kTimeBytes);
        GRID_GROW_N(d_goals, 2 * (size_t)n_goals);
        GRID_GROW_N(d_pred, cells);
        GRID_GROW(d_tiles, 4 * tiles * sizeof(uint32_t));
        GRID_GROW(d_ctl, grid::CTL_WORDS * sizeof(uint32_t));
        GRID_GROW(h_ctl, grid::CTL_WORDS * sizeof(uint32_t));
        GRID_GROW(t_ctl, grid::TC_WORDS * sizeof(unsigned long long));
        GRID_GROW(h_tctl, grid::TC_WORDS * sizeof(unsigned long long));
        GRID_GROW(d_walk, 3 * sizeof(int64_t));
        GRID_GROW(h_walk, 3 * sizeof(int64_t));
        GRID_GROW_N(d_path, 3 * room);
        GRID_TRY(copy, hipMemcpyAsync(d_cost, cost, cells, hipMemcpyHostToDevice, s));
        GRID_TRY(copy, hipMemcpyAsync(d_flags, flags, cells, hipMemcpyHostToDevice, s));
        GRID_TRY(copy, hipMemcpyAsync(d_pred, pred, cells * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (n_goals > 0) GRID_TRY(copy, hipMemcpyAsync(d_goals, goals, 2 * (size_t)n_goals * sizeof(int32_t), hipMemcpyHostToDevice, s));
        uint8_t* st = stat.p;
        uint8_t *s_cost = st + 9 * cells, *s_flags = st + 10 * cells;
        if (q.n_tracks > 0) {
            GRID_GROW(d_cls, cells);
            GRID_GROW(d_table, q.table.size());
            GRID_GROW_N(d_id, cells);
            GRID_GROW_N(d_tracks, (size_t)q.n_tracks * grid::TRACK_REC);
            GRID_TRY(copy, hipMemcpyAsync(d_cls, cls, cells, hipMemcpyHostToDevice, s));
            GRID_TRY(copy, hipMemcpyAsync(d_table, q.table.data(), q.table.size(), hipMemcpyHostToDevice, s));
            GRID_TRY(copy, hipMemcpyAsync(d_id, id, cells * sizeof(int32_t), hipMemcpyHostToDevice, s));
            GRID_TRY(copy, hipMemcpyAsync(d_tracks, tracks, (size_t)q.n_tracks * grid::TRACK_REC * sizeof(int32_t), hipMemcpyHostToDevice, s));
            grid::TimeReleaseJob rj;
            rj.pp = q.pp;
            rj.nx = nx, rj.nz = nz, rj.oa = oa, rj.ob = ob, rj.poa = poa, rj.pob = pob;
            rj.id = d_id.p, rj.tracks = d_tracks.p, rj.n_tracks = q.n_tracks;
            rj.flags = d_flags.p, rj.out = s_flags, rj.ctl = t_ctl.p;
            const int r = time_release_run(s, rj, h_tctl, &released);
            if (r) return r;
        }
        grid::PlanJob pj;
        pj.pln = q.pln;
        pj.nx = nx, pj.nz = nz, pj.oa = oa, pj.ob = ob;
        pj.cost = released > 0 ? s_cost : d_cost.p;
        pj.pot = (int32_t*)st, pj.price = (uint16_t*)(st + 4 * cells), pj.dir = st + 8 * cells;
        pj.goals = d_goals.p, pj.n_goals = n_goals;
        pj.lists = d_tiles.p, pj.flags = d_tiles.p + 2 * tiles;
        pj.ctl = d_ctl.p;
        int r;
        if (released > 0) {
            grid::TravJob tj;
            tj.trv = q.trv;
            tj.nx = nx, tj.nz = nz;
            tj.cls = d_cls.p, tj.hmean = nullptr, tj.state = nullptr;
            tj.table = d_table.p;
            tj.flags = s_flags, tj.g = (uint16_t*)(st + 6 * cells), tj.dist2 = (int32_t*)field.p, tj.cost = s_cost;
            r = time_static_run(s, tj, pj, h_ctl);
        } else {
            r = plan_run(s, pj, h_ctl);
        }
        if (r) return r;
        grid::TimeJob j;
        j.pln = q.pln, j.tp = q.tp, j.pp = q.pp;
        j.nx = nx, j.nz = nz, j.oa = oa, j.ob = ob, j.poa = poa, j.pob = pob;
        j.price = pj.price, j.rpot = pj.pot, j.rdir = pj.dir;
        j.pred = d_pred.p;
        j.tpot = (int32_t*)field.p, j.tdir = field.p + 4 * states;
        j.ctl = t_ctl.p;
        if ((r = time_sweep_run(s, j, h_tctl))) return r;
        if (a >= 0) {
            GRID_TRY(launch, (grid::launch_time_walk(s, j, a, b, d_path, room, d_walk), hipGetLastError()));
            GRID_TRY(copy, hipMemcpyAsync(h_walk, d_walk, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
            GRID_TRY(wait, hipStreamSynchronize(s));
            const int64_t m = std::min<int64_t>(h_walk.p[1], room);
            if (m > 0) GRID_TRY(copy, hipMemcpyAsync(triples, d_path, (size_t)m * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        GRID_TRY(copy, hipMemcpyAsync(tpot, j.tpot, states * 4, hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(tdir, j.tdir, states, hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(rcost, pj.cost, cells, hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(rpot, pj.pot, cells * 4, hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(rdir, pj.dir, cells, hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    stats[grid::TM_LAYERS] = q.tp.layers, stats[grid::TM_REACHED] = (int64_t)h_tctl.p[grid::TC_REACHED];
    stats[grid::TM_BLOCKED] = (int64_t)h_tctl.p[grid::TC_BLOCKED], stats[grid::TM_WAITS] = (int64_t)h_tctl.p[grid::TC_WAITS];
    stats[grid::TM_RELEASED] = released, stats[grid::TM_ROUNDS] = h_ctl.p[grid::CTL_ROUNDS];
    if (a >= 0) walk[0] = h_walk.p[0], walk[1] = h_walk.p[1], walk[2] = h_walk.p[2];
    return SVH_OK;
}

// ---- the exploration layer ------------------------------------------------------------------------------------------------
const char* const kNoExplore =": the default range does not fit this grid's cell; set one (svh_grid_set_explore)";

bool convert_explore(const svh_grid_explore_params* p, grid::ExploreParams* q) {
    if (!p) return false;
    *q = grid::ExploreParams{p->range, p->min_gain, p->w_gain, p->w_reach};
    return grid::explore_ok(*q);
}

grid::ExploreJob explore_job(const grid::ExploreParams& e, const grid::FrontParams& f, int32_t R, int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                             const uint8_t* state) {
    grid::ExploreJob j;
    j.exp = e, j.frp = f, j.R = R;
    j.nx = nx, j.nz = nz, j.oa = oa, j.ob = ob;
    j.state = state;
    return j;
}

grid::ExploreJob explore_job(const svh_grid* g) {
    return explore_job(g->exp, g->frp, g->exp_R, g->prm.nx, g->prm.nz, g->prm.oa, g->prm.ob, g->bplane(B_STATE));
}

// room for a ranking of n records, and the job's pointers to it
int explore_outputs(ExploreBufs& b, int32_t n, grid::ExploreJob& j) {
    const size_t room = n > 0 ? (size_t)n : 1;
    GRID_GROW_N(b.gain, room);
    GRID_GROW_N(b.recs, (size_t)grid::EXPLORE_REC * room);
    GRID_GROW_N(b.scores, room);
    GRID_GROW_N(b.out, 2);
    j.n = n, j.gain = b.gain.p, j.recs = b.recs.p, j.scores = b.scores.p, j.out = b.out.p;
    return SVH_OK;
}

// the job of the reach field: the planner's kernels on buffers of their own, the start as the only goal
grid::PlanJob reach_job(const svh_grid* g) {
    grid::PlanJob j = plan_job(g);
    const size_t tiles = plan_tiles(g->prm);
    j.pot = g->r_pot(), j.price = (uint16_t*)(g->reach.p + 4 * g->ncells), j.dir = g->reach.p + 6 * g->ncells;
    j.goals = g->d_start.p, j.n_goals = 1;
    j.lists = g->reach_tiles.p, j.flags = g->reach_tiles.p + 2 * tiles;
    j.ctl = g->reach_ctl.p;
    return j;
}

// the reach field from the global cell (ga, gb) is valid: the cost planes, then seed, rounds and DIR on the second job; complete
// when it returns.  The planner's goals, buffers and field play no part
int reach_field(svh_grid* g, int32_t ga, int32_t gb) {
    if (has(g, REACH) && g->reach_ga == ga && g->reach_gb == gb) return SVH_OK;
    drop(g, REACH);
    const size_t tiles = plan_tiles(g->prm);
    GRID_GROW(g->reach, g->ncells * kPlanBytes);
    GRID_GROW(g->reach_tiles, 4 * tiles * sizeof(uint32_t));
    GRID_GROW(g->reach_ctl, grid::CTL_WORDS * sizeof(uint32_t));
    GRID_GROW(g->h_reach_ctl, grid::CTL_WORDS * sizeof(uint32_t));
    GRID_GROW_N(g->d_start, 2);
    GRID_GROW(g->h_start, 2 * sizeof(int32_t));
    g->h_start[0] = ga, g->h_start[1] = gb;
    GRID_TRY(copy, hipMemcpyAsync(g->d_start, g->h_start, 2 * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    int rc = traverse(g);
    if (rc) return rc;
    if ((rc = plan_run(g->stream, reach_job(g), g->h_reach_ctl))) return rc;
    g->pending |= REACH;
    settle(g);
    g->reach_ga = ga, g->reach_gb = gb;
    g->ex_stats[grid::ES_FIELDS]++;
    return SVH_OK;
}

// the ranking from the global cell (ga, gb): *n records, the first min(*n, cap) of them and of their scores to the host (either
// array may be null), *best.  All of it stays in h_explore: the scores, then the records, then the best and the feasible count
int explore_rank(svh_grid* g, int32_t ga, int32_t gb, int32_t* recs, int64_t* scores, int64_t cap, int64_t* n, int32_t* best) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = frontiers(g))) return rc;
    const int32_t m = (int32_t)std::min<int64_t>(g->front_stats[grid::FS_KEPT], grid::EXPLORE_MAX_RECORDS);
    if ((rc = reach_field(g, ga, gb))) return rc;
    grid::ExploreJob j = explore_job(g);
    if ((rc = explore_outputs(g->ex_bufs, m, j))) return rc;
    const size_t score_bytes = (size_t)m * sizeof(int64_t), rec_bytes = (size_t)m * grid::EXPLORE_REC * sizeof(int32_t);
    GRID_GROW(g->h_explore, score_bytes + rec_bytes + 2 * sizeof(int32_t));
    j.front_recs = g->front_bufs.recs.p, j.pot = g->r_pot();
    hipStream_t s = g->stream;
    const int32_t launches = grid::launch_explore_rank(s, j);
    GRID_TRY(launch, hipGetLastError());
    uint8_t* h = g->h_explore;
    if (m > 0) {
        GRID_TRY(copy, hipMemcpyAsync(h, j.scores, score_bytes, hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(h + score_bytes, j.recs, rec_bytes, hipMemcpyDeviceToHost, s));
    }
    GRID_TRY(copy, hipMemcpyAsync(h + score_bytes + rec_bytes, j.out, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    int32_t out[2];
    memcpy(out, h + score_bytes + rec_bytes, sizeof(out));
    g->ex_stats[grid::ES_RECORDS] = m, g->ex_stats[grid::ES_FEASIBLE] = out[1], g->ex_stats[grid::ES_LAUNCHES] = launches;
    const size_t give = (size_t)std::min<int64_t>(m, cap);
    if (scores && give) memcpy(scores, h, give * sizeof(int64_t));
    if (recs && give) memcpy(recs, h + score_bytes, give * grid::EXPLORE_REC * sizeof(int32_t));
    *n = m, *best = out[0];
    return SVH_OK;
}

// GAIN of n > 0 viewpoints with arguments that have been checked
int view_gain(svh_grid* g, const int32_t* cells, int64_t n, bool on_device, int32_t* out) {
    int rc = ready(g);
    if (rc) return rc;
    if (!on_device) {
        GRID_GROW_N(g->d_vcells, 2 * n);
        GRID_GROW_N(g->d_vgain, n);
        GRID_GROW(g->h_out, (size_t)n * sizeof(int32_t));
        GRID_TRY(copy, hipMemcpyAsync(g->d_vcells, cells, (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    }
    if ((rc = finalise(g))) return rc;
    const int32_t launches = grid::launch_view_gain(g->stream, explore_job(g), on_device ? cells : g->d_vcells.p, 2, n, on_device ? out : g->d_vgain.p);
    GRID_TRY(launch, hipGetLastError());
    if ((rc = finish(g, g->d_vgain, (size_t)n * sizeof(int32_t), out, on_device))) return rc;
    g->ex_stats[grid::ES_LAUNCHES] = launches;
    return SVH_OK;
}

// the VIEW plane of the window viewpoint (va, vb) into d_view, launched on the stream
int view_plane(svh_grid* g, int32_t va, int32_t vb) {
    GRID_GROW(g->d_view, g->ncells);
    const int rc = finalise(g);
    if (rc) return rc;
    GRID_TRY(copy, hipMemsetAsync(g->d_view, 0, g->ncells, g->stream));
    GRID_TRY(launch, (grid::launch_view_mask(g->stream, explore_job(g), va, vb, g->d_view), hipGetLastError()));
    return SVH_OK;
}

int view_mask(svh_grid* g, int32_t va, int32_t vb, uint8_t* out, bool on_device) {
    int rc = ready(g);
    if (rc) return rc;
    if ((rc = view_plane(g, va, vb))) return rc;
    if ((rc = deliver(g, g->d_view, g->ncells, out, on_device))) return rc;
    settle(g);
    return SVH_OK;
}

int render_view(svh_grid* g, int32_t va, int32_t vb, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        int rc = frontiers(g);
        if (rc || (rc = view_plane(g, va, vb))) return rc;
        grid::launch_render_cost(g->stream, cost_job(g, dst));
        grid::launch_front_overlay(g->stream, g->prm.nx, g->prm.nz, g->f_flags(), dst);
        grid::launch_view_overlay(g->stream, g->prm.nx, g->prm.nz, g->d_view, va, vb, dst);
        return rc;
    });
}

// what svh_test_grid_explore and svh_test_grid_explore_device share: the arguments checked, the parameters converted, *R
bool explore_test_args(const svh_grid_front_params* f, const svh_grid_plan_params* pl, const svh_grid_explore_params* e, float cell, int32_t nx,
                       int32_t nz, int32_t oa, int32_t ob, const uint8_t* state, const uint8_t* cost, const int32_t* cells, int64_t n_cells,
                       const int32_t* gains, const int32_t* view, const int32_t* start, const int32_t* recs, const int64_t* scores, int64_t cap,
                       const int64_t* n, const int32_t* best, grid::FrontParams* fq, grid::PlanParams* pq, grid::ExploreParams* eq, int32_t* R) {
    if (!convert_front(f, fq) || !convert_explore(e, eq) || !(grid::finite_f(cell) && cell > 0.f) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 ||
        nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || !state || n_cells < 0 || n_cells > ((int64_t)1 << 26) || (n_cells > 0 && (!cells || !gains)))
        return false;
    if (!(*R = grid::explore_range(eq->range, cell))) return false;
    if (view) {
        const int64_t va = (int64_t)view[0] - oa, vb = (int64_t)view[1] - ob;
        if (va < 0 || va >= nx || vb < 0 || vb >= nz) return false;
    }
    if (start) {
        if (!pl || !cost || !n || !best || cap < 0 || (cap > 0 && !recs && !scores)) return false;
        *pq = grid::PlanParams{pl->neutral, pl->unknown, pl->max_cost};
        if (!grid::plan_ok(*pq) || start[0] <= -grid::PLAN_GOAL_LIMIT || start[0] >= grid::PLAN_GOAL_LIMIT || start[1] <= -grid::PLAN_GOAL_LIMIT ||
            start[1] >= grid::PLAN_GOAL_LIMIT)
            return false;
    }
    return true;
}

// a VIEW plane and its viewpoint drawn over an image of svh_grid_render_cost's layout, on the host
void view_overlay_host(int32_t nx, int32_t nz, const uint8_t* view, int32_t va, int32_t vb, uint8_t* rgb) {
    for (int32_t b = 0; b < nz; b++)
        for (int32_t a = 0; a < nx; a++)
            (void)grid::colour_view(view[(size_t)b * nx + a], a == va && b == vb, rgb + 3 * ((size_t)(nz - 1 - b) * (size_t)nx + (size_t)a));
}

// ---- the alignment layer ----------------------------------------------------------------------------------------------------
bool position(const double xyz[3], float p[3]);

const char* const kNoAlign =": the align parameters are not set (svh_grid_set_align)";

bool convert_align(const svh_grid_align_params* p, float cell, grid::AlignParams* q) {
    if (!p) return false;
    *q = grid::AlignParams{p->reach, p->range, p->rot_den, p->rot_n, p->trans_n, p->min_scan, 0, 0};
    return grid::align_derive(*q, cell);
}

// the job of an alignment of at most n points about the pivot sub (Pa, Pb), with room for everything it writes
int align_job(AlignBufs& b, const grid::Params& prm, const grid::AlignParams& alp, const uint8_t* state, int32_t Pa, int32_t Pb, int64_t n,
              grid::AlignJob* out) {
    grid::AlignJob& j = *out;
    j.prm = prm, j.alp = alp, j.Pa = Pa, j.Pb = Pb;
    memset(j.rot, 0, sizeof(j.rot));
    grid::align_rot_table(alp.rot_den, alp.rot_n, j.rot);
    const size_t ncells = (size_t)prm.nx * (size_t)prm.nz;
    const int64_t side = grid::align_side(alp.Rg);
    j.scan_room = std::min<int64_t>(n, side * side);
    GRID_GROW_N(b.field, ncells);
    GRID_GROW_N(b.g, ncells);
    GRID_GROW_N(b.bitmap, grid::align_words(j));
    GRID_GROW_N(b.blockcnt, grid::align_count_blocks(j));
    GRID_GROW_N(b.ctl, grid::AC_WORDS);
    GRID_GROW_N(b.scan, 2 * j.scan_room);
    GRID_GROW_N(b.volume, grid::align_volume_size(alp.rot_n, alp.trans_n));
    GRID_GROW_N(b.rec, grid::ALIGN_REC);
    j.state = state;
    j.g = b.g, j.field = b.field, j.bitmap = b.bitmap, j.blockcnt = b.blockcnt, j.scan = b.scan, j.ctl = b.ctl, j.volume = b.volume, j.rec = b.rec;
    return SVH_OK;
}

// the bitmap, the control words and the volume become zero: before the marks of an alignment
int align_begin(hipStream_t s, const grid::AlignJob& j) {
    GRID_TRY(copy, hipMemsetAsync(j.bitmap, 0, (size_t)grid::align_words(j) * sizeof(uint32_t), s));
    GRID_TRY(copy, hipMemsetAsync(j.ctl, 0, grid::AC_WORDS * sizeof(uint32_t), s));
    GRID_TRY(copy, hipMemsetAsync(j.volume, 0, (size_t)grid::align_volume_size(j.alp.rot_n, j.alp.trans_n) * sizeof(int32_t), s));
    return SVH_OK;
}

// after the marks: the list of the scan, the volume, the record
int align_finish(hipStream_t s, const grid::AlignJob& j) {
    grid::launch_align_compact(s, j);
    grid::launch_align_score(s, j, g_align_form & 3);
    GRID_TRY(launch, hipGetLastError());
    return SVH_OK;
}

// the finished planes and al.field, launched on the stream and pending until the caller has waited and settles
int align_field(svh_grid* g, const grid::AlignJob& j) {
    const int rc = finalise(g);
    if (rc || has(g, AFIELD)) return rc;
    GRID_TRY(launch, (grid::launch_align_field(g->stream, j, (g_align_form & grid::ALIGN_FORM_MASK) != 0), hipGetLastError()));
    g->pending |= AFIELD;
    return SVH_OK;
}

int object_align_job(svh_grid* g, int32_t Pa, int32_t Pb, int64_t n, grid::AlignJob* j) {
    const int rc = ready(g);
    if (rc) return rc;
    if (g->al.field.cap < g->ncells) drop(g, AFIELD);   // a growth that failed left no field
    return align_job(g->al, g->prm, g->alp, g->bplane(B_STATE), Pa, Pb, n, j);
}

// n >= 0 points, host or device, about the pivot sub, with arguments that have been checked: the record
int align(svh_grid* g, const float* xyzv, int64_t n, bool on_device, int32_t Pa, int32_t Pb, int32_t* rec) {
    drop(g, ALIGN_LAST);
    grid::AlignJob j;
    int rc = object_align_job(g, Pa, Pb, n, &j);
    if (rc) return rc;
    GRID_GROW(g->h_arec, grid::ALIGN_REC * sizeof(int32_t));
    hipStream_t s = g->stream;
    if ((rc = align_field(g, j))) return rc;
    if ((rc = align_begin(s, j))) return rc;
    if (on_device || n == 0) {
        GRID_TRY(launch, (grid::launch_align_mark(s, j, (const float4*)xyzv, nullptr, n), hipGetLastError()));
    } else {
        const int64_t room = std::min(n, kHostChunk);
        GRID_GROW(g->h_pts, (size_t)room * sizeof(float4));
        GRID_GROW(g->d_pts, (size_t)room * sizeof(float4));
        for (int64_t at = 0; at < n; at += room) {
            const int64_t m = std::min(room, n - at);
            if (at > 0) GRID_TRY(wait, hipStreamSynchronize(s));   // the staging buffer is read until here
            memcpy(g->h_pts, xyzv + 4 * at, (size_t)m * sizeof(float4));
            GRID_TRY(copy, hipMemcpyAsync(g->d_pts, g->h_pts, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, s));
            GRID_TRY(launch, (grid::launch_align_mark(s, j, g->d_pts, nullptr, m), hipGetLastError()));
        }
    }
    if ((rc = align_finish(s, j))) return rc;
    GRID_TRY(copy, hipMemcpyAsync(g->h_arec, j.rec, grid::ALIGN_REC * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GRID_TRY(wait, hipStreamSynchronize(s));
    settle(g);
    g->valid |= ALIGN_LAST;
    memcpy(g->align_rec, g->h_arec, sizeof(g->align_rec));
    g->align_Pa = Pa, g->align_Pb = Pb;
    memcpy(rec, g->align_rec, sizeof(g->align_rec));
    return SVH_OK;
}

int get_align_field(svh_grid* g, uint8_t* out, bool on_device) {
    grid::AlignJob j;
    int rc = object_align_job(g, 0, 0, 0, &j);
    if (rc) return rc;
    if ((rc = align_field(g, j))) return rc;
    if ((rc = deliver(g, j.field, g->ncells, out, on_device))) return rc;
    settle(g);
    return SVH_OK;
}

int render_align(svh_grid* g, uint8_t* rgb, bool on_device) {
    return render_with(g, rgb, on_device, false, [&](uint8_t* dst) {
        const int rc = finalise(g);
        if (rc) return rc;
        grid::launch_render(g->stream, render_job(g, grid::M_LOCAL, dst));
        grid::AlignJob j{};   // the buffers are those of the last alignment: nothing grows
        j.prm = g->prm, j.alp = g->alp, j.Pa = g->align_Pa, j.Pb = g->align_Pb;
        memcpy(j.rot, g->align_rot, sizeof(j.rot));
        j.scan = g->al.scan;
        const int32_t* rec = g->align_rec;
        grid::launch_align_overlay(g->stream, j, rec[grid::AR_SCAN], rec[grid::AR_K], rec[grid::AR_TA], rec[grid::AR_TB], dst);
        return rc;
    });
}

// what svh_test_grid_align and svh_test_grid_align_device share: the arguments checked and converted, the pivot's sub
bool align_test_args(const svh_grid_params* p, const svh_grid_align_params* a, int32_t oa, int32_t ob, const uint8_t* state, const float* xyzv,
                     int64_t n_pts, const int32_t* subs, int64_t n_subs, const double pivot[3], const int32_t pivot_sub[2], const int32_t* scan,
                     int64_t cap, const int32_t* rec, grid::Params* q, grid::AlignParams* aq, int32_t* Pa, int32_t* Pb) {
    if (!convert(p, q) || !convert_align(a, q->cell, aq) || !grid::offsets_ok(oa, ob) || !state || !rec || cap < 0 || (cap > 0 && !scan)) return false;
    q->oa = oa, q->ob = ob;
    if (pivot_sub) {
        if (n_subs < 0 || n_subs > kMaxPoints || (n_subs > 0 && !subs)) return false;
        for (int64_t i = 0; i < 2 * n_subs; i++)
            if (subs[i] <= -grid::ALIGN_SUB_LIMIT || subs[i] >= grid::ALIGN_SUB_LIMIT) return false;
        if (pivot_sub[0] <= -grid::ALIGN_SUB_LIMIT || pivot_sub[0] >= grid::ALIGN_SUB_LIMIT || pivot_sub[1] <= -grid::ALIGN_SUB_LIMIT ||
            pivot_sub[1] >= grid::ALIGN_SUB_LIMIT)
            return false;
        *Pa = pivot_sub[0], *Pb = pivot_sub[1];
        return true;
    }
    float pv[3];
    if (n_pts < 0 || n_pts > kMaxPoints || (n_pts > 0 && !xyzv) || !position(pivot, pv)) return false;
    return grid::align_pivot(*q, pv[0], pv[1], pv[2], Pa, Pb);
}

// ... and a failed add leaves the empty grid
int added(svh_grid* g, int rc) {
    if (failed(g, rc) == SVH_ERR_HIP) mark_empty(g);
    return rc;
}

// the archive's buffers exist and hold what the object says they hold; the layer is on
int archive_ready(svh_grid* g) {
    const size_t tiles = (size_t)g->arch_tiles, table = grid::archive_table_size(g->arch_tiles);
    if (g->arch_pool.cap < tiles * grid::PAGE_BYTES || g->arch_keys.cap < table * sizeof(unsigned long long)) g->arch_need_clear = true;
    GRID_GROW(g->arch_pool, tiles * grid::PAGE_BYTES);
    GRID_GROW_N(g->arch_keys, table);
    GRID_GROW_N(g->arch_page, table);
    GRID_GROW_N(g->arch_claims, table);
    GRID_GROW_N(g->arch_stack, tiles);
    GRID_GROW_N(g->arch_ctl, grid::AR_WORDS);
    GRID_GROW_N(g->h_arch_ctl, grid::AR_WORDS);
    if (g->arch_need_clear) {
        GRID_TRY(copy, hipMemsetAsync(g->arch_keys, 0xFF, table * sizeof(unsigned long long), g->stream));
        GRID_TRY(copy, hipMemsetAsync(g->arch_page, 0xFF, table * sizeof(int32_t), g->stream));
        g->arch_need_clear = false;   // in stream order before whatever the entry does next; every entry ends with a wait
        GRID_TRY(launch, (grid::launch_archive_reset(g->stream, g->archive()), hipGetLastError()));
    }
    return SVH_OK;
}

// the counts of the archive from the control words, which the entry has copied to h_arch_ctl and waited for
void read_archive_stats(svh_grid* g) {
    const unsigned long long* h = g->h_arch_ctl;
    g->arch_stats[grid::AS_PAGES] = (int64_t)g->arch_tiles - (int64_t)h[grid::AR_FREE];
    g->arch_stats[grid::AS_SAVED] = (int64_t)h[grid::AR_SAVED], g->arch_stats[grid::AS_RESTORED] = (int64_t)h[grid::AR_RESTORED];
    g->arch_stats[grid::AS_LOST] = (int64_t)h[grid::AR_LOST], g->arch_stats[grid::AS_REFUSED] = (int64_t)h[grid::AR_REFUSED];
}

// scroll() with the archive on: the leaving pass with the old offsets, then the entering pass with the new ones; one wait
int scroll_archived(svh_grid* g, int32_t da, int32_t db) {
    int rc = archive_ready(g);
    if (rc) return rc;
    if (g->dyn_on && (rc = dyn_ready(g))) return rc;
    grid::ArchScrollJob j;
    j.prm = g->prm;
    j.prm.oa -= da, j.prm.ob -= db;   // the old offsets
    j.da = da, j.db = db;
    j.cells = g->cells();
    j.dyn = g->dyn_on;
    if (j.dyn) j.planes = g->dplanes();
    j.ar = g->archive();
    GRID_TRY(launch, (grid::launch_archive_leave(g->stream, j), hipGetLastError()));
    j.prm = g->prm;
    GRID_TRY(launch, (grid::launch_archive_enter(g->stream, j), hipGetLastError()));
    g->body_valid = false;   // a restored cell has its accumulators and an empty body
    GRID_TRY(copy, hipMemcpyAsync(g->h_arch_ctl, g->arch_ctl, grid::AR_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->stream));
    GRID_TRY(wait, hipStreamSynchronize(g->stream));
    read_archive_stats(g);
    return SVH_OK;
}

// the window moves by (da, db) cells to offsets that have been checked, not both zero
int scroll(svh_grid* g, int32_t da, int32_t db) {
    g->prm.oa += da, g->prm.ob += db;
    touch(g, ACC);
    if (g->need_clear) return SVH_OK;   // the empty grid has no cell to reset, and its archive is as empty
    int rc = ready(g);
    if (rc) return rc;
    if (g->arch_tiles > 0) return scroll_archived(g, da, db);
    const int64_t ada = da < 0 ? -(int64_t)da : da, adb = db < 0 ? -(int64_t)db : db;
    const bool dyn = g->dyn_on && !g->dyn_need_clear && g->dynp.cap >= g->ncells * grid::DYN_BYTES;   // the layer has cells to reset
    if (ada >= g->prm.nx || adb >= g->prm.nz) {
        if ((rc = fill_empty(g))) return rc;
        if (dyn) GRID_TRY(copy, hipMemsetAsync(g->dynp, 0, g->ncells * grid::DYN_BYTES, g->stream));
    } else {
        grid::EnterJob j;
        j.prm = g->prm;
        j.da = da, j.db = db;
        j.cells = g->cells();
        GRID_TRY(launch, (grid::launch_enter(g->stream, j), hipGetLastError()));
        if (dyn) GRID_TRY(launch, (grid::launch_dyn_enter(g->stream, g->prm, da, db, g->dplanes()), hipGetLastError()));
    }
    GRID_TRY(wait, hipStreamSynchronize(g->stream));
    return SVH_OK;
}

// xyz rounded to float once; false: a null pointer or a position that is not finite
bool position(const double xyz[3], float p[3]) {
    if (!xyz) return false;
    for (int k = 0; k < 3; k++) {
        if (!finite_d(xyz[k])) return false;
        p[k] = (float)xyz[k];
    }
    return true;
}

// the logical index of the cell rays are cast from, or -1: the origin must be a LOW point of the window
int64_t origin_cell(const svh_grid* g, const double origin[3], int32_t* q = nullptr) {
    float p[3];
    if (!position(origin, p)) return -1;
    const grid::Placed r = grid::place(g->prm, p[0], p[1], p[2], 0.f);
    if (q) *q = r.q;   // an observation's q_o
    return r.fate == grid::LOW ? (int64_t)r.cell : -1;
}

const char* const kNoDyn =": the dynamics are not set (svh_grid_set_dynamics)";

}  // namespace

extern "C" {

int32_t svh_grid_frame_camera(double cam_height, double T[12]) {
    if (!T || !finite_d(cam_height)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_frame_camera: a finite height and T are needed");
    const double t[12] = {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, cam_height};
    memcpy(T, t, sizeof(t));
    return SVH_OK;
}

int32_t svh_grid_frame_plane(const double plane_e[3], const double H[16], double T[12]) {
    if (!plane_e || !H || !T) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_frame_plane: null argument");
    for (int k = 0; k < 3; k++)
        if (!finite_d(plane_e[k])) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_frame_plane: the plane is not finite");
    for (int k = 0; k < 16; k++)
        if (!finite_d(H[k])) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_frame_plane: the transformation is not finite");
    const double norm = sqrt((plane_e[0] * plane_e[0] + plane_e[1] * plane_e[1]) + plane_e[2] * plane_e[2]);
    if (!(norm > 0.0) || !finite_d(norm) || !finite_d(1.0 / norm))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_frame_plane: |e| == 0, the estimate found no plane");
    for (int k = 0; k < 3; k++) {
        T[k] = H[4 * k];                 // r1, the first column of H
        T[4 + k] = H[4 * k + 2];         // r3, the third
        T[8 + k] = -(plane_e[k] / norm); // -r2
    }
    T[3] = 0.0, T[7] = 0.0, T[11] = 1.0 / norm;
    return SVH_OK;
}

void svh_grid_params_default(svh_grid_params* p) {
    if (!p) return;
    p->nx = 256, p->nz = 256;
    p->cell = 0.2f, p->x0 = -25.6f, p->z0 = 0.f;
    (void)svh_grid_frame_camera(1.65, p->T);
    p->min_points = 3;
    p->step = 0.2f, p->drop = 0.3f, p->clearance = 2.0f;
    p->render_h_lo = 0.f, p->render_h_hi = 2.f;
}

void svh_grid_trav_params_default(svh_grid_trav_params* t) {
    if (!t) return;
    t->max_slope = 0.35f, t->inscribed = 0.4f, t->inflate = 1.5f;
    t->lethal = SVH_GRID_LETHAL_OBSTACLE | SVH_GRID_LETHAL_DROP | SVH_GRID_LETHAL_STEEP;
}

svh_grid* svh_grid_create(const svh_grid_params* p) {
    svh::ensure_init();
    grid::Params q;
    if (!convert(p, &q)) {
        svh::fail(SVH_ERR_BAD_ARG, "svh_grid_create: parameters out of range (include/svh_grid.h)");
        return nullptr;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
        return nullptr;
    }
    svh_grid* g = new svh_grid();
    g->prm = q;
    g->ncells = (size_t)q.nx * (size_t)q.nz;
    svh_grid_trav_params t;
    svh_grid_trav_params_default(&t);
    g->trav_ok = convert_trav(&t, q.cell, &g->trv, &g->table);   // false: no traversability until it is set
    (void)g->rol.derive(q.cell);                                 // R 0: no rollouts until svh_grid_set_roll succeeds
    g->exp_R = grid::explore_range(g->exp.range, q.cell);        // 0: no exploration until svh_grid_set_explore succeeds
    (void)hipGetDevice(&g->device);
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
        delete g;
        svh::fail(SVH_ERR_HIP, "svh_grid_create: hipStreamCreateWithFlags failed");
        return nullptr;
    }
    return g;
}

void svh_grid_destroy(svh_grid* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    const hipStream_t s = g->stream;
    if (s) (void)hipStreamSynchronize(s);
    delete g;   // the buffers free themselves, on the device selected above
    if (s) (void)hipStreamDestroy(s);
}

int32_t svh_grid_clear(svh_grid* g) {
    if (!g) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_clear: null argument");
    forget_goals(g);
    mark_empty(g);
    return SVH_OK;
}

int32_t svh_grid_set_window(svh_grid* g, float x0, float z0) {
    if (!g || !grid::finite_f(x0) || !grid::finite_f(z0)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_window: a grid and a finite corner are needed");
    g->prm.x0 = x0, g->prm.z0 = z0;
    g->prm.oa = g->prm.ob = 0;
    forget_goals(g);
    forget_tracks(g);
    mark_empty(g);
    return SVH_OK;
}

int32_t svh_grid_add_points(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device) {
    if (!g || n < 0 || (n > 0 && !xyzv)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_points: bad arguments");
    if (on_device && ((uintptr_t)xyzv & 15)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_points: a device array must be 16-byte aligned");
    if (n > kMaxPoints - g->st.added) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_grid_add_points: more than 2^31 - 1 points since the last clear");
    if (n == 0) return SVH_OK;
    return added(g, add(g, xyzv, n, on_device != 0));
}

int32_t svh_grid_add_view(svh_grid* g, svh_view* v) {
    if (!g || !v) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_view: null argument");
    const view::StoreRef r = view::store_of(v);
    if (r.device != g->device) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_view: the view lives on another device");
    if (r.n > kMaxPoints - g->st.added) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_grid_add_view: more than 2^31 - 1 points since the last clear");
    if (r.n == 0) return SVH_OK;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipSetDevice(g->device));
        GRID_TRY(wait, hipStreamSynchronize(r.stream));   // the store is complete before this stream reads it
        return add(g, (const float*)r.pts, r.n, true);
    }();
    return added(g, rc);
}

int32_t svh_grid_add_points_from(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device, const double origin[3]) {
    if (!g || n < 0 || (n > 0 && !xyzv) || !origin) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_points_from: bad arguments");
    if (on_device && ((uintptr_t)xyzv & 15)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_points_from: a device array must be 16-byte aligned");
    const int64_t oc = origin_cell(g, origin);
    if (oc < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_points_from: the origin must be finite, inside the window and not above the clearance");
    if (n > kMaxPoints - g->st.added) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_grid_add_points_from: more than 2^31 - 1 points since the last clear");
    if (n == 0) return SVH_OK;
    return added(g, add(g, xyzv, n, on_device != 0, oc));
}

int32_t svh_grid_add_view_lists_from(svh_grid* g, svh_view* v, int32_t first_list, int32_t n_lists, const double origin[3]) {
    if (!g || !v || !origin) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_view_lists_from: null argument");
    const view::StoreRef r = view::store_of(v);
    if (r.device != g->device) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_view_lists_from: the view lives on another device");
    int64_t at = 0, n = 0;
    if (!view::list_range(v, first_list, n_lists, &at, &n))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_view_lists_from: the lists are not all in the view's sequence");
    const int64_t oc = origin_cell(g, origin);
    if (oc < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_add_view_lists_from: the origin must be finite, inside the window and not above the clearance");
    if (n > kMaxPoints - g->st.added) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_grid_add_view_lists_from: more than 2^31 - 1 points since the last clear");
    if (n == 0) return SVH_OK;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipSetDevice(g->device));
        GRID_TRY(wait, hipStreamSynchronize(r.stream));   // the store is complete before this stream reads it
        return add(g, (const float*)(r.pts + at), n, true, oc);
    }();
    return added(g, rc);
}

int32_t svh_grid_scroll(svh_grid* g, int32_t da, int32_t db) {
    if (!g) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_scroll: null argument");
    const int64_t ta = (int64_t)g->prm.oa + da, tb = (int64_t)g->prm.ob + db;
    if (ta < -grid::OFFSET_LIMIT || ta > grid::OFFSET_LIMIT || tb < -grid::OFFSET_LIMIT || tb > grid::OFFSET_LIMIT)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_scroll: the offsets would leave -(2^20 - 8192) .. 2^20 - 8192");
    if (da == 0 && db == 0) return SVH_OK;
    return added(g, scroll(g, da, db));
}

int32_t svh_grid_get_window(svh_grid* g, int32_t off[2]) {
    if (!g || !off) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_window: null argument");
    off[0] = g->prm.oa, off[1] = g->prm.ob;
    return SVH_OK;
}

int32_t svh_grid_cell_of(svh_grid* g, const double xyz[3], int32_t cell[2]) {
    float p[3];
    int32_t ga, gb;
    if (!g || !cell || !position(xyz, p) || !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_cell_of: a grid, an output and a finite position with a cell below 2^20 are needed");
    cell[0] = ga, cell[1] = gb;
    return SVH_OK;
}

int32_t svh_grid_follow(svh_grid* g, const double xyz[3], int32_t ia, int32_t ib) {
    float p[3];
    int32_t ga, gb;
    if (!g || ia < 0 || ia >= g->prm.nx || ib < 0 || ib >= g->prm.nz || !position(xyz, p) ||
        !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_follow: a grid, a window cell and a finite position with a cell below 2^20 are needed");
    const int64_t da = (int64_t)ga - ia - g->prm.oa, db = (int64_t)gb - ib - g->prm.ob;   // each within +-2^22
    return svh_grid_scroll(g, (int32_t)da, (int32_t)db);
}

int32_t svh_grid_get_ray_stats(svh_grid* g, int64_t out[2]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_ray_stats: null argument");
    out[0] = g->rays, out[1] = g->ray_cells;
    return SVH_OK;
}

int32_t svh_grid_get_local(svh_grid* g, int32_t plane, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::L_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_local: a grid, a plane 0..1 and an output are needed");
    return failed(g, plane == grid::L_PASS ? get(g, false, F_PASS, out, on_device != 0) : get(g, true, B_STATE, out, on_device != 0));
}

int32_t svh_grid_render_local(svh_grid* g, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_local: a grid and an output are needed");
    return failed(g, render(g, grid::M_LOCAL, rgb, on_device != 0));
}

int32_t svh_grid_get_stats(svh_grid* g, svh_grid_stats* stats) {
    if (!g || !stats) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_stats: null argument");
    *stats = g->st;
    return SVH_OK;
}

int32_t svh_grid_get(svh_grid* g, int32_t plane, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::P_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get: a grid, a plane 0..6 and an output are needed");
    static const int word[5] = {F_COUNT, F_OVERHEAD, F_HMIN, F_HMAX, F_HMEAN};
    const bool bytes = plane >= grid::P_INTENSITY;
    return failed(g, get(g, bytes, bytes ? (plane == grid::P_INTENSITY ? B_INTENSITY : B_CLASS) : word[plane], out, on_device != 0));
}

int32_t svh_grid_render(svh_grid* g, int32_t mode, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb || mode < 0 || mode >= grid::M_MODES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render: a grid, a mode 0..2 and an output are needed");
    return failed(g, render(g, mode, rgb, on_device != 0));
}

int32_t svh_grid_set_traversability(svh_grid* g, const svh_grid_trav_params* t) {
    grid::TravParams q;
    std::vector<uint8_t> table;
    if (!g || !convert_trav(t, g->prm.cell, &q, &table))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_traversability: a grid and parameters in range, with a reach of 1..256 cells, are needed (include/svh_grid.h)");
    g->trv = q;
    g->table.swap(table);
    g->trav_ok = true;
    touch(g, TRAV_PARAMS);
    return failed(g, send_table(g));   // a failed upload is repeated by the next svh_grid_get_trav / svh_grid_render_cost
}

int32_t svh_grid_get_traversability(svh_grid* g, svh_grid_trav_params* t, int32_t* reach) {
    if (!g || (!t && !reach)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_traversability: a grid and an output are needed");
    if (t) t->max_slope = g->trv.max_slope, t->inscribed = g->trv.inscribed, t->inflate = g->trv.inflate, t->lethal = g->trv.lethal;
    if (reach) *reach = g->trav_ok ? g->trv.reach : 0;
    return SVH_OK;
}

int32_t svh_grid_get_trav(svh_grid* g, int32_t plane, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::TV_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_trav: a grid, a plane 0..2 and an output are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_trav: the default traversability does not fit this grid's cell; set one (svh_grid_set_traversability)");
    return failed(g, get_trav(g, plane, out, on_device != 0));
}

int32_t svh_grid_render_cost(svh_grid* g, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_cost: a grid and an output are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_cost: the default traversability does not fit this grid's cell; set one (svh_grid_set_traversability)");
    return failed(g, render_cost(g, rgb, on_device != 0));
}

void svh_grid_plan_params_default(svh_grid_plan_params* p) {
    if (!p) return;
    p->neutral = 50, p->unknown = -1, p->max_cost = 0x7FFFFFFE;
}

int32_t svh_grid_set_plan(svh_grid* g, const svh_grid_plan_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_plan: null argument");
    const grid::PlanParams q{p->neutral, p->unknown, p->max_cost};
    if (!grid::plan_ok(q)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_plan: parameters out of range (include/svh_grid.h)");
    g->pln = q;
    touch(g, PLAN_PARAMS);
    return SVH_OK;
}

int32_t svh_grid_get_plan(svh_grid* g, svh_grid_plan_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_plan: null argument");
    p->neutral = g->pln.neutral, p->unknown = g->pln.unknown, p->max_cost = g->pln.max_cost;
    return SVH_OK;
}

int32_t svh_grid_plan_set_goals(svh_grid* g, const int32_t* cells, int32_t n) {
    if (!g || n < 0 || n > grid::PLAN_MAX_GOALS || (n > 0 && !cells))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_plan_set_goals: a grid and 0..65536 goals are needed");
    for (int32_t k = 0; k < 2 * n; k++)
        if (cells[k] <= -grid::PLAN_GOAL_LIMIT || cells[k] >= grid::PLAN_GOAL_LIMIT)
            return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_plan_set_goals: a goal's cell is not below 2^20");
    g->goals.assign(cells, cells + 2 * (size_t)n);
    touch(g, GOALS);
    return SVH_OK;
}

int32_t svh_grid_plan_set_goal(svh_grid* g, const double xyz[3]) {
    float p[3];
    int32_t cell[2];
    if (!g || !position(xyz, p) || !grid::global_cell(g->prm, p[0], p[1], p[2], &cell[0], &cell[1]))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_plan_set_goal: a grid and a finite position with a cell below 2^20 are needed");
    return svh_grid_plan_set_goals(g, cell, 1);
}

int32_t svh_grid_get_plan_plane(svh_grid* g, int32_t plane, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::PL_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_plan_plane: a grid, a plane 0..1 and an output are needed");
    if (on_device && plane == grid::PL_POT && ((uintptr_t)out & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_plan_plane: a device array of POT must be 4-byte aligned");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_plan_plane") + kNoTrav);
    return failed(g, get_plan(g, plane, out, on_device != 0), kPlanner);
}

int32_t svh_grid_get_plan_stats(svh_grid* g, int64_t out[4]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_plan_stats: null argument");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_plan_stats") + kNoTrav);
    int rc = ready(g);
    if (!rc) rc = plan_field(g);
    if (rc) return failed(g, rc, kPlanner);
    out[0] = (int64_t)(g->goals.size() / 2), out[1] = g->plan_counted, out[2] = g->plan_reached, out[3] = g->plan_rounds;
    return SVH_OK;
}

int32_t svh_grid_plan_path(svh_grid* g, const double start_xyz[3], int32_t* cells, int64_t cap, int64_t* len, int32_t* cost) {
    float p[3];
    int32_t ga, gb;
    if (!g || !len || !cost || cap < 0 || (cap > 0 && !cells) || !position(start_xyz, p) ||
        !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_plan_path: a grid, outputs and a finite start with a cell below 2^20 are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_plan_path") + kNoTrav);
    const int64_t a = (int64_t)ga - g->prm.oa, b = (int64_t)gb - g->prm.ob;
    if (a < 0 || a >= g->prm.nx || b < 0 || b >= g->prm.nz) {
        *len = 0, *cost = grid::PLAN_FAR;
        return grid::PATH_OUTSIDE;
    }
    int64_t n = 0;
    int32_t c = grid::PLAN_FAR, status = 0;
    const int rc = failed(g, plan_path(g, (int32_t)a, (int32_t)b, cells, cap, &n, &c, &status), kPlanner);
    if (rc) return rc;
    *len = n, *cost = c;
    return status;
}

int32_t svh_grid_render_plan(svh_grid* g, const int32_t* cells, int64_t n, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb || n < 0 || (n > 0 && !cells)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_plan: a grid, n >= 0 cells and an output are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_plan") + kNoTrav);
    return failed(g, render_plan(g, cells, n, rgb, on_device != 0), kPlanner);
}

void svh_grid_front_params_default(svh_grid_front_params* p) {
    if (!p) return;
    p->max_cell_cost = 252, p->min_size = 8, p->unexplored = SVH_GRID_LETHAL_UNSEEN, p->border = 0;
}

int32_t svh_grid_set_frontier(svh_grid* g, const svh_grid_front_params* p) {
    grid::FrontParams q;
    if (!g || !convert_front(p, &q)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_frontier: a grid and parameters in range are needed (include/svh_grid.h)");
    g->frp = q;
    touch(g, FRONT_PARAMS);
    return SVH_OK;
}

int32_t svh_grid_get_frontier(svh_grid* g, svh_grid_front_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_frontier: null argument");
    p->max_cell_cost = g->frp.max_cell_cost, p->min_size = g->frp.min_size, p->unexplored = g->frp.unexplored, p->border = g->frp.border;
    return SVH_OK;
}

int32_t svh_grid_get_front_plane(svh_grid* g, int32_t plane, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::FP_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_front_plane: a grid, a plane 0..1 and an output are needed");
    if (on_device && plane == grid::FP_LABEL && ((uintptr_t)out & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_front_plane: a device array of LABEL must be 4-byte aligned");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_front_plane") + kNoTrav);
    return failed(g, get_front(g, plane, out, on_device != 0), kFrontier);
}

int32_t svh_grid_get_frontiers(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n) {
    if (!g || !n || cap < 0 || (cap > 0 && !recs)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_frontiers: a grid, a count and room for cap >= 0 records are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_frontiers") + kNoTrav);
    return failed(g, get_frontiers(g, recs, cap, n), kFrontier);
}

int32_t svh_grid_get_frontier_stats(svh_grid* g, int64_t out[5]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_frontier_stats: null argument");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_frontier_stats") + kNoTrav);
    int rc = ready(g);
    if (!rc) rc = frontiers(g);
    if (rc) return failed(g, rc, kFrontier);
    memcpy(out, g->front_stats, sizeof(g->front_stats));
    return SVH_OK;
}

int32_t svh_grid_plan_set_goals_frontiers(svh_grid* g) {
    if (!g) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_plan_set_goals_frontiers: null argument");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_plan_set_goals_frontiers") + kNoTrav);
    int64_t kept = 0;
    std::vector<int32_t> recs;
    int rc = ready(g);
    if (!rc) rc = frontiers(g);
    if (!rc) {
        recs.resize((size_t)std::min<int64_t>(g->front_stats[grid::FS_KEPT], grid::PLAN_MAX_GOALS) * grid::FRONT_REC);
        rc = get_frontiers(g, recs.data(), (int64_t)(recs.size() / grid::FRONT_REC), &kept);
    }
    if (rc) return failed(g, rc, kFrontier);                     // the goals are as they were
    const size_t m = recs.size() / grid::FRONT_REC;
    g->goals.resize(2 * m);
    for (size_t k = 0; k < m; k++)
        g->goals[2 * k] = recs[k * grid::FRONT_REC + grid::FR_REP_GA], g->goals[2 * k + 1] = recs[k * grid::FRONT_REC + grid::FR_REP_GB];
    touch(g, GOALS);
    return (int32_t)m;
}

int32_t svh_grid_render_frontiers(svh_grid* g, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_frontiers: a grid and an output are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_frontiers") + kNoTrav);
    return failed(g, render_frontiers(g, rgb, on_device != 0), kFrontier);
}

void svh_grid_obj_params_default(svh_grid_obj_params* p) {
    if (!p) return;
    p->min_size = 4, p->max_size = 4096, p->min_height = 0.3f, p->max_tracks = 1024, p->min_overlap = 1;
    p->gate = 4, p->max_missed = 2, p->min_age = 3, p->move_cells = 2, p->smooth_shift = 1;
}

int32_t svh_grid_set_objects(svh_grid* g, const svh_grid_obj_params* p) {
    grid::ObjParams q;
    if (!g || !convert_obj(p, &q)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_objects: a grid and parameters in range are needed (include/svh_grid_obj.h)");
    g->obp = q;
    touch(g, OBJ_PARAMS);
    forget_tracks(g);
    return SVH_OK;
}

int32_t svh_grid_get_objects_params(svh_grid* g, svh_grid_obj_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_objects_params: null argument");
    const grid::ObjParams& q = g->obp;
    p->min_size = q.min_size, p->max_size = q.max_size, p->min_height = q.min_height, p->max_tracks = q.max_tracks, p->min_overlap = q.min_overlap;
    p->gate = q.gate, p->max_missed = q.max_missed, p->min_age = q.min_age, p->move_cells = q.move_cells, p->smooth_shift = q.smooth_shift;
    return SVH_OK;
}

int32_t svh_grid_get_obj_plane(svh_grid* g, int32_t plane, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::OP_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_obj_plane: a grid, a plane 0..1 and an output are needed");
    if (on_device && plane == grid::OP_LABEL && ((uintptr_t)out & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_obj_plane: a device array of LABEL must be 4-byte aligned");
    return failed(g, get_obj(g, plane, out, on_device != 0), kObjects);
}

int32_t svh_grid_get_objects(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n) {
    if (!g || !n || cap < 0 || (cap > 0 && !recs)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_objects: a grid, a count and room for cap >= 0 records are needed");
    return failed(g, get_objects(g, recs, cap, n), kObjects);
}

int32_t svh_grid_get_object_stats(svh_grid* g, int64_t out[7]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_object_stats: null argument");
    int rc = ready(g);
    if (!rc) rc = objects(g);
    if (rc) return failed(g, rc, kObjects);
    memcpy(out, g->obj_stats, sizeof(g->obj_stats));
    return SVH_OK;
}

int32_t svh_grid_objects_step(svh_grid* g, int32_t* assign, int64_t cap, int64_t* n_obj) {
    if (!g || !n_obj || cap < 0 || (cap > 0 && !assign)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_objects_step: a grid, a count and room for cap >= 0 ids are needed");
    if (g->trk_stats[grid::TS_STEPS] >= 0x7FFFFFFF) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_grid_objects_step: 2^31 - 1 steps since the tracks were last emptied");
    const int rc = failed(g, objects_step(g, assign, cap, n_obj), kObjects);
    if (rc == SVH_ERR_HIP) forget_tracks(g);   // a half-done step cannot be taken back
    return rc;
}

int32_t svh_grid_objects_reset(svh_grid* g) {
    if (!g) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_objects_reset: null argument");
    forget_tracks(g);
    return SVH_OK;
}

int32_t svh_grid_get_tracks(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n) {
    if (!g || !n || cap < 0 || (cap > 0 && !recs)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_tracks: a grid, a count and room for cap >= 0 records are needed");
    return failed(g, get_tracks(g, recs, cap, n));
}

int32_t svh_grid_get_track_plane(svh_grid* g, int32_t* out, int32_t on_device, int32_t off[2]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_track_plane: a grid and an output are needed");
    if (on_device && ((uintptr_t)out & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_track_plane: a device array must be 4-byte aligned");
    const int rc = failed(g, get_track_plane(g, out, on_device != 0));
    if (!rc && off) off[0] = g->trk_plane ? g->trk_oa : g->prm.oa, off[1] = g->trk_plane ? g->trk_ob : g->prm.ob;
    return rc;
}

int32_t svh_grid_get_track_stats(svh_grid* g, int64_t out[8]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_track_stats: null argument");
    memcpy(out, g->trk_stats, sizeof(g->trk_stats));
    return SVH_OK;
}

int32_t svh_grid_render_objects(svh_grid* g, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_objects: a grid and an output are needed");
    return failed(g, render_objects(g, rgb, on_device != 0), kObjects);
}

void svh_grid_pred_params_default(svh_grid_pred_params* p) {
    if (!p) return;
    p->slots = 8, p->stride = 1, p->poses_per_step = 1, p->margin = 1, p->grow16 = 0, p->only_moving = 1;
}

int32_t svh_grid_set_predict(svh_grid* g, const svh_grid_pred_params* p) {
    grid::PredParams q;
    if (!g || !convert_pred(p, &q)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_predict: a grid and parameters in range are needed (include/svh_grid_pred.h)");
    g->prp = q;
    touch(g, PRED_PARAMS);
    return SVH_OK;
}

int32_t svh_grid_get_predict(svh_grid* g, svh_grid_pred_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_predict: null argument");
    const grid::PredParams& q = g->prp;
    p->slots = q.slots, p->stride = q.stride, p->poses_per_step = q.poses_per_step, p->margin = q.margin, p->grow16 = q.grow16, p->only_moving = q.only_moving;
    return SVH_OK;
}

int32_t svh_grid_get_pred_plane(svh_grid* g, uint32_t* out, int32_t on_device, int32_t off[2]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_pred_plane: a grid and an output are needed");
    if (on_device && ((uintptr_t)out & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_pred_plane: a device array must be 4-byte aligned");
    const int rc = failed(g, get_pred_plane(g, out, on_device != 0), kPrediction);
    if (!rc && off) off[0] = pred_oa(g), off[1] = pred_ob(g);
    return rc;
}

int32_t svh_grid_get_pred_stats(svh_grid* g, int64_t out[4]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_pred_stats: null argument");
    return failed(g, get_pred_stats(g, out), kPrediction);
}

int32_t svh_grid_footprint_pred(svh_grid* g, const int32_t* poses, int64_t n, int32_t on_device, uint32_t* out) {
    if (!g || n < 0 || n > ((int64_t)1 << 26) || (n > 0 && (!poses || !out)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_footprint_pred: a grid and 0..2^26 poses with room for their masks are needed");
    if (on_device && (((uintptr_t)poses | (uintptr_t)out) & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_footprint_pred: a device array must be 4-byte aligned");
    if (!g->rol.R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_footprint_pred") + kNoRoll);
    if (!on_device)
        for (int64_t i = 0; i < n; i++)
            if (poses[3 * i + 2] < 0 || poses[3 * i + 2] >= 8 * g->rol.p.m) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_footprint_pred: a heading is not in 0..8 m - 1");
    if (n == 0) return SVH_OK;
    return failed(g, footprint_pred(g, poses, n, on_device != 0, out), kPrediction);
}

int32_t svh_grid_roll_score_pred(svh_grid* g, const double anchor_xyz[3], int32_t set, int32_t* recs, int64_t* scores, int32_t on_device, int32_t* best) {
    float p[3];
    int32_t ga, gb;
    if (!g || !best || !position(anchor_xyz, p) || !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_score_pred: a grid, an output and a finite anchor with a cell below 2^20 are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_roll_score_pred") + kNoTrav);
    if (!g->rol.R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_roll_score_pred") + kNoRoll);
    if (g->cand_S == 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_score_pred: no candidates (svh_grid_roll_set_candidates)");
    if (set < 0 || set >= g->cand_S) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_score_pred: no such set");
    if (on_device && (((uintptr_t)recs & 3) || ((uintptr_t)scores & 7)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_score_pred: a device array of records must be 4-byte, one of scores 8-byte aligned");
    return failed(g, roll_score_pred(g, ga, gb, set, recs, scores, on_device != 0, best), kPrediction);
}

int32_t svh_grid_render_pred(svh_grid* g, int32_t mode, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb || mode < 0 || mode >= grid::M_MODES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_pred: a grid, a mode 0..2 and an output are needed");
    return failed(g, render_pred(g, mode, rgb, on_device != 0), kPrediction);
}

void svh_grid_roll_params_default(svh_grid_roll_params* p) {
    if (!p) return;
    p->front = 3.5f, p->rear = 1.0f, p->half_width = 0.9f;
    p->headings_m = 8, p->stop_cost = 253, p->unknown_cost = 254;
    p->w_pot = 1, p->w_cost = 1, p->w_cut = 0;
}

int32_t svh_grid_set_roll(svh_grid* g, const svh_grid_roll_params* p) {
    RollTable t;
    if (!g || !convert_roll(p, &t.p) || !t.derive(g->prm.cell))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_roll: a grid and parameters in range, with a reach of 1..128 cells, are needed (include/svh_grid.h)");
    if (t.p.m != g->rol.p.m) {   // the headings of the candidates were those of the old enumeration
        g->cands.clear(), g->cand_lens.clear();
        g->cand_S = g->cand_K = g->cand_T = 0;
        touch(g, CANDS);
    }
    g->rol = std::move(t);
    touch(g, ROLL_PARAMS);
    return failed(g, roll_tables(g, false));   // a failed upload is repeated by the next call that needs the table
}

int32_t svh_grid_get_roll(svh_grid* g, svh_grid_roll_params* p, int32_t* reach_R, int64_t* footprint_cells_total) {
    if (!g || (!p && !reach_R && !footprint_cells_total)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_roll: a grid and an output are needed");
    const grid::RollParams& q = g->rol.p;
    if (p) {
        p->front = q.front, p->rear = q.rear, p->half_width = q.half_width;
        p->headings_m = q.m, p->stop_cost = q.stop_cost, p->unknown_cost = q.unknown_cost;
        p->w_pot = q.w_pot, p->w_cost = q.w_cost, p->w_cut = q.w_cut;
    }
    if (reach_R) *reach_R = g->rol.R;
    if (footprint_cells_total) *footprint_cells_total = g->rol.R ? (int64_t)(g->rol.offs.size() / 2) : 0;
    return SVH_OK;
}

int32_t svh_grid_heading_of(svh_grid* g, const double dir_xyz[3], int32_t* k) {
    float d[3];
    if (!g || !k || !position(dir_xyz, d)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_heading_of: a grid, an output and a finite direction are needed");
    const float* T = g->prm.T;
    const float ua = (T[0] * d[0] + T[1] * d[1]) + T[2] * d[2], ub = (T[4] * d[0] + T[5] * d[1]) + T[6] * d[2];
    const int32_t h = grid::heading_of(g->rol.p.m, ua, ub);
    if (h < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_heading_of: the direction has no heading: it is zero on the ground, or not finite there");
    *k = h;
    return SVH_OK;
}

int32_t svh_grid_roll_footprint(svh_grid* g, int32_t k, int32_t* offsets, int64_t cap, int64_t* n) {
    if (!g || !n || cap < 0 || (cap > 0 && !offsets) || k < 0 || k >= 8 * g->rol.p.m)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_footprint: a grid, a heading 0..8 m - 1, a count and room for cap >= 0 offsets are needed");
    if (!g->rol.R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_roll_footprint") + kNoRoll);
    const int64_t at = g->rol.start[k], len = g->rol.start[k + 1] - at;
    if (cap > 0) memcpy(offsets, g->rol.offs.data() + 2 * at, (size_t)std::min(len, cap) * 2 * sizeof(int32_t));
    *n = len;
    return SVH_OK;
}

int32_t svh_grid_footprint_cost(svh_grid* g, const int32_t* poses, int64_t n, int32_t on_device, int32_t* out) {
    if (!g || n < 0 || n > ((int64_t)1 << 26) || (n > 0 && (!poses || !out)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_footprint_cost: a grid and 0..2^26 poses with room for their costs are needed");
    if (on_device && (((uintptr_t)poses | (uintptr_t)out) & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_footprint_cost: a device array must be 4-byte aligned");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_footprint_cost") + kNoTrav);
    if (!g->rol.R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_footprint_cost") + kNoRoll);
    if (!on_device)
        for (int64_t i = 0; i < n; i++)
            if (poses[3 * i + 2] < 0 || poses[3 * i + 2] >= 8 * g->rol.p.m) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_footprint_cost: a heading is not in 0..8 m - 1");
    if (n == 0) return SVH_OK;
    return failed(g, footprint_cost(g, poses, n, on_device != 0, out));
}

int32_t svh_grid_roll_set_candidates(svh_grid* g, const int32_t* table, int32_t S, int32_t K, int32_t T) {
    if (!g || !grid::roll_table_ok(table, S, K, T, 8 * g->rol.p.m))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_set_candidates: a grid and a table within the limits are needed: S, K, T >= 1, T <= 1024, K <= 65536, S K T <= 2^22, offsets within +-16384, headings -1..8 m - 1");
    const size_t n = (size_t)S * (size_t)K;
    g->cands.assign(table, table + n * (size_t)T * 3);
    g->cand_lens.resize(n);
    for (size_t c = 0; c < n; c++) g->cand_lens[c] = grid::roll_len(table + c * (size_t)T * 3, T);
    g->cand_S = S, g->cand_K = K, g->cand_T = T;
    touch(g, CANDS);
    if (!g->rol.R) return SVH_OK;                  // no table to send yet; svh_grid_roll_score sends both
    return failed(g, roll_tables(g, true));       // a failed upload is repeated by the next svh_grid_roll_score
}

int32_t svh_grid_roll_get_candidates(svh_grid* g, int32_t skt[3]) {
    if (!g || !skt) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_get_candidates: null argument");
    skt[0] = g->cand_S, skt[1] = g->cand_K, skt[2] = g->cand_T;
    return SVH_OK;
}

int32_t svh_grid_roll_score(svh_grid* g, const double anchor_xyz[3], int32_t set, int32_t* recs, int64_t* scores, int32_t on_device, int32_t* best) {
    float p[3];
    int32_t ga, gb;
    if (!g || !best || !position(anchor_xyz, p) || !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_score: a grid, an output and a finite anchor with a cell below 2^20 are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_roll_score") + kNoTrav);
    if (!g->rol.R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_roll_score") + kNoRoll);
    if (g->cand_S == 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_score: no candidates (svh_grid_roll_set_candidates)");
    if (set < 0 || set >= g->cand_S) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_score: no such set");
    if (on_device && (((uintptr_t)recs & 3) || ((uintptr_t)scores & 7)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_roll_score: a device array of records must be 4-byte, one of scores 8-byte aligned");
    return failed(g, roll_score(g, ga, gb, set, recs, scores, on_device != 0, best), kRollouts);
}

int32_t svh_grid_render_roll(svh_grid* g, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_roll: a grid and an output are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_roll") + kNoTrav);
    if (!has(g, ROLL_LAST)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_roll: nothing was scored since the tables were set (svh_grid_roll_score)");
    return failed(g, render_roll(g, rgb, on_device != 0));
}

void svh_grid_pose_params_default(svh_grid_pose_params* p) {
    if (!p) return;
    p->neutral = 50, p->max_cost = 0x7FFFFFFE, p->turn = 100, p->reverse = -1, p->spin = -1;
}

int32_t svh_grid_set_pose(svh_grid* g, const svh_grid_pose_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_pose: null argument");
    const grid::PoseParams q{p->neutral, p->max_cost, p->turn, p->reverse, p->spin};
    if (!grid::pose_ok(q)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_pose: parameters out of range (include/svh_grid_pose.h)");
    g->pose_prm = q;
    touch(g, POSE_PARAMS);
    return SVH_OK;
}

int32_t svh_grid_get_pose(svh_grid* g, svh_grid_pose_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_pose: null argument");
    const grid::PoseParams& q = g->pose_prm;
    p->neutral = q.neutral, p->max_cost = q.max_cost, p->turn = q.turn, p->reverse = q.reverse, p->spin = q.spin;
    return SVH_OK;
}

int32_t svh_grid_pose_set_goals(svh_grid* g, const int32_t* triples, int32_t n) {
    if (!g || n < 0 || n > grid::POSE_MAX_GOALS || (n > 0 && !triples))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_pose_set_goals: a grid and 0..65536 goals are needed");
    for (int32_t k = 0; k < n; k++)
        if (!grid::pose_goal_ok(triples + 3 * k))
            return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_pose_set_goals: a goal's cell is not below 2^20, or its heading not in -1..7");
    g->pose_goals.assign(triples, triples + 3 * (size_t)n);
    touch(g, POSE_GOALS);
    return SVH_OK;
}

int32_t svh_grid_pose_set_goal(svh_grid* g, const double xyz[3], int32_t d) {
    float p[3];
    int32_t t[3];
    if (!g || !position(xyz, p) || !grid::global_cell(g->prm, p[0], p[1], p[2], &t[0], &t[1]))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_pose_set_goal: a grid and a finite position with a cell below 2^20 are needed");
    t[2] = d;
    return svh_grid_pose_set_goals(g, t, 1);
}

int32_t svh_grid_get_pose_plane(svh_grid* g, int32_t plane, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::PP_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_pose_plane: a grid, a plane 0..2 and an output are needed");
    if (on_device && plane == grid::PP_POT && ((uintptr_t)out & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_pose_plane: a device array of PPOT must be 4-byte aligned");
    if (const char* why = pose_refusal(g)) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_pose_plane") + why);
    return failed(g, get_pose_plane(g, plane, out, on_device != 0), kPose);
}

int32_t svh_grid_get_pose_stats(svh_grid* g, int64_t out[4]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_pose_stats: null argument");
    if (const char* why = pose_refusal(g)) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_pose_stats") + why);
    int rc = ready(g);
    if (!rc) rc = pose_field(g);
    if (rc) return failed(g, rc, kPose);
    out[0] = (int64_t)(g->pose_goals.size() / 3), out[1] = g->pose_counted, out[2] = g->pose_reached, out[3] = g->pose_rounds;
    return SVH_OK;
}

int32_t svh_grid_pose_heading_of(svh_grid* g, const double dir_xyz[3], int32_t* d) {
    float v[3];
    if (!g || !d || !position(dir_xyz, v)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_pose_heading_of: a grid, an output and a finite direction are needed");
    const float* T = g->prm.T;
    const float ua = (T[0] * v[0] + T[1] * v[1]) + T[2] * v[2], ub = (T[4] * v[0] + T[5] * v[1]) + T[6] * v[2];
    const int32_t h = grid::heading_of(1, ua, ub);
    if (h < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_pose_heading_of: the direction has no heading: it is zero on the ground, or not finite there");
    *d = h;
    return SVH_OK;
}

int32_t svh_grid_pose_path(svh_grid* g, const double start_xyz[3], int32_t d, int32_t* poses, int64_t cap, int64_t* len, int32_t* cost) {
    float p[3];
    int32_t ga, gb;
    if (!g || !len || !cost || cap < 0 || (cap > 0 && !poses) || d < 0 || d >= grid::POSE_HEADINGS || !position(start_xyz, p) ||
        !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_pose_path: a grid, outputs, a heading 0..7 and a finite start with a cell below 2^20 are needed");
    if (const char* why = pose_refusal(g)) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_pose_path") + why);
    const int64_t a = (int64_t)ga - g->prm.oa, b = (int64_t)gb - g->prm.ob;
    if (a < 0 || a >= g->prm.nx || b < 0 || b >= g->prm.nz) {
        *len = 0, *cost = grid::PLAN_FAR;
        return grid::PATH_OUTSIDE;
    }
    int64_t n = 0;
    int32_t c = grid::PLAN_FAR, status = 0;
    const int rc = failed(g, pose_path(g, (int32_t)a, (int32_t)b, d, poses, cap, &n, &c, &status), kPose);
    if (rc) return rc;
    *len = n, *cost = c;
    return status;
}

int32_t svh_grid_render_pose(svh_grid* g, const int32_t* poses, int64_t n, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb || n < 0 || n > (int64_t)grid::POSE_HEADINGS * (int64_t)g->ncells || (n > 0 && !poses))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_pose: a grid, 0..8 nx nz poses (the longest path) and an output are needed");
    if (const char* why = pose_refusal(g)) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_pose") + why);
    return failed(g, render_pose(g, poses, n, rgb, on_device != 0), kPose);
}

void svh_grid_time_params_default(svh_grid_time_params* p) {
    if (!p) return;
    p->layers = 32, p->wait = 100, p->release = 1;
}

int32_t svh_grid_set_time(svh_grid* g, const svh_grid_time_params* p) {
    grid::TimeParams q;
    if (!g || !convert_time(p, &q)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_time: a grid and parameters in range are needed (include/svh_grid_time.h)");
    if (q.release != g->tmp.release) drop(g, closure(kDropsNewRelease));
    g->tmp = q;
    g->time_on = true;
    touch(g, TIME_PARAMS);
    return SVH_OK;
}

int32_t svh_grid_get_time(svh_grid* g, svh_grid_time_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_time: null argument");
    p->layers = g->tmp.layers, p->wait = g->tmp.wait, p->release = g->tmp.release;
    return SVH_OK;
}

int32_t svh_grid_get_time_plane(svh_grid* g, int32_t plane, int32_t t0, int32_t count, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::TP_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_time_plane: a grid, a plane 0..3 and an output are needed");
    const int32_t layers = (plane == grid::TP_RCOST || plane == grid::TP_RPOT) ? 1 : g->tmp.layers;
    if (t0 < 0 || count < 1 || t0 > layers - count) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_time_plane: the layers t0 .. t0 + count - 1 are not all in 0 .. layers - 1 (one layer for RCOST and RPOT)");
    if (on_device && (plane == grid::TP_TPOT || plane == grid::TP_RPOT) && ((uintptr_t)out & 3))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_time_plane: a device array of TPOT or RPOT must be 4-byte aligned");
    if (const char* why = time_refusal(g)) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_time_plane") + why);
    return failed(g, get_time_plane(g, plane, t0, count, out, on_device != 0), kTime);
}

int32_t svh_grid_get_time_stats(svh_grid* g, int64_t out[6]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_time_stats: null argument");
    if (const char* why = time_refusal(g)) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_time_stats") + why);
    int rc = ready(g);
    if (!rc) rc = time_field(g);
    if (rc) return failed(g, rc, kTime);
    for (int k = 0; k < grid::TM_WORDS; k++) out[k] = g->time_stats[k];
    out[grid::TM_RELEASED] = g->time_released, out[grid::TM_ROUNDS] = g->time_rounds;
    return SVH_OK;
}

int32_t svh_grid_time_path(svh_grid* g, const double start_xyz[3], int32_t* triples, int64_t cap, int64_t* len, int32_t* cost) {
    float p[3];
    int32_t ga, gb;
    if (!g || !len || !cost || cap < 0 || (cap > 0 && !triples) || !position(start_xyz, p) || !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_time_path: a grid, outputs and a finite start with a cell below 2^20 are needed");
    if (const char* why = time_refusal(g)) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_time_path") + why);
    const int64_t a = (int64_t)ga - g->prm.oa, b = (int64_t)gb - g->prm.ob;
    if (a < 0 || a >= g->prm.nx || b < 0 || b >= g->prm.nz) {
        *len = 0, *cost = grid::PLAN_FAR;
        return grid::PATH_OUTSIDE;
    }
    int64_t n = 0;
    int32_t c = grid::PLAN_FAR, status = 0;
    const int rc = failed(g, time_path(g, (int32_t)a, (int32_t)b, triples, cap, &n, &c, &status), kTime);
    if (rc) return rc;
    *len = n, *cost = c;
    return status;
}

int32_t svh_grid_render_time(svh_grid* g, int32_t t, const int32_t* triples, int64_t n, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb || t < 0 || t >= g->tmp.layers || n < 0 || n > (int64_t)g->ncells + g->tmp.layers || (n > 0 && !triples))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_time: a grid, a layer 0 .. layers - 1, 0 .. layers + nx nz triples (the longest path) and an output are needed");
    if (const char* why = time_refusal(g)) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_time") + why);
    return failed(g, render_time(g, t, triples, n, rgb, on_device != 0), kTime);
}

void svh_grid_explore_params_default(svh_grid_explore_params* p) {
    if (!p) return;
    p->range = 10.f, p->min_gain = 1, p->w_gain = 500, p->w_reach = 1;
}

int32_t svh_grid_set_explore(svh_grid* g, const svh_grid_explore_params* p) {
    grid::ExploreParams q;
    int32_t R = 0;
    if (!g || !convert_explore(p, &q) || !(R = grid::explore_range(q.range, g->prm.cell)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_explore: a grid and parameters in range, with a range of 1..128 cells, are needed (include/svh_grid.h)");
    g->exp = q, g->exp_R = R;
    return SVH_OK;
}

int32_t svh_grid_get_explore(svh_grid* g, svh_grid_explore_params* p, int32_t* range_R) {
    if (!g || (!p && !range_R)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_explore: a grid and an output are needed");
    if (p) p->range = g->exp.range, p->min_gain = g->exp.min_gain, p->w_gain = g->exp.w_gain, p->w_reach = g->exp.w_reach;
    if (range_R) *range_R = g->exp_R;
    return SVH_OK;
}

int32_t svh_grid_view_gain(svh_grid* g, const int32_t* cells, int64_t n, int32_t on_device, int32_t* out) {
    if (!g || n < 0 || n > ((int64_t)1 << 26) || (n > 0 && (!cells || !out)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_view_gain: a grid and 0..2^26 viewpoints with room for their gains are needed");
    if (on_device && (((uintptr_t)cells | (uintptr_t)out) & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_view_gain: a device array must be 4-byte aligned");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_view_gain") + kNoTrav);
    if (!g->exp_R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_view_gain") + kNoExplore);
    if (n == 0) {
        g->ex_stats[grid::ES_LAUNCHES] = 0;
        return SVH_OK;
    }
    return failed(g, view_gain(g, cells, n, on_device != 0, out), kExploration);
}

int32_t svh_grid_view_mask(svh_grid* g, int32_t ga, int32_t gb, uint8_t* out, int32_t on_device) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_view_mask: a grid and an output are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_view_mask") + kNoTrav);
    if (!g->exp_R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_view_mask") + kNoExplore);
    const int64_t va = (int64_t)ga - g->prm.oa, vb = (int64_t)gb - g->prm.ob;
    if (va < 0 || va >= g->prm.nx || vb < 0 || vb >= g->prm.nz) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_view_mask: the viewpoint is outside the window");
    return failed(g, view_mask(g, (int32_t)va, (int32_t)vb, out, on_device != 0), kExploration);
}

int32_t svh_grid_explore_rank(svh_grid* g, const double start_xyz[3], int32_t* recs, int64_t* scores, int64_t cap, int64_t* n, int32_t* best) {
    float p[3];
    int32_t ga, gb;
    if (!g || !n || !best || cap < 0 || !position(start_xyz, p) || !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_explore_rank: a grid, outputs, cap >= 0 and a finite start with a cell below 2^20 are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_explore_rank") + kNoTrav);
    if (!g->exp_R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_explore_rank") + kNoExplore);
    return failed(g, explore_rank(g, ga, gb, recs, scores, cap, n, best), kExploration);
}

int32_t svh_grid_plan_set_goal_explore(svh_grid* g, const double start_xyz[3]) {
    float p[3];
    int32_t ga, gb;
    if (!g || !position(start_xyz, p) || !grid::global_cell(g->prm, p[0], p[1], p[2], &ga, &gb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_plan_set_goal_explore: a grid and a finite start with a cell below 2^20 are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_plan_set_goal_explore") + kNoTrav);
    if (!g->exp_R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_plan_set_goal_explore") + kNoExplore);
    int64_t n = 0;
    int32_t best = -1;
    const int rc = failed(g, explore_rank(g, ga, gb, nullptr, nullptr, 0, &n, &best), kExploration);
    if (rc) return rc;                                 // the goals are as they were
    if (best < 0) return 0;
    int32_t rec[grid::EXPLORE_REC];
    memcpy(rec, g->h_explore.p + (size_t)n * sizeof(int64_t) + (size_t)best * sizeof(rec), sizeof(rec));
    g->goals.assign(rec + grid::ER_REP_GA, rec + grid::ER_REP_GA + 2);
    touch(g, GOALS);
    return 1;
}

int32_t svh_grid_get_explore_stats(svh_grid* g, int64_t out[4]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_explore_stats: null argument");
    memcpy(out, g->ex_stats, sizeof(g->ex_stats));
    return SVH_OK;
}

int32_t svh_grid_render_view(svh_grid* g, int32_t ga, int32_t gb, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_view: a grid and an output are needed");
    if (!g->trav_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_view") + kNoTrav);
    if (!g->exp_R) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_view") + kNoExplore);
    const int64_t va = (int64_t)ga - g->prm.oa, vb = (int64_t)gb - g->prm.ob;
    if (va < 0 || va >= g->prm.nx || vb < 0 || vb >= g->prm.nz) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_view: the viewpoint is outside the window");
    return failed(g, render_view(g, (int32_t)va, (int32_t)vb, rgb, on_device != 0), kExploration);
}

void svh_grid_align_params_default(svh_grid_align_params* p) {
    if (!p) return;
    p->reach = 0.6f, p->range = 25.6f, p->rot_den = 256, p->rot_n = 8, p->trans_n = 8, p->min_scan = 32;
}

int32_t svh_grid_set_align(svh_grid* g, const svh_grid_align_params* p) {
    grid::AlignParams q;
    if (!g || !convert_align(p, g->prm.cell, &q))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_align: a grid and parameters in range, with a reach of 1..32 and a range of 1..256 cells, are needed (include/svh_grid.h)");
    g->alp = q;
    memset(g->align_rot, 0, sizeof(g->align_rot));
    grid::align_rot_table(q.rot_den, q.rot_n, g->align_rot);
    g->align_ok = true;
    touch(g, ALIGN_PARAMS);
    return SVH_OK;
}

int32_t svh_grid_get_align_field(svh_grid* g, uint8_t* out, int32_t on_device) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_align_field: a grid and an output are needed");
    if (!g->align_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_align_field") + kNoAlign);
    return failed(g, get_align_field(g, out, on_device != 0), kAlign);
}

int32_t svh_grid_align_points(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device, const double pivot[3], int32_t rec[8]) {
    float pv[3];
    int32_t Pa, Pb;
    if (!g || n < 0 || n > kMaxPoints || (n > 0 && !xyzv) || !rec) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_points: bad arguments");
    if (on_device && ((uintptr_t)xyzv & 15)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_points: a device array must be 16-byte aligned");
    if (!g->align_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_align_points") + kNoAlign);
    if (!position(pivot, pv) || !grid::align_pivot(g->prm, pv[0], pv[1], pv[2], &Pa, &Pb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_points: the pivot must be finite with a cell below 2^20");
    return failed(g, align(g, xyzv, n, on_device != 0, Pa, Pb, rec), kAlign);
}

int32_t svh_grid_align_view_lists(svh_grid* g, svh_view* v, int32_t first_list, int32_t n_lists, const double pivot[3], int32_t rec[8]) {
    float pv[3];
    int32_t Pa, Pb;
    if (!g || !v || !rec) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_view_lists: null argument");
    if (!g->align_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_align_view_lists") + kNoAlign);
    const view::StoreRef r = view::store_of(v);
    if (r.device != g->device) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_view_lists: the view lives on another device");
    int64_t at = 0, n = 0;
    if (!view::list_range(v, first_list, n_lists, &at, &n))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_view_lists: the lists are not all in the view's sequence");
    if (!position(pivot, pv) || !grid::align_pivot(g->prm, pv[0], pv[1], pv[2], &Pa, &Pb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_view_lists: the pivot must be finite with a cell below 2^20");
    const int rc = [&]() -> int {
        GRID_TRY(none, hipSetDevice(g->device));
        GRID_TRY(wait, hipStreamSynchronize(r.stream));   // the store is complete before this stream reads it
        return align(g, (const float*)(r.pts + at), n, true, Pa, Pb, rec);
    }();
    return failed(g, rc, kAlign);
}

int32_t svh_grid_get_align_volume(svh_grid* g, int32_t* out, int32_t on_device) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_align_volume: a grid and an output are needed");
    if (on_device && ((uintptr_t)out & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_align_volume: a device array must be 4-byte aligned");
    if (!g->align_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_align_volume") + kNoAlign);
    if (!has(g, ALIGN_LAST) || g->align_rec[grid::AR_STATUS] == grid::ALIGN_FEW)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_align_volume: there is no volume: no alignment since the parameters were set, the last one failed or had too few subs");
    const int rc = [&]() -> int {
        GRID_TRY(none, hipSetDevice(g->device));
        return deliver(g, g->al.volume, (size_t)grid::align_volume_size(g->alp.rot_n, g->alp.trans_n) * sizeof(int32_t), out, on_device != 0);
    }();
    return failed(g, rc);
}

int32_t svh_grid_get_align_scan(svh_grid* g, int32_t* subs, int64_t cap, int64_t* n) {
    if (!g || !n || cap < 0 || (cap > 0 && !subs)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_align_scan: a grid, cap >= 0 with room and a count are needed");
    if (!g->align_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_align_scan") + kNoAlign);
    if (!has(g, ALIGN_LAST)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_align_scan: there is no scan: no alignment since the parameters were set, or the last one failed");
    const int64_t have = g->align_rec[grid::AR_SCAN], give = std::min(have, cap);
    if (give > 0) {
        const int rc = [&]() -> int {
            GRID_TRY(none, hipSetDevice(g->device));
            return deliver(g, g->al.scan, (size_t)give * 2 * sizeof(int32_t), subs, false);
        }();
        if (rc) return failed(g, rc);
    }
    *n = have;
    return SVH_OK;
}

int32_t svh_grid_align_correction(svh_grid* g, int32_t k, int32_t ta, int32_t tb, const double pivot[3], double M[16]) {
    float pv[3];
    if (!g || !M || !position(pivot, pv)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_correction: a grid, a finite pivot and an output are needed");
    if (!g->align_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_align_correction") + kNoAlign);
    if (k < -g->alp.rot_n || k > g->alp.rot_n || ta < -g->alp.trans_n || ta > g->alp.trans_n || tb < -g->alp.trans_n || tb > g->alp.trans_n)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_align_correction: (k, ta, tb) is no candidate of the parameters in force");
    grid::align_correction(g->prm, g->alp.rot_den, k, ta, tb, pv, M);
    return SVH_OK;
}

int32_t svh_grid_render_align(svh_grid* g, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_align: a grid and an output are needed");
    if (!g->align_ok) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_align") + kNoAlign);
    if (!has(g, ALIGN_LAST)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_align: there is no alignment to draw: none since the parameters were set, or the last one failed");
    return failed(g, render_align(g, rgb, on_device != 0));
}

void svh_grid_dyn_params_default(svh_grid_dyn_params* p) {
    if (!p) return;
    p->clear_frames = 2, p->min_through = 3, p->margin = 0.1f, p->max_age = 0;
}

int32_t svh_grid_set_dynamics(svh_grid* g, const svh_grid_dyn_params* p) {
    if (!g) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_dynamics: null argument");
    if (!p) {   // the layer and its planes go
        (void)hipSetDevice(g->device);
        if (g->stream) (void)hipStreamSynchronize(g->stream);
        g->dyn_on = false;
        g->dynp = HipBuf<uint8_t>();
        g->frame = HipBuf<uint8_t>();
        g->d_dyn = HipBuf<int32_t>();
        g->dyn_need_clear = true;
        g->frame_clean = g->body_valid = false;
        return SVH_OK;
    }
    grid::DynParams q{p->clear_frames, p->min_through, p->margin, p->max_age, 0};
    if (!grid::dyn_derive(q))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_dynamics: parameters out of range (include/svh_grid.h)");
    g->dyn = q;   // CONTRA and LAST stay when the layer was set already; the bodies follow the margin
    g->dyn_on = true;
    g->body_valid = false;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipSetDevice(g->device));
        if (g->dynp.cap < g->ncells * grid::DYN_BYTES) g->dyn_need_clear = true;   // a growth discards
        GRID_GROW(g->dynp, g->ncells * grid::DYN_BYTES);
        return SVH_OK;
    }();
    if (rc) g->dyn_need_clear = true;
    return failed(g, rc);
}

int32_t svh_grid_get_dynamics(svh_grid* g, svh_grid_dyn_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_dynamics: null argument");
    if (!g->dyn_on) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_dynamics") + kNoDyn);
    p->clear_frames = g->dyn.clear_frames, p->min_through = g->dyn.min_through, p->margin = g->dyn.margin, p->max_age = g->dyn.max_age;
    return SVH_OK;
}

int32_t svh_grid_observe_points(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device, const double origin[3]) {
    if (!g || n < 0 || (n > 0 && !xyzv) || !origin) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_points: bad arguments");
    if (on_device && ((uintptr_t)xyzv & 15)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_points: a device array must be 16-byte aligned");
    if (!g->dyn_on) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_observe_points") + kNoDyn);
    int32_t q_o = 0;
    const int64_t oc = origin_cell(g, origin, &q_o);
    if (oc < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_points: the origin must be finite, inside the window and not above the clearance");
    if (g->stamp == grid::STAMP_LIMIT) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_points: 2^31 - 1 observations since the last clear");
    if (n > kMaxPoints - g->st.added) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_grid_observe_points: more than 2^31 - 1 points since the last clear");
    return added(g, observe(g, xyzv, n, on_device != 0, oc, q_o));
}

int32_t svh_grid_observe_view_lists(svh_grid* g, svh_view* v, int32_t first_list, int32_t n_lists, const double origin[3]) {
    if (!g || !v || !origin) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_view_lists: null argument");
    const view::StoreRef r = view::store_of(v);
    if (r.device != g->device) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_view_lists: the view lives on another device");
    int64_t at = 0, n = 0;
    if (!view::list_range(v, first_list, n_lists, &at, &n))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_view_lists: the lists are not all in the view's sequence");
    if (!g->dyn_on) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_observe_view_lists") + kNoDyn);
    int32_t q_o = 0;
    const int64_t oc = origin_cell(g, origin, &q_o);
    if (oc < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_view_lists: the origin must be finite, inside the window and not above the clearance");
    if (g->stamp == grid::STAMP_LIMIT) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_observe_view_lists: 2^31 - 1 observations since the last clear");
    if (n > kMaxPoints - g->st.added) return svh::fail(SVH_ERR_UNSUPPORTED, "svh_grid_observe_view_lists: more than 2^31 - 1 points since the last clear");
    const int rc = [&]() -> int {
        GRID_TRY(none, hipSetDevice(g->device));
        GRID_TRY(wait, hipStreamSynchronize(r.stream));   // the store is complete before this stream reads it
        return observe(g, (const float*)(r.pts + at), n, true, oc, q_o);
    }();
    return added(g, rc);
}

int32_t svh_grid_get_dyn(svh_grid* g, int32_t plane, void* out, int32_t on_device) {
    if (!g || !out || plane < 0 || plane >= grid::D_PLANES) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_dyn: a grid, a plane 0..2 and an output are needed");
    if (!g->dyn_on) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_get_dyn") + kNoDyn);
    return failed(g, get_dyn(g, plane, (int32_t*)out, on_device != 0));
}

int32_t svh_grid_get_dyn_stats(svh_grid* g, int64_t out[4]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_dyn_stats: null argument");
    for (int k = 0; k < grid::DS_WORDS; k++) out[k] = g->dyn_stats[k];
    return SVH_OK;
}

int32_t svh_grid_render_dyn(svh_grid* g, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_dyn: a grid and an output are needed");
    if (!g->dyn_on) return svh::fail(SVH_ERR_BAD_ARG, std::string("svh_grid_render_dyn") + kNoDyn);
    return failed(g, render_dyn(g, rgb, on_device != 0));
}

// ---- the archive ----------------------------------------------------------------------------------------------------------
void svh_grid_archive_params_default(svh_grid_archive_params* p) {
    if (p) p->max_tiles = grid::ARCHIVE_DEFAULT_TILES;
}

int32_t svh_grid_set_archive(svh_grid* g, const svh_grid_archive_params* p) {
    if (!g || !p || p->max_tiles < 0 || p->max_tiles > grid::ARCHIVE_MAX_TILES)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_set_archive: a grid and max_tiles in 0 .. 2^20 are needed");
    if (p->max_tiles == g->arch_tiles) return SVH_OK;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    g->arch_pool = HipBuf<uint8_t>();   // another size is another pool, allocated at first use; 0 frees it
    g->arch_keys = HipBuf<unsigned long long>(), g->arch_skeys = HipBuf<unsigned long long>();
    g->arch_page = HipBuf<int32_t>(), g->arch_stack = HipBuf<int32_t>(), g->arch_claims = HipBuf<int32_t>(), g->arch_spages = HipBuf<int32_t>();
    g->arch_tiles = p->max_tiles;
    forget_archive(g);
    return SVH_OK;
}

int32_t svh_grid_get_archive(svh_grid* g, svh_grid_archive_params* p) {
    if (!g || !p) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_archive: null argument");
    p->max_tiles = g->arch_tiles;
    return SVH_OK;
}

int32_t svh_grid_get_archive_stats(svh_grid* g, int64_t out[6]) {
    if (!g || !out) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_archive_stats: null argument");
    for (int k = 0; k < grid::AS_WORDS; k++) out[k] = g->arch_stats[k];
    out[grid::AS_MAX_TILES] = g->arch_tiles;
    return SVH_OK;
}

int32_t svh_grid_archive_clear(svh_grid* g) {
    if (!g) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_archive_clear: null argument");
    forget_archive(g);
    return SVH_OK;
}

int32_t svh_grid_archive_trim(svh_grid* g, int32_t ga0, int32_t gb0, int32_t ga1, int32_t gb1) {
    if (!g || !grid::trim_ok(ga0, gb0, ga1, gb1))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_archive_trim: a grid and a box ga0 <= ga1, gb0 <= gb1 of global cells below 2^20 are needed");
    const grid::Archive ar = g->archive();
    if (ar.table == 0) return SVH_OK;   // no tile to drop
    const int rc = [&]() -> int {
        GRID_TRY(none, hipSetDevice(g->device));
        GRID_GROW_N(g->arch_skeys, ar.max_tiles);
        GRID_GROW_N(g->arch_spages, ar.max_tiles);
        hipStream_t s = g->stream;
        GRID_TRY(launch, (grid::launch_archive_trim_collect(s, ar, ga0, gb0, ga1, gb1, g->arch_skeys, g->arch_spages), hipGetLastError()));
        GRID_TRY(copy, hipMemsetAsync(ar.keys, 0xFF, (size_t)ar.table * sizeof(unsigned long long), s));
        GRID_TRY(copy, hipMemsetAsync(ar.page, 0xFF, (size_t)ar.table * sizeof(int32_t), s));
        GRID_TRY(launch, (grid::launch_archive_trim_insert(s, ar, g->arch_skeys, g->arch_spages), hipGetLastError()));
        GRID_TRY(copy, hipMemsetAsync(ar.ctl + grid::AR_CLAIMS, 0, sizeof(unsigned long long), s));
        GRID_TRY(copy, hipMemcpyAsync(g->h_arch_ctl, ar.ctl, grid::AR_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        read_archive_stats(g);
        return SVH_OK;
    }();
    if (failed(g, rc) == SVH_ERR_HIP) forget_archive(g);   // a table half rebuilt is no archive; the window is untouched
    return rc;
}

int32_t svh_grid_archive_tiles(svh_grid* g, int32_t* keys, int64_t cap, int64_t* n) {
    if (!g || !n || cap < 0 || (cap > 0 && !keys)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_archive_tiles: bad arguments");
    *n = 0;
    const grid::Archive ar = g->archive();
    if (ar.table == 0) return SVH_OK;
    const size_t bytes = (size_t)ar.table * sizeof(unsigned long long);
    const int rc = [&]() -> int {
        GRID_TRY(none, hipSetDevice(g->device));
        GRID_GROW(g->h_out, bytes);
        GRID_TRY(copy, hipMemcpyAsync(g->h_out, ar.keys, bytes, hipMemcpyDeviceToHost, g->stream));
        GRID_TRY(wait, hipStreamSynchronize(g->stream));
        return SVH_OK;
    }();
    if (rc) return failed(g, rc);
    const unsigned long long* k = (const unsigned long long*)g->h_out.p;
    std::vector<unsigned long long> live;
    for (uint32_t i = 0; i < ar.table; i++)
        if (k[i] != grid::TILE_NONE) live.push_back(k[i]);
    std::sort(live.begin(), live.end());   // tb is the high word: ascending by (tb, ta)
    *n = (int64_t)live.size();
    for (int64_t i = 0; i < std::min(*n, cap); i++) keys[2 * i] = grid::key_ta(live[(size_t)i]), keys[2 * i + 1] = grid::key_tb(live[(size_t)i]);
    return SVH_OK;
}

int32_t svh_grid_get_region(svh_grid* g, int32_t plane_kind, int32_t plane, int32_t ga0, int32_t gb0, int32_t w, int32_t h, void* out, int32_t on_device) {
    if (!g || !out || plane_kind < 0 || plane_kind >= grid::RK_KINDS || plane < 0 || plane >= (plane_kind == grid::RK_GRID ? (int32_t)grid::P_PLANES : (int32_t)grid::L_PLANES) ||
        !grid::region_ok(ga0, gb0, w, h))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_region: a grid, a plane of svh_grid_get (kind 0) or svh_grid_get_local (kind 1), a box of 1..8192 x 1..8192 global cells below 2^20 and an output are needed");
    const bool bytes = plane_kind == grid::RK_GRID ? plane >= grid::P_INTENSITY : plane == grid::L_STATE;
    if (on_device && !bytes && ((uintptr_t)out & 3)) return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_get_region: a device array of a 4-byte plane must be 4-byte aligned");
    const size_t size = (size_t)w * (size_t)h * (bytes ? 1 : 4);
    const int rc = [&]() -> int {
        const int r0 = ready(g);
        if (r0) return r0;
        grid::RegionJob j{g->prm, g->cells(), g->archive(), plane_kind, plane, ga0, gb0, w, h};
        if (!on_device) GRID_GROW(g->d_region, size);
        void* dst = on_device ? out : (void*)g->d_region.p;
        GRID_TRY(launch, (grid::launch_archive_region(g->stream, j, dst), hipGetLastError()));
        return finish(g, dst, size, out, on_device != 0);
    }();
    return failed(g, rc);
}

int32_t svh_grid_render_region(svh_grid* g, int32_t mode, int32_t ga0, int32_t gb0, int32_t w, int32_t h, uint8_t* rgb, int32_t on_device) {
    if (!g || !rgb || mode < 0 || mode > grid::M_LOCAL || !grid::region_ok(ga0, gb0, w, h))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_grid_render_region: a grid, a mode 0..3, a box of 1..8192 x 1..8192 global cells below 2^20 and an output are needed");
    const size_t size = (size_t)w * (size_t)h * 3;
    const int rc = [&]() -> int {
        const int r0 = ready(g);
        if (r0) return r0;
        grid::RegionJob j{g->prm, g->cells(), g->archive(), grid::RK_GRID, 0, ga0, gb0, w, h};
        if (!on_device) GRID_GROW(g->d_region, size);
        uint8_t* dst = on_device ? rgb : g->d_region.p;
        GRID_TRY(launch, (grid::launch_archive_render_region(g->stream, j, mode, dst), hipGetLastError()));
        return finish(g, dst, size, rgb, on_device != 0);
    }();
    return failed(g, rc);
}

// grid_archive_core.h on the host.  svh_test_grid_archive_key: per global cell the tile key, the tile (ta, tb) read back from it and the
// index inside the tile; *table = archive_table_size(max_tiles) when table is given
int32_t svh_test_grid_archive_key(int64_t n, const int32_t* ga, const int32_t* gb, uint64_t* key, int32_t* tile, uint32_t* index, int32_t max_tiles,
                                  uint32_t* table) {
    if (n < 0 || (n > 0 && (!ga || !gb || !key || !tile || !index)) || max_tiles < 0 || max_tiles > grid::ARCHIVE_MAX_TILES)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_archive_key: bad arguments");
    for (int64_t i = 0; i < n; i++) {
        if (!grid::region_ok(ga[i], gb[i], 1, 1)) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_archive_key: a global cell lies below 2^20");
        key[i] = grid::cell_key(ga[i], gb[i]);
        tile[2 * i] = grid::key_ta(key[i]), tile[2 * i + 1] = grid::key_tb(key[i]);
        index[i] = grid::tile_index(ga[i], gb[i]);
    }
    if (table) *table = grid::archive_table_size(max_tiles);
    return SVH_OK;
}

// strip_count and strip_cell: *count cells, the first min(*count, cap) as pairs (ia, ib) in lane order.  A scroll by (da, db) leaves the
// strip of (da, db) in the old window's cells and enters the strip of (-da, -db) in the new window's
int32_t svh_test_grid_archive_strip(int32_t nx, int32_t nz, int32_t da, int32_t db, int32_t* cells, int64_t cap, int64_t* count) {
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || (da == 0 && db == 0) || !count || cap < 0 || (cap > 0 && !cells))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_archive_strip: bad arguments");
    *count = (int64_t)grid::strip_count(nx, nz, da, db);
    for (int64_t t = 0; t < std::min(*count, cap); t++) grid::strip_cell(nx, nz, da, db, (uint32_t)t, &cells[2 * t], &cells[2 * t + 1]);
    return SVH_OK;
}

// grid_dyn_core.h on the host.  svh_test_grid_dyn_params: the checks of svh_grid_set_dynamics and *margin_q; SVH_ERR_BAD_ARG when
// they fail
int32_t svh_test_grid_dyn_params(const svh_grid_dyn_params* d, int32_t* margin_q) {
    if (!d) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_params: null argument");
    grid::DynParams q{d->clear_frames, d->min_through, d->margin, d->max_age, 0};
    if (!grid::dyn_derive(q)) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_params: parameters out of range");
    if (margin_q) *margin_q = q.margin_q;
    return SVH_OK;
}

// per item i: rdiv[i] = rdiv64(p[i], n[i]) (n > 0, |p| < 2^60), and for line steps height[i] = line_height(q_o[i], q_e[i], len[i], k[i])
// (0 <= k < len <= 8192, |q| <= 2^30).  Either group may be all NULL
int32_t svh_test_grid_dyn_height(int64_t count, const int64_t* p, const int64_t* n, int64_t* rdiv, const int32_t* q_o, const int32_t* q_e,
                                 const int32_t* len, const int32_t* k, int32_t* height) {
    if (count < 0 || (rdiv && (!p || !n)) || (height && (!q_o || !q_e || !len || !k)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_height: bad arguments");
    for (int64_t i = 0; i < count; i++) {
        if (rdiv) {
            if (n[i] <= 0 || p[i] <= -((int64_t)1 << 60) || p[i] >= ((int64_t)1 << 60) || n[i] >= ((int64_t)1 << 60))
                return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_height: n > 0 and |p|, n < 2^60 are needed");
            rdiv[i] = grid::rdiv64(p[i], n[i]);
        }
        if (height) {
            const int32_t lim = 1 << 30;
            if (len[i] < 1 || len[i] > grid::MAX_SIDE || k[i] < 0 || k[i] >= len[i] || q_o[i] < -lim || q_o[i] > lim || q_e[i] < -lim || q_e[i] > lim)
                return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_height: 0 <= k < len <= 8192 and |q| <= 2^30 are needed");
            height[i] = grid::line_height(q_o[i], q_e[i], len[i], k[i]);
        }
    }
    return SVH_OK;
}

// per stored cell i: its body (lo[i], hi[i]) and through[i] = goes_through(body, q[i]); q and through may be NULL
int32_t svh_test_grid_dyn_through(const svh_grid_params* p, const svh_grid_dyn_params* d, int64_t ncells, const int32_t* count,
                                  const uint32_t* kmin, const uint32_t* kmax, const int32_t* q, int32_t* lo, int32_t* hi, uint8_t* through) {
    grid::Params prm;
    if (!convert(p, &prm) || !d || ncells < 0 || (ncells > 0 && (!count || !kmin || !kmax || !lo || !hi)) || (through && !q))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_through: bad arguments");
    grid::DynParams dq{d->clear_frames, d->min_through, d->margin, d->max_age, 0};
    if (!grid::dyn_derive(dq)) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_through: parameters out of range");
    for (int64_t i = 0; i < ncells; i++) {
        const grid::Body b = grid::body_of(prm, dq, count[i], kmin[i], kmax[i]);
        lo[i] = b.lo, hi[i] = b.hi;
        if (through) through[i] = grid::goes_through(b, q[i]) ? 1 : 0;
    }
    return SVH_OK;
}

// settle() per cell i, in place: cell[6] = count, overhead, kmin, kmax, hsum, vsum of the stored cells, contra and last their state,
// frame[6] the frame records in the same order, through the plane of phase 2; event[i] = the DynEvent flags
int32_t svh_test_grid_dyn_settle(const svh_grid_params* p, const svh_grid_dyn_params* d, int32_t stamp, int64_t ncells, void* const cell[6],
                                 int32_t* contra, int32_t* last, const void* const frame[6], const int32_t* through, uint8_t* event) {
    grid::Params prm;
    if (!convert(p, &prm) || !d || stamp < 1 || ncells < 0 || !cell || !frame || (ncells > 0 && (!contra || !last || !through || !event)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_settle: bad arguments");
    for (int k = 0; k < 6; k++)
        if (ncells > 0 && (!cell[k] || !frame[k])) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_settle: a null plane");
    grid::DynParams dq{d->clear_frames, d->min_through, d->margin, d->max_age, 0};
    if (!grid::dyn_derive(dq)) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_settle: parameters out of range");
    for (int64_t i = 0; i < ncells; i++) {
        if (last[i] < 0 || last[i] > stamp || contra[i] < 0) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_settle: 0 <= last <= stamp and contra >= 0 are needed");
        grid::Cell c{((int32_t*)cell[0])[i], ((int32_t*)cell[1])[i], ((uint32_t*)cell[2])[i], ((uint32_t*)cell[3])[i], ((int64_t*)cell[4])[i],
                     ((uint64_t*)cell[5])[i]};
        const grid::Cell f{((const int32_t*)frame[0])[i], ((const int32_t*)frame[1])[i], ((const uint32_t*)frame[2])[i],
                           ((const uint32_t*)frame[3])[i], ((const int64_t*)frame[4])[i], ((const uint64_t*)frame[5])[i]};
        event[i] = grid::settle(prm, dq, stamp, c, contra[i], last[i], f, through[i]);
        ((int32_t*)cell[0])[i] = c.count, ((int32_t*)cell[1])[i] = c.overhead, ((uint32_t*)cell[2])[i] = c.kmin, ((uint32_t*)cell[3])[i] = c.kmax;
        ((int64_t*)cell[4])[i] = c.hsum, ((uint64_t*)cell[5])[i] = c.vsum;
    }
    return SVH_OK;
}

// colour_dyn and age_of per cell: rgb[3 i] from the class byte, the intensity, PASS, CONTRA and the event byte (COUNT taken as 1);
// age[i] from stamp and last[i].  Either group may be all NULL
int32_t svh_test_grid_dyn_colour(const svh_grid_params* p, int64_t ncells, const uint8_t* cls, const uint8_t* intensity, const int32_t* pass,
                                 const int32_t* contra, const uint8_t* event, uint8_t* rgb, int32_t stamp, const int32_t* last, int32_t* age) {
    grid::Params prm;
    if (!convert(p, &prm) || ncells < 0 || (rgb && (!cls || !intensity || !pass || !contra || !event)) || (age && !last))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_dyn_colour: bad arguments");
    for (int64_t i = 0; i < ncells; i++) {
        if (rgb) {
            const grid::Final f{0.f, 0.f, 0.f, intensity[i], cls[i]};
            grid::colour_dyn(prm, 1, f, pass[i], contra[i], event[i], rgb + 3 * i);
        }
        if (age) age[i] = grid::age_of(stamp, last[i]);
    }
    return SVH_OK;
}

// grid_explore_core.h on the host, on a caller's STATE and COST planes (nx x nz, offsets oa, ob), with R from e->range and `cell`.
// Three things, each optional: GAIN of n_cells global cells to gains; for the global cell view[2], inside the window, its VIEW
// plane to mask (nx * nz) and drawn over rgb (nx * nz * 3, the layout of svh_grid_render_cost, changed in place); from the global
// cell start[2] the ranking: *n records, the first min(*n, cap) to recs (5 each) and scores, *best, stats[0] the records and
// stats[1] the feasible ones.  Needs no device
int32_t svh_test_grid_explore(const svh_grid_front_params* f, const svh_grid_plan_params* pl, const svh_grid_explore_params* e, float cell, int32_t nx,
                              int32_t nz, int32_t oa, int32_t ob, const uint8_t* state, const uint8_t* cost, const int32_t* cells, int64_t n_cells,
                              int32_t* gains, const int32_t* view, uint8_t* mask, uint8_t* rgb, const int32_t* start, int32_t* recs,
                              int64_t* scores, int64_t cap, int64_t* n, int32_t* best, int64_t* stats) {
    grid::FrontParams fq;
    grid::PlanParams pq{50, -1, 0x7FFFFFFE};
    grid::ExploreParams eq;
    int32_t R = 0;
    if (!explore_test_args(f, pl, e, cell, nx, nz, oa, ob, state, cost, cells, n_cells, gains, view, start, recs, scores, cap, n, best, &fq, &pq, &eq, &R))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_explore: bad arguments");
    if (n_cells > 0) grid::gain_window(fq, R, nx, nz, oa, ob, state, cells, n_cells, gains);
    if (view && (mask || rgb)) {
        std::vector<uint8_t> v((size_t)nx * (size_t)nz);
        grid::view_window(fq, R, nx, nz, state, view[0] - oa, view[1] - ob, v.data());
        if (mask) memcpy(mask, v.data(), v.size());
        if (rgb) view_overlay_host(nx, nz, v.data(), view[0] - oa, view[1] - ob, rgb);
    }
    if (start) {
        std::vector<int32_t> r;
        std::vector<int64_t> sc;
        int64_t feasible = 0;
        *best = grid::explore_window(fq, pq, eq, R, nx, nz, oa, ob, state, cost, start[0], start[1], &r, &sc, &feasible);
        const size_t give = std::min(sc.size(), (size_t)cap);
        if (recs && give) memcpy(recs, r.data(), give * grid::EXPLORE_REC * sizeof(int32_t));
        if (scores && give) memcpy(scores, sc.data(), give * sizeof(int64_t));
        *n = (int64_t)sc.size();
        if (stats) stats[0] = (int64_t)sc.size(), stats[1] = feasible;
    }
    return SVH_OK;
}

// the same through the kernels: the planes go to the device, the frontiers by front_run, the reach field by plan_run
int32_t svh_test_grid_explore_device(const svh_grid_front_params* f, const svh_grid_plan_params* pl, const svh_grid_explore_params* e, float cell,
                                     int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state, const uint8_t* cost, const int32_t* cells,
                                     int64_t n_cells, int32_t* gains, const int32_t* view, uint8_t* mask, uint8_t* rgb, const int32_t* start,
                                     int32_t* recs, int64_t* scores, int64_t cap, int64_t* n, int32_t* best, int64_t* stats) {
    grid::FrontParams fq;
    grid::PlanParams pq{50, -1, 0x7FFFFFFE};
    grid::ExploreParams eq;
    int32_t R = 0;
    if (!explore_test_args(f, pl, e, cell, nx, nz, oa, ob, state, cost, cells, n_cells, gains, view, start, recs, scores, cap, n, best, &fq, &pq, &eq, &R))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_explore_device: bad arguments");
    svh::ensure_init();
    const size_t ncells = (size_t)nx * (size_t)nz;
    HipBuf<uint8_t> in, d_view, d_rgb, planes, field;
    HipBuf<int32_t> d_cells, d_gain, d_start;
    HipBuf<uint32_t> d_tiles, d_ctl;
    PinnedBuf<uint32_t> h_ctl;
    FrontBufs fbufs;
    ExploreBufs ebufs;
    int32_t out[2] = {-1, 0}, m = 0;
    hipStream_t s = nullptr;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(in, 2 * ncells);
        GRID_TRY(copy, hipMemcpyAsync(in, state, ncells, hipMemcpyHostToDevice, s));
        if (cost) GRID_TRY(copy, hipMemcpyAsync(in + ncells, cost, ncells, hipMemcpyHostToDevice, s));
        grid::ExploreJob j = explore_job(eq, fq, R, nx, nz, oa, ob, in.p);
        if (n_cells > 0) {
            GRID_GROW_N(d_cells, 2 * n_cells);
            GRID_GROW_N(d_gain, n_cells);
            GRID_TRY(copy, hipMemcpyAsync(d_cells, cells, (size_t)n_cells * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
            GRID_TRY(launch, (grid::launch_view_gain(s, j, d_cells, 2, n_cells, d_gain), hipGetLastError()));
            GRID_TRY(copy, hipMemcpyAsync(gains, d_gain, (size_t)n_cells * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        if (view && (mask || rgb)) {
            const int32_t va = view[0] - oa, vb = view[1] - ob;
            GRID_GROW(d_view, ncells);
            GRID_TRY(copy, hipMemsetAsync(d_view, 0, ncells, s));
            GRID_TRY(launch, (grid::launch_view_mask(s, j, va, vb, d_view), hipGetLastError()));
            if (mask) GRID_TRY(copy, hipMemcpyAsync(mask, d_view, ncells, hipMemcpyDeviceToHost, s));
            if (rgb) {
                GRID_GROW(d_rgb, 3 * ncells);
                GRID_TRY(copy, hipMemcpyAsync(d_rgb, rgb, 3 * ncells, hipMemcpyHostToDevice, s));
                GRID_TRY(launch, (grid::launch_view_overlay(s, nx, nz, d_view, va, vb, d_rgb), hipGetLastError()));
                GRID_TRY(copy, hipMemcpyAsync(rgb, d_rgb, 3 * ncells, hipMemcpyDeviceToHost, s));
            }
        }
        if (start) {
            grid::FrontJob fj;
            fj.frp = fq;
            fj.nx = nx, fj.nz = nz, fj.oa = oa, fj.ob = ob;
            fj.state = in.p, fj.cost = in.p + ncells;
            GRID_GROW(planes, ncells * kFrontBytes);
            fj.label = (int32_t*)planes.p, fj.flags = planes.p + 4 * ncells;
            int64_t st[grid::FS_WORDS] = {0, 0, 0, 0, 0};
            int r = front_run(s, fj, fbufs, st);
            if (r) return r;
            m = (int32_t)std::min<int64_t>(st[grid::FS_KEPT], grid::EXPLORE_MAX_RECORDS);
            grid::PlanJob pj;
            pj.pln = pq;
            pj.nx = nx, pj.nz = nz, pj.oa = oa, pj.ob = ob, pj.n_goals = 1;
            const size_t tiles = (size_t)grid::plan_tiles_x(pj) * grid::plan_tiles_y(pj);
            GRID_GROW(field, ncells * kPlanBytes);
            GRID_GROW_N(d_start, 2);
            GRID_GROW(d_tiles, 4 * tiles * sizeof(uint32_t));
            GRID_GROW(d_ctl, grid::CTL_WORDS * sizeof(uint32_t));
            GRID_GROW(h_ctl, grid::CTL_WORDS * sizeof(uint32_t));
            GRID_TRY(copy, hipMemcpyAsync(d_start, start, 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
            pj.cost = in.p + ncells;
            pj.pot = (int32_t*)field.p, pj.price = (uint16_t*)(field.p + 4 * ncells), pj.dir = field.p + 6 * ncells;
            pj.goals = d_start.p;
            pj.lists = d_tiles.p, pj.flags = d_tiles.p + 2 * tiles;
            pj.ctl = d_ctl.p;
            if ((r = plan_run(s, pj, h_ctl))) return r;
            if ((r = explore_outputs(ebufs, m, j))) return r;
            j.front_recs = fj.recs, j.pot = pj.pot;
            GRID_TRY(launch, (grid::launch_explore_rank(s, j), hipGetLastError()));
            const size_t give = (size_t)std::min<int64_t>(m, cap);
            if (recs && give) GRID_TRY(copy, hipMemcpyAsync(recs, j.recs, give * grid::EXPLORE_REC * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (scores && give) GRID_TRY(copy, hipMemcpyAsync(scores, j.scores, give * sizeof(int64_t), hipMemcpyDeviceToHost, s));
            GRID_TRY(copy, hipMemcpyAsync(out, j.out, sizeof(out), hipMemcpyDeviceToHost, s));
        }
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    if (start) {
        *n = m, *best = out[0];
        if (stats) stats[0] = m, stats[1] = out[1];
    }
    return SVH_OK;
}

// grid_align_core.h on the host, on a caller's STATE plane (p->nx x p->nz, offsets oa, ob) with the frame, cell, step and clearance of
// `p`.  The frame is n_pts points (x, y, z, val) about the map-frame position `pivot`, or -- with pivot_sub, the pivot's global sub --
// n_subs global subs (ua, ub), all of magnitude below 2^22.  field: F (nx * nz, may be null); counts[0] n_scan, counts[1] n_points
// (may be null); the first min(n_scan, cap) pairs of the scan to `scan`; volume: (2 K + 1) (2 W + 1)^2 scores, not written with
// too few subs (may be null); rec: the record.  Needs no device
int32_t svh_test_grid_align(const svh_grid_params* p, const svh_grid_align_params* a, int32_t oa, int32_t ob, const uint8_t* state, const float* xyzv,
                            int64_t n_pts, const int32_t* subs, int64_t n_subs, const double pivot[3], const int32_t pivot_sub[2], uint8_t* field,
                            int32_t* scan, int64_t cap, int64_t* counts, int32_t* volume, int32_t* rec) {
    grid::Params q;
    grid::AlignParams aq;
    int32_t Pa = 0, Pb = 0;
    if (!align_test_args(p, a, oa, ob, state, xyzv, n_pts, subs, n_subs, pivot, pivot_sub, scan, cap, rec, &q, &aq, &Pa, &Pb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_align: bad arguments");
    std::vector<uint8_t> F((size_t)q.nx * (size_t)q.nz);
    grid::align_field_window(aq.reach_cells, q.nx, q.nz, state, F.data());
    std::vector<int32_t> list;
    const int64_t kept = pivot_sub ? grid::align_scan_subs(aq.Rg, Pa, Pb, subs, n_subs, &list) : grid::align_scan_points(q, aq.Rg, Pa, Pb, xyzv, n_pts, &list);
    const int64_t n_scan = (int64_t)(list.size() / 2);
    grid::align_window(aq, q.nx, q.nz, oa, ob, F.data(), Pa, Pb, list.data(), n_scan, volume, rec);
    if (field) memcpy(field, F.data(), F.size());
    if (counts) counts[0] = n_scan, counts[1] = kept;
    const size_t give = (size_t)std::min(n_scan, cap);
    if (give) memcpy(scan, list.data(), give * 2 * sizeof(int32_t));
    return SVH_OK;
}

// the same through the kernels of csrc/grid_align_kernels.hip: the plane and the frame go to the device
int32_t svh_test_grid_align_device(const svh_grid_params* p, const svh_grid_align_params* a, int32_t oa, int32_t ob, const uint8_t* state,
                                   const float* xyzv, int64_t n_pts, const int32_t* subs, int64_t n_subs, const double pivot[3],
                                   const int32_t pivot_sub[2], uint8_t* field, int32_t* scan, int64_t cap, int64_t* counts, int32_t* volume,
                                   int32_t* rec) {
    grid::Params q;
    grid::AlignParams aq;
    int32_t Pa = 0, Pb = 0;
    if (!align_test_args(p, a, oa, ob, state, xyzv, n_pts, subs, n_subs, pivot, pivot_sub, scan, cap, rec, &q, &aq, &Pa, &Pb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_align_device: bad arguments");
    svh::ensure_init();
    const size_t ncells = (size_t)q.nx * (size_t)q.nz;
    const int64_t n = pivot_sub ? n_subs : n_pts;
    HipBuf<uint8_t> d_state, d_in;
    AlignBufs bufs;
    uint32_t ctl[grid::AC_WORDS] = {0, 0};
    int32_t r[grid::ALIGN_REC];
    hipStream_t s = nullptr;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(d_state, ncells);
        GRID_TRY(copy, hipMemcpyAsync(d_state, state, ncells, hipMemcpyHostToDevice, s));
        grid::AlignJob j;
        int e = align_job(bufs, q, aq, d_state.p, Pa, Pb, n, &j);
        if (e) return e;
        const size_t in_bytes = (size_t)n * (pivot_sub ? 2 * sizeof(int32_t) : sizeof(float4));
        GRID_GROW(d_in, in_bytes ? in_bytes : 16);
        if (n > 0) GRID_TRY(copy, hipMemcpyAsync(d_in, pivot_sub ? (const void*)subs : (const void*)xyzv, in_bytes, hipMemcpyHostToDevice, s));
        GRID_TRY(launch, (grid::launch_align_field(s, j, (g_align_form & grid::ALIGN_FORM_MASK) != 0), hipGetLastError()));
        if ((e = align_begin(s, j))) return e;
        GRID_TRY(launch, (grid::launch_align_mark(s, j, pivot_sub ? nullptr : (const float4*)d_in.p, pivot_sub ? (const int32_t*)d_in.p : nullptr, n), hipGetLastError()));
        if ((e = align_finish(s, j))) return e;
        GRID_TRY(copy, hipMemcpyAsync(r, j.rec, sizeof(r), hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(ctl, j.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
        if (field) GRID_TRY(copy, hipMemcpyAsync(field, j.field, ncells, hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        const size_t give = (size_t)std::min<int64_t>(r[grid::AR_SCAN], cap);
        if (give) GRID_TRY(copy, hipMemcpyAsync(scan, j.scan, give * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (volume && r[grid::AR_STATUS] != grid::ALIGN_FEW)
            GRID_TRY(copy, hipMemcpyAsync(volume, j.volume, (size_t)grid::align_volume_size(aq.rot_n, aq.trans_n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    memcpy(rec, r, sizeof(r));
    if (counts) counts[0] = ctl[grid::AC_SCAN], counts[1] = ctl[grid::AC_POINTS];
    return SVH_OK;
}

// a measurement's and a test's switch: the form of the score kernel becomes `form` (0 chunk, 1 plain, 2 tiled; anything else only
// reads), plus 4 for the field in three launches, the mask first, instead of two; returns what it was
int32_t svh_test_grid_align_form(int32_t form) {
    const int32_t was = g_align_form;
    if (form >= 0 && form < 8 && (form & 3) < grid::ALIGN_FORMS) g_align_form = form;
    return was;
}

// grid_roll_core.h on the host.  The footprint table for a cell side: *R, *total cells of all lists, and (k >= 0) the list of heading
// k: *n its cells, the first min(*n, cap) pairs (da, db).  Needs no device
int32_t svh_test_grid_roll_table(float cell, const svh_grid_roll_params* p, int32_t* R, int64_t* total, int32_t k, int32_t* offsets, int64_t cap,
                                 int64_t* n) {
    RollTable t;
    if (!convert_roll(p, &t.p) || !(grid::finite_f(cell) && cell > 0.f) || !R || cap < 0 || (cap > 0 && !offsets) || k < -1 || k >= 8 * t.p.m ||
        (k >= 0 && !n) || !t.derive(cell))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_roll_table: bad arguments");
    *R = t.R;
    if (total) *total = (int64_t)(t.offs.size() / 2);
    if (k >= 0) {
        const int64_t at = t.start[k], len = t.start[k + 1] - at;
        if (cap > 0) memcpy(offsets, t.offs.data() + 2 * at, (size_t)std::min(len, cap) * 2 * sizeof(int32_t));
        *n = len;
    }
    return SVH_OK;
}

// the heading of a direction (*k, -1: none) and, where vec is given and there is one, its vector.  Needs no device
int32_t svh_test_grid_roll_heading(int32_t m, float ua, float ub, int32_t* k, int32_t* vec) {
    if (m < 1 || m > grid::ROLL_MAX_M || !k) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_roll_heading: bad arguments");
    *k = grid::heading_of(m, ua, ub);
    if (vec && *k >= 0) grid::heading_vec(m, *k, &vec[0], &vec[1]);
    return SVH_OK;
}

// The header's host loops on a caller's COST and POT planes (nx x nz, offsets oa, ob; POT is read only when w_pot != 0), with the
// footprint table of roll_table_for -- built by the first call for a vehicle and cell side, kept for those that follow: F of n_poses
// free poses (global cells) to fout, and -- with a table of S x K x T -- set `set` scored at the global cell (ga0, gb0): recs (5 K) and
// scores (K) may be NULL, *best.  table NULL with S = 0: the poses alone.  Needs no device
int32_t svh_test_grid_roll(const svh_grid_roll_params* p, float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost,
                           const int32_t* pot, const int32_t* table, int32_t S, int32_t K, int32_t T, int32_t set, int32_t ga0, int32_t gb0,
                           const int32_t* poses, int64_t n_poses, int32_t* fout, int32_t* recs, int64_t* scores, int32_t* best) {
    grid::RollParams q;
    std::shared_ptr<const RollTable> t;
    if (!roll_test_args(p, cell, nx, nz, oa, ob, cost, pot, table, S, K, T, set, ga0, gb0, poses, n_poses, fout, best, &q, &t))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_roll: bad arguments");
    if (n_poses > 0) grid::footprint_window(q, nx, nz, oa, ob, cost, t->offs.data(), t->start.data(), poses, n_poses, fout);
    if (S > 0)
        *best = grid::roll_window(q, nx, nz, oa, ob, cost, pot, t->offs.data(), t->start.data(), table + (size_t)set * (size_t)K * (size_t)T * 3, K, T,
                                  ga0, gb0, recs, scores);
    return SVH_OK;
}

// the same through the kernels
int32_t svh_test_grid_roll_device(const svh_grid_roll_params* p, float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost,
                                  const int32_t* pot, const int32_t* table, int32_t S, int32_t K, int32_t T, int32_t set, int32_t ga0,
                                  int32_t gb0, const int32_t* poses, int64_t n_poses, int32_t* fout, int32_t* recs, int64_t* scores,
                                  int32_t* best) {
    grid::RollParams q;
    std::shared_ptr<const RollTable> t;
    if (!roll_test_args(p, cell, nx, nz, oa, ob, cost, pot, table, S, K, T, set, ga0, gb0, poses, n_poses, fout, best, &q, &t))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_roll_device: bad arguments");
    svh::ensure_init();
    return roll_device(q, *t, nx, nz, oa, ob, cost, pot, table, S, K, T, set, ga0, gb0, poses, n_poses, fout, recs, scores, best);
}

// the lanes that share a pose in the kernels, for a longest footprint list
int32_t svh_test_grid_roll_group(int64_t longest) { return grid::roll_group(longest); }

// grid_front_core.h on the host.  Needs no device
int32_t svh_test_grid_front(const svh_grid_front_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state,
                            const uint8_t* cost, uint8_t* flags, int32_t* label, int32_t* recs, int64_t cap, int64_t* n, int64_t* stats) {
    grid::FrontParams q;
    if (!convert_front(p, &q) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || !state || !cost ||
        cap < 0 || (cap > 0 && !recs))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_front: bad arguments");
    const size_t cells = (size_t)nx * (size_t)nz;
    std::vector<uint8_t> f(cells);
    std::vector<int32_t> l(cells), r;
    int64_t st[grid::FS_WORDS];
    grid::front_window(q, nx, nz, oa, ob, state, cost, f.data(), l.data(), &r, st);
    if (flags) memcpy(flags, f.data(), cells);
    if (label) memcpy(label, l.data(), cells * sizeof(int32_t));
    if (cap > 0) memcpy(recs, r.data(), std::min(r.size(), (size_t)cap * grid::FRONT_REC) * sizeof(int32_t));
    if (n) *n = st[grid::FS_KEPT];
    if (stats) memcpy(stats, st, sizeof(st));
    return SVH_OK;
}

int32_t svh_test_grid_front_tile(void) { return grid::FRONT_TILE; }

// the kernels of the frontiers on a caller's STATE and COST planes (host, nx x nz)
int32_t svh_test_grid_front_device(const svh_grid_front_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state,
                                   const uint8_t* cost, uint8_t* flags, int32_t* label, int32_t* recs, int64_t cap, int64_t* n,
                                   int64_t* stats) {
    grid::FrontJob j;
    if (!convert_front(p, &j.frp) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || !state || !cost ||
        cap < 0 || (cap > 0 && !recs))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_front_device: bad arguments");
    svh::ensure_init();
    j.nx = nx, j.nz = nz, j.oa = oa, j.ob = ob;
    const size_t cells = (size_t)nx * (size_t)nz;
    HipBuf<uint8_t> in, planes;
    FrontBufs bufs;
    int64_t st[grid::FS_WORDS] = {0, 0, 0, 0, 0};
    hipStream_t s = nullptr;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(in, 2 * cells);
        GRID_GROW(planes, cells * kFrontBytes);
        GRID_TRY(copy, hipMemcpyAsync(in, state, cells, hipMemcpyHostToDevice, s));
        GRID_TRY(copy, hipMemcpyAsync(in + cells, cost, cells, hipMemcpyHostToDevice, s));
        j.state = in.p, j.cost = in.p + cells;
        j.label = (int32_t*)planes.p, j.flags = planes.p + 4 * cells;
        const int r = front_run(s, j, bufs, st);
        if (r) return r;
        const size_t m = (size_t)std::min<int64_t>(st[grid::FS_KEPT], cap);
        if (flags) GRID_TRY(copy, hipMemcpyAsync(flags, j.flags, cells, hipMemcpyDeviceToHost, s));
        if (label) GRID_TRY(copy, hipMemcpyAsync(label, j.label, cells * 4, hipMemcpyDeviceToHost, s));
        if (m > 0) GRID_TRY(copy, hipMemcpyAsync(recs, j.recs, m * grid::FRONT_REC * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    if (n) *n = st[grid::FS_KEPT];
    if (stats) memcpy(stats, st, sizeof(st));
    return SVH_OK;
}

// the labelling stage alone on a mask (host, nx x nz, nonzero: a cell to label)
int32_t svh_test_grid_front_label_device(int32_t nx, int32_t nz, const uint8_t* mask, int32_t* label, int64_t* launches) {
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !mask || !label)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_front_label_device: bad arguments");
    svh::ensure_init();
    grid::FrontJob j{};
    j.nx = nx, j.nz = nz;
    const size_t cells = (size_t)nx * (size_t)nz;
    for (size_t i = 0; i < cells; i++) label[i] = mask[i] ? (int32_t)i : -1;
    HipBuf<int32_t> d_label;
    HipBuf<unsigned long long> d_ctl;
    PinnedBuf<unsigned long long> h_ctl;
    const size_t ctl_bytes = grid::FC_WORDS * sizeof(unsigned long long);
    int64_t launched = 0;
    hipStream_t s = nullptr;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(d_label, cells * sizeof(int32_t));
        GRID_GROW(d_ctl, ctl_bytes);
        GRID_GROW(h_ctl, ctl_bytes);
        GRID_TRY(copy, hipMemsetAsync(d_ctl, 0, ctl_bytes, s));
        GRID_TRY(copy, hipMemcpyAsync(d_label, label, cells * sizeof(int32_t), hipMemcpyHostToDevice, s));
        j.label = d_label, j.ctl = d_ctl;
        launched = grid::launch_front_label(s, j);
        GRID_TRY(launch, hipGetLastError());
        GRID_TRY(copy, hipMemcpyAsync(label, d_label, cells * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(h_ctl, d_ctl, ctl_bytes, hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        if (h_ctl.p[grid::FC_UNSETTLED]) return svh::fail(SVH_ERR_HIP, kUnsettled);
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    if (launches) *launches = launched;
    return SVH_OK;
}

// grid_obj_core.h's objects on the host.  Needs no device
int32_t svh_test_grid_obj(const svh_grid_obj_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state, const float* hmax,
                          const int32_t* count, uint8_t* flags, int32_t* label, int32_t* recs, int64_t cap, int64_t* n, int64_t* stats) {
    grid::ObjParams q;
    if (!convert_obj(p, &q) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || !state || !hmax ||
        !count || cap < 0 || (cap > 0 && !recs))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_obj: bad arguments");
    const size_t cells = (size_t)nx * (size_t)nz;
    std::vector<uint8_t> f(cells);
    std::vector<int32_t> l(cells), r;
    int64_t st[grid::OS_WORDS];
    grid::obj_window(q, nx, nz, oa, ob, state, hmax, count, f.data(), l.data(), &r, st);
    if (flags) memcpy(flags, f.data(), cells);
    if (label) memcpy(label, l.data(), cells * sizeof(int32_t));
    if (cap > 0) memcpy(recs, r.data(), std::min(r.size(), (size_t)cap * grid::OBJ_REC) * sizeof(int32_t));
    if (n) *n = st[grid::OS_KEPT];
    if (stats) memcpy(stats, st, sizeof(st));
    return SVH_OK;
}

// the kernels of the objects on a caller's STATE, HMAX and COUNT planes (host, nx x nz)
int32_t svh_test_grid_obj_device(const svh_grid_obj_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state,
                                 const float* hmax, const int32_t* count, uint8_t* flags, int32_t* label, int32_t* recs, int64_t cap, int64_t* n,
                                 int64_t* stats) {
    grid::ObjJob j;
    if (!convert_obj(p, &j.op) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || !state || !hmax ||
        !count || cap < 0 || (cap > 0 && !recs))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_obj_device: bad arguments");
    svh::ensure_init();
    j.nx = nx, j.nz = nz, j.oa = oa, j.ob = ob;
    const size_t cells = (size_t)nx * (size_t)nz;
    HipBuf<uint8_t> in, planes;
    ObjBufs bufs;
    int64_t st[grid::OS_WORDS] = {0, 0, 0, 0, 0, 0, 0};
    hipStream_t s = nullptr;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(in, 9 * cells);
        GRID_GROW(planes, cells * kFrontBytes);
        GRID_TRY(copy, hipMemcpyAsync(in, hmax, 4 * cells, hipMemcpyHostToDevice, s));
        GRID_TRY(copy, hipMemcpyAsync(in + 4 * cells, count, 4 * cells, hipMemcpyHostToDevice, s));
        GRID_TRY(copy, hipMemcpyAsync(in + 8 * cells, state, cells, hipMemcpyHostToDevice, s));
        j.hmax = (const float*)in.p, j.count = (const int32_t*)(in.p + 4 * cells), j.state = in.p + 8 * cells;
        j.label = (int32_t*)planes.p, j.flags = planes.p + 4 * cells;
        const int r = obj_run(s, j, bufs, st);
        if (r) return r;
        const size_t m = (size_t)std::min<int64_t>(st[grid::OS_KEPT], cap);
        if (flags) GRID_TRY(copy, hipMemcpyAsync(flags, j.flags, cells, hipMemcpyDeviceToHost, s));
        if (label) GRID_TRY(copy, hipMemcpyAsync(label, j.label, cells * 4, hipMemcpyDeviceToHost, s));
        if (m > 0) GRID_TRY(copy, hipMemcpyAsync(recs, j.recs, m * grid::OBJ_REC * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    if (n) *n = st[grid::OS_KEPT];
    if (stats) memcpy(stats, st, sizeof(st));
    return SVH_OK;
}

// grid_obj_core.h's step on the host: the inputs of obj_step; tracks has room for p->max_tracks records.  *n_tracks = the records of
// the new table, stats[TS_WORDS] (TS_STEPS is not touched), *next_out = the next id afterwards.  Needs no device
int32_t svh_test_grid_obj_step(const svh_grid_obj_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const int32_t* recs, int32_t n_obj,
                               const int32_t* label, int32_t poa, int32_t pob, const int32_t* prev_id, const int32_t* prev, int32_t n_prev,
                               int32_t next_id, int32_t* tracks, int32_t* n_tracks, int32_t* assign, int32_t* id, int64_t* stats,
                               int32_t* next_out) {
    grid::ObjParams q;
    if (!convert_obj(p, &q) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) ||
        !grid::offsets_ok(poa, pob) || n_obj < 0 || (n_obj > 0 && (!recs || !assign)) || !label || n_prev < 0 || n_prev > q.max_tracks ||
        (n_prev > 0 && (!prev || !prev_id)) || next_id < 0 || !tracks || !n_tracks || !id)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_obj_step: bad arguments");
    std::vector<int32_t> t;
    int64_t st[grid::TS_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t next = grid::obj_step(q, nx, nz, oa, ob, recs, n_obj, label, poa, pob, prev_id, prev, n_prev, next_id, &t, assign, id, st);
    memcpy(tracks, t.data(), t.size() * sizeof(int32_t));
    *n_tracks = (int32_t)(t.size() / grid::TRACK_REC);
    if (stats)
        for (int k = grid::TS_TRACKS; k < grid::TS_WORDS; k++) stats[k] = st[k];
    if (next_out) *next_out = next;
    return SVH_OK;
}

// grid_obj_core.h's colours on the host: rgb[3] per cell from FLAGS, the track id of the cell (-1: none) and whether that track moves;
// cells that keep their colour are not written
int32_t svh_test_grid_obj_colour(int64_t ncells, const uint8_t* flags, const int32_t* id, const uint8_t* moving, uint8_t* rgb) {
    if (ncells < 0 || (ncells > 0 && (!flags || !id || !moving || !rgb))) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_obj_colour: bad arguments");
    for (int64_t i = 0; i < ncells; i++) (void)grid::colour_obj(flags[i], id[i], moving[i] != 0, rgb + 3 * i);
    return SVH_OK;
}

// grid_pred_core.h's PRED on the host: the ID plane [nz * nx] (NULL: all -1) and n_tracks track records in ascending order of id ->
// pred [nz * nx], stats[4] (the launches are 0).  Needs no device
int32_t svh_test_grid_pred(const svh_grid_pred_params* p, int32_t nx, int32_t nz, const int32_t* id, const int32_t* tracks, int32_t n_tracks,
                           uint32_t* pred, int64_t* stats) {
    grid::PredParams q;
    if (!convert_pred(p, &q) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || n_tracks < 0 || n_tracks > grid::OBJ_MAX_TRACKS ||
        (n_tracks > 0 && !tracks) || !pred)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pred: bad arguments");
    for (int32_t t = 1; t < n_tracks; t++)
        if (tracks[(size_t)t * grid::TRACK_REC] <= tracks[(size_t)(t - 1) * grid::TRACK_REC])
            return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pred: the track table is not in ascending order of id");
    grid::pred_window(q, nx, nz, id, tracks, n_tracks, pred, stats);
    return SVH_OK;
}

// the kernels of the prediction on a caller's ID plane and track table (host); stats[3] the launches
int32_t svh_test_grid_pred_device(const svh_grid_pred_params* p, int32_t nx, int32_t nz, const int32_t* id, const int32_t* tracks, int32_t n_tracks,
                                  uint32_t* pred, int64_t* stats) {
    grid::PredParams q;
    if (!convert_pred(p, &q) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || n_tracks < 0 || n_tracks > grid::OBJ_MAX_TRACKS ||
        (n_tracks > 0 && (!tracks || !id)) || !pred)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pred_device: bad arguments");
    for (int32_t t = 1; t < n_tracks; t++)
        if (tracks[(size_t)t * grid::TRACK_REC] <= tracks[(size_t)(t - 1) * grid::TRACK_REC])
            return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pred_device: the track table is not in ascending order of id");
    svh::ensure_init();
    const size_t cells = (size_t)nx * (size_t)nz;
    HipBuf<int32_t> d_id, d_tracks;
    PredBufs b;
    hipStream_t s = nullptr;
    int32_t launches = 0;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        if (n_tracks > 0) {
            GRID_GROW_N(d_id, cells);
            GRID_GROW_N(d_tracks, (size_t)n_tracks * grid::TRACK_REC);
            GRID_TRY(copy, hipMemcpyAsync(d_id, id, cells * sizeof(int32_t), hipMemcpyHostToDevice, s));
            GRID_TRY(copy, hipMemcpyAsync(d_tracks, tracks, (size_t)n_tracks * grid::TRACK_REC * sizeof(int32_t), hipMemcpyHostToDevice, s));
        }
        grid::PredJob j;
        const int r = pred_job(s, q, nx, nz, d_id, d_tracks, n_tracks, b, &j);
        if (r) return r;
        if (n_tracks > 0) GRID_TRY(launch, (launches = grid::launch_pred(s, j), hipGetLastError()));
        GRID_TRY(copy, hipMemcpyAsync(pred, b.plane, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(b.h_ctl, b.ctl, grid::PRED_CTL_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    if (stats) {
        for (int k = 0; k < grid::PS_LAUNCHES; k++) stats[k] = (int64_t)b.h_ctl[k];
        stats[grid::PS_LAUNCHES] = launches;
    }
    return SVH_OK;
}

// grid_pred_core.h's slots, radii and displacements on the host: slot[t] = the slot of pose t for t < T, radius[s] and ge[r] for
// s < 32 and r <= 16, and (n > 0) disp[i * 32 + s] = D(s) of the velocity v16[i] on one axis.  Any output may be NULL.  Needs no device
int32_t svh_test_grid_pred_slots(const svh_grid_pred_params* p, int32_t T, int32_t* slot, int32_t* radius, uint32_t* ge, const int32_t* v16, int32_t n,
                                 int32_t* disp) {
    grid::PredParams q;
    if (!convert_pred(p, &q) || T < 0 || T > grid::ROLL_MAX_T || n < 0 || (n > 0 && (!v16 || !disp)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pred_slots: bad arguments");
    for (int32_t t = 0; slot && t < T; t++) slot[t] = grid::pred_slot(q, t);
    for (int32_t s = 0; radius && s < grid::PRED_MAX_SLOTS; s++) radius[s] = grid::pred_radius(q, s);
    for (int32_t r = 0; ge && r <= grid::PRED_MAX_RADIUS; r++) ge[r] = grid::pred_ge(q, r);
    for (int32_t i = 0; i < n; i++)
        for (int32_t s = 0; s < grid::PRED_MAX_SLOTS; s++) disp[(size_t)i * grid::PRED_MAX_SLOTS + s] = grid::pred_disp(q, v16[i], s);
    return SVH_OK;
}

// grid_pred_core.h's scoring on the host, with the footprint table of roll_table_for: the arguments of svh_test_grid_roll, the
// prediction parameters and a PRED plane of the window's size under the offsets (poa, pob); mout[n_poses] the footprint predictions
// of the free poses, recs 6 per candidate.  Needs no device
int32_t svh_test_grid_pred_roll(const svh_grid_roll_params* p, const svh_grid_pred_params* pp, float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                                const uint8_t* cost, const int32_t* pot, int32_t poa, int32_t pob, const uint32_t* pred, const int32_t* table, int32_t S,
                                int32_t K, int32_t T, int32_t set, int32_t ga0, int32_t gb0, const int32_t* poses, int64_t n_poses, uint32_t* mout,
                                int32_t* recs, int64_t* scores, int32_t* best) {
    grid::RollParams q;
    grid::PredParams qp;
    std::shared_ptr<const RollTable> t;
    int32_t fdummy = 0;
    if (!convert_pred(pp, &qp) || !pred || !grid::offsets_ok(poa, pob) || (n_poses > 0 && !mout) ||
        !roll_test_args(p, cell, nx, nz, oa, ob, cost, pot, table, S, K, T, set, ga0, gb0, poses, n_poses, n_poses > 0 ? &fdummy : nullptr, best, &q, &t))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pred_roll: bad arguments");
    if (n_poses > 0) grid::footprint_pred_window(q, nx, nz, poa, pob, pred, t->offs.data(), t->start.data(), poses, n_poses, mout);
    if (table)
        *best = grid::roll_pred_window(q, qp, nx, nz, oa, ob, cost, pot, nx, nz, poa, pob, pred, t->offs.data(), t->start.data(),
                                       table + (size_t)set * (size_t)K * (size_t)T * 3, K, T, ga0, gb0, recs, scores);
    return SVH_OK;
}

// grid_plan_core.h on the host: POT and DIR of a window of nx x nz cells from its COST plane and n goals (global cells under
// the offsets oa, ob), by the heap Dijkstra of the header; returns the goals that count.  Needs no device
int32_t svh_test_grid_plan(const svh_grid_plan_params* p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost,
                           const int32_t* goals, int32_t n, int32_t* pot, uint8_t* dir) {
    if (!p || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || !cost || n < 0 ||
        n > grid::PLAN_MAX_GOALS || (n > 0 && !goals) || !pot || !dir)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_plan: bad arguments");
    const grid::PlanParams q{p->neutral, p->unknown, p->max_cost};
    if (!grid::plan_ok(q)) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_plan: parameters out of range");
    for (int32_t k = 0; k < 2 * n; k++)
        if (goals[k] <= -grid::PLAN_GOAL_LIMIT || goals[k] >= grid::PLAN_GOAL_LIMIT) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_plan: a goal's cell is not below 2^20");
    return grid::plan_window(q, nx, nz, oa, ob, cost, goals, n, pot, dir);
}

// grid_plan_core.h's walk over a DIR plane from the window cell (a, b): *len cells (0: outside, or DIR leads nowhere), the
// first min(*len, cap) of them as global cells.  Needs no device
int32_t svh_test_grid_path(int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* dir, int32_t a, int32_t b, int32_t* cells,
                           int64_t cap, int64_t* len) {
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || !dir || cap < 0 || (cap > 0 && !cells) || !len)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_path: bad arguments");
    *len = grid::walk_window(nx, nz, oa, ob, dir, a, b, cells, cap);
    return SVH_OK;
}

int32_t svh_test_grid_plan_tile(void) { return grid::PLAN_TILE; }

// the rounds enqueued per wait become n (1..64; anything else only reads); returns what they were.  Not thread safe: a
// measurement's switch
int32_t svh_test_grid_plan_rounds_per_wait(int32_t n) {
    const int32_t was = g_rounds_per_wait;
    if (n >= 1 && n <= 64) g_rounds_per_wait = n;
    return was;
}

// the planner's kernels and round loop on a caller's COST plane (host, nx x nz, offsets 0) and goals: POT and DIR to the
// host, out[0] the goals that counted, out[1] the cells reached, out[2] the rounds
int32_t svh_test_grid_plan_device(int32_t nx, int32_t nz, const svh_grid_plan_params* p, const uint8_t* cost, const int32_t* goals,
                                  int32_t n, int32_t* pot, uint8_t* dir, int64_t out[3]) {
    if (!p || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !cost || n < 0 || n > grid::PLAN_MAX_GOALS ||
        (n > 0 && !goals) || !pot || !dir || !out)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_plan_device: bad arguments");
    grid::PlanJob j;
    j.pln = grid::PlanParams{p->neutral, p->unknown, p->max_cost};
    if (!grid::plan_ok(j.pln)) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_plan_device: parameters out of range");
    for (int32_t k = 0; k < 2 * n; k++)
        if (goals[k] <= -grid::PLAN_GOAL_LIMIT || goals[k] >= grid::PLAN_GOAL_LIMIT) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_plan_device: a goal's cell is not below 2^20");
    svh::ensure_init();
    j.nx = nx, j.nz = nz, j.oa = j.ob = 0, j.n_goals = n;
    const size_t cells = (size_t)nx * (size_t)nz, tiles = (size_t)grid::plan_tiles_x(j) * grid::plan_tiles_y(j);
    HipBuf<uint8_t> d_cost, field;
    HipBuf<int32_t> d_goals;
    HipBuf<uint32_t> d_tiles, d_ctl;
    PinnedBuf<uint32_t> h_ctl;
    hipStream_t s = nullptr;
    const int rc = [&]() -> int {
        GRID_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        GRID_GROW(d_cost, cells);
        GRID_GROW(field, cells * kPlanBytes);
        GRID_GROW_N(d_goals, 2 * (size_t)n);
        GRID_GROW(d_tiles, 4 * tiles * sizeof(uint32_t));
        GRID_GROW(d_ctl, grid::CTL_WORDS * sizeof(uint32_t));
        GRID_GROW(h_ctl, grid::CTL_WORDS * sizeof(uint32_t));
        GRID_TRY(copy, hipMemcpyAsync(d_cost, cost, cells, hipMemcpyHostToDevice, s));
        if (n > 0) GRID_TRY(copy, hipMemcpyAsync(d_goals, goals, 2 * (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        j.cost = d_cost.p;
        j.pot = (int32_t*)field.p, j.price = (uint16_t*)(field.p + 4 * cells), j.dir = field.p + 6 * cells;
        j.goals = d_goals.p;
        j.lists = d_tiles.p, j.flags = d_tiles.p + 2 * tiles;
        j.ctl = d_ctl.p;
        const int r = plan_run(s, j, h_ctl);
        if (r) return r;
        GRID_TRY(copy, hipMemcpyAsync(pot, j.pot, cells * 4, hipMemcpyDeviceToHost, s));
        GRID_TRY(copy, hipMemcpyAsync(dir, j.dir, cells, hipMemcpyDeviceToHost, s));
        GRID_TRY(wait, hipStreamSynchronize(s));
        return SVH_OK;
    }();
    if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    if (rc) return rc;
    out[0] = h_ctl.p[grid::CTL_COUNTED];
    out[1] = (int64_t)((uint64_t)h_ctl.p[grid::CTL_REACHED] | ((uint64_t)h_ctl.p[grid::CTL_REACHED + 1] << 32));
    out[2] = h_ctl.p[grid::CTL_ROUNDS];
    return SVH_OK;
}

// grid_pose_core.h on the host: CF, PPOT and PDIR (8 planes each, heading-major) of a window of nx x nz cells from its COST plane,
// the vehicle of `r` on cells of side `cell` and n goal triples (global cells under the offsets oa, ob), by the loops of the header;
// *counted the goal states that count.  Needs no device
int32_t svh_test_grid_pose(const svh_grid_roll_params* r, const svh_grid_pose_params* p, float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                           const uint8_t* cost, const int32_t* goals, int32_t n, uint8_t* cf, int32_t* pot, uint8_t* dir, int64_t* counted) {
    grid::RollParams q;
    grid::PoseParams pp;
    std::shared_ptr<const RollTable> t;
    if (!counted || !pose_test_args(r, p, cell, nx, nz, oa, ob, cost, goals, n, cf, pot, dir, &q, &pp, &t))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pose: bad arguments");
    grid::pose_cf_window(nx, nz, cost, t->offs.data(), t->start.data(), q.m, q.unknown_cost, cf);
    *counted = grid::pose_window(pp, q.stop_cost, nx, nz, oa, ob, cf, goals, n, pot, dir);
    return SVH_OK;
}

// grid_pose_core.h's walk over a PDIR field from the window state (a, b, d): *len poses (0: outside, or PDIR leads nowhere), the
// first min(*len, cap) of them as (global cell, d m).  Needs no device
int32_t svh_test_grid_pose_walk(int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t m, const uint8_t* dir, int32_t a, int32_t b, int32_t d,
                                int32_t* poses, int64_t cap, int64_t* len) {
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || m < 1 || m > grid::ROLL_MAX_M || !dir || cap < 0 ||
        (cap > 0 && !poses) || !len)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pose_walk: bad arguments");
    *len = grid::pose_walk(nx, nz, oa, ob, m, dir, a, b, d, poses, cap);
    return SVH_OK;
}

// the same field through the kernels and the round loop: out[0] the goal states that counted, out[1] the states reached, out[2] the rounds
int32_t svh_test_grid_pose_device(const svh_grid_roll_params* r, const svh_grid_pose_params* p, float cell, int32_t nx, int32_t nz, int32_t oa,
                                  int32_t ob, const uint8_t* cost, const int32_t* goals, int32_t n, uint8_t* cf, int32_t* pot, uint8_t* dir,
                                  int64_t out[3]) {
    grid::RollParams q;
    grid::PoseParams pp;
    std::shared_ptr<const RollTable> t;
    if (!out || !pose_test_args(r, p, cell, nx, nz, oa, ob, cost, goals, n, cf, pot, dir, &q, &pp, &t))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_pose_device: bad arguments");
    svh::ensure_init();
    RollTable own = *t;   // the table is that of the vehicle; the costs are this call's
    own.p = q;
    return pose_device(pp, own, nx, nz, oa, ob, cost, goals, n, cf, pot, dir, out);
}

// the tile side of k_grid_time_sweep, and the layers of a chunk to *k
int32_t svh_test_grid_time_tile(int32_t* k) {
    if (k) *k = grid::TIME_K;
    return grid::TIME_TILE;
}

// the checks that svh_test_grid_time and svh_test_grid_time_device share.  The ID plane and the tracks count only with release = 1,
// and then CLASS and the traversability parameters are needed for the distance passes
static bool time_test_args(const svh_grid_plan_params* pl, const svh_grid_pred_params* pp, const svh_grid_time_params* tp, const svh_grid_trav_params* tv,
                           float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost, const uint8_t* flags, const uint8_t* cls,
                           const int32_t* goals, int32_t n_goals, const uint32_t* pred, int32_t poa, int32_t pob, const int32_t* id, const int32_t* tracks,
                           int32_t n_tracks, const void* tpot, const void* tdir, const void* rcost, const void* rpot, const void* rdir, const void* stats,
                           int32_t a, int32_t b, const int32_t* triples, int64_t cap, const void* walk, TimeTestArgs* q) {
    if (!pl || !convert_pred(pp, &q->pp) || !convert_time(tp, &q->tp) || nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE ||
        !grid::time_fits(q->tp, nx, nz) || !grid::offsets_ok(oa, ob) || !grid::offsets_ok(poa, pob) || !cost || !flags || !pred || n_goals < 0 ||
        n_goals > grid::PLAN_MAX_GOALS || (n_goals > 0 && !goals) || n_tracks < 0 || n_tracks > grid::OBJ_MAX_TRACKS || (n_tracks > 0 && (!tracks || !id)) ||
        !tpot || !tdir || !rcost || !rpot || !rdir || !stats || cap < 0 || (a >= 0 && (a >= nx || b < 0 || b >= nz || !walk || (cap > 0 && !triples))))
        return false;
    q->pln = grid::PlanParams{pl->neutral, pl->unknown, pl->max_cost};
    if (!grid::plan_ok(q->pln)) return false;
    for (int32_t k = 0; k < 2 * n_goals; k++)
        if (goals[k] <= -grid::PLAN_GOAL_LIMIT || goals[k] >= grid::PLAN_GOAL_LIMIT) return false;
    for (int32_t t = 1; t < n_tracks; t++)
        if (tracks[(size_t)t * grid::TRACK_REC] <= tracks[(size_t)(t - 1) * grid::TRACK_REC]) return false;
    q->n_tracks = q->tp.release ? n_tracks : 0;
    q->trv.reach = 0;
    if (q->n_tracks > 0 && (!cls || !(grid::finite_f(cell) && cell > 0.f) || !convert_trav(tv, cell, &q->trv, &q->table))) return false;
    return true;
}

// grid_time_core.h on the host: the window of nx x nz cells under (oa, ob) with its COST and FLAGS planes (and CLASS, for the distance
// passes of release = 1), the planner's goals, PRED of the frame of nx x nz cells under (poa, pob), the ID plane of that frame and
// n_tracks track records in ascending order of id -> tpot, tdir [layers * nz * nx], rcost, rpot, rdir [nz * nx], stats[6] (the rounds
// are 0).  With a >= 0 the path from the window cell (a, b): walk[0] the status, walk[1] the entries, walk[2] the cost, the first
// min(walk[1], cap) triples.  Needs no device
int32_t svh_test_grid_time(const svh_grid_plan_params* pl, const svh_grid_pred_params* pp, const svh_grid_time_params* tp, const svh_grid_trav_params* tv,
                           float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost, const uint8_t* flags, const uint8_t* cls,
                           const int32_t* goals, int32_t n_goals, const uint32_t* pred, int32_t poa, int32_t pob, const int32_t* id, const int32_t* tracks,
                           int32_t n_tracks, int32_t* tpot, uint8_t* tdir, uint8_t* rcost, int32_t* rpot, uint8_t* rdir, int64_t* stats, int32_t a,
                           int32_t b, int32_t* triples, int64_t cap, int64_t* walk) {
    TimeTestArgs q;
    if (!time_test_args(pl, pp, tp, tv, cell, nx, nz, oa, ob, cost, flags, cls, goals, n_goals, pred, poa, pob, id, tracks, n_tracks, tpot, tdir, rcost, rpot,
                        rdir, stats, a, b, triples, cap, walk, &q))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_time: bad arguments");
    const size_t cells = (size_t)nx * (size_t)nz;
    int64_t released = 0;
    time_static_host(q, nx, nz, oa, ob, cost, flags, cls, goals, n_goals, poa, pob, id, tracks, rcost, rpot, rdir, &released);
    std::vector<uint16_t> price(cells);
    for (size_t i = 0; i < cells; i++) price[i] = grid::price_of(q.pln, rcost[i]);
    grid::time_window(q.pln, q.tp, q.pp, nx, nz, oa, ob, price.data(), rpot, rdir, pred, poa, pob, tpot, tdir, stats);
    stats[grid::TM_RELEASED] = released, stats[grid::TM_ROUNDS] = 0;
    if (a >= 0) {
        const size_t i = (size_t)b * (size_t)nx + (size_t)a;
        const grid::TimeBlock B{pred, nx, nz, oa, ob, poa, pob};
        int32_t status = grid::time_start_status(price[i], B(a, b), tpot[i]);
        int64_t len = 0;
        if (status == grid::PATH_FOUND && (len = grid::time_walk(nx, nz, oa, ob, q.tp.layers, tdir, rdir, a, b, triples, cap)) == 0) status = grid::PATH_UNREACHABLE;
        walk[0] = status, walk[1] = len, walk[2] = tpot[i];
    }
    return SVH_OK;
}

// the same through the kernels of csrc/grid_time_kernels.hip, the distance launches and the planner's round loop; stats[5] the rounds
int32_t svh_test_grid_time_device(const svh_grid_plan_params* pl, const svh_grid_pred_params* pp, const svh_grid_time_params* tp,
                                  const svh_grid_trav_params* tv, float cell, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost,
                                  const uint8_t* flags, const uint8_t* cls, const int32_t* goals, int32_t n_goals, const uint32_t* pred, int32_t poa,
                                  int32_t pob, const int32_t* id, const int32_t* tracks, int32_t n_tracks, int32_t* tpot, uint8_t* tdir, uint8_t* rcost,
                                  int32_t* rpot, uint8_t* rdir, int64_t* stats, int32_t a, int32_t b, int32_t* triples, int64_t cap, int64_t* walk) {
    TimeTestArgs q;
    if (!time_test_args(pl, pp, tp, tv, cell, nx, nz, oa, ob, cost, flags, cls, goals, n_goals, pred, poa, pob, id, tracks, n_tracks, tpot, tdir, rcost, rpot,
                        rdir, stats, a, b, triples, cap, walk, &q))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_time_device: bad arguments");
    svh::ensure_init();
    return time_device(q, nx, nz, oa, ob, cost, flags, cls, goals, n_goals, pred, poa, pob, id, tracks, tpot, tdir, rcost, rpot, rdir, stats, a, b, triples, cap,
                       walk);
}

// grid_core.h's traversability layer on the host: the planes of a window of p->nx x p->nz cells from CLASS, HMEAN and STATE;
// rgb[3] per cell is colour_cost (cell order, no row flip).  Any output may be NULL
int32_t svh_test_grid_trav(const svh_grid_params* p, const svh_grid_trav_params* t, const uint8_t* cls, const float* hmean,
                           const uint8_t* state, uint8_t* flags, int32_t* dist2, uint8_t* cost, uint8_t* rgb) {
    grid::Params prm;
    grid::TravParams trv;
    std::vector<uint8_t> table;
    if (!convert(p, &prm) || !convert_trav(t, prm.cell, &trv, &table) || !cls || !hmean || !state)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_trav: bad arguments");
    const size_t n = (size_t)prm.nx * (size_t)prm.nz;
    std::vector<uint8_t> f(n), c(n);
    std::vector<uint16_t> gcol(n);
    grid::trav_window(trv, prm.nx, prm.nz, cls, hmean, state, table.data(), f.data(), gcol.data(), dist2, c.data());
    if (flags) memcpy(flags, f.data(), n);
    if (cost) memcpy(cost, c.data(), n);
    if (rgb)
        for (size_t i = 0; i < n; i++) grid::colour_cost(c[i], f[i], rgb + 3 * i);
    return SVH_OK;
}

// the cost table for a cell side: *reach, and the first min(reach^2 + 1, cap) bytes
int32_t svh_test_grid_cost_table(float cell, const svh_grid_trav_params* t, int32_t* reach, uint8_t* table, int64_t cap) {
    grid::TravParams trv;
    std::vector<uint8_t> tb;
    if (!(grid::finite_f(cell) && cell > 0.f) || !reach || cap < 0 || (cap > 0 && !table) || !convert_trav(t, cell, &trv, &tb))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_cost_table: bad arguments");
    *reach = trv.reach;
    if (cap > 0) memcpy(table, tb.data(), std::min((size_t)cap, tb.size()));
    return SVH_OK;
}

int32_t svh_test_grid_points(const svh_grid_params* p, const float* xyzv, int64_t n, int32_t* fate, uint32_t* cell,
                             uint32_t* key, int32_t* q, uint8_t* v) {
    grid::Params prm;
    if (!convert(p, &prm) || n < 0 || (n > 0 && !xyzv)) return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_points: bad arguments");
    for (int64_t i = 0; i < n; i++) {
        const grid::Placed r = grid::place(prm, xyzv[4 * i], xyzv[4 * i + 1], xyzv[4 * i + 2], xyzv[4 * i + 3]);
        if (fate) fate[i] = r.fate;
        if (cell) cell[i] = r.cell;
        if (key) key[i] = r.key;
        if (q) q[i] = r.q;
        if (v) v[i] = (uint8_t)r.v;
    }
    return SVH_OK;
}

// grid_core.h's place() under window offsets, on the host
int32_t svh_test_grid_points_at(const svh_grid_params* p, int32_t oa, int32_t ob, const float* xyzv, int64_t n, int32_t* fate,
                                uint32_t* cell, uint32_t* slot) {
    grid::Params prm;
    if (!convert(p, &prm) || !grid::offsets_ok(oa, ob) || n < 0 || (n > 0 && !xyzv))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_points_at: bad arguments");
    prm.oa = oa, prm.ob = ob;
    for (int64_t i = 0; i < n; i++) {
        const grid::Placed r = grid::place(prm, xyzv[4 * i], xyzv[4 * i + 1], xyzv[4 * i + 2], xyzv[4 * i + 3]);
        if (fate) fate[i] = r.fate;
        if (cell) cell[i] = r.cell;
        if (slot) slot[i] = r.cell == grid::NO_CELL ? grid::NO_CELL : r.slot;
    }
    return SVH_OK;
}

// grid_core.h's line on the host: *n = its length, and the first min(*n, cap) cells as (a, b) pairs
int32_t svh_test_grid_line(int32_t oa, int32_t ob, int32_t ea, int32_t eb, int32_t* n, int32_t* cells, int32_t cap) {
    const int64_t dx = (int64_t)ea - oa, dz = (int64_t)eb - ob;
    if (!n || cap < 0 || (cap > 0 && !cells) || dx <= -grid::MAX_SIDE || dx >= grid::MAX_SIDE || dz <= -grid::MAX_SIDE ||
        dz >= grid::MAX_SIDE)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_line: an output and two cells less than 8192 apart are needed");
    const int32_t len = grid::line_len((int32_t)dx, (int32_t)dz);
    for (int32_t k = 0; k < len && k < cap; k++) {
        int32_t sx, sz;
        grid::line_step((int32_t)dx, (int32_t)dz, len, k, &sx, &sz);
        cells[2 * k] = oa + sx, cells[2 * k + 1] = ob + sz;
    }
    *n = len;
    return SVH_OK;
}

// grid_core.h's state byte and local colour on the host, per cell
int32_t svh_test_grid_local(const svh_grid_params* p, int64_t ncells, const uint8_t* cls, const uint8_t* intensity,
                            const int32_t* pass, uint8_t* state, uint8_t* rgb) {
    grid::Params prm;
    if (!convert(p, &prm) || ncells < 0 || (ncells > 0 && (!cls || !intensity || !pass)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_local: bad arguments");
    for (int64_t i = 0; i < ncells; i++) {
        const grid::Final f{0.f, 0.f, 0.f, intensity[i], cls[i]};
        if (state) state[i] = grid::state_of(prm, cls[i], pass[i]);
        if (rgb) grid::colour_local(prm, 1, f, pass[i], rgb + 3 * i);
    }
    return SVH_OK;
}

int32_t svh_test_grid_finalise(const svh_grid_params* p, int64_t ncells, const int32_t* count, const int32_t* overhead,
                               const uint32_t* kmin, const uint32_t* kmax, const int64_t* hsum, const uint64_t* vsum,
                               float* hmin, float* hmax, float* hmean, uint8_t* intensity, uint8_t* cls, uint8_t* rgb) {
    grid::Params prm;
    if (!convert(p, &prm) || ncells < 0 || (ncells > 0 && (!count || !overhead || !kmin || !kmax || !hsum || !vsum)))
        return svh::fail(SVH_ERR_BAD_ARG, "svh_test_grid_finalise: bad arguments");
    for (int64_t i = 0; i < ncells; i++) {
        const grid::Cell c{count[i], overhead[i], kmin[i], kmax[i], hsum[i], vsum[i]};
        const grid::Final f = grid::finalise(prm, c);
        if (hmin) hmin[i] = f.hmin;
        if (hmax) hmax[i] = f.hmax;
        if (hmean) hmean[i] = f.hmean;
        if (intensity) intensity[i] = f.intensity;
        if (cls) cls[i] = f.cls;
        if (rgb)
            for (int32_t m = 0; m < grid::M_MODES; m++) grid::colour(prm, m, c.count, f, rgb + 9 * i + 3 * m);
    }
    return SVH_OK;
}

}  // extern "C"

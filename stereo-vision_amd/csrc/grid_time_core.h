// The arithmetic of the ground grid's time-layered planner (svh_grid_set_time, svh_grid_get_time_plane, svh_grid_get_time_stats,
// svh_grid_time_path, svh_grid_render_time; include/svh_grid_time.h, "TIME"): a cost-to-go over cell x time that knows where the
// predicted objects will be, and paths that wait for them.  THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_time_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entry svh_test_grid_time, which runs the loops below on the host),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_time_check.cpp,
// and restated in numpy and plain Python by tests/grid_time_ref.py, which tests/test_grid_time.py pins by hand and against the test
// entry.  Integers throughout.
//
// PARAMETERS.  layers L 1..256; wait -1 (no wait move) or 1..65535, its weight; release 0 or 1.  L nx nz is at most 2^28.  neutral,
// unknown and max_cost are the planner's (grid_plan_core.h), and so are the goals.
// LAYERS AND SLOTS.  A move of this layer is a pose of the prediction (grid_pred_core.h): layer 0 is now, slot 0; layer t >= 1 is at
// slot pred_slot(t - 1) = min(slots - 1, rdiv(t, poses_per_step stride)).  Up to layer L - 1 a path of this layer without its first
// entry is a candidate whose pose t - 1 is the path's entry t, so it goes into a candidate table unchanged.
// BLOCK(p, t) is bit slot(t) of PRED at p's GLOBAL cell (pred_at): 0 outside the ID frame, 0 before the first step.  The word is
// unsigned: slot 31 is bit 31.
//
// STATIC PLANES.  With release = 0, RCOST = COST, RPOT = POT and RDIR = DIR.  With release = 1, FLAGS' is FLAGS with TF_LETHAL
// cleared on every window cell whose global cell lies in the ID frame and holds the id of a predicting track (pred_predicts: the
// source cells of the prediction's statistics); the RELEASED cells are those.  RCOST is DIST2 -> table -> cell_cost over FLAGS', the
// column and row passes of grid_core.h (dist_window) unchanged: a released cell costs what a free cell there would, the inflation of
// a wall beside the object stays, the object's own inflation goes.  RPRICE = price_of(plan, RCOST); RPOT and RDIR are the planner's
// POT and DIR over RPRICE with the planner's goals.  With no released cell the planes are those of release = 0.
// release = 1 is meant for only_moving = 1: a standing track that predicts is released too, and is blocked by its own PRED bits in
// every layer instead.
//
// TPOT(p, t), int32, layer-major: state (a, b, t) lies at (t nz + b) nx + a.
//   Last layer:  TPOT(p, L - 1) = RPOT(p), or PLAN_FAR when BLOCK(p, L - 1).
//   t < L - 1, the first rule that applies:
//     FAR  when RPRICE(p) = 0 or BLOCK(p, t);
//     0    when RPOT(p) = 0, a goal that counts;
//     else the least candidate, each dropped above max_cost (the planner's `candidate`); FAR when none is left.
//   CANDIDATES of (p, t):
//     move d = 0..7 to the neighbour v: w = step_weight(RPRICE, p, d) is not 0, no BLOCK at t + 1 on v nor, for a corner step, on the
//       two cells that share an edge with both, and TPOT(v, t + 1) is not FAR: TPOT(v, t + 1) + w;
//     wait, when wait >= 1: no BLOCK(p, t + 1) and TPOT(p, t + 1) is not FAR: TPOT(p, t + 1) + wait.
//   Everything is formed in uint32: a TPOT is at most 0x7FFFFFFF and a weight at most 65535, so nothing wraps.
// TDIR(p, t), uint8: for t < L - 1, 8 goal (TPOT 0), 9 none (TPOT FAR), else the LOWEST d in 0..7 that attains the minimum, and
// TDIR_WAIT = 10 only when no move attains it.  TDIR(., L - 1) = RDIR, or 9 when blocked.
// PATH from (start cell, layer 0): follow TDIR through the layers, a move or a wait advancing t by one; from layer L - 1 on follow
// RDIR with t kept at L - 1; stop at a goal, or after L + nx nz entries.  Entries are triples (ga, gb, t).  The status is the
// planner's: FOUND, UNREACHABLE (TPOT of the start is FAR), BLOCKED (the start is impassable in RPRICE, or BLOCK(start, 0)), OUTSIDE.
//
// NOT A RELAXATION.  Unlike POT this field is no fixed point: layer t is a pure function of layer t + 1 and the static planes, so it
// is one backward sweep, and no byte depends on launch shape or scheduling.
// INVARIANT.  With PRED all 0, every layer of TPOT equals POT and every layer of TDIR equals DIR, byte for byte, for either value of
// release (nothing predicts, so nothing is released): the recursion above is the Bellman equation of POT, whose least candidate is
// POT itself and is attained first by DIR; a wait costs POT + wait > POT, so it never attains the minimum on a static graph.
#pragma once
#include <stdint.h>

#include <vector>

#include "grid_core.h"
#include "grid_obj_core.h"
#include "grid_plan_core.h"
#include "grid_pred_core.h"

namespace svh {
namespace grid {

constexpr int32_t TIME_MAX_LAYERS = 256, TIME_MAX_WAIT = 65535;
constexpr int64_t TIME_MAX_STATES = (int64_t)1 << 28;   // L nx nz
constexpr uint8_t TDIR_WAIT = 10;
enum TimePlane : int32_t { TP_TPOT = 0, TP_TDIR, TP_RCOST, TP_RPOT, TP_PLANES };
// layers; states with TPOT != FAR; statically passable states with BLOCK set; states whose TDIR is wait; released cells; the
// relaxation rounds of RPOT
enum TimeStat : int32_t { TM_LAYERS = 0, TM_REACHED, TM_BLOCKED, TM_WAITS, TM_RELEASED, TM_ROUNDS, TM_WORDS };

struct TimeParams {
    int32_t layers;    // 1..256
    int32_t wait;      // -1, or 1..65535
    int32_t release;   // 0 or 1
};

MC_FN bool time_ok(const TimeParams& p) {
    return p.layers >= 1 && p.layers <= TIME_MAX_LAYERS && (p.wait == -1 || (p.wait >= 1 && p.wait <= TIME_MAX_WAIT)) &&
           (p.release == 0 || p.release == 1);
}
MC_FN bool time_fits(const TimeParams& p, int32_t nx, int32_t nz) { return (int64_t)p.layers * (int64_t)nx * (int64_t)nz <= TIME_MAX_STATES; }

// the slot of layer t
MC_FN int32_t time_slot(const PredParams& pp, int32_t t) { return t == 0 ? 0 : pred_slot(pp, t - 1); }

MC_FN bool time_bit(uint32_t word, int32_t slot) { return ((word >> slot) & 1u) != 0u; }

// the PRED word of a window cell: the window lies under (oa, ob), the ID frame of nx x nz cells under (poa, pob); null: PRED is all 0
struct TimeBlock {
    const uint32_t* pred;
    int32_t nx, nz, oa, ob, poa, pob;
    MC_FN uint32_t operator()(int32_t a, int32_t b) const { return pred ? pred_at(pred, nx, nz, poa, pob, (int64_t)oa + a, (int64_t)ob + b) : 0u; }
};

// the rank of `id` among n track records in ascending order of id, -1 when it is not there
MC_FN int32_t time_track_rank(const int32_t* tracks, int32_t n, int32_t id) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {   // at most 13 rounds
        const int32_t mid = (lo + hi) >> 1;
        if (tracks[(size_t)mid * TRACK_REC + TR_ID] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && tracks[(size_t)lo * TRACK_REC + TR_ID] == id ? lo : -1;
}

// whether the window cell (a, b) is released: `id` is the ID plane of the frame (null: all -1)
MC_FN bool time_released(const PredParams& pp, int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t poa, int32_t pob, const int32_t* id,
                         const int32_t* tracks, int32_t n_tracks, int32_t a, int32_t b) {
    const int64_t pa = (int64_t)oa + a - poa, pb = (int64_t)ob + b - pob;
    if (!id || n_tracks < 1 || pa < 0 || pa >= nx || pb < 0 || pb >= nz) return false;
    const int32_t v = id[(size_t)pb * (size_t)nx + (size_t)pa];
    if (v < 0) return false;
    const int32_t r = time_track_rank(tracks, n_tracks, v);
    return r >= 0 && pred_predicts(pp, tracks + (size_t)r * TRACK_REC);
}

// One state of a layer t < L - 1 at the window cell (a, b).  `price(a, b)` is RPRICE, 0 outside the window; `next(a, b)` is
// TPOT(., t + 1), read only inside the window; `block(a, b)` the PRED word of a window cell; s_now and s_next the slots of t and t + 1;
// rpot RPOT of the cell.
template <class Price, class Next, class Block>
MC_FN void time_state(const PlanParams& pl, const TimeParams& tp, const Price& price, const Next& next, const Block& block, int32_t s_now,
                      int32_t s_next, int32_t rpot, int32_t a, int32_t b, int32_t* tpot, uint8_t* tdir) {
    const uint32_t pu = price(a, b);
    const uint32_t own = pu ? block(a, b) : 0u;
    if (pu == 0 || time_bit(own, s_now)) {
        *tpot = PLAN_FAR, *tdir = DIR_NONE;
        return;
    }
    if (rpot == 0) {
        *tpot = 0, *tdir = DIR_GOAL;
        return;
    }
    uint32_t best = (uint32_t)PLAN_FAR;
    uint8_t dir = DIR_NONE;
    for (int32_t d = 0; d < 8; d++) {
        const uint32_t w = step_weight(price, a, b, pu, d);
        if (w == 0) continue;
        const int32_t va = a + step_da(d), vb = b + step_db(d);
        if (time_bit(block(va, vb), s_next)) continue;
        if ((d & 1) && (time_bit(block(va, b), s_next) || time_bit(block(a, vb), s_next))) continue;
        const int32_t nv = next(va, vb);
        if (nv == PLAN_FAR) continue;
        const uint32_t c = candidate((uint32_t)nv, w, (uint32_t)pl.max_cost);
        if (c < best) best = c, dir = (uint8_t)d;
    }
    if (tp.wait >= 1 && !time_bit(own, s_next)) {
        const int32_t nv = next(a, b);
        if (nv != PLAN_FAR) {
            const uint32_t c = candidate((uint32_t)nv, (uint32_t)tp.wait, (uint32_t)pl.max_cost);
            if (c < best) best = c, dir = TDIR_WAIT;
        }
    }
    *tpot = (int32_t)best, *tdir = dir;
}

// the last layer at a cell: RPOT and RDIR, or FAR and none when blocked at the slot of L - 1
MC_FN void time_last(uint32_t word, int32_t s_last, int32_t rpot, uint8_t rdir, int32_t* tpot, uint8_t* tdir) {
    const bool blocked = time_bit(word, s_last);
    *tpot = blocked ? PLAN_FAR : rpot, *tdir = blocked ? DIR_NONE : rdir;
}

// the colour of a cell with BLOCK at a layer of slot s in svh_grid_render_time: the prediction's colour of that slot
MC_FN void colour_time_block(int32_t s, uint8_t* rgb) { colour_pred(1u << s, rgb); }

// ---- the host loops ---------------------------------------------------------------------------------------------------------
// FLAGS' [nz * nx] from FLAGS; returns the released cells
inline int64_t time_release_window(const PredParams& pp, int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t poa, int32_t pob, const int32_t* id,
                                   const int32_t* tracks, int32_t n_tracks, const uint8_t* flags, uint8_t* out) {
    int64_t released = 0;
    for (int32_t b = 0; b < nz; b++)
        for (int32_t a = 0; a < nx; a++) {
            const size_t i = (size_t)b * (size_t)nx + (size_t)a;
            const bool r = time_released(pp, nx, nz, oa, ob, poa, pob, id, tracks, n_tracks, a, b);
            out[i] = r ? (uint8_t)(flags[i] & ~(uint8_t)TF_LETHAL) : flags[i];
            released += r ? 1 : 0;
        }
    return released;
}

struct TimeLayer {
    const int32_t* p;
    int32_t nx;
    MC_FN int32_t operator()(int32_t a, int32_t b) const { return p[(size_t)b * (size_t)nx + (size_t)a]; }
};

// the sweep: rprice, rpot, rdir [nz * nx] and PRED (the frame of nx x nz cells under poa, pob; null: all 0) -> tpot, tdir [L * nz * nx],
// stats[TM_LAYERS .. TM_WAITS] (the others are not touched)
inline void time_window(const PlanParams& pl, const TimeParams& tp, const PredParams& pp, int32_t nx, int32_t nz, int32_t oa, int32_t ob,
                        const uint16_t* rprice, const int32_t* rpot, const uint8_t* rdir, const uint32_t* pred, int32_t poa, int32_t pob, int32_t* tpot,
                        uint8_t* tdir, int64_t* stats) {
    const size_t cells = (size_t)nx * (size_t)nz;
    const TimeBlock B{pred, nx, nz, oa, ob, poa, pob};
    const WindowPrice P{rprice, nx, nz};
    const int32_t L = tp.layers;
    int64_t st[TM_WORDS] = {L, 0, 0, 0, 0, 0};
    for (int32_t t = L - 1; t >= 0; t--) {
        int32_t* cur = tpot + (size_t)t * cells;
        uint8_t* dir = tdir + (size_t)t * cells;
        const int32_t s_now = time_slot(pp, t), s_next = time_slot(pp, t + 1);
        const TimeLayer N{cur + cells, nx};   // read only when t < L - 1
        for (int32_t b = 0; b < nz; b++)
            for (int32_t a = 0; a < nx; a++) {
                const size_t i = (size_t)b * (size_t)nx + (size_t)a;
                if (t == L - 1) time_last(B(a, b), s_now, rpot[i], rdir[i], &cur[i], &dir[i]);
                else time_state(pl, tp, P, N, B, s_now, s_next, rpot[i], a, b, &cur[i], &dir[i]);
                st[TM_REACHED] += cur[i] != PLAN_FAR ? 1 : 0;
                st[TM_BLOCKED] += (rprice[i] != 0 && time_bit(B(a, b), s_now)) ? 1 : 0;
                st[TM_WAITS] += dir[i] == TDIR_WAIT ? 1 : 0;
            }
    }
    if (stats)
        for (int32_t k = TM_LAYERS; k <= TM_WAITS; k++) stats[k] = st[k];
}

// the status of a path from the window cell (a, b), inside the window: what is known before the walk
MC_FN int32_t time_start_status(uint32_t rprice, uint32_t word, int32_t tpot0) {
    if (rprice == 0 || time_bit(word, 0)) return PATH_BLOCKED;
    return tpot0 == PLAN_FAR ? PATH_UNREACHABLE : PATH_FOUND;
}

// one entry of the walk at (a, b, t): the move d read there (TDIR below L - 1, RDIR from there on); false: it leads nowhere
MC_FN bool time_walk_step(int32_t nx, int32_t nz, int32_t L, uint8_t d, int32_t* a, int32_t* b, int32_t* t) {
    if (d == TDIR_WAIT) {
        if (*t >= L - 1) return false;   // never: RDIR holds no wait
    } else {
        if (d >= DIR_GOAL) return false;
        *a += step_da(d), *b += step_db(d);
        if (*a < 0 || *a >= nx || *b < 0 || *b >= nz) return false;   // never: a step that exists stays inside
    }
    if (*t < L - 1) (*t)++;
    return true;
}

// the walk over TDIR [L * nz * nx] and RDIR [nz * nx] from the window cell (a, b) at layer 0: the number of entries of the path, the
// first min(that, cap) of them written as (global cell, layer); 0: the cell is outside the window, or the fields do not lead to a goal
// within L + nx nz entries
inline int64_t time_walk(int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t L, const uint8_t* tdir, const uint8_t* rdir, int32_t a, int32_t b,
                         int32_t* triples, int64_t cap) {
    if (a < 0 || a >= nx || b < 0 || b >= nz) return 0;
    const size_t cells = (size_t)nx * (size_t)nz;
    const int64_t limit = (int64_t)L + (int64_t)cells;
    int32_t t = 0;
    for (int64_t len = 0; len < limit;) {
        const size_t i = (size_t)b * (size_t)nx + (size_t)a;
        const uint8_t d = t < L - 1 ? tdir[(size_t)t * cells + i] : rdir[i];
        if (d == DIR_NONE || d > TDIR_WAIT) return 0;
        if (len < cap) triples[3 * len] = oa + a, triples[3 * len + 1] = ob + b, triples[3 * len + 2] = t;
        len++;
        if (d == DIR_GOAL) return len;
        if (!time_walk_step(nx, nz, L, d, &a, &b, &t)) return 0;
    }
    return 0;
}

}  // namespace grid
}  // namespace svh

// The arithmetic of the ground grid's pose planner (svh_grid_pose_*, include/svh_grid_pose.h): from the finished COST plane of the
// window, the footprint table of the rollouts and a set of goal states a configuration-space cost CF, a cost-to-go field PPOT and a
// move field PDIR over cell x heading, and the cheapest pose sequence from any start state.  THE CONTRACT IS THIS ARITHMETIC.
// Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_pose_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entry svh_test_grid_pose, which runs the loops below on the host),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_pose_check.cpp,
// and restated in numpy / heapq by tests/grid_pose_ref.py, which tests/test_grid_pose.py pins by hand and against the test entry.
// Everything is integer arithmetic on the COST plane in logical (window) order; the torus plays no part.
//
// STATES.  A state is (a, b, d): a window cell and one of 8 headings.  Heading d is the planner's step d (grid_plan_core.h, STEPS),
// (da, db) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1).  It is the rollout heading k = d m (m = headings_m), whose vector
// (grid_roll_core.h, heading_vec) is (m da, m db) for every m: the footprint table always has its list.  Planes are heading-major:
// state (a, b, d) lies at (d nz + b) nx + a.
// CF, uint8: CF(a, b, d) = footprint_cost(COST, a, b, list(d m), unknown_cost), stored as F for 0..254 and 255 for F = -1, where a
// footprint cell lies outside the window.  r(c) is at most 254, so 255 means nothing else.
// PRICE.  A state is passable when CF < stop_cost and CF <= 252, stop_cost and unknown_cost those of the rollouts.  Its price is
// neutral + CF, at most 255 + 252 (uint16); 0 for an impassable state or a cell outside the window.
// MOVES out of a passable u = (a, b, d), kd = 5 for even d and 7 for odd d, P the price:
//   0 forward              v = (a + da, b + db, d)            w = kd (P(u) + P(v))
//   1 forward, turn left   v = (a + da, b + db, (d + 1) & 7)  w = kd (P(u) + P(v)) + turn
//   2 forward, turn right  v = (a + da, b + db, (d + 7) & 7)  w = kd (P(u) + P(v)) + turn
//   3 reverse              v = (a - da, b - db, d)            w = kd (P(u) + P(v)) + reverse    only when reverse >= 0
//   4 spin left            v = (a, b, (d + 1) & 7)            w = spin                          only when spin >= 1
//   5 spin right           v = (a, b, (d + 7) & 7)            w = spin                          only when spin >= 1
// A move exists when v is passable and, for the moves 0..3 at odd d, the two states of heading d in the cells that share an edge
// with both cells -- (a + s da, b, d) and (a, b + s db, d), s = -1 for the reverse and 1 otherwise -- are passable too: the planner's
// corner rule.  The graph is DIRECTED: what leads from u to v need not lead back.  A weight is at least 1 (a forward move at least
// 10) and at most 7 * 2 * 507 + 65535 = 72633.
// PPOT, int32: 0 for a goal state that counts (inside the window, passable); for every other passable state the least sum of weights
// over all move sequences from it to a goal state where that is at most max_cost; PLAN_FAR elsewhere.  The cap is applied per
// relaxation as in the planner: every suffix of a cheapest sequence is cheaper than the sequence.  Candidates are formed in uint32:
// a PPOT is at most 0x7FFFFFFF and a weight at most 72633, so they cannot wrap.
// PDIR, uint8, a function of PPOT alone: 8 for PPOT 0, 9 for PPOT FAR, else the LOWEST move index among the existing moves whose
// PPOT(v) + w is least; that least value is PPOT(u).  The path from a start state follows PDIR until it reaches 8; PPOT falls by at
// least 1 per move, and no state repeats, so the walk ends within 8 nx nz states.
// GOALS are triples (ga, gb, d), a global cell and a heading; d = -1 stands for every passable heading of the cell.
//
// SCHEDULE INDEPENDENCE.  The argument is the planner's, on successors.  The relaxation PULLS: a state takes the least
// candidate(PPOT(v), w(u, v)) over the moves u -> v out of it.  It only lowers values, and every value it writes is the weight
// of a real move sequence from the state to a goal, so no value falls below the true least sum.  At a fixed point -- a goal has 0,
// every other passable state the least candidate not above max_cost, else FAR -- no state can be lowered, which is the Bellman
// equation of a graph with positive weights: its solution among such fields is unique.  So PPOT, PDIR and the path do not depend on
// the launch shape, the scheduling, the order of the goals, how the states are dealt to lanes or how often a tile was relaxed.  The
// host below reaches the same field from the other side, pushing along the REVERSED moves out of a heap.
#pragma once
#include <stdint.h>

#include <queue>
#include <utility>
#include <vector>

#include "grid_plan_core.h"
#include "grid_roll_core.h"

namespace svh {
namespace grid {

constexpr int32_t POSE_HEADINGS = 8, POSE_MOVES = 6;
constexpr int32_t POSE_MAX_GOALS = 65536;
constexpr int64_t POSE_MAX_CELLS = (int64_t)1 << 24;   // nx nz: PPOT has 32 bytes per cell
constexpr uint8_t POSE_CF_OUTSIDE = 255;
constexpr int32_t POSE_MAX_CF = 252;                   // the last CF a state is passable at
constexpr uint8_t PDIR_GOAL = 8, PDIR_NONE = 9;
enum PosePlane : int32_t { PP_CF = 0, PP_POT, PP_DIR, PP_PLANES };
enum PoseMove : int32_t { PM_FORWARD = 0, PM_LEFT, PM_RIGHT, PM_REVERSE, PM_SPIN_LEFT, PM_SPIN_RIGHT };

struct PoseParams {
    int32_t neutral;     // 1..255
    int32_t max_cost;    // 1..0x7FFFFFFE
    int32_t turn;        // 0..65535
    int32_t reverse;     // -1, or 0..65535
    int32_t spin;        // -1, or 1..65535
};

MC_FN bool pose_ok(const PoseParams& p) {
    return p.neutral >= 1 && p.neutral <= 255 && p.max_cost >= 1 && p.max_cost <= 0x7FFFFFFE && p.turn >= 0 && p.turn <= 65535 &&
           p.reverse >= -1 && p.reverse <= 65535 && (p.spin == -1 || (p.spin >= 1 && p.spin <= 65535));
}

// a goal triple: the cell as the planner's goals, the heading -1..7
MC_FN bool pose_goal_ok(const int32_t* t) {
    return t[0] > -PLAN_GOAL_LIMIT && t[0] < PLAN_GOAL_LIMIT && t[1] > -PLAN_GOAL_LIMIT && t[1] < PLAN_GOAL_LIMIT && t[2] >= -1 && t[2] < POSE_HEADINGS;
}

// the byte of CF from a footprint cost F (-1, or 0..254)
MC_FN uint8_t pose_cf(int32_t f) { return f < 0 ? POSE_CF_OUTSIDE : (uint8_t)f; }

// 0: impassable
MC_FN uint16_t pose_price(int32_t neutral, int32_t stop_cost, uint8_t cf) {
    return ((int32_t)cf < stop_cost && (int32_t)cf <= POSE_MAX_CF) ? (uint16_t)(neutral + (int32_t)cf) : (uint16_t)0;
}

// where move m out of (a, b, d) arrives
MC_FN void pose_arrival(int32_t a, int32_t b, int32_t d, int32_t m, int32_t* va, int32_t* vb, int32_t* vd) {
    const int32_t s = m <= PM_RIGHT ? 1 : (m == PM_REVERSE ? -1 : 0);
    *va = a + s * step_da(d), *vb = b + s * step_db(d);
    *vd = (m == PM_LEFT || m == PM_SPIN_LEFT) ? ((d + 1) & 7) : ((m == PM_RIGHT || m == PM_SPIN_RIGHT) ? ((d + 7) & 7) : d);
}

// The weight of move m out of the state (a, b, d), whose price pu is not 0; 0: the move does not exist.  `price(a, b, d)` is the
// price of a state, 0 for one that is impassable or outside the window.
template <class Price>
MC_FN uint32_t move_weight(const PoseParams& p, const Price& price, int32_t a, int32_t b, int32_t d, uint32_t pu, int32_t m) {
    int32_t va, vb, vd;
    pose_arrival(a, b, d, m, &va, &vb, &vd);
    if (m >= PM_SPIN_LEFT) return (p.spin >= 1 && price(va, vb, vd) != 0) ? (uint32_t)p.spin : 0u;
    if (m == PM_REVERSE && p.reverse < 0) return 0;
    const uint32_t pv = price(va, vb, vd);
    if (pv == 0) return 0;
    if ((d & 1) && (price(va, b, d) == 0 || price(a, vb, d) == 0)) return 0;
    const uint32_t extra = m == PM_FORWARD ? 0u : (m == PM_REVERSE ? (uint32_t)p.reverse : (uint32_t)p.turn);
    return ((d & 1) ? 7u : 5u) * (pu + pv) + extra;
}

// PDIR of the state (a, b, d) with price pu (not 0) from the finished PPOT: `pot(a, b, d)` is read only where the move exists
template <class Price, class Pot>
MC_FN uint8_t pdir_of(const PoseParams& p, const Price& price, const Pot& pot, int32_t a, int32_t b, int32_t d, uint32_t pu, int32_t own) {
    if (own == 0) return PDIR_GOAL;
    if (own == PLAN_FAR) return PDIR_NONE;
    uint32_t best = 0xFFFFFFFFu;
    uint8_t dir = PDIR_NONE;
    for (int32_t m = 0; m < POSE_MOVES; m++) {
        const uint32_t w = move_weight(p, price, a, b, d, pu, m);
        if (w == 0) continue;
        int32_t va, vb, vd;
        pose_arrival(a, b, d, m, &va, &vb, &vd);
        const uint32_t c = (uint32_t)pot(va, vb, vd) + w;
        if (c < best) best = c, dir = (uint8_t)m;
    }
    return dir;
}

// ---- the whole window on the host ------------------------------------------------------------------------------------------
struct PoseWindowPrice {
    const uint16_t* p;
    int32_t nx, nz;
    MC_FN uint32_t operator()(int32_t a, int32_t b, int32_t d) const {
        return a >= 0 && a < nx && b >= 0 && b < nz ? p[((size_t)d * (size_t)nz + (size_t)b) * (size_t)nx + (size_t)a] : 0u;
    }
};
struct PoseWindowPot {
    const int32_t* p;
    int32_t nx, nz;
    MC_FN int32_t operator()(int32_t a, int32_t b, int32_t d) const { return p[((size_t)d * (size_t)nz + (size_t)b) * (size_t)nx + (size_t)a]; }
};

// CF [8 * nz * nx] from cost [nz * nx] and the footprint table (offs, start) of m headings per octant
inline void pose_cf_window(int32_t nx, int32_t nz, const uint8_t* cost, const int32_t* offs, const int64_t* start, int32_t m, int32_t unknown_cost,
                           uint8_t* cf) {
    for (int32_t d = 0; d < POSE_HEADINGS; d++) {
        const int64_t at = start[d * m], n = start[d * m + 1] - at;
        for (int32_t b = 0; b < nz; b++)
            for (int32_t a = 0; a < nx; a++)
                cf[((size_t)d * (size_t)nz + (size_t)b) * (size_t)nx + (size_t)a] = pose_cf(footprint_cost(cost, nx, nz, a, b, offs + 2 * at, n, unknown_cost));
    }
}

// cf [8 * nz * nx] and n goal triples (ga, gb, d) as global cells under the offsets (oa, ob) -> pot, dir [8 * nz * nx] (dir may be
// null); returns the number of goal states that count (inside the window, passable, not a duplicate of an earlier one).  A heap
// Dijkstra over the reversed graph: the states that have a move INTO the popped state are found among the six places such a move can
// start from, each checked by move_weight itself.
inline int64_t pose_window(const PoseParams& p, int32_t stop_cost, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cf,
                           const int32_t* goals, int32_t n, int32_t* pot, uint8_t* dir) {
    const size_t cells = (size_t)nx * (size_t)nz, states = cells * POSE_HEADINGS;
    std::vector<uint16_t> price(states);
    for (size_t i = 0; i < states; i++) price[i] = pose_price(p.neutral, stop_cost, cf[i]), pot[i] = PLAN_FAR;
    const PoseWindowPrice P{price.data(), nx, nz};
    typedef std::pair<uint32_t, uint32_t> Item;   // (PPOT, state)
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    int64_t counted = 0;
    for (int32_t k = 0; k < n; k++) {
        const int64_t a = (int64_t)goals[3 * k] - oa, b = (int64_t)goals[3 * k + 1] - ob;
        const int32_t gd = goals[3 * k + 2];
        if (a < 0 || a >= nx || b < 0 || b >= nz) continue;
        for (int32_t d = gd < 0 ? 0 : gd; d <= (gd < 0 ? POSE_HEADINGS - 1 : gd); d++) {
            const size_t i = ((size_t)d * (size_t)nz + (size_t)b) * (size_t)nx + (size_t)a;
            if (price[i] == 0 || pot[i] == 0) continue;
            pot[i] = 0, counted++;
            heap.push(Item(0u, (uint32_t)i));
        }
    }
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        const uint32_t i = it.second;
        if (it.first != (uint32_t)pot[i]) continue;   // a stale entry
        const int32_t d = (int32_t)(i / (uint32_t)cells), c = (int32_t)(i - (uint32_t)d * (uint32_t)cells);
        const int32_t b = c / nx, a = c - b * nx;
        for (int32_t m = 0; m < POSE_MOVES; m++) {
            // u with move m into (a, b, d): its heading from the arrival's, its cell one step against its own heading
            const int32_t ud = (m == PM_LEFT || m == PM_SPIN_LEFT) ? ((d + 7) & 7) : ((m == PM_RIGHT || m == PM_SPIN_RIGHT) ? ((d + 1) & 7) : d);
            const int32_t s = m <= PM_RIGHT ? 1 : (m == PM_REVERSE ? -1 : 0);
            const int32_t ua = a - s * step_da(ud), ub = b - s * step_db(ud);
            const uint32_t pu = P(ua, ub, ud);
            if (pu == 0) continue;
            const uint32_t w = move_weight(p, P, ua, ub, ud, pu, m);
            if (w == 0) continue;
            const size_t j = ((size_t)ud * (size_t)nz + (size_t)ub) * (size_t)nx + (size_t)ua;
            const uint32_t cnd = candidate(it.first, w, (uint32_t)p.max_cost);
            if (cnd < (uint32_t)pot[j]) pot[j] = (int32_t)cnd, heap.push(Item(cnd, (uint32_t)j));
        }
    }
    if (dir) {
        const PoseWindowPot V{pot, nx, nz};
        for (int32_t d = 0; d < POSE_HEADINGS; d++)
            for (int32_t b = 0; b < nz; b++)
                for (int32_t a = 0; a < nx; a++) {
                    const size_t i = ((size_t)d * (size_t)nz + (size_t)b) * (size_t)nx + (size_t)a;
                    dir[i] = price[i] ? pdir_of(p, P, V, a, b, d, price[i], pot[i]) : PDIR_NONE;
                }
    }
    return counted;
}

// the walk over a PDIR field from the window state (a, b, d): the number of poses of the path, the first min(that, cap) of them
// written as (global cell, rollout heading d m); 0: the state is outside the window, or PDIR does not lead to a goal within
// 8 nx nz states
inline int64_t pose_walk(int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t m, const uint8_t* dir, int32_t a, int32_t b, int32_t d,
                         int32_t* poses, int64_t cap) {
    if (a < 0 || a >= nx || b < 0 || b >= nz || d < 0 || d >= POSE_HEADINGS) return 0;
    const int64_t limit = (int64_t)POSE_HEADINGS * (int64_t)nx * (int64_t)nz;
    for (int64_t len = 0; len < limit;) {
        const uint8_t mv = dir[((size_t)d * (size_t)nz + (size_t)b) * (size_t)nx + (size_t)a];
        if (mv > PDIR_GOAL || (mv >= POSE_MOVES && mv != PDIR_GOAL)) return 0;
        if (len < cap) poses[3 * len] = oa + a, poses[3 * len + 1] = ob + b, poses[3 * len + 2] = d * m;
        len++;
        if (mv == PDIR_GOAL) return len;
        pose_arrival(a, b, d, mv, &a, &b, &d);
        if (a < 0 || a >= nx || b < 0 || b >= nz) return 0;
    }
    return 0;
}

}  // namespace grid
}  // namespace svh

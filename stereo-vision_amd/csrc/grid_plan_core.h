// The arithmetic of the ground grid's planner (svh_grid_plan_*, include/svh_grid.h, "PLANNING"): from the finished COST
// plane of the window and a set of goal cells a cost-to-go field POT, a direction field DIR and the shortest path from any
// start.  THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_plan_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entries svh_test_grid_plan / svh_test_grid_path, which run the
//     heap Dijkstra below on the host),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_plan_check.cpp,
// and restated in numpy / heapq by tests/grid_plan_ref.py, which tests/test_grid_plan.py pins by hand and against the test
// entries.  Everything is integer arithmetic on the COST plane in logical (window) order; the torus plays no part.
//
// PRICE of a cell from its COST byte c: neutral + c for c in 0..252; neutral + unknown for c = 255 when unknown >= 0;
// impassable (price 0) for 253, 254, and for 255 when unknown < 0.  A price is at most 255 + 252 and fits uint16.
// STEPS d = 0..7 are (da, db) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1): even d crosses an edge, odd d a
// corner.  A step u -> v exists when both cells are inside the window and passable and, for a corner step, the two cells
// that share an edge with both, (a + da, b) and (a, b + db), are passable too.  Its weight is k (price(u) + price(v)), k = 5
// across an edge and 7 across a corner: symmetric, at least 10, at most 7 * 2 * 507 = 7098.
// POT: 0 for a goal cell that is inside the window and passable; for every other passable cell the least sum of weights over
// all step sequences to a goal where that is at most max_cost; PLAN_FAR elsewhere.  Every prefix of a shortest path is
// shorter than the path, so the cap is applied per relaxation: a candidate above max_cost is dropped.  Candidates are
// formed in uint32: a POT is at most 0x7FFFFFFF and a weight at most 7098, so they cannot wrap.
// DIR, a function of POT alone: 8 for POT 0, 9 for POT FAR, else the LOWEST d among the existing steps whose POT(v) + w(u, v)
// is least; that least value is POT(u).  The path from a start follows DIR until it reaches 8; POT falls by at least 10 per
// step, so the walk ends within nx * nz cells.
//
// SCHEDULE INDEPENDENCE.  POT is the unique fixed point of "a goal has 0, every other cell the least candidate not above
// max_cost, else FAR" among the fields whose values are lengths of real step sequences: relaxation only lowers values,
// every value it writes is such a length, and at the fixed point no cell can be lowered -- which is the Bellman equation
// of a graph with positive weights.  So POT, DIR and the path do not depend on the launch shape, the scheduling, the order
// of the goals or how often a tile was relaxed.
#pragma once
#include <stdint.h>

#include <queue>
#include <utility>
#include <vector>

#include "grid_core.h"

namespace svh {
namespace grid {

constexpr int32_t PLAN_FAR = 0x7FFFFFFF;
constexpr int32_t PLAN_MAX_GOALS = 65536;
constexpr int32_t PLAN_GOAL_LIMIT = 1 << 20;       // |ga|, |gb| of a goal are below this
constexpr uint8_t DIR_GOAL = 8, DIR_NONE = 9;
constexpr uint8_t GOAL_R = 255, GOAL_G = 255, GOAL_B = 0;
constexpr uint8_t PATH_R = 255, PATH_G = 255, PATH_B = 255;
enum PlanPlane : int32_t { PL_POT = 0, PL_DIR, PL_PLANES };
enum PathStatus : int32_t { PATH_FOUND = 0, PATH_UNREACHABLE, PATH_BLOCKED, PATH_OUTSIDE };

struct PlanParams {
    int32_t neutral;     // 1..255
    int32_t unknown;     // -1, or 0..252
    int32_t max_cost;    // 1..0x7FFFFFFE
};

MC_FN bool plan_ok(const PlanParams& p) {
    return p.neutral >= 1 && p.neutral <= 255 && p.unknown >= -1 && p.unknown <= 252 && p.max_cost >= 1 && p.max_cost <= 0x7FFFFFFE;
}

// 0: impassable
MC_FN uint16_t price_of(const PlanParams& p, uint8_t c) {
    if (c <= 252) return (uint16_t)(p.neutral + (int32_t)c);
    if (c == COST_NO_INFORMATION && p.unknown >= 0) return (uint16_t)(p.neutral + p.unknown);
    return 0;
}

MC_FN int32_t step_da(int32_t d) { return d == 0 || d == 1 || d == 7 ? 1 : (d >= 3 && d <= 5 ? -1 : 0); }
MC_FN int32_t step_db(int32_t d) { return d >= 1 && d <= 3 ? 1 : (d >= 5 ? -1 : 0); }

// The weight of step d out of the cell (a, b), whose price pu is not 0; 0: the step does not exist.  `price(a, b)` is the
// price of a cell, 0 for one that is impassable or outside the window.
template <class Price>
MC_FN uint32_t step_weight(const Price& price, int32_t a, int32_t b, uint32_t pu, int32_t d) {
    const int32_t da = step_da(d), db = step_db(d);
    const uint32_t pv = price(a + da, b + db);
    if (pv == 0) return 0;
    if (d & 1) {
        if (price(a + da, b) == 0 || price(a, b + db) == 0) return 0;
        return 7u * (pu + pv);
    }
    return 5u * (pu + pv);
}

// one relaxation through a step of weight w (not 0) to a neighbour whose POT is pv: the candidate, PLAN_FAR when dropped
MC_FN uint32_t candidate(uint32_t pv, uint32_t w, uint32_t max_cost) {
    const uint32_t c = pv + w;   // <= 0x7FFFFFFF + 7098
    return c <= max_cost ? c : (uint32_t)PLAN_FAR;
}

// DIR of the cell (a, b) with price pu (not 0) from the finished POT: `pot(a, b)` is read only where the step exists
template <class Price, class Pot>
MC_FN uint8_t dir_of(const Price& price, const Pot& pot, int32_t a, int32_t b, uint32_t pu, int32_t own) {
    if (own == 0) return DIR_GOAL;
    if (own == PLAN_FAR) return DIR_NONE;
    uint32_t best = 0xFFFFFFFFu;
    uint8_t dir = DIR_NONE;
    for (int32_t d = 0; d < 8; d++) {
        const uint32_t w = step_weight(price, a, b, pu, d);
        if (w == 0) continue;
        const uint32_t c = (uint32_t)pot(a + step_da(d), b + step_db(d)) + w;
        if (c < best) best = c, dir = (uint8_t)d;
    }
    return dir;
}

// the colour a goal that counts and a cell of a path are drawn in
MC_FN void colour_plan(bool path, uint8_t* rgb) {
    rgb[0] = path ? PATH_R : GOAL_R, rgb[1] = path ? PATH_G : GOAL_G, rgb[2] = path ? PATH_B : GOAL_B;
}

// ---- the whole window on the host: a plain heap Dijkstra from all goals at once --------------------------------------------
struct WindowPrice {
    const uint16_t* p;
    int32_t nx, nz;
    MC_FN uint32_t operator()(int32_t a, int32_t b) const { return a >= 0 && a < nx && b >= 0 && b < nz ? p[(size_t)b * (size_t)nx + (size_t)a] : 0u; }
};
struct WindowPot {
    const int32_t* p;
    int32_t nx;
    MC_FN int32_t operator()(int32_t a, int32_t b) const { return p[(size_t)b * (size_t)nx + (size_t)a]; }
};

// cost [nz * nx] and n goals as global cells (ga, gb) under the offsets (oa, ob) -> pot, dir [nz * nx]; returns the number
// of goals that count (inside the window, passable, not a duplicate of an earlier one)
inline int32_t plan_window(const PlanParams& p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost,
                           const int32_t* goals, int32_t n, int32_t* pot, uint8_t* dir) {
    const size_t cells = (size_t)nx * (size_t)nz;
    std::vector<uint16_t> price(cells);
    for (size_t i = 0; i < cells; i++) price[i] = price_of(p, cost[i]), pot[i] = PLAN_FAR;
    const WindowPrice P{price.data(), nx, nz};
    typedef std::pair<uint32_t, uint32_t> Item;   // (POT, cell)
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    int32_t counted = 0;
    for (int32_t k = 0; k < n; k++) {
        const int64_t a = (int64_t)goals[2 * k] - oa, b = (int64_t)goals[2 * k + 1] - ob;
        if (a < 0 || a >= nx || b < 0 || b >= nz) continue;
        const size_t i = (size_t)b * (size_t)nx + (size_t)a;
        if (price[i] == 0 || pot[i] == 0) continue;
        pot[i] = 0, counted++;
        heap.push(Item(0u, (uint32_t)i));
    }
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        const uint32_t i = it.second;
        if (it.first != (uint32_t)pot[i]) continue;   // a stale entry
        const int32_t b = (int32_t)(i / (uint32_t)nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)nx);
        for (int32_t d = 0; d < 8; d++) {
            const uint32_t w = step_weight(P, a, b, price[i], d);   // symmetric: the step back exists with the same weight
            if (w == 0) continue;
            const size_t j = (size_t)(b + step_db(d)) * (size_t)nx + (size_t)(a + step_da(d));
            const uint32_t c = candidate(it.first, w, (uint32_t)p.max_cost);
            if (c < (uint32_t)pot[j]) pot[j] = (int32_t)c, heap.push(Item(c, (uint32_t)j));
        }
    }
    if (dir) {
        const WindowPot V{pot, nx};
        for (int32_t b = 0; b < nz; b++)
            for (int32_t a = 0; a < nx; a++) {
                const size_t i = (size_t)b * (size_t)nx + (size_t)a;
                dir[i] = dir_of(P, V, a, b, price[i], pot[i]);
            }
    }
    return counted;
}

// the walk over a DIR plane from the window cell (a, b): the number of cells of the path, the first min(that, cap) of them
// written as global cells; 0: the cell is outside the window, or DIR does not lead to a goal within nx * nz cells
inline int64_t walk_window(int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* dir, int32_t a, int32_t b, int32_t* cells,
                           int64_t cap) {
    if (a < 0 || a >= nx || b < 0 || b >= nz) return 0;
    const int64_t limit = (int64_t)nx * (int64_t)nz;
    for (int64_t len = 0; len < limit;) {
        const uint8_t d = dir[(size_t)b * (size_t)nx + (size_t)a];
        if (d > DIR_GOAL) return 0;
        if (len < cap) cells[2 * len] = oa + a, cells[2 * len + 1] = ob + b;
        len++;
        if (d == DIR_GOAL) return len;
        a += step_da(d), b += step_db(d);
        if (a < 0 || a >= nx || b < 0 || b >= nz) return 0;
    }
    return 0;
}

}  // namespace grid
}  // namespace svh

// The arithmetic of the ground grid's exploration layer (svh_grid_*explore*, svh_grid_view_gain, svh_grid_view_mask,
// svh_grid_render_view; include/svh_grid.h, "EXPLORATION"): what a vehicle standing on a cell would see of the unexplored ground,
// what it costs to get there, and which frontier is the best to drive to.  THE CONTRACT IS THIS ARITHMETIC.  Compiled from this
// one header by
//   * hipcc into the kernels of csrc/grid_explore_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entry svh_test_grid_explore, which runs explore_window below),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_explore_check.cpp,
// and restated in numpy and plain Python by tests/grid_explore_ref.py, which tests/test_grid_explore.py pins by hand and against
// the test entry.  Everything is integer arithmetic on the finished STATE and COST planes in logical (window) order; the torus
// plays no part.
//
// RANGE.  R = (int)floorf(range / cell), the quotient IEEE's and compared as a float before it becomes an integer; R lies in
// 1..EXPLORE_MAX_R = 128.
// RAYS.  From a viewpoint, the window cell (va, vb), one ray goes to each of the 8 R offsets (dx, dz) on the perimeter of the
// square [-R, R]^2; ray r = 0 .. 8 R - 1 has, with side = r / (2 R) and t = r % (2 R), the offset (-R + t, -R), (R, -R + t),
// (R - t, R), (-R, R - t) for side 0, 1, 2, 3.  For k = 1 .. R the ray visits the offset (sx, sz) = (rdiv(k dx, R), rdiv(k dz, R)):
// the line of grid_core.h (line_step with n = R; |k dx| <= 2^14).  One of |dx|, |dz| is R, so that coordinate of the offset is
// +-k: a ray never visits the viewpoint's own cell, and |sx|, |sz| <= R.  The ray ENDS before the first k at which
//   * sx^2 + sz^2 > R^2, or
//   * the cell (va + sx, vb + sz) lies outside the window, or
//   * the cell's class (bits 0-1 of STATE) is obstacle.
// Only obstacle cells block: unknown cells, drops, steep cells and the lethal inflation of the cost map do not.  Only VISITED
// cells block: a viewpoint that is itself an obstacle cell still casts its rays.  A ray is a sequence of cells, not a swept
// segment: A DIAGONAL STEP BETWEEN TWO OBSTACLE CELLS PASSES -- from (0, 0) to (1, 1) with obstacles on (1, 0) and (0, 1) the
// ray goes on, because neither of the two is a cell it visits.
// VIEW, one byte per window cell for one viewpoint: VIEW_NONE 0 no ray visits the cell (the viewpoint's own cell included),
// VIEW_VISITED 1 a ray visits it, VIEW_COUNTED 2 a ray visits it and it is UNEXPLORED: unexplored_state() of grid_front_core.h
// under the frontier parameters in force.  The value of a visited cell is a function of the cell alone, so every ray that
// visits it writes the same byte.
// GAIN of a viewpoint: the number of cells whose VIEW is 2, each counted once however many rays visit it; -1 for a viewpoint
// outside the window.  In a window without obstacles the visited set is exactly the disc 0 < sx^2 + sz^2 <= R^2 clipped to the
// window (checked for R = 1..39, 63, 64, 65, 127, 128: 4 / 12 / 28 / 196 / 3208 / 51432 cells for R = 1 / 2 / 3 / 8 / 32 / 128).
// REACH of a cell from a start cell: POT of grid_plan_core.h under the plan parameters in force with the start as the only goal,
// read at the cell.  Step weights and the corner rule are symmetric, so it is the cost of the path from the start to the cell.
// PLAN_FAR when the start is outside the window or impassable, the cell unreachable or the cost beyond max_cost.
// RANKING.  For each kept frontier component (grid_front_core.h), the first EXPLORE_MAX_RECORDS in ascending label, one record of
// EXPLORE_REC int32: label, rep_ga, rep_gb, GAIN of the representative, REACH of the representative.  A record is FEASIBLE iff
// reach != PLAN_FAR and gain >= min_gain; its int64 score is w_reach * reach - w_gain * gain (|.| < 2^48), EXPLORE_INFEASIBLE
// (INT64_MAX) when it is not feasible.  BEST is the feasible record with the least (score, index), -1 when there is none.
//
// SCHEDULE INDEPENDENCE.  GAIN is the size of a set (the union of what the rays visit), VIEW a function of that set and the
// cell, REACH a value of the planner's unique fixed point, the score a function of the two and BEST the minimum of unique keys:
// no byte depends on launch shape or scheduling.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "grid_core.h"
#include "grid_front_core.h"
#include "grid_plan_core.h"

namespace svh {
namespace grid {

constexpr int32_t EXPLORE_MAX_R = 128;
constexpr int32_t EXPLORE_REC = 5;                      // int32 per record
constexpr int32_t EXPLORE_MAX_RECORDS = 65536;
constexpr int32_t EXPLORE_MAX_MIN_GAIN = 1 << 26;       // 8192^2
constexpr int32_t EXPLORE_MAX_WEIGHT = 65535;
constexpr int64_t EXPLORE_INFEASIBLE = 0x7FFFFFFFFFFFFFFFll;
enum ExploreRec : int32_t { ER_LABEL = 0, ER_REP_GA, ER_REP_GB, ER_GAIN, ER_REACH };
enum ViewCell : uint8_t { VIEW_NONE = 0, VIEW_VISITED = 1, VIEW_COUNTED = 2 };
enum ExploreStat : int32_t { ES_RECORDS = 0, ES_FEASIBLE, ES_FIELDS, ES_LAUNCHES, ES_WORDS };
constexpr uint8_t VIEW_R = 255, VIEW_G = 0, VIEW_B = 255;

struct ExploreParams {
    float range;         // metres; finite, > 0
    int32_t min_gain;    // 0..2^26
    int32_t w_gain;      // 0..65535
    int32_t w_reach;     // 0..65535
};

MC_FN bool explore_ok(const ExploreParams& p) {
    return finite_f(p.range) && p.range > 0.f && p.min_gain >= 0 && p.min_gain <= EXPLORE_MAX_MIN_GAIN && p.w_gain >= 0 &&
           p.w_gain <= EXPLORE_MAX_WEIGHT && p.w_reach >= 0 && p.w_reach <= EXPLORE_MAX_WEIGHT;
}

// R for a cell side; 0: outside 1..EXPLORE_MAX_R
MC_FN int32_t explore_range(float range, float cell) {
    const float q = floorf(div_rn(range, cell));
    return (q >= 1.f && q <= (float)EXPLORE_MAX_R) ? (int32_t)q : 0;
}

// the offset that ray r = 0 .. 8 R - 1 goes to
MC_FN void ray_end(int32_t R, int32_t r, int32_t* dx, int32_t* dz) {
    const int32_t side = r / (2 * R), t = r - side * 2 * R;
    *dx = side == 0 ? -R + t : (side == 1 ? R : (side == 2 ? R - t : -R));
    *dz = side == 0 ? -R : (side == 1 ? -R + t : (side == 2 ? R : R - t));
}

// Ray r of the viewpoint (va, vb), a window cell: visit(sx, sz, state byte) for every cell it visits, in the order of k.
// `state` is read only inside the window.
template <class Visit>
MC_FN void view_ray(int32_t R, int32_t nx, int32_t nz, const uint8_t* state, int32_t va, int32_t vb, int32_t r, const Visit& visit) {
    int32_t dx, dz;
    ray_end(R, r, &dx, &dz);
    for (int32_t k = 1; k <= R; k++) {
        int32_t sx, sz;
        line_step(dx, dz, R, k, &sx, &sz);
        if (sx * sx + sz * sz > R * R) return;
        const int32_t a = va + sx, b = vb + sz;
        if (a < 0 || a >= nx || b < 0 || b >= nz) return;
        const uint8_t s = state[(size_t)b * (size_t)nx + (size_t)a];
        if ((s & 3) == C_OBSTACLE) return;
        visit(sx, sz, s);
    }
}

// the VIEW byte of a visited cell
MC_FN uint8_t view_value(const FrontParams& f, uint8_t state) { return unexplored_state(f, state) ? VIEW_COUNTED : VIEW_VISITED; }

// feasible: the score; else EXPLORE_INFEASIBLE
MC_FN int64_t explore_score(const ExploreParams& p, int32_t gain, int32_t reach) {
    if (reach == PLAN_FAR || gain < p.min_gain) return EXPLORE_INFEASIBLE;
    return (int64_t)p.w_reach * (int64_t)reach - (int64_t)p.w_gain * (int64_t)gain;
}

// what svh_grid_render_view draws over the image of svh_grid_render_frontiers: the viewpoint white, a counted cell (255, 0, 255),
// a visited cell brightened half way to white (c + (255 - c) / 2 per byte); false: the cell keeps its colour
MC_FN bool colour_view(uint8_t view, bool viewpoint, uint8_t* rgb) {
    if (viewpoint) rgb[0] = rgb[1] = rgb[2] = 255;
    else if (view == VIEW_COUNTED) rgb[0] = VIEW_R, rgb[1] = VIEW_G, rgb[2] = VIEW_B;
    else if (view == VIEW_VISITED)
        for (int32_t c = 0; c < 3; c++) rgb[c] = (uint8_t)(rgb[c] + (255 - rgb[c]) / 2);
    else return false;
    return true;
}

// ---- the host forms --------------------------------------------------------------------------------------------------------
// the VIEW plane [nz * nx] of the window viewpoint (va, vb), which is inside the window; returns its GAIN
inline int32_t view_window(const FrontParams& f, int32_t R, int32_t nx, int32_t nz, const uint8_t* state, int32_t va, int32_t vb, uint8_t* view) {
    const size_t cells = (size_t)nx * (size_t)nz;
    for (size_t i = 0; i < cells; i++) view[i] = VIEW_NONE;
    int32_t gain = 0;
    for (int32_t r = 0; r < 8 * R; r++)
        view_ray(R, nx, nz, state, va, vb, r, [&](int32_t sx, int32_t sz, uint8_t s) {
            uint8_t& v = view[(size_t)(vb + sz) * (size_t)nx + (size_t)(va + sx)];
            const uint8_t now = view_value(f, s);
            gain += (v == VIEW_NONE && now == VIEW_COUNTED) ? 1 : 0;
            v = now;
        });
    return gain;
}

// GAIN of n global cells (ga, gb) under the offsets (oa, ob): the counted cells are marked in a square of (2 R + 1)^2 bytes
inline void gain_window(const FrontParams& f, int32_t R, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state, const int32_t* cells,
                        int64_t n, int32_t* out) {
    const int32_t side = 2 * R + 1;
    std::vector<uint8_t> seen((size_t)side * (size_t)side);
    for (int64_t i = 0; i < n; i++) {
        const int64_t va = (int64_t)cells[2 * i] - oa, vb = (int64_t)cells[2 * i + 1] - ob;
        if (va < 0 || va >= nx || vb < 0 || vb >= nz) {
            out[i] = -1;
            continue;
        }
        std::fill(seen.begin(), seen.end(), (uint8_t)0);
        int32_t gain = 0;
        for (int32_t r = 0; r < 8 * R; r++)
            view_ray(R, nx, nz, state, (int32_t)va, (int32_t)vb, r, [&](int32_t sx, int32_t sz, uint8_t s) {
                uint8_t& m = seen[(size_t)(sz + R) * (size_t)side + (size_t)(sx + R)];
                gain += (!m && unexplored_state(f, s)) ? 1 : 0;
                m = 1;
            });
        out[i] = gain;
    }
}

// The ranking of a whole window on the host: the frontiers by front_window, the reach field by plan_window (the heap Dijkstra)
// from the start, a global cell, the gains by gain_window.  The records (EXPLORE_REC each) and the scores of the first
// EXPLORE_MAX_RECORDS kept components are appended; *feasible counts the feasible ones; returns BEST.
inline int32_t explore_window(const FrontParams& f, const PlanParams& pl, const ExploreParams& e, int32_t R, int32_t nx, int32_t nz, int32_t oa,
                              int32_t ob, const uint8_t* state, const uint8_t* cost, int32_t start_ga, int32_t start_gb, std::vector<int32_t>* recs,
                              std::vector<int64_t>* scores, int64_t* feasible) {
    const size_t cells = (size_t)nx * (size_t)nz;
    std::vector<uint8_t> flags(cells);
    std::vector<int32_t> label(cells), front, pot(cells);
    front_window(f, nx, nz, oa, ob, state, cost, flags.data(), label.data(), &front, nullptr);
    const int32_t start[2] = {start_ga, start_gb};
    plan_window(pl, nx, nz, oa, ob, cost, start, 1, pot.data(), nullptr);
    const size_t kept = front.size() / FRONT_REC, n = kept < (size_t)EXPLORE_MAX_RECORDS ? kept : (size_t)EXPLORE_MAX_RECORDS;
    std::vector<int32_t> reps(2 * n), gains(n);
    for (size_t k = 0; k < n; k++) reps[2 * k] = front[k * FRONT_REC + FR_REP_GA], reps[2 * k + 1] = front[k * FRONT_REC + FR_REP_GB];
    gain_window(f, R, nx, nz, oa, ob, state, reps.data(), (int64_t)n, gains.data());
    int32_t best = -1;
    int64_t best_score = EXPLORE_INFEASIBLE, n_feasible = 0;
    for (size_t k = 0; k < n; k++) {
        const int32_t reach = pot[(size_t)(reps[2 * k + 1] - ob) * (size_t)nx + (size_t)(reps[2 * k] - oa)];   // a representative is inside
        const int64_t s = explore_score(e, gains[k], reach);
        if (s != EXPLORE_INFEASIBLE) {
            n_feasible++;
            if (best < 0 || s < best_score) best = (int32_t)k, best_score = s;   // ascending k: the first of equal scores stays
        }
        if (recs) {
            const int32_t r[EXPLORE_REC] = {front[k * FRONT_REC + FR_LABEL], reps[2 * k], reps[2 * k + 1], gains[k], reach};
            recs->insert(recs->end(), r, r + EXPLORE_REC);
        }
        if (scores) scores->push_back(s);
    }
    if (feasible) *feasible = n_feasible;
    return best;
}

}  // namespace grid
}  // namespace svh

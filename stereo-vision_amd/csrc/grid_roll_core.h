// The arithmetic of the ground grid's rollouts (svh_grid_set_roll, svh_grid_footprint_cost, svh_grid_roll_*, include/svh_grid.h,
// "ROLLOUT"): the worst COST under an oriented vehicle rectangle at a pose, and K candidate pose sequences cut, summed up, scored
// and the best picked.  THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_roll_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the footprint table of svh_grid_set_roll, and the test entries
//     svh_test_grid_roll / svh_test_grid_roll_table / svh_test_grid_roll_heading, which run the loops below on the host),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_roll_check.cpp,
// and restated in numpy by tests/grid_roll_ref.py, which tests/test_grid_roll.py pins by hand and against the test entries.
// Everything but the heading of a direction (fp32, one rounding per operation) and the footprint table (double, on the host, once
// per svh_grid_set_roll) is integer arithmetic on the finished COST and POT planes in logical (window) order.
//
// HEADINGS are integer direction vectors; no trigonometric function appears.  With m = headings_m in 1..32 there are H = 8 m
// headings: heading k is the vector (ux, uz) in (lateral a, forward b) on the perimeter of the square [-m, m]^2, counter-clockwise
// from (m, 0): (m, k) for k in 0..m, (2m - k, m) for m..3m, (-m, 4m - k) for 3m..5m, (k - 6m, -m) for 5m..7m, (m, k - 8m) for
// 7m..8m.  Straight ahead is k = 2m.  The heading of a direction (ua, ub): if |ua| >= |ub|, q = (int)rintf(div_rn(ub * (float)m,
// |ua|)) and k = (q + 8m) mod 8m for ua > 0, 4m - q for ua < 0; otherwise q = (int)rintf(div_rn(ua * (float)m, |ub|)) and k = 2m -
// q for ub > 0, 6m + q for ub < 0.  No heading: a component that is not finite, both zero, or a quotient that is not within
// [-m, m] (the product overflowed) -- decided on the float before the conversion.
//
// THE FOOTPRINT TABLE has one list of cell offsets (da, db) per heading; the vehicle's reference point is taken at the centre of
// its cell.  With c = (double)cell, h = 0.5 c, rt = sqrt((double)(ux ux + uz uz)), l = da ux + db uz and t = db ux - da uz (integers)
// the offset is in the list iff  (double)l c <= ((double)front + h) rt,  -(double)l c <= ((double)rear + h) rt  and
// fabs((double)t) c <= ((double)half_width + h) rt, each product one double operation.  (0, 0) is always in; a point vehicle covers
// exactly one cell at every heading.  Offsets are searched in [-R, R]^2, R = (int)ceil((max(front, rear) + half_width + c) / c) in
// 1..128 -- |(da, db)| = sqrt(l^2 + t^2) / rt <= (front + half_width + c) / c, so nothing lies beyond.  A list is ascending by (db, da).
//
// FOOTPRINT COST F of a pose (ga, gb, k): -1 if a footprint cell lies outside the window (or k is no heading), else the maximum over
// the footprint cells of r(COST), r(c) = c for 0..254 and r(255) = unknown_cost.
//
// CANDIDATES: S sets x K candidates x T poses of (dga, dgb, k), offsets from an anchor cell and an absolute heading; k = -1 ends a
// candidate, its length n_c is the number of poses before the first -1.  SCORING a set at an anchor: F_t at every t < n_c; the cut is
// the first t with F_t = -1 (status 2) or F_t >= stop_cost (status 1), else the candidate is complete (0); n_c = 0 is status 3.  L is
// the number of poses before the cut.  The record: L, status, maxF over the L poses (-1 for L = 0), sumF over them, pot_end = POT at
// the reference cell of pose L - 1 (PLAN_FAR for L = 0 or w_pot = 0, when POT is not read).  Feasible: L >= 1 and (w_pot = 0 or
// pot_end != FAR).  Score (int64): w_pot pot_end + w_cost sumF + w_cut (n_c - L), INT64_MAX when infeasible.  The best is the
// feasible candidate with the least (score, index), -1 if none.  F is a maximum, sumF an integer sum, the cut a first index and the
// best the minimum of unique keys: nothing depends on order, launch shape or scheduling.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "grid_core.h"
#include "grid_plan_core.h"

namespace svh {
namespace grid {

constexpr int32_t ROLL_MAX_M = 32;                   // headings_m
constexpr int32_t ROLL_MAX_R = 128;                  // the reach of the footprint in cells
constexpr int32_t ROLL_MAX_T = 1024, ROLL_MAX_K = 65536;
constexpr int64_t ROLL_MAX_TABLE = (int64_t)1 << 22; // S * K * T
constexpr int32_t ROLL_MAX_OFFSET = 16384;           // |dga|, |dgb|
constexpr int32_t ROLL_REC = 5;
constexpr int64_t ROLL_INFEASIBLE = 0x7FFFFFFFFFFFFFFFll;
constexpr int32_t ROLL_OUTSIDE = 256;                // what a cell outside the window reads as under the maximum: above every r(c)
enum RollField : int32_t { RR_LEN = 0, RR_STATUS, RR_MAXF, RR_SUMF, RR_POT_END };
enum RollStatus : int32_t { ROLL_COMPLETE = 0, ROLL_CUT_COST, ROLL_CUT_WINDOW, ROLL_EMPTY };
constexpr uint8_t ROLL_R = 0, ROLL_G = 192, ROLL_B = 255;
constexpr uint8_t ROLL_BEST_R = 255, ROLL_BEST_G = 255, ROLL_BEST_B = 255;

struct RollParams {
    float front, rear, half_width;   // finite, >= 0
    int32_t m;                       // 1..32
    int32_t stop_cost;               // 1..255
    int32_t unknown_cost;            // 0..254
    int32_t w_pot, w_cost, w_cut;    // 0..65535
};

MC_FN bool roll_ok(const RollParams& p) {
    return finite_f(p.front) && p.front >= 0.f && finite_f(p.rear) && p.rear >= 0.f && finite_f(p.half_width) && p.half_width >= 0.f &&
           p.m >= 1 && p.m <= ROLL_MAX_M && p.stop_cost >= 1 && p.stop_cost <= 255 && p.unknown_cost >= 0 && p.unknown_cost <= 254 &&
           p.w_pot >= 0 && p.w_pot <= 65535 && p.w_cost >= 0 && p.w_cost <= 65535 && p.w_cut >= 0 && p.w_cut <= 65535;
}

// the vector of heading k, 0 <= k < 8 m
MC_FN void heading_vec(int32_t m, int32_t k, int32_t* ux, int32_t* uz) {
    if (k <= m) *ux = m, *uz = k;
    else if (k <= 3 * m) *ux = 2 * m - k, *uz = m;
    else if (k <= 5 * m) *ux = -m, *uz = 4 * m - k;
    else if (k <= 7 * m) *ux = k - 6 * m, *uz = -m;
    else *ux = m, *uz = k - 8 * m;
}

// the heading of a direction, -1: none
MC_FN int32_t heading_of(int32_t m, float ua, float ub) {
    if (!(finite_f(ua) && finite_f(ub)) || (ua == 0.f && ub == 0.f)) return -1;
    const float aa = fabsf(ua), ab = fabsf(ub), fm = (float)m;
    if (aa >= ab) {
        const float qf = rintf(div_rn(ub * fm, aa));
        if (!(fabsf(qf) <= fm)) return -1;
        const int32_t q = (int32_t)qf;
        return ua > 0.f ? (q + 8 * m) % (8 * m) : 4 * m - q;
    }
    const float qf = rintf(div_rn(ua * fm, ab));
    if (!(fabsf(qf) <= fm)) return -1;
    const int32_t q = (int32_t)qf;
    return ub > 0.f ? 2 * m - q : 6 * m + q;
}

// the reach R of the footprint for a cell side, 0: outside 1..128 (compared as a double before it becomes an integer)
inline int32_t roll_reach(const RollParams& p, float cell) {
    const double c = (double)cell;
    const double r = ceil(((double)(p.front > p.rear ? p.front : p.rear) + (double)p.half_width + c) / c);
    return (r >= 1.0 && r <= (double)ROLL_MAX_R) ? (int32_t)r : 0;
}

// is the offset (da, db) under the vehicle at the heading (ux, uz)?  Host only: the device reads the table
inline bool roll_covers(const RollParams& p, float cell, int32_t ux, int32_t uz, int32_t da, int32_t db) {
    const double c = (double)cell, h = 0.5 * c, rt = sqrt((double)(ux * ux + uz * uz));
    const int32_t l = da * ux + db * uz, t = db * ux - da * uz;   // |.| <= 2 * 128 * 32
    return (double)l * c <= ((double)p.front + h) * rt && -(double)l * c <= ((double)p.rear + h) * rt &&
           fabs((double)t) * c <= ((double)p.half_width + h) * rt;
}

// The table for a cell side: `offs` holds the lists one after the other as pairs (da, db), `start` H + 1 pair indexes.  Returns R,
// 0 (nothing written): the parameters or the reach are out of range
inline int32_t roll_table(const RollParams& p, float cell, std::vector<int32_t>* offs, std::vector<int64_t>* start) {
    if (!roll_ok(p) || !(finite_f(cell) && cell > 0.f)) return 0;
    const int32_t R = roll_reach(p, cell);
    if (R == 0) return 0;
    const int32_t H = 8 * p.m;
    offs->clear();
    start->assign((size_t)H + 1, 0);
    for (int32_t k = 0; k < H; k++) {
        int32_t ux, uz;
        heading_vec(p.m, k, &ux, &uz);
        for (int32_t db = -R; db <= R; db++)
            for (int32_t da = -R; da <= R; da++)
                if (roll_covers(p, cell, ux, uz, da, db)) offs->push_back(da), offs->push_back(db);
        (*start)[(size_t)k + 1] = (int64_t)(offs->size() / 2);
    }
    return R;
}

MC_FN int32_t roll_cost(uint8_t c, int32_t unknown_cost) { return c == COST_NO_INFORMATION ? unknown_cost : (int32_t)c; }

// what one footprint cell at the window position (a, b) contributes to the maximum
MC_FN int32_t roll_cell(const uint8_t* cost, int32_t nx, int32_t nz, int64_t a, int64_t b, int32_t unknown_cost) {
    if (a < 0 || a >= nx || b < 0 || b >= nz) return ROLL_OUTSIDE;
    return roll_cost(cost[(size_t)b * (size_t)nx + (size_t)a], unknown_cost);
}
// F from the maximum over the footprint cells
MC_FN int32_t roll_f(int32_t worst) { return worst >= ROLL_OUTSIDE ? -1 : worst; }

// F of the pose whose reference cell is the window position (a, b), with the list of its heading: n pairs
MC_FN int32_t footprint_cost(const uint8_t* cost, int32_t nx, int32_t nz, int64_t a, int64_t b, const int32_t* list, int64_t n,
                             int32_t unknown_cost) {
    int32_t worst = 0;
    for (int64_t i = 0; i < n; i++) {
        const int32_t v = roll_cell(cost, nx, nz, a + list[2 * i], b + list[2 * i + 1], unknown_cost);
        worst = v > worst ? v : worst;
    }
    return roll_f(worst);
}

// is pose t cut, and how: 0 no, else the status
MC_FN int32_t roll_cut(int32_t f, int32_t stop_cost) { return f < 0 ? (int32_t)ROLL_CUT_WINDOW : (f >= stop_cost ? (int32_t)ROLL_CUT_COST : 0); }

MC_FN int64_t roll_score(const RollParams& p, int32_t n_c, const int32_t* rec) {
    const int32_t L = rec[RR_LEN];
    if (L < 1 || (p.w_pot != 0 && rec[RR_POT_END] == PLAN_FAR)) return ROLL_INFEASIBLE;
    return (int64_t)p.w_pot * (int64_t)rec[RR_POT_END] + (int64_t)p.w_cost * (int64_t)rec[RR_SUMF] + (int64_t)p.w_cut * (int64_t)(n_c - L);
}

// the length of a candidate: the poses before the first heading of -1
MC_FN int32_t roll_len(const int32_t* cand, int32_t T) {
    int32_t n = 0;
    while (n < T && cand[3 * n + 2] != -1) n++;
    return n;
}

// the colour of a valid pose's reference cell in svh_grid_render_roll
MC_FN void colour_roll(bool best, uint8_t* rgb) {
    rgb[0] = best ? ROLL_BEST_R : ROLL_R, rgb[1] = best ? ROLL_BEST_G : ROLL_G, rgb[2] = best ? ROLL_BEST_B : ROLL_B;
}

// ---- the host loops ---------------------------------------------------------------------------------------------------------
// F of n free poses (ga, gb, k) as global cells under the offsets (oa, ob); a heading outside 0..H-1 gives -1
inline void footprint_window(const RollParams& p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost, const int32_t* offs,
                             const int64_t* start, const int32_t* poses, int64_t n, int32_t* out) {
    for (int64_t i = 0; i < n; i++) {
        const int32_t k = poses[3 * i + 2];
        if (k < 0 || k >= 8 * p.m) {
            out[i] = -1;
            continue;
        }
        out[i] = footprint_cost(cost, nx, nz, (int64_t)poses[3 * i] - oa, (int64_t)poses[3 * i + 1] - ob, offs + 2 * start[k], start[k + 1] - start[k],
                                p.unknown_cost);
    }
}

// One set of K candidates of T poses (`cands`: K * T * 3) at the anchor (ga0, gb0), a global cell: recs (5 K), scores (K), either may
// be null; returns the best.  `pot` is read only when w_pot != 0
inline int32_t roll_window(const RollParams& p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost, const int32_t* pot,
                           const int32_t* offs, const int64_t* start, const int32_t* cands, int32_t K, int32_t T, int32_t ga0, int32_t gb0,
                           int32_t* recs, int64_t* scores) {
    int32_t best = -1;
    int64_t best_score = ROLL_INFEASIBLE;
    for (int32_t c = 0; c < K; c++) {
        const int32_t* cand = cands + (size_t)c * (size_t)T * 3;
        const int32_t n_c = roll_len(cand, T);
        int32_t rec[ROLL_REC] = {0, n_c == 0 ? (int32_t)ROLL_EMPTY : (int32_t)ROLL_COMPLETE, -1, 0, PLAN_FAR};
        for (int32_t t = 0; t < n_c; t++) {
            const int32_t k = cand[3 * t + 2];
            const int64_t a = (int64_t)ga0 + cand[3 * t] - oa, b = (int64_t)gb0 + cand[3 * t + 1] - ob;
            const int32_t f = footprint_cost(cost, nx, nz, a, b, offs + 2 * start[k], start[k + 1] - start[k], p.unknown_cost);
            const int32_t cut = roll_cut(f, p.stop_cost);
            if (cut) {
                rec[RR_STATUS] = cut;
                break;
            }
            rec[RR_LEN] = t + 1;
            rec[RR_MAXF] = f > rec[RR_MAXF] ? f : rec[RR_MAXF];
            rec[RR_SUMF] += f;
            if (p.w_pot != 0) rec[RR_POT_END] = pot[(size_t)b * (size_t)nx + (size_t)a];
        }
        const int64_t s = roll_score(p, n_c, rec);
        if (s < best_score) best_score = s, best = c;   // ascending c: the lower index wins a tie
        if (recs)
            for (int32_t k = 0; k < ROLL_REC; k++) recs[(size_t)c * ROLL_REC + k] = rec[k];
        if (scores) scores[c] = s;
    }
    return best;
}

// the checks of a candidate table against H headings: the sizes, and every pose before a candidate's first -1
inline bool roll_table_ok(const int32_t* table, int64_t S, int64_t K, int64_t T, int32_t H) {
    if (!table || S < 1 || K < 1 || T < 1 || T > ROLL_MAX_T || K > ROLL_MAX_K || S > ROLL_MAX_TABLE || S * K * T > ROLL_MAX_TABLE) return false;
    for (int64_t c = 0; c < S * K; c++) {
        const int32_t* cand = table + c * T * 3;
        for (int64_t t = 0; t < T && cand[3 * t + 2] != -1; t++) {
            const int32_t da = cand[3 * t], db = cand[3 * t + 1], k = cand[3 * t + 2];
            if (k < 0 || k >= H || da < -ROLL_MAX_OFFSET || da > ROLL_MAX_OFFSET || db < -ROLL_MAX_OFFSET || db > ROLL_MAX_OFFSET) return false;
        }
    }
    return true;
}

}  // namespace grid
}  // namespace svh

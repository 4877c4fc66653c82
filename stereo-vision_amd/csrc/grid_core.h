// The arithmetic of the ground grid (svh_grid_*, include/svh_grid.h): the 2.5-D bird's-eye grid over the road plane that
// the accumulated map is binned into -- where a point goes, what a cell accumulates, what a finished cell says and how it
// is coloured.  THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entries svh_test_grid_points / svh_test_grid_finalise, which
//     evaluate every function below on the host),
//   * g++ -fsanitize=undefined into tests/cxx/grid_core_check.cpp, which guards the float-to-integer conversions, and
//     into tests/cxx/grid_line_check.cpp, which runs the line and the offset place() at their extremes,
// and restated in numpy by tests/grid_ref.py, which tests/test_grid.py pins by hand and against the test entries; the
// window's offsets, the line of a ray, the state byte and the local colour (svh_test_grid_points_at / svh_test_grid_line
// / svh_test_grid_local) by tests/grid_local_ref.py and tests/test_grid_local.py; the traversability layer (the kernels of
// csrc/grid_trav_kernels.hip, svh_test_grid_trav / svh_test_grid_cost_table, tests/cxx/grid_trav_check.cpp) by
// tests/grid_trav_ref.py and tests/test_grid_trav.py.
// fp32 in the order written, every operation rounded once (-ffp-contract=off on every build, no fast-math), the
// divisions IEEE's (div_rn), denormals kept.  Every range decision is made on the float BEFORE a conversion to an
// integer: an out-of-range conversion is undefined on the host and saturates on the device.
//
// ORDER INDEPENDENCE.  Every quantity a cell accumulates is an integer under a commutative, associative update: two
// counts (+), two keys (min, max), a sum of heights quantised to 1/1024 (+, int64) and a sum of intensity bytes (+,
// uint64).  The grid after any set of adds therefore depends only on the MULTISET of points, never on their order, the
// launch shape or the scheduling; add(A) then add(B) is add(A ++ B).  The pass count of the rays (below) is one more
// integer sum: it depends only on the multiset of (origin cell, end cell) pairs.
#pragma once
#include <math.h>
#include <stdint.h>

#include "view2d_core.h"   // MC_FN, div_rn, byte_of, disparity_colour, finite_f

namespace svh {
namespace grid {

using view2d::div_rn;
using view2d::finite_f;

constexpr int32_t MAX_SIDE = 8192;                 // nx and nz lie in 1..8192
constexpr float H_LIMIT = 1048576.f;               // a height is binned iff |h| < 2^20: |rintf(h * 1024)| <= 2^30
constexpr uint32_t KMIN_EMPTY = 0xFFFFFFFFu;       // the keys of a cell without a low point; no finite float has them
constexpr uint32_t KMAX_EMPTY = 0u;
constexpr uint32_t NO_CELL = 0xFFFFFFFFu;          // the cell of a point that is outside or unplaced
constexpr uint32_t NAN_BITS = 0x7FC00000u;         // HMIN, HMAX, HMEAN of a cell without a low point
constexpr int32_t OFFSET_LIMIT = (1 << 20) - MAX_SIDE;   // |oa|, |ob| <= this: every global cell of a window is below 2^20
constexpr float CELL_LIMIT = 1048576.f;            // a position has a global cell iff |floorf(...)| < 2^20, both axes

// what becomes of a point
enum Fate : int32_t { LOW = 0, OVERHEAD = 1, OUTSIDE = 2, UNPLACED = 3 };
// planes of svh_grid_get, modes of svh_grid_render, classes of a cell (bits 0-1 of the class byte; bit 7: overhang)
enum Plane : int32_t { P_COUNT = 0, P_OVERHEAD, P_HMIN, P_HMAX, P_HMEAN, P_INTENSITY, P_CLASS, P_PLANES };
enum Mode : int32_t { M_CLASS = 0, M_HEIGHT, M_INTENSITY, M_MODES, M_LOCAL = M_MODES };   // M_LOCAL: svh_grid_render_local only
enum Class : uint8_t { C_UNKNOWN = 0, C_FREE = 1, C_OBSTACLE = 2, C_DROP = 3, C_SEEN = 0x40, C_OVERHANG = 0x80 };
// planes of svh_grid_get_local; the colour of a cell that is unknown and seen in svh_grid_render_local
enum LocalPlane : int32_t { L_PASS = 0, L_STATE, L_PLANES };
constexpr uint8_t SEEN_R = 96, SEEN_G = 112, SEEN_B = 96;

// svh_grid_params with T rounded to float (once, at create)
struct Params {
    int32_t nx, nz;
    float cell, x0, z0;
    float T[12];
    int32_t min_points;
    float step, drop, clearance, h_lo, h_hi;
    int32_t oa = 0, ob = 0;   // the window's offsets in whole cells (svh_grid_scroll): it holds global cells oa .. oa + nx - 1
};

struct Placed {
    int32_t fate;
    uint32_t cell;      // the logical index (gb - ob) * nx + (ga - oa); NO_CELL when outside or unplaced
    uint32_t key;       // LOW: key_of(h)
    int32_t q;          // LOW: rintf(h * 1024)
    uint32_t v;         // LOW: q8(val)
    uint32_t slot;      // where the cell's accumulators lie (slot_at); the logical index while the offsets are zero
};

// what a cell has accumulated
struct Cell {
    int32_t count, overhead;
    uint32_t kmin, kmax;
    int64_t hsum;
    uint64_t vsum;
};

// what a finished cell says: the planes of svh_grid_get besides the two counts
struct Final {
    float hmin, hmax, hmean;
    uint8_t intensity, cls;
};

MC_FN uint32_t bits_of(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
MC_FN float float_of(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// the order-preserving map of a float's bits to uint32: a < b  <=>  key_of(a) < key_of(b) for finite a, b (-0.0 never
// arrives here)
MC_FN uint32_t key_of(float h) {
    const uint32_t b = bits_of(h);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
MC_FN float height_of(uint32_t key) { return float_of((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

// one row of T on (x, y, z, 1)
MC_FN float row(const float* t, float x, float y, float z) { return ((t[0] * x + t[1] * y) + t[2] * z) + t[3]; }

// (uint8)rintf(clamp(val, 0, 1) * 255), 0 for NaN: round-half-even, 127.5 -> 128, 128.5 -> 128
MC_FN uint32_t q8(float val) {
    if (!(val == val)) return 0u;
    const float lo = val < 0.f ? 0.f : val;
    const float hi = lo > 1.f ? 1.f : lo;
    return (uint32_t)rintf(hi * 255.f);
}

// THE WINDOW.  A point's global cell is (ga, gb) = (floorf((a - x0) / cell), floorf((b - z0) / cell)); the window holds
// ga in oa .. oa + nx - 1 and gb in ob .. ob + nz - 1.  |oa|, |ob| <= OFFSET_LIMIT, so every value compared below is an
// integer of magnitude below 2^20 + 2^13 and exact in fp32.  The accumulators are addressed as a torus over the global
// cell, slot = mod(gb, nz) * nx + mod(ga, nx) with the non-negative mod: a scroll (svh_grid_scroll) moves no data, cells
// that stay keep their slot and the strips that enter take the slots of those that left.  The planes that leave the
// object are in logical order.
MC_FN int32_t mod_floor(int32_t v, int32_t n) {
    const int32_t r = v % n;
    return r < 0 ? r + n : r;
}
// window cell (ia, ib) -> slot.  mod(oa + ia, nx) without a division per cell: mod(oa, nx) is the same for every cell
MC_FN uint32_t slot_at(const Params& p, int32_t ia, int32_t ib) {
    int32_t sa = mod_floor(p.oa, p.nx) + ia, sb = mod_floor(p.ob, p.nz) + ib;
    sa = sa >= p.nx ? sa - p.nx : sa;
    sb = sb >= p.nz ? sb - p.nz : sb;
    return (uint32_t)sb * (uint32_t)p.nx + (uint32_t)sa;
}
// logical index -> slot
MC_FN uint32_t slot_of(const Params& p, uint32_t logical) {
    const uint32_t ib = logical / (uint32_t)p.nx;
    return slot_at(p, (int32_t)(logical - ib * (uint32_t)p.nx), (int32_t)ib);
}
MC_FN bool offsets_ok(int32_t oa, int32_t ob) {
    return oa >= -OFFSET_LIMIT && oa <= OFFSET_LIMIT && ob >= -OFFSET_LIMIT && ob <= OFFSET_LIMIT;
}

// the global cell of a position, for svh_grid_cell_of; false: not placeable (not finite, or a cell not below 2^20)
MC_FN bool global_cell(const Params& p, float x, float y, float z, int32_t* ga, int32_t* gb) {
    const float a = row(p.T, x, y, z), b = row(p.T + 4, x, y, z);
    if (!(finite_f(x) && finite_f(y) && finite_f(z) && finite_f(a) && finite_f(b))) return false;
    const float ca = floorf(div_rn(a - p.x0, p.cell)), cb = floorf(div_rn(b - p.z0, p.cell));
    if (!(fabsf(ca) < CELL_LIMIT && fabsf(cb) < CELL_LIMIT)) return false;
    *ga = (int32_t)ca, *gb = (int32_t)cb;
    return true;
}

MC_FN Placed place(const Params& p, float x, float y, float z, float val) {
    Placed r{UNPLACED, NO_CELL, 0u, 0, 0u, 0u};
    const float a = row(p.T, x, y, z), b = row(p.T + 4, x, y, z);
    float h = row(p.T + 8, x, y, z);
    if (!(finite_f(x) && finite_f(y) && finite_f(z) && finite_f(a) && finite_f(b) && finite_f(h))) return r;
    // a - x0 can overflow to +-Inf, and so can the quotient: both fail the comparisons below
    const float ca = floorf(div_rn(a - p.x0, p.cell)), cb = floorf(div_rn(b - p.z0, p.cell));
    if (!(ca >= (float)p.oa && ca < (float)(p.oa + p.nx) && cb >= (float)p.ob && cb < (float)(p.ob + p.nz) &&
          fabsf(h) < H_LIMIT)) {
        r.fate = OUTSIDE;
        return r;
    }
    const int32_t ia = (int32_t)ca - p.oa, ib = (int32_t)cb - p.ob;
    r.cell = (uint32_t)ib * (uint32_t)p.nx + (uint32_t)ia;
    r.slot = slot_at(p, ia, ib);
    if (h == 0.f) h = 0.f;   // -0.0f -> +0.0f
    if (h > p.clearance) {
        r.fate = OVERHEAD;
        return r;
    }
    r.fate = LOW;
    r.key = key_of(h);
    r.q = (int32_t)rintf(h * 1024.f);   // exact scaling, |h| < 2^20: within 2^30
    r.v = q8(val);
    return r;
}

MC_FN Cell empty_cell() { return Cell{0, 0, KMIN_EMPTY, KMAX_EMPTY, 0, 0u}; }

// the five updates of a low point, the one of an overhead point (host form; the kernels do the same with atomics)
MC_FN void accumulate(Cell& c, const Placed& r) {
    if (r.fate == OVERHEAD) c.overhead += 1;
    if (r.fate != LOW) return;
    c.count += 1;
    c.kmin = r.key < c.kmin ? r.key : c.kmin;
    c.kmax = r.key > c.kmax ? r.key : c.kmax;
    c.hsum += (int64_t)r.q;
    c.vsum += (uint64_t)r.v;
}

MC_FN Final finalise(const Params& p, const Cell& c) {
    Final f;
    f.cls = C_UNKNOWN;
    if (c.count <= 0) {
        f.hmin = f.hmax = f.hmean = float_of(NAN_BITS);
        f.intensity = 0;
    } else {
        f.hmin = height_of(c.kmin);
        f.hmax = height_of(c.kmax);
        f.hmean = (float)((double)c.hsum / (1024.0 * (double)c.count));
        f.intensity = (uint8_t)((2u * c.vsum + (uint64_t)c.count) / (2u * (uint64_t)c.count));
        if (c.count >= p.min_points) f.cls = f.hmax > p.step ? C_OBSTACLE : f.hmin < -p.drop ? C_DROP : C_FREE;
    }
    if (c.overhead >= p.min_points) f.cls |= C_OVERHANG;
    return f;
}

// the colour of a finished cell
MC_FN void colour(const Params& p, int32_t mode, int32_t count, const Final& f, uint8_t* rgb) {
    rgb[0] = rgb[1] = rgb[2] = 0;
    if (mode == M_CLASS) {
        switch (f.cls & 3) {
        case C_UNKNOWN: rgb[0] = rgb[1] = rgb[2] = 32; break;
        case C_FREE: rgb[1] = (uint8_t)(64u + 3u * (uint32_t)f.intensity / 4u); break;
        case C_OBSTACLE: rgb[0] = 255; break;
        default: rgb[2] = 160; break;
        }
        if (f.cls & C_OVERHANG) rgb[2] = 255;
    } else if (mode == M_HEIGHT) {
        if (count <= 0) return;
        const float q = div_rn(f.hmax - p.h_lo, p.h_hi - p.h_lo);
        const float t = q < 0.f ? 0.f : (q > 1.f ? 1.f : q);
        float c[3];
        view2d::disparity_colour(200.f * t, c);   // t == 0 is black, as a disparity of 0 is
        rgb[0] = view2d::byte_of(c[0]), rgb[1] = view2d::byte_of(c[1]), rgb[2] = view2d::byte_of(c[2]);
    } else {
        if (count <= 0) return;
        rgb[0] = rgb[1] = rgb[2] = f.intensity;
    }
}

// RAYS (svh_grid_add_*_from).  A low point casts one ray from the origin's cell (oa_c, ob_c) to its own (ea, eb), both
// in the window: with dx = ea - oa_c, dz = eb - ob_c, n = max(|dx|, |dz|) the ray passes, for k = 0 .. n - 1, the cell
// (oa_c + rdiv(k * dx, n), ob_c + rdiv(k * dz, n)): the origin's cell is counted, the end cell is not, a point in the
// origin's cell casts nothing.  Both coordinates stay between the origin's and the end's, so every cell is in the window.
// The line depends only on the two cells, so the pass plane depends only on the multiset of (origin cell, end cell).
// rdiv(p, n) = floor((2 p + n) / (2 n)), n > 0: p / n rounded to the nearest integer, halves towards +infinity.  A true
// floor: C's / truncates, which is wrong for a negative numerator.  |p| < 2^26 (k < 2^13, |dx| < 2^13): 32 bits suffice.
MC_FN int32_t rdiv(int32_t p, int32_t n) {
    const int32_t num = 2 * p + n, den = 2 * n;
    const int32_t q = num / den;
    return (num < 0 && q * den != num) ? q - 1 : q;
}
MC_FN int32_t line_len(int32_t dx, int32_t dz) {
    const int32_t ax = dx < 0 ? -dx : dx, az = dz < 0 ? -dz : dz;
    return ax > az ? ax : az;
}
// the k-th cell of the line as an offset from the origin's cell, 0 <= k < n = line_len(dx, dz)
MC_FN void line_step(int32_t dx, int32_t dz, int32_t n, int32_t k, int32_t* sx, int32_t* sz) {
    *sx = rdiv(k * dx, n), *sz = rdiv(k * dz, n);
}

// the state byte of svh_grid_get_local: the class byte with bit 6 where at least min_points rays passed the cell
MC_FN uint8_t state_of(const Params& p, uint8_t cls, int32_t pass) {
    return pass >= p.min_points ? (uint8_t)(cls | C_SEEN) : cls;
}
// svh_grid_render_local: the class colours, but a cell that is unknown and seen has the SEEN colour instead of the dark
// grey (the overhang bit still fills its blue byte)
MC_FN void colour_local(const Params& p, int32_t count, const Final& f, int32_t pass, uint8_t* rgb) {
    colour(p, M_CLASS, count, f, rgb);
    if ((f.cls & 3) == C_UNKNOWN && pass >= p.min_points) {
        rgb[0] = SEEN_R, rgb[1] = SEEN_G, rgb[2] = (f.cls & C_OVERHANG) ? 255 : SEEN_B;
    }
}

// TRAVERSABILITY (svh_grid_set_traversability, svh_grid_get_trav, svh_grid_render_cost): what a planner reads.  All of it
// is computed from the finished planes CLASS, HMEAN and STATE in logical order; the torus plays no part.
//   FLAGS  bit 0 steep: a free cell with a free neighbour (of its up to eight inside the window) whose HMEAN differs by
//          more than the rise -- rise4 across an edge, rise8 across a corner.  Only free-free pairs are tested, and the
//          relation is symmetric: both cells of a steep pair are steep.  Bit 1 lethal: the cell's state matches a bit of
//          the lethal mask.
//   DIST2  the exact squared distance, in cells, to the nearest lethal cell of the window where that is at most reach^2,
//          else DIST2_FAR.  Separable: g(ia, ib) is the distance along ib to the nearest lethal cell of column ia, capped
//          at reach + 1 (col_step, forwards and backwards); DIST2(ia, ib) is the least (ia - j)^2 + g(j, ib)^2 over
//          |j - ia| <= reach with g(j, ib) <= reach (row_dist2).  A lethal cell within reach^2 is at most reach away on
//          either axis, so the cap and the bound lose nothing.
//   COST   one byte, table[DIST2] with the table of cost_of (reach^2 + 1 bytes, filled on the host in double), 0 for FAR;
//          a cell that is unknown and not lethal says 255, "no information", where the table says 0.
enum TravPlane : int32_t { TV_FLAGS = 0, TV_DIST2, TV_COST, TV_PLANES };
enum TravFlag : uint8_t { TF_STEEP = 1, TF_LETHAL = 2 };
enum Lethal : uint32_t { LETHAL_OBSTACLE = 1, LETHAL_DROP = 2, LETHAL_STEEP = 4, LETHAL_UNSEEN = 8, LETHAL_UNKNOWN_SEEN = 16,
                         LETHAL_ALL = 31 };
constexpr int32_t DIST2_FAR = 0x7FFFFFFF;
constexpr int32_t MAX_REACH = 256;
constexpr uint8_t COST_LETHAL = 254, COST_INSCRIBED = 253, COST_NO_INFORMATION = 255;

// svh_grid_trav_params and what trav_derive derives from it for the grid's cell
struct TravParams {
    float max_slope, inscribed, inflate;
    uint32_t lethal;
    float rise4, rise8;   // the largest difference of HMEAN that is not steep, across an edge and across a corner
    int32_t reach;        // cells; 0 until trav_derive succeeds
};

// the checks behind SVH_ERR_BAD_ARG of svh_grid_set_traversability, and the derived values.  The quotient is compared
// as a double before it becomes an integer.
MC_FN bool trav_derive(TravParams& t, float cell) {
    t.reach = 0;
    if (!(finite_f(t.max_slope) && t.max_slope > 0.f && finite_f(t.inscribed) && t.inscribed >= 0.f && finite_f(t.inflate) &&
          t.inflate > t.inscribed && (t.lethal & ~(uint32_t)LETHAL_ALL) == 0u))
        return false;
    t.rise4 = t.max_slope * cell;
    t.rise8 = t.rise4 * 1.41421354f;
    const double r = ceil((double)t.inflate / (double)cell);
    if (!(r >= 1.0 && r <= (double)MAX_REACH)) return false;
    t.reach = (int32_t)r;
    return true;
}

// the flags byte of window cell (ia, ib) from the finished planes
MC_FN uint8_t trav_flags(const TravParams& t, int32_t nx, int32_t nz, const uint8_t* cls, const float* hmean,
                         const uint8_t* state, int32_t ia, int32_t ib) {
    const size_t i = (size_t)ib * (size_t)nx + (size_t)ia;
    const uint8_t c = cls[i] & 3;
    bool steep = false;
    if (c == C_FREE) {
        const float h = hmean[i];
        for (int32_t db = -1; db <= 1; db++)
            for (int32_t da = -1; da <= 1; da++) {
                const int32_t ja = ia + da, jb = ib + db;
                if ((da == 0 && db == 0) || ja < 0 || ja >= nx || jb < 0 || jb >= nz) continue;
                const size_t j = (size_t)jb * (size_t)nx + (size_t)ja;
                if ((cls[j] & 3) != C_FREE) continue;
                steep = steep || fabsf(h - hmean[j]) > ((da != 0 && db != 0) ? t.rise8 : t.rise4);
            }
    }
    const uint32_t is = c == C_OBSTACLE ? LETHAL_OBSTACLE : c == C_DROP ? LETHAL_DROP
                        : c == C_UNKNOWN ? ((state[i] & C_SEEN) ? LETHAL_UNKNOWN_SEEN : LETHAL_UNSEEN) : 0u;
    const bool lethal = ((is | (steep ? (uint32_t)LETHAL_STEEP : 0u)) & t.lethal) != 0u;
    return (uint8_t)((steep ? TF_STEEP : 0) | (lethal ? TF_LETHAL : 0));
}

// one step of a column sweep: d is the capped distance at the cell before (reach + 1 in front of the first)
MC_FN int32_t col_step(int32_t d, bool lethal, int32_t reach) { return lethal ? 0 : (d < reach ? d + 1 : reach + 1); }

// DIST2 of column ia from one row of g: g[j - base] for the columns j = lo .. hi, which are those of the window within
// reach of ia.  At most 2 * 256^2.
MC_FN int32_t row_dist2(const uint16_t* g, int32_t base, int32_t ia, int32_t lo, int32_t hi, int32_t reach) {
    int32_t best = DIST2_FAR;
    for (int32_t j = lo; j <= hi; j++) {
        const int32_t gv = (int32_t)g[j - base];
        const int32_t d = (ia - j) * (ia - j) + gv * gv;
        best = (gv <= reach && d < best) ? d : best;
    }
    return best <= reach * reach ? best : DIST2_FAR;
}

// the cost table's entry for a squared distance in cells: double, in the order written.  Host only: the device reads the table.
inline uint8_t cost_of(int32_t d2, float cell, float inscribed, float inflate) {
    if (d2 == 0) return COST_LETHAL;
    if (d2 == DIST2_FAR) return 0;
    const double d = sqrt((double)d2) * (double)cell;
    if (d <= (double)inscribed) return COST_INSCRIBED;
    if (d < (double)inflate) return (uint8_t)(1 + (int)floor(251.0 * ((double)inflate - d) / ((double)inflate - (double)inscribed)));
    return 0;
}

// the cost byte of a cell from its table entry (0 for DIST2_FAR)
MC_FN uint8_t cell_cost(uint8_t table_cost, uint8_t cls, uint8_t flags) {
    return ((cls & 3) == C_UNKNOWN && !(flags & TF_LETHAL) && table_cost == 0) ? COST_NO_INFORMATION : table_cost;
}

// svh_grid_render_cost
MC_FN void colour_cost(uint8_t cost, uint8_t flags, uint8_t* rgb) {
    if (cost == COST_LETHAL) rgb[0] = 255, rgb[1] = 0, rgb[2] = 0;
    else if (cost == COST_INSCRIBED) rgb[0] = 255, rgb[1] = 128, rgb[2] = 0;
    else if (cost == COST_NO_INFORMATION) rgb[0] = rgb[1] = rgb[2] = 32;
    else if (cost == 0) rgb[0] = 0, rgb[1] = 96, rgb[2] = 0;
    else rgb[0] = cost, rgb[1] = 0, rgb[2] = (uint8_t)(255 - cost);
    if (flags & TF_STEEP) rgb[1] = 255;
}

// The whole layer on the host (svh_test_grid_trav, tests/cxx/grid_trav_check.cpp): the planes of a window from CLASS,
// HMEAN and STATE.  `table` has reach^2 + 1 bytes, `g` is nx * nz of scratch; any of dist2, cost may be null.
// The column and row passes alone, on a FLAGS plane that exists: DIST2 -> table -> cell_cost.  The time layer
// (grid_time_core.h) runs them on a FLAGS plane of its own.
inline void dist_window(int32_t reach, int32_t nx, int32_t nz, const uint8_t* cls, const uint8_t* table, const uint8_t* flags, uint16_t* g,
                        int32_t* dist2, uint8_t* cost) {
    for (int32_t ia = 0; ia < nx; ia++) {
        int32_t d = reach + 1;
        for (int32_t ib = 0; ib < nz; ib++) {
            const size_t i = (size_t)ib * nx + ia;
            g[i] = (uint16_t)(d = col_step(d, (flags[i] & TF_LETHAL) != 0, reach));
        }
        d = reach + 1;
        for (int32_t ib = nz - 1; ib >= 0; ib--) {
            const size_t i = (size_t)ib * nx + ia;
            d = col_step(d, (flags[i] & TF_LETHAL) != 0, reach);
            g[i] = (uint16_t)(d < (int32_t)g[i] ? d : (int32_t)g[i]);
        }
    }
    for (int32_t ib = 0; ib < nz; ib++)
        for (int32_t ia = 0; ia < nx; ia++) {
            const size_t i = (size_t)ib * nx + ia;
            const int32_t lo = ia - reach < 0 ? 0 : ia - reach, hi = ia + reach > nx - 1 ? nx - 1 : ia + reach;
            const int32_t d2 = row_dist2(g + (size_t)ib * nx, 0, ia, lo, hi, reach);
            if (dist2) dist2[i] = d2;
            if (cost) cost[i] = cell_cost(d2 == DIST2_FAR ? (uint8_t)0 : table[d2], cls[i], flags[i]);
        }
}

inline void trav_window(const TravParams& t, int32_t nx, int32_t nz, const uint8_t* cls, const float* hmean, const uint8_t* state,
                        const uint8_t* table, uint8_t* flags, uint16_t* g, int32_t* dist2, uint8_t* cost) {
    for (int32_t ib = 0; ib < nz; ib++)
        for (int32_t ia = 0; ia < nx; ia++) flags[(size_t)ib * nx + ia] = trav_flags(t, nx, nz, cls, hmean, state, ia, ib);
    dist_window(t.reach, nx, nz, cls, table, flags, g, dist2, cost);
}

// the checks behind SVH_ERR_BAD_ARG of svh_grid_create
MC_FN bool params_ok(const Params& p) {
    for (int k = 0; k < 12; k++)
        if (!finite_f(p.T[k])) return false;
    return p.nx >= 1 && p.nx <= MAX_SIDE && p.nz >= 1 && p.nz <= MAX_SIDE && finite_f(p.cell) && p.cell > 0.f &&
           finite_f(p.x0) && finite_f(p.z0) && p.min_points >= 1 && finite_f(p.step) && p.step >= 0.f && finite_f(p.drop) &&
           p.drop >= 0.f && finite_f(p.clearance) && p.clearance > p.step && finite_f(p.h_lo) && finite_f(p.h_hi) &&
           p.h_lo < p.h_hi && offsets_ok(p.oa, p.ob);
}

}  // namespace grid
}  // namespace svh

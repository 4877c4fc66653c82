// The arithmetic of the ground grid (svh_grid_*, include/svh_grid.h): the 2.5-D bird's-eye grid over the road plane that
// the accumulated map is binned into -- where a point goes, what a cell accumulates, what a finished cell says and how it
// is coloured.  THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entries svh_test_grid_points / svh_test_grid_finalise, which
//     evaluate every function below on the host),
//   * g++ -fsanitize=undefined into tests/cxx/grid_core_check.cpp, which guards the float-to-integer conversions,
// and restated in numpy by tests/grid_ref.py, which tests/test_grid.py pins by hand and against the test entries.
// fp32 in the order written, every operation rounded once (-ffp-contract=off on every build, no fast-math), the
// divisions IEEE's (div_rn), denormals kept.  Every range decision is made on the float BEFORE a conversion to an
// integer: an out-of-range conversion is undefined on the host and saturates on the device.
//
// ORDER INDEPENDENCE.  Every quantity a cell accumulates is an integer under a commutative, associative update: two
// counts (+), two keys (min, max), a sum of heights quantised to 1/1024 (+, int64) and a sum of intensity bytes (+,
// uint64).  The grid after any set of adds therefore depends only on the MULTISET of points, never on their order, the
// launch shape or the scheduling; add(A) then add(B) is add(A ++ B).
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

// what becomes of a point
enum Fate : int32_t { LOW = 0, OVERHEAD = 1, OUTSIDE = 2, UNPLACED = 3 };
// planes of svh_grid_get, modes of svh_grid_render, classes of a cell (bits 0-1 of the class byte; bit 7: overhang)
enum Plane : int32_t { P_COUNT = 0, P_OVERHEAD, P_HMIN, P_HMAX, P_HMEAN, P_INTENSITY, P_CLASS, P_PLANES };
enum Mode : int32_t { M_CLASS = 0, M_HEIGHT, M_INTENSITY, M_MODES };
enum Class : uint8_t { C_UNKNOWN = 0, C_FREE = 1, C_OBSTACLE = 2, C_DROP = 3, C_OVERHANG = 0x80 };

// svh_grid_params with T rounded to float (once, at create)
struct Params {
    int32_t nx, nz;
    float cell, x0, z0;
    float T[12];
    int32_t min_points;
    float step, drop, clearance, h_lo, h_hi;
};

struct Placed {
    int32_t fate;
    uint32_t cell;      // ib * nx + ia; NO_CELL when outside or unplaced
    uint32_t key;       // LOW: key_of(h)
    int32_t q;          // LOW: rintf(h * 1024)
    uint32_t v;         // LOW: q8(val)
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

MC_FN Placed place(const Params& p, float x, float y, float z, float val) {
    Placed r{UNPLACED, NO_CELL, 0u, 0, 0u};
    const float a = row(p.T, x, y, z), b = row(p.T + 4, x, y, z);
    float h = row(p.T + 8, x, y, z);
    if (!(finite_f(x) && finite_f(y) && finite_f(z) && finite_f(a) && finite_f(b) && finite_f(h))) return r;
    // a - x0 can overflow to +-Inf, and so can the quotient: both fail the comparisons below
    const float ca = floorf(div_rn(a - p.x0, p.cell)), cb = floorf(div_rn(b - p.z0, p.cell));
    if (!(ca >= 0.f && ca < (float)p.nx && cb >= 0.f && cb < (float)p.nz && fabsf(h) < H_LIMIT)) {
        r.fate = OUTSIDE;
        return r;
    }
    r.cell = (uint32_t)(int32_t)cb * (uint32_t)p.nx + (uint32_t)(int32_t)ca;
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

// the checks behind SVH_ERR_BAD_ARG of svh_grid_create
MC_FN bool params_ok(const Params& p) {
    for (int k = 0; k < 12; k++)
        if (!finite_f(p.T[k])) return false;
    return p.nx >= 1 && p.nx <= MAX_SIDE && p.nz >= 1 && p.nz <= MAX_SIDE && finite_f(p.cell) && p.cell > 0.f &&
           finite_f(p.x0) && finite_f(p.z0) && p.min_points >= 1 && finite_f(p.step) && p.step >= 0.f && finite_f(p.drop) &&
           p.drop >= 0.f && finite_f(p.clearance) && p.clearance > p.step && finite_f(p.h_lo) && finite_f(p.h_hi) &&
           p.h_lo < p.h_hi;
}

}  // namespace grid
}  // namespace svh

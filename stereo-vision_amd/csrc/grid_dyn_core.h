// The arithmetic of the ground grid's dynamics (svh_grid_set_dynamics, svh_grid_observe_*, include/svh_grid.h "DYNAMICS"): timed
// observations that clear moved obstacles and age cells.  THE CONTRACT IS THIS ARITHMETIC, integers after place().  Compiled from this
// one header by hipcc into the kernels of csrc/grid_dyn_kernels.hip, by the host compiler into csrc/grid_engine.cpp (the test
// entries svh_test_grid_dyn_height / _through / _settle / _colour, which evaluate every function below on the host) and by g++
// -fsanitize=address,undefined into tests/cxx/grid_dyn_check.cpp, which runs the integer paths at their extremes; restated in numpy
// by tests/grid_dyn_ref.py, which tests/test_grid_dyn.py pins by hand and against the test entries.
//
// AN OBSERVATION is one frame: a list of points and an origin, the arguments of svh_grid_add_points_from, numbered by a STAMP (int32,
// 1 for the first observation after a clear).  It is defined in three phases, each a pure function of its inputs, so the result
// depends only on the state before it and on the MULTISET of the frame's points:
//   1  FRAME RECORD.  Every point is placed by place() unchanged; the low and overhead points are accumulated per cell into a frame
//      record (fcount, foverhead, fkmin, fkmax, fhsum, fvsum; the updates of accumulate()) that lives in scratch, not in the cell.
//   2  SIGHT LINES.  For every end cell with fcount > 0 one line of weight fcount runs from the origin's cell, the line of
//      line_step(), k = 0 .. n - 1.  Every cell of it gains fcount in the stored PASS (what svh_grid_add_points_from leaves).  The line
//      has a height in 1/1024: q_k = q_o + rdiv64(k (q_e - q_o), n) with q_o = place(origin).q and q_e = q_of_key(fkmin), the frame's
//      lowest low point of the end cell.  A stored cell is TALL if count > 0 and height_of(kmax) > step; its BODY is the interval
//      [q_of_key(kmin), q_of_key(kmax) - margin_q].  A line step in a tall cell goes THROUGH it iff q_k lies in the body, both ends
//      inclusive; a line above it sees over the obstacle, one below passes under it, neither contradicts it.  THROUGH[cell] is the sum
//      of the weights of the lines that go through.  Phase 2 reads the stored accumulators; nothing writes them before phase 3.
//   3  SETTLE, per window cell: settle() below.
#pragma once
#include "grid_core.h"

namespace svh {
namespace grid {

// planes of svh_grid_get_dyn; the flags of what an observation did to a cell; the words of svh_grid_get_dyn_stats
enum DynPlane : int32_t { D_AGE = 0, D_CONTRA, D_THROUGH, D_PLANES };
enum DynEvent : uint8_t { DE_CLEARED = 1, DE_AGED = 2, DE_CONFIRMED = 4 };
enum DynStat : int32_t { DS_OBSERVATIONS = 0, DS_CLEARED, DS_AGED, DS_CONFIRMED, DS_WORDS };
constexpr int32_t MAX_CLEAR_FRAMES = 65535;
constexpr float MARGIN_LIMIT = 1048576.f;          // 0 <= margin < 2^20: margin_q <= 2^30
constexpr int32_t STAMP_LIMIT = 0x7FFFFFFF;        // no observation after this stamp
constexpr uint8_t EVENT_R = 255, EVENT_G = 0, EVENT_B = 255;   // svh_grid_render_dyn: a cell the last observation cleared or aged

// svh_grid_dyn_params and what dyn_derive derives from it
struct DynParams {
    int32_t clear_frames, min_through;
    float margin;
    int32_t max_age;
    int32_t margin_q;   // (int32)rintf(margin * 1024)
};

// the checks behind SVH_ERR_BAD_ARG of svh_grid_set_dynamics, and the derived value
MC_FN bool dyn_derive(DynParams& d) {
    d.margin_q = 0;
    if (!(d.clear_frames >= 0 && d.clear_frames <= MAX_CLEAR_FRAMES && d.min_through >= 1 && finite_f(d.margin) && d.margin >= 0.f &&
          d.margin < MARGIN_LIMIT && d.max_age >= 0))
        return false;
    d.margin_q = (int32_t)rintf(d.margin * 1024.f);   // exact scaling, below 2^30 + 1
    return true;
}

// rdiv's formula in 64 bits: floor((2 p + n) / (2 n)), n > 0.  |p| < 2^45 here
MC_FN int64_t rdiv64(int64_t p, int64_t n) {
    const int64_t num = 2 * p + n, den = 2 * n;
    const int64_t q = num / den;
    return (num < 0 && q * den != num) ? q - 1 : q;
}

// a key's height in 1/1024; the key of a binned height, |h| < 2^20: within 2^30
MC_FN int32_t q_of_key(uint32_t key) { return (int32_t)rintf(height_of(key) * 1024.f); }

// the height of line step k, 0 <= k < n: between q_o and q_e, |q| <= 2^30 and k < 2^13, so the product needs 64 bits
MC_FN int32_t line_height(int32_t q_o, int32_t q_e, int32_t n, int32_t k) {
    return (int32_t)((int64_t)q_o + rdiv64((int64_t)k * ((int64_t)q_e - (int64_t)q_o), (int64_t)n));
}

// line_height stepped, as the kernel walks it: q = rdiv64(k dq, n) and r = (2 k dq + n) - 2 n q in [0, 2n) with dq = q_e - q_o.
// |dq| may be far above n, so a step moves q by a = floor(2 dq / 2 n) and r by b = 2 dq - a * 2 n in [0, 2n), with one carry: the
// closed form's value at every step, and one division per line.  n >= 1; height() is q_k
struct HeightStepper {
    int64_t q_o, q, a;
    int32_t r, b, n2;
    MC_FN HeightStepper(int32_t q_o_, int32_t q_e, int32_t n) : q_o(q_o_), q(0), r(n), n2(2 * n) {
        const int64_t d2 = 2 * ((int64_t)q_e - (int64_t)q_o_);
        int64_t fl = d2 / n2;
        if (d2 < 0 && fl * n2 != d2) fl -= 1;
        a = fl;
        b = (int32_t)(d2 - fl * n2);
    }
    MC_FN void step() {
        q += a;
        r += b;
        if (r >= n2) r -= n2, q += 1;
    }
    MC_FN int32_t height() const { return (int32_t)(q_o + q); }
};

// the body of a stored cell; lo > hi: nothing goes through (the cell is not tall, or the margin is larger than the body)
struct Body {
    int32_t lo, hi;
};
MC_FN bool is_tall(const Params& p, int32_t count, uint32_t kmax) { return count > 0 && height_of(kmax) > p.step; }
MC_FN Body body_of(const Params& p, const DynParams& d, int32_t count, uint32_t kmin, uint32_t kmax) {
    if (!is_tall(p, count, kmax)) return Body{1, 0};
    return Body{q_of_key(kmin), q_of_key(kmax) - d.margin_q};   // the top is above step >= 0: above -2^30
}
MC_FN bool goes_through(const Body& b, int32_t q) { return b.lo <= q && q <= b.hi; }

// SETTLE: what phase 3 does to one cell.  `c` is the stored cell, (contra, last) its state (0 = never), `f` the frame record,
// `through` the plane of phase 2, `stamp` this observation's.  In this order:
//   1  confirm: fcount > 0 and height_of(fkmax) > step -- something tall is seen there now: CONTRA = 0
//   2  otherwise, if the stored cell is tall and THROUGH >= min_through: CONTRA += 1
//   3  if clear_frames > 0 and CONTRA >= clear_frames: the five low accumulators become empty_cell()'s (overhead stays: a bridge
//      over a cleared car is still a bridge), CONTRA = 0: DE_CLEARED
//   4  if max_age > 0, the cell stores anything and stamp - LAST > max_age: all six accumulators become empty, CONTRA = 0: DE_AGED,
//      unless the cell was cleared in step 3 (it counts once)
//   5  the frame record is merged (+, min, max, +, +, +); if fcount + foverhead > 0: LAST = stamp
// Returns the DynEvent flags.  PASS is not touched.
MC_FN uint8_t settle(const Params& p, const DynParams& d, int32_t stamp, Cell& c, int32_t& contra, int32_t& last, const Cell& f,
                     int32_t through) {
    uint8_t ev = 0;
    if (f.count > 0 && height_of(f.kmax) > p.step) {
        contra = 0;
        ev |= DE_CONFIRMED;
    } else if (is_tall(p, c.count, c.kmax) && through >= d.min_through) {
        contra += 1;   // at most one per stamp: below 2^31
    }
    if (d.clear_frames > 0 && contra >= d.clear_frames) {
        const int32_t over = c.overhead;
        c = empty_cell();
        c.overhead = over;
        contra = 0;
        ev |= DE_CLEARED;
    }
    if (d.max_age > 0 && (c.count > 0 || c.overhead > 0) && stamp - last > d.max_age) {   // 0 <= last <= stamp
        c = empty_cell();
        contra = 0;
        if (!(ev & DE_CLEARED)) ev |= DE_AGED;
    }
    c.count += f.count, c.overhead += f.overhead;
    c.kmin = f.kmin < c.kmin ? f.kmin : c.kmin;
    c.kmax = f.kmax > c.kmax ? f.kmax : c.kmax;
    c.hsum += f.hsum, c.vsum += f.vsum;
    if (f.count > 0 || f.overhead > 0) last = stamp;
    return ev;
}

// SVH_GRID_DYN_AGE
MC_FN int32_t age_of(int32_t stamp, int32_t last) { return last == 0 ? -1 : stamp - last; }

// svh_grid_render_dyn: the local colours; a cell with CONTRA > 0 is tinted (red and green c + (255 - c) / 2, blue stays); a cell
// that the last observation cleared or aged has the EVENT colour
MC_FN void colour_dyn(const Params& p, int32_t count, const Final& f, int32_t pass, int32_t contra, uint8_t event, uint8_t* rgb) {
    colour_local(p, count, f, pass, rgb);
    if (contra > 0) {
        rgb[0] = (uint8_t)(rgb[0] + (255 - rgb[0]) / 2);
        rgb[1] = (uint8_t)(rgb[1] + (255 - rgb[1]) / 2);
    }
    if (event & (DE_CLEARED | DE_AGED)) rgb[0] = EVENT_R, rgb[1] = EVENT_G, rgb[2] = EVENT_B;
}

}  // namespace grid
}  // namespace svh

// The arithmetic of the ground grid's frontiers (svh_grid_*frontier*, svh_grid_get_front_plane, svh_grid_render_frontiers;
// include/svh_grid.h, "FRONTIERS"): from the finished STATE and COST planes of the window the cells where drivable ground ends
// and unlooked-at ground begins, their 8-connected components and one table record per component that is large enough.
// THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_front_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entry svh_test_grid_front, which runs front_window below),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_front_check.cpp,
// and restated in numpy and plain Python by tests/grid_front_ref.py, which tests/test_grid_front.py pins by hand and against
// the test entry.  Everything is integer arithmetic on planes in logical (window) order; the torus plays no part.
//
// A cell is UNEXPLORED if its class (bits 0-1 of STATE) is unknown and its seen bit (bit 6) matches the mask `unexplored`: not
// seen matches LETHAL_UNSEEN, seen matches LETHAL_UNKNOWN_SEEN.  A cell is a FRONTIER cell if its class is free, its COST is
// at most max_cell_cost (0..252: never lethal, never inside the inscribed radius, always passable for the planner) and one of
// its four EDGE neighbours is unexplored; a neighbour position outside the window counts as unexplored only when border != 0.
// COMPONENTS are the 8-connected sets of frontier cells.  LABEL is -1 off the frontier, elsewhere the LOWEST window index
// ib * nx + ia of the cell's component.  A component is KEPT when it has at least min_size cells; each kept component has one
// record of FRONT_REC int32, the records in ascending order of label:
//   label, size, ga_min, gb_min, ga_max, gb_max   the bounding box in GLOBAL cells (window cell + offsets)
//   cen_ga, cen_gb    the centroid: per axis floor((2 * sum + size) / (2 * size)) of the window coordinates (nearest, halves
//                     up; the sums in int64), then the offset
//   rep_ga, rep_gb    the REPRESENTATIVE: the component's cell with the least (ia - ca)^2 + (ib - cb)^2 to the centroid cell
//                     (ca, cb), ties to the lowest window index -- the least key dist2 << 32 | index.  The centroid of a curved
//                     frontier usually lies off it; the representative is always a frontier cell.
// FRONT is one byte: bit 0 frontier, bit 1 in a kept component, bit 2 representative (of a kept component).
//
// SCHEDULE INDEPENDENCE.  The frontier bit is a function of the cell's neighbourhood.  The label is the minimum of a set, the
// size and the coordinate sums are integer sums, the box is minima and maxima, the representative the minimum of keys that
// are unique within a component: all commutative.  The order of the records is that of their labels.  No byte depends on
// launch shape or scheduling.
#pragma once
#include <stdint.h>

#include <vector>

#include "grid_core.h"

namespace svh {
namespace grid {

constexpr int32_t FRONT_REC = 10;                       // int32 per record
constexpr int32_t FRONT_MAX_MIN_SIZE = 1 << 26;         // 8192^2
enum FrontPlane : int32_t { FP_FLAGS = 0, FP_LABEL, FP_PLANES };
enum FrontFlag : uint8_t { FF_FRONTIER = 1, FF_KEPT = 2, FF_REP = 4 };
enum FrontRec : int32_t { FR_LABEL = 0, FR_SIZE, FR_GA_MIN, FR_GB_MIN, FR_GA_MAX, FR_GB_MAX, FR_CEN_GA, FR_CEN_GB, FR_REP_GA, FR_REP_GB };
enum FrontStat : int32_t { FS_CELLS = 0, FS_COMPONENTS, FS_KEPT, FS_KEPT_CELLS, FS_LAUNCHES, FS_WORDS };

struct FrontParams {
    int32_t max_cell_cost;   // 0..252
    int32_t min_size;        // 1..2^26
    uint32_t unexplored;     // LETHAL_UNSEEN, LETHAL_UNKNOWN_SEEN or both
    int32_t border;          // 0 or 1
};

MC_FN bool front_ok(const FrontParams& p) {
    return p.max_cell_cost >= 0 && p.max_cell_cost <= 252 && p.min_size >= 1 && p.min_size <= FRONT_MAX_MIN_SIZE && p.unexplored != 0u &&
           (p.unexplored & ~(uint32_t)(LETHAL_UNSEEN | LETHAL_UNKNOWN_SEEN)) == 0u && (p.border == 0 || p.border == 1);
}

MC_FN bool unexplored_state(const FrontParams& p, uint8_t state) {
    if ((state & 3) != C_UNKNOWN) return false;
    return (p.unexplored & ((state & C_SEEN) ? (uint32_t)LETHAL_UNKNOWN_SEEN : (uint32_t)LETHAL_UNSEEN)) != 0u;
}

// the frontier bit of window cell (ia, ib) from the finished planes
MC_FN bool front_cell(const FrontParams& p, int32_t nx, int32_t nz, const uint8_t* state, const uint8_t* cost, int32_t ia, int32_t ib) {
    const size_t i = (size_t)ib * (size_t)nx + (size_t)ia;
    if ((state[i] & 3) != C_FREE || (int32_t)cost[i] > p.max_cell_cost) return false;
    const bool out = p.border != 0;
    return (ia > 0 ? unexplored_state(p, state[i - 1]) : out) || (ia < nx - 1 ? unexplored_state(p, state[i + 1]) : out) ||
           (ib > 0 ? unexplored_state(p, state[i - (size_t)nx]) : out) || (ib < nz - 1 ? unexplored_state(p, state[i + (size_t)nx]) : out);
}

// one axis of the centroid in window coordinates: sum >= 0 of `size` >= 1 coordinates
MC_FN int32_t front_centre(int64_t sum, int64_t size) { return (int32_t)((2 * sum + size) / (2 * size)); }

// the key whose minimum over a component is its representative; |ia - ca|, |ib - cb| < 8192, so dist2 < 2^27
MC_FN uint64_t front_key(int32_t ia, int32_t ib, int32_t ca, int32_t cb, uint32_t index) {
    const int32_t da = ia - ca, db = ib - cb;
    return ((uint64_t)(uint32_t)(da * da + db * db) << 32) | (uint64_t)index;
}

// what svh_grid_render_frontiers draws over the cost image; false: the cell keeps the colour of its cost
MC_FN bool colour_front(uint8_t f, uint8_t* rgb) {
    if (!(f & FF_FRONTIER)) return false;
    if (f & FF_REP) rgb[0] = 255, rgb[1] = 255, rgb[2] = 0;
    else if (f & FF_KEPT) rgb[0] = 0, rgb[1] = 255, rgb[2] = 255;
    else rgb[0] = 0, rgb[1] = 96, rgb[2] = 128;
    return true;
}

// ---- the whole window on the host: a flood fill in ascending order of index --------------------------------------------------
// state, cost [nz * nx] under the offsets (oa, ob) -> flags, label [nz * nx], the records of all kept components appended to
// `recs`, stats[FS_CELLS .. FS_KEPT_CELLS] (FS_LAUNCHES is 0).  The first cell of a component that an ascending scan meets
// is its lowest index, so the components are found in the order of their labels.
inline void front_window(const FrontParams& p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state, const uint8_t* cost,
                         uint8_t* flags, int32_t* label, std::vector<int32_t>* recs, int64_t* stats) {
    const size_t cells = (size_t)nx * (size_t)nz;
    int64_t n_cells = 0, n_comp = 0, n_kept = 0, n_kept_cells = 0;
    for (int32_t ib = 0; ib < nz; ib++)
        for (int32_t ia = 0; ia < nx; ia++) {
            const size_t i = (size_t)ib * (size_t)nx + (size_t)ia;
            const bool f = front_cell(p, nx, nz, state, cost, ia, ib);
            flags[i] = f ? (uint8_t)FF_FRONTIER : (uint8_t)0;
            label[i] = -1;
            n_cells += f ? 1 : 0;
        }
    std::vector<uint32_t> members;
    for (size_t seed = 0; seed < cells; seed++) {
        if (!flags[seed] || label[seed] >= 0) continue;
        members.clear();
        members.push_back((uint32_t)seed);
        label[seed] = (int32_t)seed;
        int64_t sa = 0, sb = 0;
        int32_t a0 = nx, b0 = nz, a1 = -1, b1 = -1;
        for (size_t at = 0; at < members.size(); at++) {
            const uint32_t i = members[at];
            const int32_t ib = (int32_t)(i / (uint32_t)nx), ia = (int32_t)(i - (uint32_t)ib * (uint32_t)nx);
            sa += ia, sb += ib;
            a0 = ia < a0 ? ia : a0, a1 = ia > a1 ? ia : a1, b0 = ib < b0 ? ib : b0, b1 = ib > b1 ? ib : b1;
            for (int32_t db = -1; db <= 1; db++)
                for (int32_t da = -1; da <= 1; da++) {
                    const int32_t ja = ia + da, jb = ib + db;
                    if (ja < 0 || ja >= nx || jb < 0 || jb >= nz) continue;
                    const size_t j = (size_t)jb * (size_t)nx + (size_t)ja;
                    if (!flags[j] || label[j] >= 0) continue;
                    label[j] = (int32_t)seed;
                    members.push_back((uint32_t)j);
                }
        }
        n_comp++;
        const int64_t size = (int64_t)members.size();
        if (size < p.min_size) continue;
        n_kept++, n_kept_cells += size;
        const int32_t ca = front_centre(sa, size), cb = front_centre(sb, size);
        uint64_t best = ~(uint64_t)0;
        for (const uint32_t i : members) {
            const int32_t ib = (int32_t)(i / (uint32_t)nx), ia = (int32_t)(i - (uint32_t)ib * (uint32_t)nx);
            const uint64_t k = front_key(ia, ib, ca, cb, i);
            best = k < best ? k : best;
            flags[i] |= FF_KEPT;
        }
        const uint32_t rep = (uint32_t)(best & 0xFFFFFFFFu);
        flags[rep] |= FF_REP;
        const int32_t rb = (int32_t)(rep / (uint32_t)nx), ra = (int32_t)(rep - (uint32_t)rb * (uint32_t)nx);
        if (recs) {
            const int32_t r[FRONT_REC] = {(int32_t)seed, (int32_t)size, oa + a0, ob + b0, oa + a1, ob + b1, oa + ca, ob + cb, oa + ra, ob + rb};
            recs->insert(recs->end(), r, r + FRONT_REC);
        }
    }
    if (stats) stats[FS_CELLS] = n_cells, stats[FS_COMPONENTS] = n_comp, stats[FS_KEPT] = n_kept, stats[FS_KEPT_CELLS] = n_kept_cells, stats[FS_LAUNCHES] = 0;
}

}  // namespace grid
}  // namespace svh

// The arithmetic of the ground grid's objects and their tracks (svh_grid_set_objects, svh_grid_get_obj_plane, svh_grid_get_objects,
// svh_grid_objects_step, svh_grid_get_tracks, svh_grid_render_objects; include/svh_grid_obj.h, "OBJECTS").
// THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_obj_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entries svh_test_grid_obj and svh_test_grid_obj_step, which run
//     obj_window and obj_step below),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_obj_check.cpp,
// and restated in numpy and plain Python by tests/grid_obj_ref.py, which tests/test_grid_obj.py pins by hand and against the test
// entries.  Everything is integer arithmetic on planes in logical (window) order; the one float, min_height, is compared once per
// component.
//
// OBJECTS.  A cell is an OBJECT cell if its class (bits 0-1 of STATE) is obstacle.  COMPONENTS are the 8-connected sets of object
// cells; LABEL is -1 elsewhere and the LOWEST window index ib * nx + ia of the cell's component on them.  Of a component:
//   size       its cells
//   hmax_bits  the largest of the bits of HMAX over its cells, compared as int32.  HMAX of an obstacle cell is a positive float, whose
//              bits order as the floats do
//   points     the sum of COUNT over its cells, saturated at INT32_MAX
// A component is LARGE if size > max_size, LOW if min_size <= size <= max_size and not float_of(hmax_bits) >= min_height, and KEPT if
// min_size <= size <= max_size and float_of(hmax_bits) >= min_height.  Each kept component has one record of OBJ_REC int32, the
// records in ascending order of label; the RANK of an object is its position in that table:
//   label, size, ga_min, gb_min, ga_max, gb_max   the box in GLOBAL cells (window cell + offsets)
//   c16_a, c16_b   the centroid in sixteenths of a global cell, a cell's centre at 16 i + 8: per axis
//                  (16 * (2 * sum + size)) / (2 * size) + 16 * offset, the sum of the window coordinates in int64 (>= 0: the
//                  division is a floor)
//   hmax_bits, points
// FLAGS is one byte: bit 0 object cell, bit 1 in a kept component, bit 2 in a large one.
//
// TRACKS.  obj_step is a pure function of the object table, the LABEL plane, the ID plane of the step before with the offsets it
// was written under, and the track table of the step before.  The ID plane holds, per window cell, the id of the track of the kept
// component that covered the cell, or -1.  Cells are compared as GLOBAL cells; a global cell outside the previous window has no
// track.
//   overlap  O[i, t]: the cells of object i (rank) whose global cell held track t.  Pairs with O >= min_overlap COUNT.  Object i
//            claims the counting track with the greatest O, ties to the lowest id; track t claims the counting object with the
//            greatest O, ties to the lowest rank: the maxima of O << 32 | ~index.  Mutual claims MATCH (BY_OVERLAP).  An object
//            with two or more counting tracks sets MERGED on the track it ends up with, a track with two or more counting
//            objects has SPLIT.
//   gate     when gate > 0, one round over the objects and tracks left unmatched: the prediction of a track is c16 + v16 *
//            (missed + 1) per axis, d2 the squared distance from it to the object's c16 (int64); pairs with d2 <= (16 * gate)^2
//            count.  An object picks the least d2 << 32 | track index, a track the least d2 << 32 | rank.  Mutual picks MATCH
//            (BY_GATE).  The track table is in ascending order of id, so the lowest index is the lowest id.
//   update   a matched track: age++, raw = rdiv(c16_now - c16_before, missed + 1) per axis; at the first match (age was 0)
//            v16 = raw, afterwards v16 += rdiv(raw - v16, 1 << smooth_shift); missed = 0; label, size, c16, hmax_bits those of
//            the object; overlap the winning O (0 by the gate).  An unmatched track: missed++, label -1, overlap 0, MISSED; it
//            is DROPPED once missed > max_missed; its size, c16, v16 and hmax_bits stay.  Then the unmatched objects in ascending
//            rank become NEW tracks with the next ids (age 0, missed 0, v16 0, birth = c16) while the table has fewer than
//            max_tracks records (and ids below INT32_MAX remain); the others stay UNTRACKED.
//            MOVING: age >= min_age and the squared distance of c16 from the birth position >= (16 * move_cells)^2 (int64).
//            The flags are those of this step alone.
//   assign   per object the id of its track, or ASSIGN_UNTRACKED.  The new ID plane: the id on the cells of a tracked object, -1
//            elsewhere.
// The table is in ascending order of id: the survivors in their order, then the new tracks.  TRACK_REC int32 per record:
//   id, flags, age, missed, label, size, c16_a, c16_b, v16_a, v16_b, birth_a, birth_b, overlap, hmax_bits
//
// SCHEDULE INDEPENDENCE.  Labels are minima of sets, the accumulators integer sums, minima and maxima, every choice the
// minimum or maximum of keys that are unique among the candidates: all commutative.  No byte depends on launch shape or
// scheduling.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "grid_core.h"

namespace svh {
namespace grid {

constexpr int32_t OBJ_REC = 10, TRACK_REC = 14;
constexpr int32_t OBJ_MAX_SIZE = 1 << 26;                // 8192^2
constexpr int32_t OBJ_MAX_TRACKS = 4096, OBJ_MAX_GATE = 64, OBJ_MAX_MISSED = 255, OBJ_MAX_MOVE = 8192, OBJ_MAX_SHIFT = 4;
constexpr int32_t OBJ_MAX_AGE = 1 << 30;
constexpr int32_t ASSIGN_UNTRACKED = -2;
enum ObjPlane : int32_t { OP_FLAGS = 0, OP_LABEL, OP_PLANES };
enum ObjFlag : uint8_t { OF_OBJECT = 1, OF_KEPT = 2, OF_LARGE = 4 };
enum ObjRec : int32_t { OR_LABEL = 0, OR_SIZE, OR_GA_MIN, OR_GB_MIN, OR_GA_MAX, OR_GB_MAX, OR_C16_A, OR_C16_B, OR_HMAX_BITS, OR_POINTS };
enum ObjStat : int32_t { OS_CELLS = 0, OS_COMPONENTS, OS_KEPT, OS_KEPT_CELLS, OS_LARGE, OS_LOW, OS_LAUNCHES, OS_WORDS };
enum TrackFlag : int32_t { TK_NEW = 1, TK_BY_OVERLAP = 2, TK_BY_GATE = 4, TK_MISSED = 8, TK_MOVING = 16, TK_MERGED = 32, TK_SPLIT = 64 };
enum TrackRec : int32_t { TR_ID = 0, TR_FLAGS, TR_AGE, TR_MISSED, TR_LABEL, TR_SIZE, TR_C16_A, TR_C16_B, TR_V16_A, TR_V16_B, TR_BIRTH_A,
                          TR_BIRTH_B, TR_OVERLAP, TR_HMAX_BITS };
// steps since the last reset; the tracks of the table; of the last step: matched by overlap, matched by the gate, new, missed and
// still in the table, dropped, objects left untracked
enum TrackStat : int32_t { TS_STEPS = 0, TS_TRACKS, TS_BY_OVERLAP, TS_BY_GATE, TS_NEW, TS_MISSED, TS_DROPPED, TS_UNTRACKED, TS_WORDS };

struct ObjParams {
    int32_t min_size;        // 1..2^26
    int32_t max_size;        // min_size..2^26
    float min_height;        // finite, >= 0
    int32_t max_tracks;      // 1..4096
    int32_t min_overlap;     // >= 1
    int32_t gate;            // 0..64 cells; 0: no centroid fallback
    int32_t max_missed;      // 0..255
    int32_t min_age;         // 0..2^30 steps
    int32_t move_cells;      // 1..8192
    int32_t smooth_shift;    // 0..4
};

MC_FN bool obj_ok(const ObjParams& p) {
    return p.min_size >= 1 && p.max_size >= p.min_size && p.max_size <= OBJ_MAX_SIZE && finite_f(p.min_height) && p.min_height >= 0.f &&
           p.max_tracks >= 1 && p.max_tracks <= OBJ_MAX_TRACKS && p.min_overlap >= 1 && p.gate >= 0 && p.gate <= OBJ_MAX_GATE &&
           p.max_missed >= 0 && p.max_missed <= OBJ_MAX_MISSED && p.min_age >= 0 && p.min_age <= OBJ_MAX_AGE && p.move_cells >= 1 &&
           p.move_cells <= OBJ_MAX_MOVE && p.smooth_shift >= 0 && p.smooth_shift <= OBJ_MAX_SHIFT;
}

MC_FN bool obj_cell(uint8_t state) { return (state & 3) == C_OBSTACLE; }

// what becomes of a component: 0 dropped without a word (too small), else OF_KEPT, OF_LARGE, or OF_OBJECT for LOW
MC_FN uint8_t obj_verdict(const ObjParams& p, int32_t size, int32_t hmax_bits) {
    if (size > p.max_size) return OF_LARGE;
    if (size < p.min_size) return 0;
    return float_of((uint32_t)hmax_bits) >= p.min_height ? OF_KEPT : OF_OBJECT;
}

// one axis of the centroid in sixteenths of a window cell: sum >= 0 of `size` >= 1 coordinates below 8192
MC_FN int32_t obj_c16(int64_t sum, int64_t size) { return (int32_t)((16 * (2 * sum + size)) / (2 * size)); }

MC_FN int32_t obj_points(int64_t sum) { return sum > (int64_t)0x7FFFFFFF ? 0x7FFFFFFF : (int32_t)sum; }

// the two claims of a counting pair: the maximum over the tracks of an object, over the objects of a track
MC_FN uint64_t obj_claim_key(int32_t overlap, int32_t index) { return ((uint64_t)(uint32_t)overlap << 32) | (uint64_t)(~(uint32_t)index); }
MC_FN int32_t obj_claim_index(uint64_t key) { return (int32_t)(~(uint32_t)(key & 0xFFFFFFFFu)); }
MC_FN int32_t obj_claim_overlap(uint64_t key) { return (int32_t)(key >> 32); }

constexpr uint64_t GATE_NONE = ~(uint64_t)0;
// the key of a gate pair, GATE_NONE when the object lies beyond the gate of the track's prediction
MC_FN uint64_t obj_gate_key(const ObjParams& p, const int32_t* track, const int32_t* obj, int32_t index) {
    const int64_t ahead = (int64_t)track[TR_MISSED] + 1;
    const int64_t da = (int64_t)obj[OR_C16_A] - ((int64_t)track[TR_C16_A] + (int64_t)track[TR_V16_A] * ahead);
    const int64_t db = (int64_t)obj[OR_C16_B] - ((int64_t)track[TR_C16_B] + (int64_t)track[TR_V16_B] * ahead);
    const int64_t lim = 16 * (int64_t)p.gate;
    if (da < -lim || da > lim || db < -lim || db > lim) return GATE_NONE;   // before the squares: they stay below 2^21
    const int64_t d2 = da * da + db * db;
    return d2 <= lim * lim ? (((uint64_t)d2 << 32) | (uint64_t)(uint32_t)index) : GATE_NONE;
}

MC_FN int32_t track_moving(const ObjParams& p, const int32_t* t) {
    const int64_t da = (int64_t)t[TR_C16_A] - t[TR_BIRTH_A], db = (int64_t)t[TR_C16_B] - t[TR_BIRTH_B], lim = 16 * (int64_t)p.move_cells;
    return (t[TR_AGE] >= p.min_age && da * da + db * db >= lim * lim) ? (int32_t)TK_MOVING : 0;
}

// a track matched with the object record `obj`: `how` is TK_BY_OVERLAP or TK_BY_GATE, `extra` TK_MERGED and TK_SPLIT as they hold
MC_FN void track_match(const ObjParams& p, const int32_t* before, const int32_t* obj, int32_t how, int32_t overlap, int32_t extra, int32_t* t) {
    const int32_t n = before[TR_MISSED] + 1;
    const int32_t ra = rdiv(obj[OR_C16_A] - before[TR_C16_A], n), rb = rdiv(obj[OR_C16_B] - before[TR_C16_B], n);
    const bool first = before[TR_AGE] == 0;
    t[TR_ID] = before[TR_ID];
    t[TR_AGE] = before[TR_AGE] < 0x7FFFFFFF ? before[TR_AGE] + 1 : before[TR_AGE];
    t[TR_MISSED] = 0;
    t[TR_LABEL] = obj[OR_LABEL], t[TR_SIZE] = obj[OR_SIZE];
    t[TR_C16_A] = obj[OR_C16_A], t[TR_C16_B] = obj[OR_C16_B];
    t[TR_V16_A] = first ? ra : before[TR_V16_A] + rdiv(ra - before[TR_V16_A], 1 << p.smooth_shift);
    t[TR_V16_B] = first ? rb : before[TR_V16_B] + rdiv(rb - before[TR_V16_B], 1 << p.smooth_shift);
    t[TR_BIRTH_A] = before[TR_BIRTH_A], t[TR_BIRTH_B] = before[TR_BIRTH_B];
    t[TR_OVERLAP] = overlap;
    t[TR_HMAX_BITS] = obj[OR_HMAX_BITS];
    t[TR_FLAGS] = how | extra | track_moving(p, t);
}

// an unmatched track; false: it is dropped (t is written all the same)
MC_FN bool track_miss(const ObjParams& p, const int32_t* before, int32_t extra, int32_t* t) {
    for (int32_t k = 0; k < TRACK_REC; k++) t[k] = before[k];
    t[TR_MISSED] = before[TR_MISSED] + 1;
    t[TR_LABEL] = -1, t[TR_OVERLAP] = 0;
    t[TR_FLAGS] = TK_MISSED | extra | track_moving(p, t);
    return t[TR_MISSED] <= p.max_missed;
}

MC_FN void track_new(const ObjParams& p, int32_t id, const int32_t* obj, int32_t extra, int32_t* t) {
    t[TR_ID] = id, t[TR_AGE] = 0, t[TR_MISSED] = 0;
    t[TR_LABEL] = obj[OR_LABEL], t[TR_SIZE] = obj[OR_SIZE];
    t[TR_C16_A] = t[TR_BIRTH_A] = obj[OR_C16_A], t[TR_C16_B] = t[TR_BIRTH_B] = obj[OR_C16_B];
    t[TR_V16_A] = t[TR_V16_B] = 0;
    t[TR_OVERLAP] = 0;
    t[TR_HMAX_BITS] = obj[OR_HMAX_BITS];
    t[TR_FLAGS] = TK_NEW | extra | track_moving(p, t);
}

// how many new tracks a step may make: room in the table and ids below INT32_MAX
MC_FN int32_t track_room(const ObjParams& p, int32_t survivors, int32_t next_id) {
    const int32_t room = p.max_tracks - survivors, ids = 0x7FFFFFFF - next_id;
    return room < 0 ? 0 : (room < ids ? room : ids);
}

// the colour of a track id: a fixed function, bright enough on black; `moving` at full brightness, else at half
MC_FN void colour_track(int32_t id, bool moving, uint8_t* rgb) {
    const uint32_t h = (uint32_t)id * 2654435761u;
    uint32_t r = 96u + ((h >> 8) & 0x7Fu), g = 96u + ((h >> 16) & 0x7Fu), b = 96u + ((h >> 24) & 0x7Fu);
    if (moving) r += 32u, g += 32u, b += 32u;
    else r >>= 1, g >>= 1, b >>= 1;
    rgb[0] = (uint8_t)r, rgb[1] = (uint8_t)g, rgb[2] = (uint8_t)b;
}
// what svh_grid_render_objects draws over the class image on a cell with FLAGS f and the track id (or -1) of the ID plane; false: the
// cell keeps its colour.  Large components are grey, kept cells without a track dark red, other object cells keep the class colour
MC_FN bool colour_obj(uint8_t f, int32_t id, bool moving, uint8_t* rgb) {
    if (f & OF_LARGE) {
        rgb[0] = rgb[1] = rgb[2] = 128;
        return true;
    }
    if (!(f & OF_KEPT)) return false;
    if (id < 0) rgb[0] = 128, rgb[1] = 0, rgb[2] = 0;
    else colour_track(id, moving, rgb);
    return true;
}
// the two marks of a track with a label: the centroid's global cell and that of c16 + 8 * v16 (floor of sixteenths)
MC_FN int32_t cell_of_c16(int64_t c16) { return (int32_t)((c16 >= 0 ? c16 : c16 - 15) / 16); }
// ... the cell ahead (255, 255, 0), drawn first, then the centroid's (255, 255, 255)
MC_FN void colour_mark(bool centre, uint8_t* rgb) { rgb[0] = 255, rgb[1] = 255, rgb[2] = centre ? 255 : 0; }

// ---- the objects of a whole window on the host: a flood fill in ascending order of index ------------------------------------------
// state, hmax, count [nz * nx] under the offsets (oa, ob) -> flags, label [nz * nx], the records of all kept components appended
// to `recs`, stats[OS_CELLS .. OS_LOW] (OS_LAUNCHES is 0)
inline void obj_window(const ObjParams& p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* state, const float* hmax,
                       const int32_t* count, uint8_t* flags, int32_t* label, std::vector<int32_t>* recs, int64_t* stats) {
    const size_t cells = (size_t)nx * (size_t)nz;
    int64_t st[OS_WORDS] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < cells; i++) {
        const bool f = obj_cell(state[i]);
        flags[i] = f ? (uint8_t)OF_OBJECT : (uint8_t)0;
        label[i] = -1;
        st[OS_CELLS] += f ? 1 : 0;
    }
    std::vector<uint32_t> members;
    for (size_t seed = 0; seed < cells; seed++) {
        if (!flags[seed] || label[seed] >= 0) continue;
        members.clear();
        members.push_back((uint32_t)seed);
        label[seed] = (int32_t)seed;
        int64_t sa = 0, sb = 0, pts = 0;
        int32_t a0 = nx, b0 = nz, a1 = -1, b1 = -1, hb = (int32_t)0x80000000;
        for (size_t at = 0; at < members.size(); at++) {
            const uint32_t i = members[at];
            const int32_t ib = (int32_t)(i / (uint32_t)nx), ia = (int32_t)(i - (uint32_t)ib * (uint32_t)nx);
            sa += ia, sb += ib, pts += count[i];
            a0 = ia < a0 ? ia : a0, a1 = ia > a1 ? ia : a1, b0 = ib < b0 ? ib : b0, b1 = ib > b1 ? ib : b1;
            const int32_t h = (int32_t)bits_of(hmax[i]);
            hb = h > hb ? h : hb;
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
        st[OS_COMPONENTS]++;
        const int64_t size = (int64_t)members.size();
        const uint8_t v = obj_verdict(p, (int32_t)size, hb);
        if (v == OF_LARGE) st[OS_LARGE]++;
        if (v == OF_OBJECT) st[OS_LOW]++;
        if (v != OF_KEPT && v != OF_LARGE) continue;
        for (const uint32_t i : members) flags[i] |= v;
        if (v != OF_KEPT) continue;
        st[OS_KEPT]++, st[OS_KEPT_CELLS] += size;
        if (recs) {
            const int32_t r[OBJ_REC] = {(int32_t)seed, (int32_t)size, oa + a0, ob + b0, oa + a1, ob + b1, obj_c16(sa, size) + 16 * oa,
                                        obj_c16(sb, size) + 16 * ob, hb, obj_points(pts)};
            recs->insert(recs->end(), r, r + OBJ_REC);
        }
    }
    if (stats)
        for (int32_t k = 0; k < OS_WORDS; k++) stats[k] = st[k];
}

// the rank of a label among the labels of n ascending records of `stride` int32 (the label first); -1 when it is not among them
inline int32_t obj_rank_of(const int32_t* recs, int32_t n, int32_t stride, int32_t label) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (recs[(size_t)mid * stride] < label) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && recs[(size_t)lo * stride] == label ? lo : -1;
}

// ---- one step of the tracks on the host ------------------------------------------------------------------------------------------
// recs: n_obj object records of a window of nx x nz cells under (oa, ob), label its LABEL plane.  prev_id (may be null when
// n_prev == 0): the ID plane of the step before, written under (poa, pob); prev: its n_prev track records.  next_id: the id the
// next new track gets.  -> tracks (the new table), assign [n_obj], id [nz * nx] (may alias nothing of the inputs),
// stats[TS_BY_OVERLAP .. TS_UNTRACKED] and stats[TS_TRACKS]; returns the next id afterwards
inline int32_t obj_step(const ObjParams& p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const int32_t* recs, int32_t n_obj,
                        const int32_t* label, int32_t poa, int32_t pob, const int32_t* prev_id, const int32_t* prev, int32_t n_prev,
                        int32_t next_id, std::vector<int32_t>* tracks, int32_t* assign, int32_t* id, int64_t* stats) {
    const size_t cells = (size_t)nx * (size_t)nz;
    // the overlap counts of the pairs that occur
    std::unordered_map<uint64_t, int32_t> pairs;
    std::vector<int32_t> rank_at(cells, -1);
    for (size_t i = 0; i < cells; i++) {
        if (label[i] < 0) continue;
        const int32_t r = (i > 0 && label[i - 1] == label[i]) ? rank_at[i - 1] : obj_rank_of(recs, n_obj, OBJ_REC, label[i]);
        rank_at[i] = r;
        if (r < 0 || n_prev < 1 || !prev_id) continue;
        const int32_t ib = (int32_t)(i / (uint32_t)nx), ia = (int32_t)(i - (size_t)ib * (size_t)nx);
        const int64_t pa = (int64_t)ia + oa - poa, pb = (int64_t)ib + ob - pob;
        if (pa < 0 || pa >= nx || pb < 0 || pb >= nz) continue;
        const int32_t tid = prev_id[(size_t)pb * (size_t)nx + (size_t)pa];
        if (tid < 0) continue;
        const int32_t t = obj_rank_of(prev, n_prev, TRACK_REC, tid);
        if (t >= 0) pairs[((uint64_t)(uint32_t)r << 32) | (uint32_t)t]++;
    }
    std::vector<uint64_t> claim_obj((size_t)n_obj, 0), claim_trk((size_t)n_prev, 0);
    std::vector<int32_t> cnt_obj((size_t)n_obj, 0), cnt_trk((size_t)n_prev, 0);
    for (const auto& kv : pairs) {
        if (kv.second < p.min_overlap) continue;
        const int32_t i = (int32_t)(kv.first >> 32), t = (int32_t)(kv.first & 0xFFFFFFFFu);
        claim_obj[i] = std::max(claim_obj[i], obj_claim_key(kv.second, t)), cnt_obj[i]++;
        claim_trk[t] = std::max(claim_trk[t], obj_claim_key(kv.second, i)), cnt_trk[t]++;
    }
    std::vector<int32_t> obj_trk((size_t)n_obj, -1), trk_obj((size_t)n_prev, -1), how((size_t)n_prev, 0), won((size_t)n_prev, 0);
    for (int32_t i = 0; i < n_obj; i++) {
        if (!claim_obj[i]) continue;
        const int32_t t = obj_claim_index(claim_obj[i]);
        if (obj_claim_index(claim_trk[t]) != i) continue;
        obj_trk[i] = t, trk_obj[t] = i, how[t] = TK_BY_OVERLAP, won[t] = obj_claim_overlap(claim_obj[i]);
    }
    if (p.gate > 0) {
        std::vector<uint64_t> pick_obj((size_t)n_obj, GATE_NONE), pick_trk((size_t)n_prev, GATE_NONE);
        for (int32_t i = 0; i < n_obj; i++) {
            if (obj_trk[i] >= 0) continue;
            for (int32_t t = 0; t < n_prev; t++) {
                if (how[t] == TK_BY_OVERLAP) continue;
                const uint64_t d = obj_gate_key(p, prev + (size_t)t * TRACK_REC, recs + (size_t)i * OBJ_REC, 0);
                if (d == GATE_NONE) continue;
                pick_obj[i] = std::min(pick_obj[i], d | (uint32_t)t), pick_trk[t] = std::min(pick_trk[t], d | (uint32_t)i);
            }
        }
        for (int32_t i = 0; i < n_obj; i++) {
            if (pick_obj[i] == GATE_NONE) continue;
            const int32_t t = (int32_t)(pick_obj[i] & 0xFFFFFFFFu);
            if ((int32_t)(pick_trk[t] & 0xFFFFFFFFu) != i) continue;
            obj_trk[i] = t, trk_obj[t] = i, how[t] = TK_BY_GATE;
        }
    }
    int64_t st[TS_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    tracks->clear();
    int32_t t_new[TRACK_REC];
    for (int32_t t = 0; t < n_prev; t++) {
        const int32_t* before = prev + (size_t)t * TRACK_REC;
        const int32_t i = trk_obj[t], split = cnt_trk[t] >= 2 ? (int32_t)TK_SPLIT : 0;
        if (i >= 0) {
            track_match(p, before, recs + (size_t)i * OBJ_REC, how[t], won[t], split | (cnt_obj[i] >= 2 ? (int32_t)TK_MERGED : 0), t_new);
            st[how[t] == TK_BY_OVERLAP ? TS_BY_OVERLAP : TS_BY_GATE]++;
            assign[i] = before[TR_ID];
        } else if (track_miss(p, before, split, t_new)) {
            st[TS_MISSED]++;
        } else {
            st[TS_DROPPED]++;
            continue;
        }
        tracks->insert(tracks->end(), t_new, t_new + TRACK_REC);
    }
    int32_t room = track_room(p, (int32_t)(tracks->size() / TRACK_REC), next_id);
    for (int32_t i = 0; i < n_obj; i++) {
        if (obj_trk[i] >= 0) continue;
        if (room < 1) {
            assign[i] = ASSIGN_UNTRACKED, st[TS_UNTRACKED]++;
            continue;
        }
        track_new(p, next_id, recs + (size_t)i * OBJ_REC, cnt_obj[i] >= 2 ? (int32_t)TK_MERGED : 0, t_new);
        tracks->insert(tracks->end(), t_new, t_new + TRACK_REC);
        assign[i] = next_id++, room--, st[TS_NEW]++;
    }
    st[TS_TRACKS] = (int64_t)(tracks->size() / TRACK_REC);
    for (size_t i = 0; i < cells; i++) id[i] = (rank_at[i] >= 0 && assign[rank_at[i]] >= 0) ? assign[rank_at[i]] : -1;
    if (stats)
        for (int32_t k = TS_TRACKS; k < TS_WORDS; k++) stats[k] = st[k];
    return next_id;
}

}  // namespace grid
}  // namespace svh

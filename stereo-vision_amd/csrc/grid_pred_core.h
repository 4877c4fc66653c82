// The arithmetic of the ground grid's prediction (svh_grid_set_predict, svh_grid_get_pred_plane, svh_grid_get_pred_stats,
// svh_grid_footprint_pred, svh_grid_roll_score_pred, svh_grid_render_pred; include/svh_grid_pred.h, "PREDICTION"): the tracks of
// the objects carried ahead at constant velocity into time slots, and the rollouts cut where the vehicle would meet one.
// THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_pred_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entries svh_test_grid_pred, svh_test_grid_pred_slots and
//     svh_test_grid_pred_roll, which run the host loops below),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_pred_check.cpp,
// and restated in numpy and plain Python by tests/grid_pred_ref.py, which tests/test_grid_pred.py pins by hand and against the test
// entries.  Integers throughout.
//
// PARAMETERS.  slots 1..32 time slots, one bit each of a 32-bit word; stride 1..64 track steps per slot: slot s stands for the time
// s * stride steps after the last step of the tracks; poses_per_step 1..1024 candidate poses per track step; margin 0..16 cells of
// square inflation at slot 0; grow16 0..256 sixteenths of a cell the inflation grows per slot; only_moving 0 or 1.
// The RADIUS of slot s is m(s) = min(16, margin + ((s * grow16) >> 4)).
//
// PREDICTING TRACKS are the tracks of the table as the last step left it that have a label (!= -1) and, if only_moving, the MOVING
// flag.  A missed track has no cell in the ID plane and predicts nothing.
// The DISPLACEMENT of track i at slot s is, per axis, D_i(s) = rdiv64(v16 * s * stride, 16): to the nearest cell, halves towards
// +infinity, in 64 bits (|v16| * 31 * 64 does not fit 32).
//
// PRED is one uint32 per cell of the ID FRAME: the ID plane of the last step under the offsets it was written under, nx x nz cells.
// Bit s of cell p is set iff there is a cell q of the frame with ID[q] the id of a predicting track i, q + D_i(s) inside the frame,
// and the Chebyshev distance of p from q + D_i(s) at most m(s).  A shifted cell outside the frame is dropped before the inflation,
// and the inflation does not leave the frame.  Bits at or above `slots` are 0.  With no tracks PRED is all 0.  PRED is addressed by
// GLOBAL cell; a global cell outside the ID frame reads 0.
// The square inflation is separable, and so it is computed: S = the shifted cells, R[b][a] = OR over |r| <= 16 of S[b][a + r] & ge(|r|),
// PRED[b][a] = OR over |r| <= 16 of R[b + r][a] & ge(|r|), with ge(r) the slots whose radius is at least r.
//
// The SLOT OF POSE t of a candidate is s_t = min(slots - 1, rdiv(t + 1, poses_per_step * stride)).
// The FOOTPRINT PREDICTION of a pose (ga, gb, k) is the OR of PRED over the footprint cells of heading k (the lists of
// grid_roll_core.h): the slots at which the vehicle, standing there, overlaps a predicted object.  It looks neither at the window
// nor at COST.
// SCORING WITH PREDICTION is roll_window of grid_roll_core.h with one more cut: at pose t, F_t = -1 gives status 2, F_t >= stop_cost
// status 1, and then bit s_t of the pose's footprint prediction status ROLL_CUT_OBJECT = 4.  The record has ROLL_PRED_REC = 6 int32:
// the five of the roll record and `slot`, s_t of the cut pose when the status is 4 and -1 otherwise.  Score, feasibility and the best
// are those of grid_roll_core.h.  With PRED all zero the first five fields, the scores and the best are roll_window's.
//
// PRED is an OR, the statistics integer sums, the cut a first index: no byte depends on launch shape or scheduling.
#pragma once
#include <stdint.h>

#include <vector>

#include "grid_core.h"
#include "grid_dyn_core.h"   // rdiv64
#include "grid_obj_core.h"
#include "grid_roll_core.h"

namespace svh {
namespace grid {

constexpr int32_t PRED_MAX_SLOTS = 32, PRED_MAX_STRIDE = 64, PRED_MAX_PPS = 1024, PRED_MAX_RADIUS = 16, PRED_MAX_GROW = 256;
constexpr int32_t ROLL_PRED_REC = 6, RR_SLOT = 5;
constexpr int32_t ROLL_CUT_OBJECT = 4;
// a displacement beyond this leaves every frame (a side is at most 8192 cells); what is stored in 32 bits is clamped here
constexpr int64_t PRED_FAR = (int64_t)1 << 20;
// predicting tracks, source cells (the ID cells of predicting tracks), PRED cells with a bit set, launches of the computation
enum PredStat : int32_t { PS_TRACKS = 0, PS_SOURCES, PS_CELLS, PS_LAUNCHES, PS_WORDS };

struct PredParams {
    int32_t slots;            // 1..32
    int32_t stride;           // 1..64
    int32_t poses_per_step;   // 1..1024
    int32_t margin;           // 0..16
    int32_t grow16;           // 0..256
    int32_t only_moving;      // 0 or 1
};

MC_FN bool pred_ok(const PredParams& p) {
    return p.slots >= 1 && p.slots <= PRED_MAX_SLOTS && p.stride >= 1 && p.stride <= PRED_MAX_STRIDE && p.poses_per_step >= 1 &&
           p.poses_per_step <= PRED_MAX_PPS && p.margin >= 0 && p.margin <= PRED_MAX_RADIUS && p.grow16 >= 0 && p.grow16 <= PRED_MAX_GROW &&
           (p.only_moving == 0 || p.only_moving == 1);
}

MC_FN int32_t pred_radius(const PredParams& p, int32_t s) {
    const int32_t m = p.margin + ((s * p.grow16) >> 4);
    return m < PRED_MAX_RADIUS ? m : PRED_MAX_RADIUS;
}
// the slots below `slots` whose radius is at least r
MC_FN uint32_t pred_ge(const PredParams& p, int32_t r) {
    uint32_t m = 0;
    for (int32_t s = 0; s < p.slots; s++)
        if (pred_radius(p, s) >= r) m |= 1u << s;
    return m;
}
MC_FN uint32_t pred_all(const PredParams& p) { return p.slots >= 32 ? 0xFFFFFFFFu : ((1u << p.slots) - 1u); }

MC_FN bool pred_predicts(const PredParams& p, const int32_t* track) {
    return track[TR_LABEL] != -1 && (!p.only_moving || (track[TR_FLAGS] & TK_MOVING));
}

// one axis of D_i(s), clamped to +-PRED_FAR: beyond it the shifted cell lies outside every frame all the same
MC_FN int32_t pred_disp(const PredParams& p, int32_t v16, int32_t s) {
    const int64_t d = rdiv64((int64_t)v16 * (int64_t)s * (int64_t)p.stride, 16);
    return (int32_t)(d > PRED_FAR ? PRED_FAR : (d < -PRED_FAR ? -PRED_FAR : d));
}

MC_FN int32_t pred_slot(const PredParams& p, int32_t t) {
    const int32_t s = rdiv(t + 1, p.poses_per_step * p.stride);   // t < 1024, the divisor at most 65536
    return s < p.slots - 1 ? s : p.slots - 1;
}

// PRED at the global cell (ga, gb): the frame of nx x nz cells lies under the offsets (poa, pob)
MC_FN uint32_t pred_at(const uint32_t* pred, int32_t nx, int32_t nz, int32_t poa, int32_t pob, int64_t ga, int64_t gb) {
    const int64_t a = ga - poa, b = gb - pob;
    if (a < 0 || a >= nx || b < 0 || b >= nz) return 0u;
    return pred[(size_t)b * (size_t)nx + (size_t)a];
}

// the footprint prediction of the pose whose reference cell is the global cell (ga, gb), with the list of its heading: n pairs
MC_FN uint32_t footprint_pred(const uint32_t* pred, int32_t nx, int32_t nz, int32_t poa, int32_t pob, int64_t ga, int64_t gb, const int32_t* list,
                              int64_t n) {
    uint32_t m = 0;
    for (int64_t i = 0; i < n; i++) m |= pred_at(pred, nx, nz, poa, pob, ga + list[2 * i], gb + list[2 * i + 1]);
    return m;
}

// the colour of a window cell whose PRED word is w != 0 in svh_grid_render_pred: by its lowest set slot
MC_FN void colour_pred(uint32_t w, uint8_t* rgb) {
    int32_t s = 0;
    while (!((w >> s) & 1u)) s++;
    rgb[0] = 255, rgb[1] = (uint8_t)(8 * s), rgb[2] = (uint8_t)(255 - 8 * s);
}

// ---- the host loops ---------------------------------------------------------------------------------------------------------
// id [nz * nx]: the ID plane (null: all -1); tracks: n_tracks records in ascending order of id -> pred [nz * nx],
// stats[PS_TRACKS .. PS_CELLS] (PS_LAUNCHES is 0)
inline void pred_window(const PredParams& p, int32_t nx, int32_t nz, const int32_t* id, const int32_t* tracks, int32_t n_tracks, uint32_t* pred,
                        int64_t* stats) {
    const size_t cells = (size_t)nx * (size_t)nz;
    int64_t st[PS_WORDS] = {0, 0, 0, 0};
    std::vector<uint32_t> shifted(cells, 0u), rows(cells, 0u);
    for (int32_t t = 0; t < n_tracks; t++) st[PS_TRACKS] += pred_predicts(p, tracks + (size_t)t * TRACK_REC) ? 1 : 0;
    for (size_t i = 0; id && n_tracks > 0 && i < cells; i++) {
        if (id[i] < 0) continue;
        const int32_t t = obj_rank_of(tracks, n_tracks, TRACK_REC, id[i]);
        if (t < 0 || !pred_predicts(p, tracks + (size_t)t * TRACK_REC)) continue;
        st[PS_SOURCES]++;
        const int32_t* trk = tracks + (size_t)t * TRACK_REC;
        const int64_t ib = (int64_t)(i / (size_t)nx), ia = (int64_t)(i - (size_t)ib * (size_t)nx);
        for (int32_t s = 0; s < p.slots; s++) {
            const int64_t a = ia + pred_disp(p, trk[TR_V16_A], s), b = ib + pred_disp(p, trk[TR_V16_B], s);
            if (a < 0 || a >= nx || b < 0 || b >= nz) continue;
            shifted[(size_t)b * (size_t)nx + (size_t)a] |= 1u << s;
        }
    }
    uint32_t ge[PRED_MAX_RADIUS + 1];
    for (int32_t r = 0; r <= PRED_MAX_RADIUS; r++) ge[r] = pred_ge(p, r);
    for (int32_t pass = 0; pass < 2; pass++) {
        const uint32_t* src = pass ? rows.data() : shifted.data();
        uint32_t* dst = pass ? pred : rows.data();
        for (int32_t b = 0; b < nz; b++)
            for (int32_t a = 0; a < nx; a++) {
                uint32_t w = 0;
                for (int32_t r = -PRED_MAX_RADIUS; r <= PRED_MAX_RADIUS; r++) {
                    const int32_t qa = pass ? a : a + r, qb = pass ? b + r : b;
                    if (qa < 0 || qa >= nx || qb < 0 || qb >= nz) continue;
                    w |= src[(size_t)qb * (size_t)nx + (size_t)qa] & ge[r < 0 ? -r : r];
                }
                dst[(size_t)b * (size_t)nx + (size_t)a] = w;
            }
    }
    for (size_t i = 0; i < cells; i++) st[PS_CELLS] += pred[i] ? 1 : 0;
    if (stats)
        for (int32_t k = 0; k < PS_WORDS; k++) stats[k] = st[k];
}

// the footprint predictions of n free poses (ga, gb, k), global cells; a heading outside 0..H-1 gives 0
inline void footprint_pred_window(const RollParams& rp, int32_t nx, int32_t nz, int32_t poa, int32_t pob, const uint32_t* pred, const int32_t* offs,
                                  const int64_t* start, const int32_t* poses, int64_t n, uint32_t* out) {
    for (int64_t i = 0; i < n; i++) {
        const int32_t k = poses[3 * i + 2];
        out[i] = (k < 0 || k >= 8 * rp.m) ? 0u
                                          : footprint_pred(pred, nx, nz, poa, pob, poses[3 * i], poses[3 * i + 1], offs + 2 * start[k],
                                                           start[k + 1] - start[k]);
    }
}

// roll_window of grid_roll_core.h with the PRED plane of a frame of pnx x pnz cells under (poa, pob): recs (6 K), scores (K), either
// may be null; returns the best
inline int32_t roll_pred_window(const RollParams& p, const PredParams& pp, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* cost,
                                const int32_t* pot, int32_t pnx, int32_t pnz, int32_t poa, int32_t pob, const uint32_t* pred, const int32_t* offs,
                                const int64_t* start, const int32_t* cands, int32_t K, int32_t T, int32_t ga0, int32_t gb0, int32_t* recs,
                                int64_t* scores) {
    int32_t best = -1;
    int64_t best_score = ROLL_INFEASIBLE;
    for (int32_t c = 0; c < K; c++) {
        const int32_t* cand = cands + (size_t)c * (size_t)T * 3;
        const int32_t n_c = roll_len(cand, T);
        int32_t rec[ROLL_PRED_REC] = {0, n_c == 0 ? (int32_t)ROLL_EMPTY : (int32_t)ROLL_COMPLETE, -1, 0, PLAN_FAR, -1};
        for (int32_t t = 0; t < n_c; t++) {
            const int32_t k = cand[3 * t + 2];
            const int64_t ga = (int64_t)ga0 + cand[3 * t], gb = (int64_t)gb0 + cand[3 * t + 1], a = ga - oa, b = gb - ob;
            const int32_t* list = offs + 2 * start[k];
            const int64_t n = start[k + 1] - start[k];
            const int32_t f = footprint_cost(cost, nx, nz, a, b, list, n, p.unknown_cost);
            int32_t cut = roll_cut(f, p.stop_cost);
            const int32_t s = pred_slot(pp, t);
            if (!cut && ((footprint_pred(pred, pnx, pnz, poa, pob, ga, gb, list, n) >> s) & 1u)) cut = ROLL_CUT_OBJECT, rec[RR_SLOT] = s;
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
            for (int32_t k = 0; k < ROLL_PRED_REC; k++) recs[(size_t)c * ROLL_PRED_REC + k] = rec[k];
        if (scores) scores[c] = s;
    }
    return best;
}

}  // namespace grid
}  // namespace svh

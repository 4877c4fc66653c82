// The arithmetic of the ground grid's alignment layer (svh_grid_*align*; include/svh_grid.h, "ALIGN"): correlative scan-to-map
// matching.  Every pose correction of a small window -- a rotation about the vertical through a pivot and a translation -- is
// scored by how well the obstacle points of a frame that is about to be added fall on the obstacle cells the window already holds,
// and the best is taken.  THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/grid_align_kernels.hip,
//   * the host compiler into csrc/grid_engine.cpp (the test entry svh_test_grid_align, which runs align_window below),
//   * g++ -fsanitize=address,undefined into tests/cxx/grid_align_check.cpp,
// and restated in numpy by tests/grid_align_ref.py, which tests/test_grid_align.py pins by hand and against the test entry.
// After the placement of a point (fp32 in the order written, one rounding per operation, as grid_core.h) everything is integer
// arithmetic on the finished STATE plane in logical (window) order; the torus plays no part.
//
// SUBS.  A sub is a quarter of a cell per axis (ALIGN_SUB = 4).  The global sub of a ground position (a, b) is
// ua = (int)floorf(div_rn(a - x0, cell) * 4.f), ub likewise with z0; the multiplication by 4 is exact.  The range decision is
// made on the float before the conversion, as global_cell does: fabsf(floorf(quotient)) < CELL_LIMIT, so |ua| < 2^22, and
// ua >> 2 is exactly the global cell ga of place().
// PIVOT.  A map-frame position (the camera's) rounded to float once; its ground coordinates are row(T, .) and row(T + 4, .), its
// global sub (Pa, Pb).  It need not lie inside the window.
// SCAN.  A point (x, y, z, val) is a scan point iff x, y, z, a, b, h are finite, |h| < H_LIMIT, step < h <= clearance (what would
// make its cell an obstacle) and it has a global sub.  With Rg = (int)floorf(div_rn(range, cell)) in 1..256 it is KEPT iff
// |ua - Pa| <= 4 Rg and |ub - Pb| <= 4 Rg.  The SCAN is the set of distinct kept subs, each counted once however many points fall
// into it: near surfaces do not outvote far ones, and the scan depends on neither order nor multiplicity.  n_scan is its size, at
// most (8 Rg + 1)^2; n_points the number of kept points before the set is formed.  The scan may hold subs outside the window.
// The list of the scan ascends by (ub, ua).
// FIELD.  F is one byte per window cell.  reach_cells = (int)ceil((double)reach / (double)cell) in 1..32, R2 = reach_cells^2.
// d2 is the exact squared distance in cells to the nearest cell of the window whose class (bits 0-1 of STATE) is obstacle
// (col_step / row_dist2 of grid_core.h); F = (255 * (R2 + 1 - d2)) / (R2 + 1) in integer division for d2 <= R2, else 0.
// SAMPLE.  The field at a global sub (ua, ub) is bilinear between cell centres, in eighths of a cell: pa = 2 ua - 3 - 8 oa,
// g0a = pa >> 3 (arithmetic), fa = pa - 8 g0a, one of 1, 3, 5, 7; the b axis alike with ob.  The four cells (g0a + i, g0b + j),
// i, j in {0, 1}, weigh (i ? fa : 8 - fa) * (j ? fb : 8 - fb); a cell outside the window contributes 0; the sample is
// (sum + 32) >> 6, in 0..255.
// CANDIDATES.  (k, ta, tb): k in -K..K, K = rot_n in 0..32, D = rot_den in 16..4096; ta, tb in -W..W subs, W = trans_n in 0..32.
// Rotation k is the rotation by the direction (D, k), from the a axis towards the b axis: with n = sqrt((double)(D D + k k)),
// cq = (int32)rint((double)D * 16384.0 / n), sq = (int32)rint((double)k * 16384.0 / n) -- filled once on the host in double, one
// IEEE operation per step, no trigonometric function.  k = 0 gives cq = 16384, sq = 0, the identity on every (ra, rb).  A scan
// sub with (ra, rb) = (ua - Pa, ub - Pb) is placed at
//   (Pa + ((cq ra - sq rb + 8192) >> 14) + ta, Pb + ((sq ra + cq rb + 8192) >> 14) + tb);
// |ra|, |rb| <= 1024 and cq, |sq| <= 16384: the products stay below 2^25 and their sum below 2^26.
// VOLUME AND BEST.  SCORE(k, ta, tb) is the sum of the samples over the scan, int32 (2049^2 * 255 < 2^31), stored as
// [(k + K)][(tb + W)][(ta + W)].  BEST is the candidate with the greatest score; among equal scores the least
// m = k^2 + ta^2 + tb^2, among those the lowest volume index: the minimum of the unique key align_key.  `ties` is the number of
// candidates whose score equals the best.  A flat volume returns the identity, the only candidate with m = 0.
// RECORD, ALIGN_REC = 8 int32: status, k, ta, tb, score, SCORE(0, 0, 0), n_scan, ties.  ALIGN_OK 0; ALIGN_FEW 1: n_scan < min_scan,
// no volume, k = ta = tb = score = identity = ties = 0; ALIGN_FLAT 2: the best score is 0, the identity is returned.
//
// SCHEDULE INDEPENDENCE.  The scan is a set, the field a function of STATE, a score an integer sum over a set and the best the
// minimum of a unique key: no byte depends on launch shape or scheduling.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "grid_core.h"

namespace svh {
namespace grid {

constexpr int32_t ALIGN_SUB = 4;
constexpr int32_t ALIGN_MAX_REACH = 32, ALIGN_MAX_RG = 256, ALIGN_MAX_K = 32, ALIGN_MAX_W = 32;
constexpr int32_t ALIGN_MIN_D = 16, ALIGN_MAX_D = 4096;
constexpr int32_t ALIGN_ROT = 16384, ALIGN_ROT_SHIFT = 14;
constexpr int32_t ALIGN_SUB_LIMIT = 1 << 22;            // |ua|, |ub| < this
constexpr int32_t ALIGN_REC = 8;
constexpr int32_t ALIGN_MAX_ROTS = 2 * ALIGN_MAX_K + 1;
enum AlignRec : int32_t { AR_STATUS = 0, AR_K, AR_TA, AR_TB, AR_SCORE, AR_IDENTITY, AR_SCAN, AR_TIES };
enum AlignStatus : int32_t { ALIGN_OK = 0, ALIGN_FEW = 1, ALIGN_FLAT = 2 };
// svh_grid_render_align: the cells of the scan at the identity, those of the scan placed at the best, the pivot's cell
constexpr uint8_t ALIGN_SCAN_R = 255, ALIGN_SCAN_G = 224, ALIGN_SCAN_B = 0, ALIGN_BEST_R = 0, ALIGN_BEST_G = 224, ALIGN_BEST_B = 255;

// svh_grid_align_params and what align_derive derives from it for the grid's cell
struct AlignParams {
    float reach, range;
    int32_t rot_den, rot_n, trans_n, min_scan;
    int32_t reach_cells, Rg;   // 0 until align_derive succeeds
};

// the checks behind SVH_ERR_BAD_ARG of svh_grid_set_align, and the derived values
MC_FN bool align_derive(AlignParams& p, float cell) {
    p.reach_cells = p.Rg = 0;
    if (!(finite_f(p.reach) && p.reach > 0.f && finite_f(p.range) && p.range > 0.f && p.rot_den >= ALIGN_MIN_D && p.rot_den <= ALIGN_MAX_D &&
          p.rot_n >= 0 && p.rot_n <= ALIGN_MAX_K && p.trans_n >= 0 && p.trans_n <= ALIGN_MAX_W && p.min_scan >= 1))
        return false;
    const double r = ceil((double)p.reach / (double)cell);
    const float q = floorf(div_rn(p.range, cell));
    if (!(r >= 1.0 && r <= (double)ALIGN_MAX_REACH && q >= 1.f && q <= (float)ALIGN_MAX_RG)) return false;
    p.reach_cells = (int32_t)r, p.Rg = (int32_t)q;
    return true;
}

// cs[2 i], cs[2 i + 1] = cq, sq of rotation k = i - K, i = 0 .. 2 K.  Host only: double, one operation per step
inline void align_rot_table(int32_t D, int32_t K, int32_t* cs) {
    for (int32_t k = -K; k <= K; k++) {
        const double n = sqrt((double)(D * D + k * k));
        const double c = (double)D * 16384.0, s = (double)k * 16384.0;
        cs[2 * (k + K)] = (int32_t)rint(c / n), cs[2 * (k + K) + 1] = (int32_t)rint(s / n);
    }
}

// the global sub of a ground position; false: it has none
MC_FN bool align_sub(const Params& p, float a, float b, int32_t* ua, int32_t* ub) {
    const float qa = div_rn(a - p.x0, p.cell), qb = div_rn(b - p.z0, p.cell);
    if (!(fabsf(floorf(qa)) < CELL_LIMIT && fabsf(floorf(qb)) < CELL_LIMIT)) return false;   // NaN and Inf fail here
    *ua = (int32_t)floorf(qa * 4.f), *ub = (int32_t)floorf(qb * 4.f);
    return true;
}

// the pivot's global sub from its float-rounded position; false: not finite or not placeable
MC_FN bool align_pivot(const Params& p, float x, float y, float z, int32_t* Pa, int32_t* Pb) {
    const float a = row(p.T, x, y, z), b = row(p.T + 4, x, y, z);
    if (!(finite_f(x) && finite_f(y) && finite_f(z) && finite_f(a) && finite_f(b))) return false;
    return align_sub(p, a, b, Pa, Pb);
}

// a scan point's global sub; false: the point is no scan point
MC_FN bool align_scan_point(const Params& p, float x, float y, float z, int32_t* ua, int32_t* ub) {
    const float a = row(p.T, x, y, z), b = row(p.T + 4, x, y, z), h = row(p.T + 8, x, y, z);
    if (!(finite_f(x) && finite_f(y) && finite_f(z) && finite_f(a) && finite_f(b) && finite_f(h))) return false;
    if (!(fabsf(h) < H_LIMIT && h > p.step && h <= p.clearance)) return false;
    return align_sub(p, a, b, ua, ub);
}

// kept: inside the box about the pivot.  |ua|, |Pa| < 2^22: the differences are exact
MC_FN bool align_kept(int32_t Rg, int32_t Pa, int32_t Pb, int32_t ua, int32_t ub) {
    const int32_t ra = ua - Pa, rb = ub - Pb, lim = ALIGN_SUB * Rg;
    return ra >= -lim && ra <= lim && rb >= -lim && rb <= lim;
}

// the side of the box in subs, and the bit of a kept sub in the bitmap of the box: rows of ub, ascending by (ub, ua)
MC_FN int32_t align_side(int32_t Rg) { return 2 * ALIGN_SUB * Rg + 1; }
MC_FN uint32_t align_bit(int32_t Rg, int32_t Pa, int32_t Pb, int32_t ua, int32_t ub) {
    return (uint32_t)(ub - Pb + ALIGN_SUB * Rg) * (uint32_t)align_side(Rg) + (uint32_t)(ua - Pa + ALIGN_SUB * Rg);
}

MC_FN uint8_t align_field(int32_t d2, int32_t R2) { return d2 <= R2 ? (uint8_t)((255 * (R2 + 1 - d2)) / (R2 + 1)) : (uint8_t)0; }

// the field sampled at the global sub (ua, ub); |ua|, |ub| < 2^23
MC_FN int32_t align_sample(const uint8_t* F, int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t ua, int32_t ub) {
    const int32_t pa = 2 * ua - 3 - 8 * oa, pb = 2 * ub - 3 - 8 * ob;
    const int32_t g0a = pa >> 3, g0b = pb >> 3;
    if (g0a < -1 || g0a >= nx || g0b < -1 || g0b >= nz) return 0;   // all four cells are outside
    const int32_t fa = pa - 8 * g0a, fb = pb - 8 * g0b;
    const bool a0 = g0a >= 0, a1 = g0a + 1 < nx, b0 = g0b >= 0, b1 = g0b + 1 < nz;
    const size_t at = (size_t)(b0 ? g0b : 0) * (size_t)nx, at1 = (size_t)(g0b + 1) * (size_t)nx;
    int32_t sum = 0;
    if (b0 && a0) sum += (8 - fa) * (8 - fb) * (int32_t)F[at + (size_t)g0a];
    if (b0 && a1) sum += fa * (8 - fb) * (int32_t)F[at + (size_t)(g0a + 1)];
    if (b1 && a0) sum += (8 - fa) * fb * (int32_t)F[at1 + (size_t)g0a];
    if (b1 && a1) sum += fa * fb * (int32_t)F[at1 + (size_t)(g0a + 1)];
    return (sum + 32) >> 6;
}

// (ra, rb) turned by rotation (cq, sq)
MC_FN void align_turn(int32_t cq, int32_t sq, int32_t ra, int32_t rb, int32_t* qa, int32_t* qb) {
    *qa = (cq * ra - sq * rb + (ALIGN_ROT >> 1)) >> ALIGN_ROT_SHIFT;
    *qb = (sq * ra + cq * rb + (ALIGN_ROT >> 1)) >> ALIGN_ROT_SHIFT;
}

MC_FN int32_t align_volume_size(int32_t K, int32_t W) { return (2 * K + 1) * (2 * W + 1) * (2 * W + 1); }

// the unique key whose minimum is the best: the inverted score (30 bits), m (12 bits), the volume index (19 bits)
MC_FN uint64_t align_key(int32_t score, int32_t K, int32_t W, int32_t idx) {
    const int32_t side = 2 * W + 1;
    const int32_t k = idx / (side * side) - K, rem = idx % (side * side), tb = rem / side - W, ta = rem % side - W;
    const int32_t m = k * k + ta * ta + tb * tb;
    return ((uint64_t)(0x3FFFFFFF - score) << 31) | ((uint64_t)m << 19) | (uint64_t)idx;
}

// the record of the best key and its ties
MC_FN void align_record(uint64_t key, int32_t K, int32_t W, int32_t identity, int32_t n_scan, int32_t ties, int32_t* rec) {
    const int32_t side = 2 * W + 1, idx = (int32_t)(key & 0x7FFFFu), score = 0x3FFFFFFF - (int32_t)(key >> 31);
    const int32_t rem = idx % (side * side);
    const bool flat = score == 0;
    rec[AR_STATUS] = flat ? ALIGN_FLAT : ALIGN_OK;
    rec[AR_K] = idx / (side * side) - K, rec[AR_TA] = rem % side - W, rec[AR_TB] = rem / side - W;
    rec[AR_SCORE] = score, rec[AR_IDENTITY] = identity, rec[AR_SCAN] = n_scan, rec[AR_TIES] = ties;
}
MC_FN void align_record_few(int32_t n_scan, int32_t* rec) {
    for (int32_t i = 0; i < ALIGN_REC; i++) rec[i] = 0;
    rec[AR_STATUS] = ALIGN_FEW, rec[AR_SCAN] = n_scan;
}

// the colour of svh_grid_render_align's primitive `what` (0 the scan at the identity, 1 the scan at the best, 2 the pivot)
MC_FN void colour_align(int32_t what, uint8_t* rgb) {
    if (what == 0) rgb[0] = ALIGN_SCAN_R, rgb[1] = ALIGN_SCAN_G, rgb[2] = ALIGN_SCAN_B;
    else if (what == 1) rgb[0] = ALIGN_BEST_R, rgb[1] = ALIGN_BEST_G, rgb[2] = ALIGN_BEST_B;
    else rgb[0] = rgb[1] = rgb[2] = 255;
}

// ---- the host forms --------------------------------------------------------------------------------------------------------
// F [nz * nx] from the STATE plane
inline void align_field_window(int32_t reach, int32_t nx, int32_t nz, const uint8_t* state, uint8_t* F) {
    std::vector<uint16_t> g((size_t)nx * (size_t)nz);
    for (int32_t ia = 0; ia < nx; ia++) {
        int32_t d = reach + 1;
        for (int32_t ib = 0; ib < nz; ib++) {
            const size_t i = (size_t)ib * nx + ia;
            g[i] = (uint16_t)(d = col_step(d, (state[i] & 3) == C_OBSTACLE, reach));
        }
        d = reach + 1;
        for (int32_t ib = nz - 1; ib >= 0; ib--) {
            const size_t i = (size_t)ib * nx + ia;
            d = col_step(d, (state[i] & 3) == C_OBSTACLE, reach);
            g[i] = (uint16_t)(d < (int32_t)g[i] ? d : (int32_t)g[i]);
        }
    }
    for (int32_t ib = 0; ib < nz; ib++)
        for (int32_t ia = 0; ia < nx; ia++) {
            const int32_t lo = ia - reach < 0 ? 0 : ia - reach, hi = ia + reach > nx - 1 ? nx - 1 : ia + reach;
            const int32_t d2 = row_dist2(g.data() + (size_t)ib * nx, 0, ia, lo, hi, reach);
            F[(size_t)ib * nx + ia] = align_field(d2 == DIST2_FAR ? reach * reach + 1 : d2, reach * reach);
        }
}

// the scan of n points about the pivot sub: the distinct kept subs as pairs (ua, ub) ascending by (ub, ua); returns n_points
inline int64_t align_scan_points(const Params& p, int32_t Rg, int32_t Pa, int32_t Pb, const float* xyzv, int64_t n, std::vector<int32_t>* scan) {
    std::vector<uint32_t> bits;
    int64_t kept = 0;
    for (int64_t i = 0; i < n; i++) {
        int32_t ua, ub;
        if (!align_scan_point(p, xyzv[4 * i], xyzv[4 * i + 1], xyzv[4 * i + 2], &ua, &ub) || !align_kept(Rg, Pa, Pb, ua, ub)) continue;
        bits.push_back(align_bit(Rg, Pa, Pb, ua, ub));
        kept++;
    }
    std::sort(bits.begin(), bits.end());
    bits.erase(std::unique(bits.begin(), bits.end()), bits.end());
    const uint32_t side = (uint32_t)align_side(Rg);
    scan->clear();
    for (uint32_t b : bits) {
        scan->push_back((int32_t)(b % side) - ALIGN_SUB * Rg + Pa);
        scan->push_back((int32_t)(b / side) - ALIGN_SUB * Rg + Pb);
    }
    return kept;
}

// ... of n subs given as pairs (ua, ub), |ua|, |ub| < 2^22
inline int64_t align_scan_subs(int32_t Rg, int32_t Pa, int32_t Pb, const int32_t* subs, int64_t n, std::vector<int32_t>* scan) {
    std::vector<uint32_t> bits;
    int64_t kept = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!align_kept(Rg, Pa, Pb, subs[2 * i], subs[2 * i + 1])) continue;
        bits.push_back(align_bit(Rg, Pa, Pb, subs[2 * i], subs[2 * i + 1]));
        kept++;
    }
    std::sort(bits.begin(), bits.end());
    bits.erase(std::unique(bits.begin(), bits.end()), bits.end());
    const uint32_t side = (uint32_t)align_side(Rg);
    scan->clear();
    for (uint32_t b : bits) {
        scan->push_back((int32_t)(b % side) - ALIGN_SUB * Rg + Pa);
        scan->push_back((int32_t)(b / side) - ALIGN_SUB * Rg + Pb);
    }
    return kept;
}

// The volume and the record of a scan on a field.  `volume` has align_volume_size(K, W) entries and may be null; with fewer than
// min_scan subs it is not written.
inline void align_window(const AlignParams& p, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* F, int32_t Pa, int32_t Pb,
                         const int32_t* scan, int64_t n_scan, int32_t* volume, int32_t* rec) {
    if (n_scan < (int64_t)p.min_scan) {
        align_record_few((int32_t)n_scan, rec);
        return;
    }
    const int32_t K = p.rot_n, W = p.trans_n, side = 2 * W + 1;
    int32_t cs[2 * ALIGN_MAX_ROTS];
    align_rot_table(p.rot_den, K, cs);
    std::vector<int32_t> vol((size_t)align_volume_size(K, W), 0), turned(2 * (size_t)n_scan);
    for (int32_t k = -K; k <= K; k++) {
        for (int64_t i = 0; i < n_scan; i++) {
            align_turn(cs[2 * (k + K)], cs[2 * (k + K) + 1], scan[2 * i] - Pa, scan[2 * i + 1] - Pb, &turned[2 * i], &turned[2 * i + 1]);
            turned[2 * i] += Pa, turned[2 * i + 1] += Pb;
        }
        for (int32_t tb = -W; tb <= W; tb++)
            for (int32_t ta = -W; ta <= W; ta++) {
                int32_t s = 0;
                for (int64_t i = 0; i < n_scan; i++) s += align_sample(F, nx, nz, oa, ob, turned[2 * i] + ta, turned[2 * i + 1] + tb);
                vol[((size_t)(k + K) * side + (size_t)(tb + W)) * side + (size_t)(ta + W)] = s;
            }
    }
    uint64_t best = ~(uint64_t)0;
    for (size_t i = 0; i < vol.size(); i++) best = std::min(best, align_key(vol[i], K, W, (int32_t)i));
    const int32_t top = 0x3FFFFFFF - (int32_t)(best >> 31);
    int32_t ties = 0;
    for (size_t i = 0; i < vol.size(); i++) ties += vol[i] == top ? 1 : 0;
    align_record(best, K, W, vol[((size_t)K * side + (size_t)W) * side + (size_t)W], (int32_t)n_scan, ties, rec);
    if (volume) std::copy(vol.begin(), vol.end(), volume);
}

// svh_grid_align_correction: M (4 x 4, row major) from the float-rounded T, the float-rounded pivot and (k, ta, tb), in double:
// X' = p + Rot(X - p) + (ta cell / 4) e_a + (tb cell / 4) e_b with e_a, e_b, e_h the first three columns of T's rows; Rot turns
// the e_a / e_b components by (cos, sin) = (D / n, k / n) and leaves the e_h component alone.  Exact for a T with orthonormal rows.
inline void align_correction(const Params& p, int32_t D, int32_t k, int32_t ta, int32_t tb, const float pivot[3], double M[16]) {
    const double n = sqrt((double)(D * D + k * k)), c = (double)D / n, s = (double)k / n;
    const double ea[3] = {p.T[0], p.T[1], p.T[2]}, eb[3] = {p.T[4], p.T[5], p.T[6]}, eh[3] = {p.T[8], p.T[9], p.T[10]};
    const double da = (double)ta * (double)p.cell / 4.0, db = (double)tb * (double)p.cell / 4.0;
    for (int i = 0; i < 3; i++) {
        double t = (double)pivot[i];   // p - R p first: exactly zero where R is the identity
        for (int j = 0; j < 3; j++) {
            const double r = ((c * (ea[i] * ea[j]) - s * (ea[i] * eb[j])) + (s * (eb[i] * ea[j]) + c * (eb[i] * eb[j]))) + eh[i] * eh[j];
            M[4 * i + j] = r;
            t -= r * (double)pivot[j];
        }
        M[4 * i + 3] = t + (da * ea[i] + db * eb[i]);
    }
    M[12] = M[13] = M[14] = 0.0, M[15] = 1.0;
}

}  // namespace grid
}  // namespace svh

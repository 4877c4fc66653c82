// The prediction of the ground grid on the device (svh_grid_get_pred_plane, svh_grid_footprint_pred, svh_grid_roll_score_pred,
// svh_grid_render_pred; include/svh_grid_pred.h, "PREDICTION").  The arithmetic is csrc/grid_pred_core.h: PRED is an OR, the
// statistics integer sums, the cut a first index and the best the minimum of unique keys, so nothing here depends on the launch shape
// or the scheduling.
//
//   k_grid_pred_disp        one lane per (track, slot): whether the track predicts, and D_i(s), 64-bit products clamped into an int2.
//   k_grid_pred_scatter     the lanes stride over the ID frame.  A cell with an id finds its track's row by binary search over the
//                           ids (ascending, not contiguous; at most 4096, staged in LDS, 16 KiB), walks the row of displacements,
//                           merges consecutive slots with equal displacement into one mask and issues one atomicOr per distinct
//                           target cell: a slow object costs one atomic per cell, not 32.
//   k_grid_pred_rows, _cols the square inflation as two separable passes over LDS tiles with a halo of 16, word-parallel over the
//                           slots: at radius r the neighbour's word is ORed in under the mask of the slots whose radius is at least
//                           r.  Skipped when every radius is 0; the scatter then counts the cells itself (the atomicOr that finds a
//                           word zero is the one that makes it non-zero).
//   k_grid_roll_score_pred  the shape of k_grid_roll_score (csrc/grid_roll_kernels.hip): a workgroup per candidate, lane groups sized
//                           by the longest footprint list, the LDS `cut_at` minimum.  Each footprint cell costs two reads: the COST
//                           byte under the window's offsets and the PRED word under the ID frame's.  An object cut is marked in
//                           bit 14 of the pose's F in LDS (F < 256).
//   k_grid_footprint_pred   free poses: a group of lanes per pose, the groups stride over the poses.
//   k_grid_pred_overlay     one lane per window cell.
// All loops are bounded and no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grid_internal.h"
#include "grid_pred_core.h"

namespace svh {
namespace grid {
namespace {

constexpr int32_t OBJECT_CUT_BIT = 0x4000;   // in the int16 F of a pose kept in LDS

__global__ __launch_bounds__(PRED_BLOCK) void k_grid_pred_disp(PredJob j) {
    const int32_t i = (int32_t)(blockIdx.x * PRED_BLOCK + threadIdx.x);
    if (i >= j.n_tracks * PRED_MAX_SLOTS) return;
    const int32_t row = i / PRED_MAX_SLOTS, s = i % PRED_MAX_SLOTS;
    const int32_t* t = j.tracks + (size_t)row * TRACK_REC;
    j.disp[i] = s < j.pp.slots ? make_int2(pred_disp(j.pp, t[TR_V16_A], s), pred_disp(j.pp, t[TR_V16_B], s)) : make_int2(0, 0);
    if (s == 0) {
        const bool p = pred_predicts(j.pp, t);
        j.predicts[row] = p ? 1 : 0;
        if (p) atomicAdd(&j.ctl[PS_TRACKS], 1ull);
    }
}

__global__ __launch_bounds__(PRED_BLOCK) void k_grid_pred_scatter(PredJob j) {
    __shared__ int32_t ids[OBJ_MAX_TRACKS];
    for (int32_t i = (int32_t)threadIdx.x; i < j.n_tracks; i += (int32_t)PRED_BLOCK) ids[i] = j.tracks[(size_t)i * TRACK_REC + TR_ID];
    __syncthreads();
    const int64_t cells = (int64_t)j.nx * j.nz;
    const bool flat = j.max_r == 0;
    unsigned long long sources = 0, lit = 0;
    for (int64_t c = (int64_t)blockIdx.x * PRED_BLOCK + threadIdx.x; c < cells; c += (int64_t)gridDim.x * PRED_BLOCK) {
        const int32_t id = j.id[c];
        if (id < 0) continue;
        int32_t lo = 0, hi = j.n_tracks;
        while (lo < hi) {   // at most 13 rounds
            const int32_t mid = (lo + hi) >> 1;
            if (ids[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= j.n_tracks || ids[lo] != id || !j.predicts[lo]) continue;
        sources++;
        const int32_t ib = (int32_t)(c / j.nx), ia = (int32_t)(c - (int64_t)ib * j.nx);
        const int2* d = j.disp + (size_t)lo * PRED_MAX_SLOTS;
        int2 cur = d[0];
        uint32_t mask = 1u;
        for (int32_t s = 1; s <= j.pp.slots; s++) {
            if (s < j.pp.slots) {
                const int2 nxt = d[s];
                if (nxt.x == cur.x && nxt.y == cur.y) {
                    mask |= 1u << s;
                    continue;
                }
            }
            const int32_t a = ia + cur.x, b = ib + cur.y;   // |D| <= 2^20
            if (a >= 0 && a < j.nx && b >= 0 && b < j.nz) {
                const uint32_t old = atomicOr(&j.pred[(size_t)b * (size_t)j.nx + (size_t)a], mask);
                if (flat && old == 0u) lit++;
            }
            if (s < j.pp.slots) cur = d[s], mask = 1u << s;
        }
    }
    if (sources) atomicAdd(&j.ctl[PS_SOURCES], sources);
    if (lit) atomicAdd(&j.ctl[PS_CELLS], lit);
}

// pred (the shifted cells) -> rows: one workgroup per 256 cells of a row
__global__ __launch_bounds__(PRED_BLOCK) void k_grid_pred_rows(PredJob j) {
    __shared__ uint32_t tile[PRED_ROWS_TILE];
    const int32_t b = (int32_t)blockIdx.y, x0 = (int32_t)(blockIdx.x * PRED_BLOCK), tid = (int32_t)threadIdx.x;
    const uint32_t* src = j.pred + (size_t)b * (size_t)j.nx;
    for (int32_t i = tid; i < PRED_ROWS_TILE; i += (int32_t)PRED_BLOCK) {
        const int32_t a = x0 - PRED_MAX_RADIUS + i;
        tile[i] = (a >= 0 && a < j.nx) ? src[a] : 0u;
    }
    __syncthreads();
    const int32_t a = x0 + tid;
    if (a >= j.nx) return;
    uint32_t w = 0;
    for (int32_t r = -j.max_r; r <= j.max_r; r++) w |= tile[tid + PRED_MAX_RADIUS + r] & j.ge[r < 0 ? -r : r];
    j.rows[(size_t)b * (size_t)j.nx + (size_t)a] = w;
}

// rows -> pred: one workgroup of 64 x 4 lanes per 64 x 32 cells, a lane writes 8 cells of its column
__global__ __launch_bounds__(PRED_BLOCK) void k_grid_pred_cols(PredJob j) {
    constexpr int32_t H = PRED_COLS_Y + 2 * PRED_MAX_RADIUS;
    __shared__ uint32_t tile[H][PRED_COLS_X];
    const int32_t tx = (int32_t)threadIdx.x % PRED_COLS_X, ty = (int32_t)threadIdx.x / PRED_COLS_X;
    const int32_t a = (int32_t)blockIdx.x * PRED_COLS_X + tx, y0 = (int32_t)blockIdx.y * PRED_COLS_Y;
    for (int32_t rr = ty; rr < H; rr += (int32_t)PRED_BLOCK / PRED_COLS_X) {
        const int32_t b = y0 - PRED_MAX_RADIUS + rr;
        tile[rr][tx] = (a < j.nx && b >= 0 && b < j.nz) ? j.rows[(size_t)b * (size_t)j.nx + (size_t)a] : 0u;
    }
    __syncthreads();
    constexpr int32_t PER = PRED_COLS_Y / ((int32_t)PRED_BLOCK / PRED_COLS_X);
    unsigned long long lit = 0;
    for (int32_t k = 0; k < PER; k++) {
        const int32_t yy = ty * PER + k, b = y0 + yy;
        if (a >= j.nx || b >= j.nz) continue;
        uint32_t w = 0;
        for (int32_t r = -j.max_r; r <= j.max_r; r++) w |= tile[yy + PRED_MAX_RADIUS + r][tx] & j.ge[r < 0 ? -r : r];
        j.pred[(size_t)b * (size_t)j.nx + (size_t)a] = w;
        lit += w ? 1 : 0;
    }
    if (lit) atomicAdd(&j.ctl[PS_CELLS], lit);
}

// the maximum of COST and the OR of PRED over the footprint cells of the list [s, s + n) round the global cell (ga, gb), in every lane
// of a group of j.r.group lanes (a power of two, at most 64)
__device__ __forceinline__ void group_worst_pred(const RollPredJob& j, int64_t ga, int64_t gb, int32_t s, int32_t n, int32_t lane, bool cost,
                                                 int32_t* worst_out, uint32_t* mask_out) {
    const RollJob& r = j.r;
    int32_t worst = 0;
    uint32_t m = 0;
    for (int32_t i = lane; i < n; i += r.group) {
        const int2 o = r.offs[s + i];
        if (cost) {
            const int32_t v = roll_cell(r.cost, r.nx, r.nz, ga - r.oa + o.x, gb - r.ob + o.y, r.rp.unknown_cost);
            worst = v > worst ? v : worst;
        }
        m |= pred_at(j.pred, r.nx, r.nz, j.poa, j.pob, ga + o.x, gb + o.y);
    }
    for (int32_t off = r.group >> 1; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(worst, off);
        worst = o > worst ? o : worst;
        m |= (uint32_t)__shfl_xor((int32_t)m, off);
    }
    *worst_out = worst, *mask_out = m;
}

__global__ __launch_bounds__(ROLL_BLOCK) void k_grid_roll_score_pred(RollPredJob j) {
    __shared__ int16_t fs[ROLL_MAX_T];
    __shared__ int32_t cut_at;
    __shared__ int32_t red_max[ROLL_BLOCK / 64], red_sum[ROLL_BLOCK / 64];
    const RollJob& r = j.r;
    const int32_t c = (int32_t)blockIdx.x, tid = (int32_t)threadIdx.x;
    const int32_t n_c = r.lens[c];
    const int32_t* cand = r.cands + (size_t)c * (size_t)r.T * 3;
    if (tid == 0) cut_at = n_c;
    __syncthreads();
    const int32_t per_block = (int32_t)ROLL_BLOCK / r.group, grp = tid / r.group, lane = tid % r.group;
    for (int32_t t = grp; t < n_c; t += per_block) {
        // one lane reads for its group: the lanes of a group leave the loop together
        int32_t seen = lane == 0 ? atomicAdd(&cut_at, 0) : 0;
        seen = __shfl(seen, 0, r.group);
        if (t > seen) break;
        const int32_t k = cand[3 * t + 2];
        const int64_t ga = (int64_t)r.ga0 + cand[3 * t], gb = (int64_t)r.gb0 + cand[3 * t + 1];
        const int32_t s = r.start[k];
        int32_t worst;
        uint32_t m;
        group_worst_pred(j, ga, gb, s, r.start[k + 1] - s, lane, true, &worst, &m);
        if (lane == 0) {
            const int32_t f = roll_f(worst);
            const bool cut = roll_cut(f, r.rp.stop_cost) != 0, object = !cut && ((m >> pred_slot(j.pp, t)) & 1u);
            fs[t] = (int16_t)(object ? (f | OBJECT_CUT_BIT) : f);
            if (cut || object) atomicMin(&cut_at, t);
        }
    }
    __syncthreads();
    const int32_t L = cut_at;
    int32_t mx = -1, sum = 0;
    for (int32_t t = tid; t < L; t += (int32_t)ROLL_BLOCK) {
        const int32_t f = fs[t];
        mx = f > mx ? f : mx, sum += f;
    }
    for (int32_t off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx, sum += __shfl_xor(sum, off);
    }
    if ((tid & 63) == 0) red_max[tid >> 6] = mx, red_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid != 0) return;
    for (int32_t w = 1; w < (int32_t)ROLL_BLOCK / 64; w++) mx = red_max[w] > mx ? red_max[w] : mx, sum += red_sum[w];
    int32_t rec[ROLL_PRED_REC] = {L, n_c == 0 ? (int32_t)ROLL_EMPTY : (int32_t)ROLL_COMPLETE, mx, sum, PLAN_FAR, -1};
    if (L < n_c) {
        const int32_t f = fs[L];
        if (f >= 0 && (f & OBJECT_CUT_BIT)) rec[RR_STATUS] = ROLL_CUT_OBJECT, rec[RR_SLOT] = pred_slot(j.pp, L);
        else rec[RR_STATUS] = roll_cut(f, r.rp.stop_cost);
    }
    if (L > 0 && r.rp.w_pot != 0) {
        const int64_t a = (int64_t)r.ga0 + cand[3 * (L - 1)] - r.oa, b = (int64_t)r.gb0 + cand[3 * (L - 1) + 1] - r.ob;
        rec[RR_POT_END] = r.pot[(size_t)b * (size_t)r.nx + (size_t)a];   // inside: (0, 0) is in every list and F was not -1
    }
    for (int32_t k = 0; k < ROLL_PRED_REC; k++) r.recs[(size_t)c * ROLL_PRED_REC + k] = rec[k];
    r.scores[c] = roll_score(r.rp, n_c, rec);
}

__global__ __launch_bounds__(ROLL_BLOCK) void k_grid_footprint_pred(RollPredJob j, const int32_t* __restrict__ poses, int64_t n, uint32_t* out) {
    const RollJob& r = j.r;
    const int32_t tid = (int32_t)threadIdx.x, lane = tid % r.group;
    const int64_t per_block = (int64_t)ROLL_BLOCK / r.group;
    for (int64_t i = (int64_t)blockIdx.x * per_block + tid / r.group; i < n; i += (int64_t)gridDim.x * per_block) {
        const int32_t k = poses[3 * i + 2];
        int32_t worst = 0;
        uint32_t m = 0;
        if (k >= 0 && k < 8 * r.rp.m) {   // the same for every lane of the group
            const int32_t s = r.start[k];
            group_worst_pred(j, poses[3 * i], poses[3 * i + 1], s, r.start[k + 1] - s, lane, false, &worst, &m);
        }
        if (lane == 0) out[i] = m;
    }
}

__global__ __launch_bounds__(PRED_BLOCK) void k_grid_pred_overlay(int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t poa, int32_t pob,
                                                                  const uint32_t* __restrict__ pred, uint8_t* rgb) {
    const int64_t cells = (int64_t)nx * nz;
    for (int64_t c = (int64_t)blockIdx.x * PRED_BLOCK + threadIdx.x; c < cells; c += (int64_t)gridDim.x * PRED_BLOCK) {
        const int32_t ib = (int32_t)(c / nx), ia = (int32_t)(c - (int64_t)ib * nx);
        const uint32_t w = pred_at(pred, nx, nz, poa, pob, (int64_t)ia + oa, (int64_t)ib + ob);
        if (!w) continue;
        uint8_t px[3];
        colour_pred(w, px);
        const size_t o = 3 * ((size_t)(nz - 1 - ib) * (size_t)nx + (size_t)ia);
        rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
    }
}

}  // namespace

int32_t launch_pred(hipStream_t s, const PredJob& j) {
    const int64_t cells = (int64_t)j.nx * j.nz, lanes = (int64_t)j.n_tracks * PRED_MAX_SLOTS;
    hipLaunchKernelGGL(k_grid_pred_disp, dim3((unsigned)((lanes + PRED_BLOCK - 1) / PRED_BLOCK)), dim3(PRED_BLOCK), 0, s, j);
    hipLaunchKernelGGL(k_grid_pred_scatter, dim3((unsigned)std::min<int64_t>((cells + PRED_BLOCK - 1) / PRED_BLOCK, PRED_MAX_BLOCKS)), dim3(PRED_BLOCK),
                       0, s, j);
    if (j.max_r == 0) return PRED_LAUNCHES_FLAT;
    hipLaunchKernelGGL(k_grid_pred_rows, dim3(((unsigned)j.nx + PRED_BLOCK - 1) / PRED_BLOCK, (unsigned)j.nz), dim3(PRED_BLOCK), 0, s, j);
    hipLaunchKernelGGL(k_grid_pred_cols, dim3(((unsigned)j.nx + PRED_COLS_X - 1) / PRED_COLS_X, ((unsigned)j.nz + PRED_COLS_Y - 1) / PRED_COLS_Y),
                       dim3(PRED_BLOCK), 0, s, j);
    return PRED_LAUNCHES;
}

void launch_roll_score_pred(hipStream_t s, const RollPredJob& j) {
    hipLaunchKernelGGL(k_grid_roll_score_pred, dim3((unsigned)j.r.K), dim3(ROLL_BLOCK), 0, s, j);
    launch_roll_best(s, j.r.scores, j.r.K, j.r.best);
}

void launch_footprint_pred(hipStream_t s, const RollPredJob& j, const int32_t* poses, int64_t n, uint32_t* out) {
    if (n <= 0) return;
    const int64_t per_block = (int64_t)ROLL_BLOCK / j.r.group;
    const int64_t blocks = std::min<int64_t>((n + per_block - 1) / per_block, 8192);
    hipLaunchKernelGGL(k_grid_footprint_pred, dim3((unsigned)blocks), dim3(ROLL_BLOCK), 0, s, j, poses, n, out);
}

void launch_pred_overlay(hipStream_t s, int32_t nx, int32_t nz, int32_t oa, int32_t ob, int32_t poa, int32_t pob, const uint32_t* pred, uint8_t* rgb) {
    const int64_t cells = (int64_t)nx * nz;
    hipLaunchKernelGGL(k_grid_pred_overlay, dim3((unsigned)std::min<int64_t>((cells + PRED_BLOCK - 1) / PRED_BLOCK, 4096)), dim3(PRED_BLOCK), 0, s, nx,
                       nz, oa, ob, poa, pob, pred, rgb);
}

}  // namespace grid
}  // namespace svh

// The dynamics of the ground grid on the device (svh_grid_observe_*, include/svh_grid.h "DYNAMICS").  The arithmetic is
// csrc/grid_dyn_core.h.  Phase 1 of an observation is k_grid_bin<true> (grid_kernels.hip) on a scratch set of accumulators.
//
//   k_grid_body      one lane per slot: the body of the stored cell as (q_lo, q_hi + 1), (0, 0) for a cell that is not tall, so that
//                    a line step costs one 8-byte load.  The plane belongs to the layer and k_grid_settle keeps it for the cells it
//                    writes, so this pre-pass runs only after something else wrote the accumulators (a plain add, a clear).
//   k_grid_sight     phase 2.  k_grid_rays' deal: a wave takes 64 end cells of one row (forward-major lines) or one column
//                    (lateral-major lines), the lanes share the major step, equal cells are runs of neighbouring lanes, and a
//                    segmented wave scan sums a run so that its last lane issues the atomics.  Two lanes of one run stand in the
//                    same cell at DIFFERENT heights, so the through-test is made per lane before the scan and the scan carries two
//                    sums: the pass weight and the through weight.  The height is stepped like the cells: with dq = q_e - q_o,
//                    2 dq = a * 2n + b (a = floor, 0 <= b < 2n, one 64-bit division per lane before the loop) a step adds a to the
//                    quotient and b to the remainder, with one carry -- the closed form's value at every step.  No atomic returns
//                    a value.  Every lane zeroes its `ends` entry, as k_grid_rays does.  The form that reads count, kmin and kmax of
//                    the cell at every step instead of its body was measured against this one, alternating in one process
//                    (profiles/grid_dyn_forms_ab.jsonl, DESIGN.md "Dynamics": 0.25 against 0.23 ms for the local step on the urban store
//                    at 256 x 256, 4.64 against 4.38 ms with every cell of 1024 x 1024 an end cell, 2.08 against 2.06 ms at 8192 x
//                    8192), and then deleted.
//   k_grid_settle    phase 3, one lane per cell: settle() on the stored cell, its state and the frame record, all at the cell's
//                    slot; writes what changed (and the body of a cell it writes), keeps THROUGH and the event byte of this observation
//                    for the getters, returns the frame scratch to empty.  It is bound by memory: a cell is 81 bytes of traffic, so a
//                    cell the frame did not touch (no point, no contradiction, nothing due) is recognised from 16 of them.  The three statistics are counted per wave by ballot / popcount and added once per wave.
//   k_grid_dyn_enter svh_grid_scroll with the layer set: the body, CONTRA, LAST, the kept THROUGH and the event byte of the entering strips
//                    become empty (k_grid_enter's lanes).  Not launched without the layer.
//   k_grid_dyn_get   one lane per cell: AGE, CONTRA or THROUGH in logical order.
//   k_grid_render_dyn  one lane per pixel: colour_dyn of the cell, rows flipped so that forward is up.
#include <hip/hip_runtime.h>

#include "grid_core.h"
#include "grid_dyn_core.h"
#include "grid_internal.h"

namespace svh {
namespace grid {
namespace {

// what the body plane holds: lo <= q < end is goes_through(); all zero is "not tall", the state of the empty layer
__device__ __forceinline__ int2 packed_body(const Params& prm, const DynParams& dyn, int32_t count, uint32_t kmin, uint32_t kmax) {
    if (!is_tall(prm, count, kmax)) return make_int2(0, 0);
    const Body b = body_of(prm, dyn, count, kmin, kmax);
    return make_int2(b.lo, b.hi + 1);   // q_hi <= 2^30
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_body(Params prm, DynParams dyn, Cells c, int2* __restrict__ body) {
    const uint32_t s = blockIdx.x * FIN_BLOCK + threadIdx.x;
    if (s >= (uint32_t)prm.nx * (uint32_t)prm.nz) return;
    body[s] = packed_body(prm, dyn, c.count[s], c.kmin[s], c.kmax[s]);
}

// One coordinate of the line, stepped (k_grid_rays' Stepper): q = rdiv(k * d, n), r = (2 k d + n) - 2 n q in [0, 2n)
struct CellStepper {
    int32_t q, r, d2, n2;
    __device__ __forceinline__ CellStepper(int32_t d, int32_t n) : q(0), r(n), d2(2 * d), n2(2 * n) {}
    __device__ __forceinline__ void step() {
        r += d2;
        if (r >= n2) r -= n2, q += 1;
        else if (r < 0) r += n2, q -= 1;
    }
};

__global__ __launch_bounds__(RAY_BLOCK) void k_grid_sight(Params prm, uint32_t origin, int32_t q_o, int32_t* __restrict__ ends,
                                                          const uint32_t* __restrict__ fkmin, const int2* __restrict__ body,
                                                          int32_t* __restrict__ pass, int32_t* __restrict__ through,
                                                          unsigned long long* __restrict__ ray_cells) {
    const int lane = threadIdx.x & 63;
    const uint32_t nx = (uint32_t)prm.nx, nz = (uint32_t)prm.nz;
    const uint32_t segs_row = (nx + 63u) / 64u, segs_col = (nz + 63u) / 64u;
    const uint32_t waves_rows = nz * segs_row, waves_cols = nx * segs_col;
    const uint32_t wv = blockIdx.x * (RAY_BLOCK / 64u) + (threadIdx.x >> 6);
    if (wv >= waves_rows + waves_cols) return;   // the whole wave
    const bool rows = wv < waves_rows;
    uint32_t ea, eb;
    if (rows) {
        eb = wv / segs_row;
        ea = (wv - eb * segs_row) * 64u + (uint32_t)lane;
    } else {
        const uint32_t t = wv - waves_rows;
        ea = t / segs_col;
        eb = (t - ea * segs_col) * 64u + (uint32_t)lane;
    }
    const int32_t ocb = (int32_t)(origin / nx), oca = (int32_t)(origin - (uint32_t)ocb * nx);
    const int32_t dx = (int32_t)ea - oca, dz = (int32_t)eb - ocb;
    const int32_t ax = dx < 0 ? -dx : dx, az = dz < 0 ? -dz : dz;
    const bool mine = ea < nx && eb < nz && (rows ? az >= ax : ax > az);
    int32_t w = 0;
    if (mine) {
        w = ends[eb * nx + ea];
        if (w != 0) ends[eb * nx + ea] = 0;
    }
    if (__ballot(w != 0) == 0ull) return;
    // the major distance of this row (column): the same in every lane of the wave, and line_len() in those that cast
    const int32_t n = rows ? az : ax;
    if (n == 0) return;   // the origin's own row segment with dz == 0 == dx: no lane has a step, and none adds to ray_cells
    const int32_t q_e = w != 0 ? q_of_key(fkmin[slot_at(prm, (int32_t)ea, (int32_t)eb)]) : q_o;
    CellStepper sx(dx, n), sz(dz, n);
    HeightStepper sq(q_o, q_e, n);
    for (int32_t k = 0; k < n; k++) {
        const uint32_t cid = w != 0 ? (uint32_t)(ocb + sz.q) * nx + (uint32_t)(oca + sx.q) : NO_CELL;
        int32_t tsum = 0;
        uint32_t s = 0;
        if (w != 0) {
            s = slot_at(prm, oca + sx.q, ocb + sz.q);
            const int32_t q = sq.height();
            const int2 b = body[s];
            tsum = (b.x <= q && q < b.y) ? w : 0;
        }
        const uint32_t before = __shfl_up(cid, 1, 64), after = __shfl_down(cid, 1, 64);
        int head = lane == 0 || before != cid;
        const bool tail = lane == 63 || after != cid;
        int32_t sum = w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t sum2 = __shfl_up(sum, d, 64), tsum2 = __shfl_up(tsum, d, 64);
            const int head2 = __shfl_up(head, d, 64);
            if (lane >= d && !head) {
                sum += sum2;
                tsum += tsum2;
                head = head2;
            }
        }
        if (w != 0 && tail) {
            atomicAdd(&pass[s], sum);
            if (tsum != 0) atomicAdd(&through[s], tsum);
        }
        if (w != 0) sx.step(), sz.step(), sq.step();
    }
    unsigned long long total = (unsigned long long)(uint32_t)w * (unsigned long long)(w != 0 ? n : 0);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) total += __shfl_down(total, d, 64);
    if (lane == 0 && total) atomicAdd(ray_cells, total);
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_settle(Params prm, DynParams dyn, int32_t stamp, Cells c, Cells f, DynPlanes d,
                                                           unsigned long long* __restrict__ stats) {
    const uint32_t i = blockIdx.x * FIN_BLOCK + threadIdx.x;
    uint8_t ev = 0;
    if (i < (uint32_t)prm.nx * (uint32_t)prm.nz) {
        const uint32_t s = slot_of(prm, i);
        const int32_t fcount = f.count[s], fover = f.overhead[s], thr = d.through[s], contra0 = d.contra[s];
        // A QUIET cell: the frame has no point in it, its lines do not contradict it and nothing is due -- settle() would change
        // nothing, so the other 60 bytes of the cell are not read.  Most cells of a large window are quiet
        bool quiet = fcount == 0 && fover == 0 && thr < dyn.min_through && !(dyn.clear_frames > 0 && contra0 >= dyn.clear_frames);
        if (quiet && dyn.max_age > 0) quiet = !((c.count[s] > 0 || c.overhead[s] > 0) && stamp - d.last[s] > dyn.max_age);
        if (!quiet) {
            Cell cell{c.count[s], c.overhead[s], c.kmin[s], c.kmax[s], (int64_t)c.hsum[s], (uint64_t)c.vsum[s]};
            const Cell rec{fcount, fover, f.kmin[s], f.kmax[s], (int64_t)f.hsum[s], (uint64_t)f.vsum[s]};
            const int32_t last0 = d.last[s];
            int32_t contra = contra0, last = last0;
            ev = settle(prm, dyn, stamp, cell, contra, last, rec, thr);
            if ((ev & (DE_CLEARED | DE_AGED)) || rec.count > 0 || rec.overhead > 0) {
                c.count[s] = cell.count, c.overhead[s] = cell.overhead;
                c.kmin[s] = cell.kmin, c.kmax[s] = cell.kmax;
                c.hsum[s] = (unsigned long long)cell.hsum, c.vsum[s] = (unsigned long long)cell.vsum;
                d.body[s] = packed_body(prm, dyn, cell.count, cell.kmin, cell.kmax);
            }
            if (contra != contra0) d.contra[s] = contra;
            if (last != last0) d.last[s] = last;
            if (rec.count > 0) {
                f.count[s] = 0, f.kmin[s] = KMIN_EMPTY, f.kmax[s] = KMAX_EMPTY;
                f.hsum[s] = 0ull, f.vsum[s] = 0ull;
            }
            if (rec.overhead > 0) f.overhead[s] = 0;
        }
        d.kept[s] = thr;
        d.event[s] = ev;
        if (thr != 0) d.through[s] = 0;
    }
    // the statistics: per wave by ballot / popcount, the four waves of a workgroup through LDS, then at most three atomics per
    // workgroup -- one per wave queued 16 384 adds at one address when every cell of 1024 x 1024 was confirmed (0.20 ms of settle)
    __shared__ uint32_t tally[3];
    if (threadIdx.x < 3) tally[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t cleared = (uint32_t)__popcll(__ballot((ev & DE_CLEARED) != 0)), aged = (uint32_t)__popcll(__ballot((ev & DE_AGED) != 0)),
                   confirmed = (uint32_t)__popcll(__ballot((ev & DE_CONFIRMED) != 0));
    if ((threadIdx.x & 63) == 0) {
        if (cleared) atomicAdd(&tally[0], cleared);
        if (aged) atomicAdd(&tally[1], aged);
        if (confirmed) atomicAdd(&tally[2], confirmed);
    }
    __syncthreads();
    if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(&stats[DS_CLEARED + threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_dyn_enter(Params prm, int32_t da, int32_t db, DynPlanes d) {
    const uint32_t nx = (uint32_t)prm.nx, nz = (uint32_t)prm.nz;
    const uint32_t cols = (uint32_t)(da < 0 ? -da : da), rows = (uint32_t)(db < 0 ? -db : db);
    const uint32_t in_cols = cols * nz;
    uint32_t t = blockIdx.x * FIN_BLOCK + threadIdx.x;
    if (t >= in_cols + rows * nx) return;
    uint32_t ia, ib;
    if (t < in_cols) {   // the entering columns: the high side when the window moved up
        ib = t / cols;
        ia = t - ib * cols;
        if (da > 0) ia += nx - cols;
    } else {
        t -= in_cols;
        ib = t / nx;
        ia = t - ib * nx;
        if (db > 0) ib += nz - rows;
    }
    const uint32_t s = slot_at(prm, (int32_t)ia, (int32_t)ib);
    d.body[s] = make_int2(0, 0);
    d.contra[s] = 0, d.last[s] = 0, d.kept[s] = 0, d.event[s] = 0;
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_dyn_get(Params prm, int32_t plane, int32_t stamp, DynPlanes d, int32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * FIN_BLOCK + threadIdx.x;
    if (i >= (uint32_t)prm.nx * (uint32_t)prm.nz) return;
    const uint32_t s = slot_of(prm, i);
    out[i] = plane == D_AGE ? age_of(stamp, d.last[s]) : plane == D_CONTRA ? d.contra[s] : d.kept[s];
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_render_dyn(Params prm, DynPlanes d, const int32_t* __restrict__ count,
                                                               const int32_t* __restrict__ pass, const float* __restrict__ hmin,
                                                               const float* __restrict__ hmax, const float* __restrict__ hmean,
                                                               const uint8_t* __restrict__ intensity, const uint8_t* __restrict__ cls,
                                                               uint8_t* __restrict__ rgb) {
    const uint32_t o = blockIdx.x * FIN_BLOCK + threadIdx.x;
    if (o >= (uint32_t)prm.nx * (uint32_t)prm.nz) return;
    const uint32_t row = o / (uint32_t)prm.nx, col = o - row * (uint32_t)prm.nx;
    const uint32_t i = ((uint32_t)prm.nz - 1u - row) * (uint32_t)prm.nx + col;
    const uint32_t s = slot_of(prm, i);
    const Final f{hmin[i], hmax[i], hmean[i], intensity[i], cls[i]};
    uint8_t px[3];
    colour_dyn(prm, count[i], f, pass[i], d.contra[s], d.event[s], px);
    rgb[3 * (size_t)o] = px[0], rgb[3 * (size_t)o + 1] = px[1], rgb[3 * (size_t)o + 2] = px[2];
}

inline unsigned cell_blocks(const Params& p) { return ((unsigned)p.nx * (unsigned)p.nz + FIN_BLOCK - 1) / FIN_BLOCK; }

}  // namespace

void launch_sight(hipStream_t s, const SightJob& j) {
    const unsigned nx = (unsigned)j.prm.nx, nz = (unsigned)j.prm.nz;
    const unsigned waves = nz * ((nx + 63u) / 64u) + nx * ((nz + 63u) / 64u), per = RAY_BLOCK / 64u;
    if (j.write_body) hipLaunchKernelGGL(k_grid_body, dim3(cell_blocks(j.prm)), dim3(FIN_BLOCK), 0, s, j.prm, j.dyn, j.cells, j.planes.body);
    hipLaunchKernelGGL(k_grid_sight, dim3((waves + per - 1) / per), dim3(RAY_BLOCK), 0, s, j.prm, j.origin, j.q_o, j.ends, j.frame.kmin, j.planes.body,
                       j.cells.pass, j.planes.through, j.ray_cells);
}

void launch_settle(hipStream_t s, const SettleJob& j) {
    hipLaunchKernelGGL(k_grid_settle, dim3(cell_blocks(j.prm)), dim3(FIN_BLOCK), 0, s, j.prm, j.dyn, j.stamp, j.cells, j.frame, j.planes, j.stats);
}

void launch_dyn_enter(hipStream_t s, const Params& prm, int32_t da, int32_t db, const DynPlanes& d) {
    const unsigned cols = (unsigned)(da < 0 ? -da : da), rows = (unsigned)(db < 0 ? -db : db);
    const unsigned lanes = cols * (unsigned)prm.nz + rows * (unsigned)prm.nx;
    if (lanes == 0) return;
    hipLaunchKernelGGL(k_grid_dyn_enter, dim3((lanes + FIN_BLOCK - 1) / FIN_BLOCK), dim3(FIN_BLOCK), 0, s, prm, da, db, d);
}

void launch_dyn_get(hipStream_t s, const Params& prm, int32_t plane, int32_t stamp, const DynPlanes& d, int32_t* out) {
    hipLaunchKernelGGL(k_grid_dyn_get, dim3(cell_blocks(prm)), dim3(FIN_BLOCK), 0, s, prm, plane, stamp, d, out);
}

void launch_render_dyn(hipStream_t s, const RenderJob& j, const DynPlanes& d) {
    hipLaunchKernelGGL(k_grid_render_dyn, dim3(cell_blocks(j.prm)), dim3(FIN_BLOCK), 0, s, j.prm, d, j.count, j.pass, j.hmin, j.hmax, j.hmean,
                       j.intensity, j.cls, j.rgb);
}

}  // namespace grid
}  // namespace svh

// The ground grid on the device (svh_grid_*, include/svh_grid.h).  The arithmetic is csrc/grid_core.h.
//
//   k_grid_bin       one lane per point, one 16-byte load per lane, grid-stride beyond BIN_MAX_BLOCKS workgroups.  A low
//                    point updates its cell with five no-return integer atomics at device scope (HIP's default on global
//                    memory, which is what the eight XCDs need): count +, kmin min, kmax max, hsum + (64 bits), vsum +
//                    (64 bits); an overhead point with one.  Integer +, min and max commute, so the grid is the same
//                    under every schedule.  The four statistics are counted per wave by ballot / popcount, kept in a
//                    register over the wave's passes and added once per wave.
//                    Runs are combined first: the store arrives in frame order and the map fusion emits points column by
//                    column, so consecutive lanes often hit the same cell.  Each lane compares its cell with the lane
//                    before it, a segmented wave scan (six __shfl_up steps) combines count, min key, max key, hsum and
//                    vsum along each run of equal cells, and only the last lane of a run issues atomics.  A lane that is
//                    not a low point ends the run on both sides of it; a run that crosses a wave boundary is two runs.
//                    It is the same multiset of updates as five atomics from every low lane -- the plain form this was
//                    measured against (profiles/grid_times.jsonl, DESIGN.md "Ground grid") and which was then deleted.
//                    The accumulators lie at the cell's slot (the torus of grid_core.h).  k_grid_bin<true>, the form of
//                    svh_grid_add_*_from, also adds a run's count to the scratch plane `ends` (logical order): this
//                    call's low points per cell, the end cells of its rays.  k_grid_bin<false> has no such code.
//   k_grid_rays      the rays of one svh_grid_add_*_from.  The line depends only on the origin's and the end's cell, so a
//                    ray is cast per end CELL with ends != 0, weighted by ends, never per point: the cost is bounded by
//                    the cells.  Every lane steps its line incrementally (the quotient and remainder of rdiv, which move
//                    by at most one per step: the same cells as the closed form) and zeroes its ends entry; the sum of
//                    increments is reduced per wave and added once.  All rays share the cells next to the origin, so a
//                    wave takes 64 end cells of one row (one column for lateral-major lines): at every step they stand in
//                    one row with slowly varying minor coordinate, equal cells are runs of neighbouring lanes, and a
//                    segmented wave scan sums the weights of a run so that its last lane issues one atomic.  The plain
//                    form -- one lane per end cell, one atomic per lane and step -- was measured against it
//                    (profiles/grid_local_times.jsonl, DESIGN.md "Ground grid": 0.34 against 0.30 ms on the urban store,
//                    1.48 against 0.44 ms for 10^6 points in every cell of 256 x 256) and then deleted.
//   k_grid_enter     svh_grid_scroll: one lane per cell of the entering strips (columns, then rows), reset to the empty cell.
//   k_grid_finalise  one lane per cell: the accumulators at the cell's slot become COUNT, OVERHEAD, HMIN, HMAX, HMEAN,
//                    INTENSITY, CLASS, PASS and STATE in logical order.
//   k_grid_render    one lane per pixel: the colour of the cell, rows flipped so that forward is up.
#include <hip/hip_runtime.h>

#include "grid_core.h"
#include "grid_internal.h"

namespace svh {
namespace grid {
namespace {

template <bool ENDS>
__global__ __launch_bounds__(BIN_BLOCK) void k_grid_bin(Params prm, const float4* __restrict__ pts, long long n, Cells c,
                                                        unsigned long long* __restrict__ stats, int32_t* __restrict__ ends) {
    const int lane = threadIdx.x & 63;
    uint32_t seen[4] = {0u, 0u, 0u, 0u};   // per fate, the same in every lane of the wave
    const long long stride = (long long)gridDim.x * BIN_BLOCK;
    // a wave goes on while its first lane has a point: all 64 lanes make every pass, the shuffles below have them all
    for (long long base = (long long)blockIdx.x * BIN_BLOCK + (threadIdx.x & ~63u); base < n; base += stride) {
        const long long i = base + lane;
        Placed r{-1, NO_CELL, 0u, 0, 0u, 0u};
        if (i < n) {
            const float4 p = pts[i];
            r = place(prm, p.x, p.y, p.z, p.w);
        }
#pragma unroll
        for (int f = 0; f < 4; f++) seen[f] += (uint32_t)__popcll(__ballot(r.fate == f));
        if (r.fate == OVERHEAD) atomicAdd(&c.overhead[r.slot], 1);
        const bool low = r.fate == LOW;
        const uint32_t rid = low ? r.cell : NO_CELL;   // a cell index is below 2^26
        const uint32_t before = __shfl_up(rid, 1, 64), after = __shfl_down(rid, 1, 64);
        int head = lane == 0 || before != rid;
        const bool tail = lane == 63 || after != rid;
        uint32_t cnt = 1u, mn = r.key, mx = r.key, vs = r.v;
        long long hs = r.q;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t cnt2 = __shfl_up(cnt, d, 64), mn2 = __shfl_up(mn, d, 64), mx2 = __shfl_up(mx, d, 64),
                           vs2 = __shfl_up(vs, d, 64);
            const long long hs2 = __shfl_up(hs, d, 64);
            const int head2 = __shfl_up(head, d, 64);
            if (lane >= d && !head) {
                cnt += cnt2;
                mn = mn2 < mn ? mn2 : mn;
                mx = mx2 > mx ? mx2 : mx;
                vs += vs2;
                hs += hs2;
                head = head2;
            }
        }
        if (low && tail) {
            atomicAdd(&c.count[r.slot], (int32_t)cnt);
            atomicMin(&c.kmin[r.slot], mn);
            atomicMax(&c.kmax[r.slot], mx);
            atomicAdd(&c.hsum[r.slot], (unsigned long long)hs);
            atomicAdd(&c.vsum[r.slot], (unsigned long long)vs);
            if (ENDS) atomicAdd(&ends[r.cell], (int32_t)cnt);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int f = 0; f < 4; f++)
            if (seen[f]) atomicAdd(&stats[f], (unsigned long long)seen[f]);
    }
}

// One coordinate of the line, stepped: q = rdiv(k * d, n) and r = (2 k d + n) - 2 n q in [0, 2n).  |2 d| <= 2 n, so a
// step moves q by at most one.
struct Stepper {
    int32_t q, r, d2, n2;
    __device__ __forceinline__ Stepper(int32_t d, int32_t n) : q(0), r(n), d2(2 * d), n2(2 * n) {}
    __device__ __forceinline__ void step() {
        r += d2;
        if (r >= n2) r -= n2, q += 1;
        else if (r < 0) r += n2, q -= 1;
    }
};

// the sum over the wave, in lane 0
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// A wave takes 64 end cells of one ROW and casts those whose line is forward-major (|dz| >= |dx|),
// or 64 end cells of one COLUMN and casts those that are lateral-major (|dx| > |dz|): every end cell is cast by exactly
// one of the two.  The lanes of a wave then share the major step -- the same n, and at step k the same row (column) --
// and their minor coordinates vary slowly from lane to lane, so equal cells are runs of neighbouring lanes: near the
// origin all 64 lanes stand in one cell.  The weights of a run are summed by a segmented wave scan, as k_grid_bin sums
// its runs, and the last lane of a run issues the one atomic.  It is the same multiset of increments as one atomic per
// lane and step.
__global__ __launch_bounds__(RAY_BLOCK) void k_grid_rays(Params prm, uint32_t origin, int32_t* __restrict__ ends,
                                                              int32_t* __restrict__ pass,
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
    Stepper sx(dx, n), sz(dz, n);
    for (int32_t k = 0; k < n; k++) {
        const uint32_t cid = w != 0 ? (uint32_t)(ocb + sz.q) * nx + (uint32_t)(oca + sx.q) : NO_CELL;
        const uint32_t before = __shfl_up(cid, 1, 64), after = __shfl_down(cid, 1, 64);
        int head = lane == 0 || before != cid;
        const bool tail = lane == 63 || after != cid;
        int32_t sum = w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t sum2 = __shfl_up(sum, d, 64);
            const int head2 = __shfl_up(head, d, 64);
            if (lane >= d && !head) {
                sum += sum2;
                head = head2;
            }
        }
        if (w != 0 && tail) atomicAdd(&pass[slot_at(prm, oca + sx.q, ocb + sz.q)], sum);
        if (w != 0) sx.step(), sz.step();
    }
    const unsigned long long total = wave_sum((unsigned long long)(uint32_t)w * (unsigned long long)(w != 0 ? n : 0));
    if (lane == 0 && total) atomicAdd(ray_cells, total);
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_enter(Params prm, int32_t da, int32_t db, Cells c) {
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
    c.kmin[s] = KMIN_EMPTY, c.kmax[s] = KMAX_EMPTY;
    c.count[s] = 0, c.overhead[s] = 0, c.pass[s] = 0;
    c.hsum[s] = 0ull, c.vsum[s] = 0ull;
}

__device__ __forceinline__ Cell load_cell(const Cells& c, uint32_t i) {
    return Cell{c.count[i], c.overhead[i], c.kmin[i], c.kmax[i], (int64_t)c.hsum[i], (uint64_t)c.vsum[i]};
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_finalise(Params prm, Cells c, int32_t* __restrict__ count,
                                                             int32_t* __restrict__ overhead, int32_t* __restrict__ pass,
                                                             float* __restrict__ hmin, float* __restrict__ hmax,
                                                             float* __restrict__ hmean, uint8_t* __restrict__ intensity,
                                                             uint8_t* __restrict__ cls, uint8_t* __restrict__ state) {
    const uint32_t i = blockIdx.x * FIN_BLOCK + threadIdx.x;
    if (i >= (uint32_t)prm.nx * (uint32_t)prm.nz) return;
    const uint32_t s = slot_of(prm, i);
    const Cell cell = load_cell(c, s);
    const int32_t passed = c.pass[s];
    const Final f = finalise(prm, cell);
    count[i] = cell.count, overhead[i] = cell.overhead, pass[i] = passed;
    hmin[i] = f.hmin, hmax[i] = f.hmax, hmean[i] = f.hmean;
    intensity[i] = f.intensity, cls[i] = f.cls, state[i] = state_of(prm, f.cls, passed);
}

__global__ __launch_bounds__(FIN_BLOCK) void k_grid_render(Params prm, int32_t mode, const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ pass,
                                                           const float* __restrict__ hmin, const float* __restrict__ hmax,
                                                           const float* __restrict__ hmean,
                                                           const uint8_t* __restrict__ intensity,
                                                           const uint8_t* __restrict__ cls, uint8_t* __restrict__ rgb) {
    const uint32_t o = blockIdx.x * FIN_BLOCK + threadIdx.x;
    if (o >= (uint32_t)prm.nx * (uint32_t)prm.nz) return;
    const uint32_t row = o / (uint32_t)prm.nx, col = o - row * (uint32_t)prm.nx;
    const uint32_t i = ((uint32_t)prm.nz - 1u - row) * (uint32_t)prm.nx + col;
    const Final f{hmin[i], hmax[i], hmean[i], intensity[i], cls[i]};
    uint8_t px[3];
    if (mode == M_LOCAL) colour_local(prm, count[i], f, pass[i], px);
    else colour(prm, mode, count[i], f, px);
    rgb[3 * (size_t)o] = px[0], rgb[3 * (size_t)o + 1] = px[1], rgb[3 * (size_t)o + 2] = px[2];
}

}  // namespace

void launch_bin(hipStream_t s, const BinJob& j) {
    if (j.n <= 0) return;
    const long long want = (j.n + BIN_BLOCK - 1) / BIN_BLOCK;
    const unsigned blocks = (unsigned)(want < (long long)BIN_MAX_BLOCKS ? want : (long long)BIN_MAX_BLOCKS);
    if (j.ends)
        hipLaunchKernelGGL(k_grid_bin<true>, dim3(blocks), dim3(BIN_BLOCK), 0, s, j.prm, j.pts, (long long)j.n, j.cells, j.stats,
                           j.ends);
    else
        hipLaunchKernelGGL(k_grid_bin<false>, dim3(blocks), dim3(BIN_BLOCK), 0, s, j.prm, j.pts, (long long)j.n, j.cells, j.stats,
                           (int32_t*)nullptr);
}

void launch_rays(hipStream_t s, const RayJob& j) {
    const unsigned nx = (unsigned)j.prm.nx, nz = (unsigned)j.prm.nz;
    const unsigned waves = nz * ((nx + 63u) / 64u) + nx * ((nz + 63u) / 64u), per = RAY_BLOCK / 64u;
    hipLaunchKernelGGL(k_grid_rays, dim3((waves + per - 1) / per), dim3(RAY_BLOCK), 0, s, j.prm, j.origin, j.ends, j.pass,
                       j.ray_cells);
}

void launch_enter(hipStream_t s, const EnterJob& j) {
    const unsigned cols = (unsigned)(j.da < 0 ? -j.da : j.da), rows = (unsigned)(j.db < 0 ? -j.db : j.db);
    const unsigned lanes = cols * (unsigned)j.prm.nz + rows * (unsigned)j.prm.nx;
    if (lanes == 0) return;
    hipLaunchKernelGGL(k_grid_enter, dim3((lanes + FIN_BLOCK - 1) / FIN_BLOCK), dim3(FIN_BLOCK), 0, s, j.prm, j.da, j.db, j.cells);
}

void launch_finalise(hipStream_t s, const FinalJob& j) {
    const unsigned cells = (unsigned)j.prm.nx * (unsigned)j.prm.nz;
    hipLaunchKernelGGL(k_grid_finalise, dim3((cells + FIN_BLOCK - 1) / FIN_BLOCK), dim3(FIN_BLOCK), 0, s, j.prm, j.cells, j.count,
                       j.overhead, j.pass, j.hmin, j.hmax, j.hmean, j.intensity, j.cls, j.state);
}

void launch_render(hipStream_t s, const RenderJob& j) {
    const unsigned cells = (unsigned)j.prm.nx * (unsigned)j.prm.nz;
    hipLaunchKernelGGL(k_grid_render, dim3((cells + FIN_BLOCK - 1) / FIN_BLOCK), dim3(FIN_BLOCK), 0, s, j.prm, j.mode, j.count,
                       j.pass, j.hmin, j.hmax, j.hmean, j.intensity, j.cls, j.rgb);
}

}  // namespace grid
}  // namespace svh

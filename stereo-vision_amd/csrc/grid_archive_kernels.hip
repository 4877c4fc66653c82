// The ground grid's archive on the device (svh_grid_set_archive, svh_grid_get_region, include/svh_grid_archive.h).  The arithmetic is
// csrc/grid_archive_core.h.
//
// The index is a lock-free open-addressing table from tile key to page (the scheme of view_thin_kernels.hip and grid_obj_kernels.hip:
// atomicCAS on the 64-bit key, linear probing bounded by the table's size, a load factor of at most one half between calls).  A key
// is only ever removed together with every key that entered after it (the claims of one call, withdrawn), or by rebuilding the
// table (trim): no probe chain ever breaks, and no tombstone exists.
//
// A scroll, in stream order:
//   k_grid_arch_claim   one lane per leaving cell (strip_cell: the corner block once).  A lane whose record is not empty probes for
//                       its tile and claims an empty slot for it when it is not there; the claimed slots are listed and counted.
//                       The page of an empty slot is -1, so a claim is pending from the moment it exists.
//   k_grid_arch_assign  one workgroup per claim.  Every lane reads the same two counters: with claims <= unused pages (and no claim
//                       that found the table full) claim b takes the page at stack[free - 1 - b] and the workgroup fills it with
//                       the empty record, one lane per cell; otherwise every claim is withdrawn.  All or nothing: what survives
//                       does not depend on scheduling, only the page NUMBER of a tile does, and no byte that leaves the object
//                       shows it.
//   k_grid_arch_store   one lane per leaving cell: the record goes to the tile's page when it has one, empty or not; a record that
//                       is not empty and has no page is lost.  Both are counted per wave (ballot, popcount, one atomic).  The first
//                       lane of the launch then takes the assigned pages off the stack's count, or counts the refusal, and zeroes
//                       the claim counters: nothing else in this launch reads them.
//   k_grid_arch_enter   one lane per entering cell: the record of the tile's page, or the empty cell; with the dynamics also CONTRA and
//                       LAST from the record, the body, the kept THROUGH and the event byte empty.  Reads the pages, writes none.
// The leaving pass is complete before the entering pass rewrites a slot: a leaving and an entering cell can share one.
//   k_grid_arch_region  one lane per cell of a box of global cells: the record from the window's slot, from the tile's page or empty,
//                       finished by finalise() of grid_core.h, one plane written.
//   k_grid_arch_render  ... coloured by colour() / colour_local(), rows flipped so that forward is up.
//   k_grid_arch_collect, k_grid_arch_insert   svh_grid_archive_trim: the table rebuilt from the tiles that meet the box.
//   k_grid_arch_reset   the stack filled with every page.
// One probe per lane.  The form that probes once per run of equal tiles inside a wave has not been built (README "Archive").
// Vector stores and plain C++ only; every loop is bounded, the probe by the table's size.
#include <hip/hip_runtime.h>

#include "grid_archive_core.h"
#include "grid_core.h"
#include "grid_internal.h"

namespace svh {
namespace grid {
namespace {

__device__ __forceinline__ unsigned long long key_at(const unsigned long long* keys, uint32_t s) {
    return __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the page of a tile, -1: it has none
__device__ __forceinline__ int32_t find_page(const Archive& ar, unsigned long long key) {
    if (ar.table == 0) return -1;
    const uint32_t mask = ar.table - 1u;
    uint32_t s = tile_home(key, mask);
    for (uint32_t step = 0; step < ar.table; step++) {
        const unsigned long long k = key_at(ar.keys, s);
        if (k == key) {
            const int32_t pg = ar.page[s];
            return pg < ar.max_tiles ? pg : -1;
        }
        if (k == TILE_NONE) return -1;
        s = (s + 1u) & mask;
    }
    return -1;
}

__device__ __forceinline__ Record window_record(const Cells& c, bool dyn, const DynPlanes& d, uint32_t s) {
    Record r;
    r.cell = Cell{c.count[s], c.overhead[s], c.kmin[s], c.kmax[s], (int64_t)c.hsum[s], (uint64_t)c.vsum[s]};
    r.pass = c.pass[s];
    r.contra = dyn ? d.contra[s] : 0;
    r.last = dyn ? d.last[s] : 0;
    return r;
}

__device__ __forceinline__ Record page_record(const Pages& p, int32_t page, uint32_t idx) {
    const size_t i = (size_t)page * (size_t)TILE_CELLS + idx;
    Record r;
    r.cell = Cell{p.count[i], p.overhead[i], p.kmin[i], p.kmax[i], (int64_t)p.hsum[i], (uint64_t)p.vsum[i]};
    r.pass = p.pass[i], r.contra = p.contra[i], r.last = p.last[i];
    return r;
}

__device__ __forceinline__ void store_record(const Pages& p, int32_t page, uint32_t idx, const Record& r) {
    const size_t i = (size_t)page * (size_t)TILE_CELLS + idx;
    p.kmin[i] = r.cell.kmin, p.kmax[i] = r.cell.kmax;
    p.count[i] = r.cell.count, p.overhead[i] = r.cell.overhead;
    p.hsum[i] = (unsigned long long)r.cell.hsum, p.vsum[i] = (unsigned long long)r.cell.vsum;
    p.pass[i] = r.pass, p.contra[i] = r.contra, p.last[i] = r.last;
}

// the leaving cell of lane t: its slot and its global cell
__device__ __forceinline__ uint32_t strip_slot(const Params& prm, int64_t da, int64_t db, uint32_t t, int32_t* ga, int32_t* gb) {
    int32_t ia, ib;
    strip_cell(prm.nx, prm.nz, da, db, t, &ia, &ib);
    *ga = prm.oa + ia, *gb = prm.ob + ib;
    return slot_at(prm, ia, ib);
}

__device__ __forceinline__ void wave_count(bool flag, unsigned long long* word) {
    const unsigned long long m = __ballot(flag);
    if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(word, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_claim(Params prm, int32_t da, int32_t db, Cells c, bool dyn, DynPlanes d, Archive ar) {
    const uint32_t t = blockIdx.x * ARCH_BLOCK + threadIdx.x;
    if (t >= strip_count(prm.nx, prm.nz, da, db)) return;
    int32_t ga, gb;
    const uint32_t slot = strip_slot(prm, da, db, t, &ga, &gb);
    if (record_empty(window_record(c, dyn, d, slot))) return;
    const unsigned long long key = cell_key(ga, gb);
    const uint32_t mask = ar.table - 1u;
    uint32_t s = tile_home(key, mask);
    for (uint32_t step = 0; step < ar.table; step++) {
        unsigned long long k = key_at(ar.keys, s);
        if (k == TILE_NONE) {
            k = atomicCAS(&ar.keys[s], TILE_NONE, key);
            if (k == TILE_NONE) {   // this lane claimed the slot for its tile
                const unsigned long long at = atomicAdd(&ar.ctl[AR_CLAIMS], 1ull);
                if (at < (unsigned long long)ar.table) ar.claims[at] = (int32_t)s;
                return;
            }
        }
        if (k == key) return;
        s = (s + 1u) & mask;
    }
    atomicOr(&ar.ctl[AR_OVERFLOW], 1ull);   // more tiles than slots: far more than pages, the call is refused
}

// the decision of a call, the same in every lane that asks
__device__ __forceinline__ bool claims_granted(const Archive& ar, unsigned long long claims) {
    return ar.ctl[AR_OVERFLOW] == 0ull && claims <= ar.ctl[AR_FREE] && claims <= (unsigned long long)ar.table;
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_assign(Archive ar) {
    const unsigned long long claims = ar.ctl[AR_CLAIMS];
    const unsigned long long listed = claims < (unsigned long long)ar.table ? claims : (unsigned long long)ar.table;
    if ((unsigned long long)blockIdx.x >= listed) return;
    const uint32_t s = (uint32_t)ar.claims[blockIdx.x];
    if (s >= ar.table) return;
    if (!claims_granted(ar, claims)) {
        if (threadIdx.x == 0) ar.keys[s] = TILE_NONE;   // its page is -1 still
        return;
    }
    const int32_t pg = ar.stack[ar.ctl[AR_FREE] - 1ull - (unsigned long long)blockIdx.x];
    if (pg < 0 || pg >= ar.max_tiles) return;
    store_record(ar.pages, pg, threadIdx.x, empty_record());
    if (threadIdx.x == 0) ar.page[s] = pg;
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_store(Params prm, int32_t da, int32_t db, Cells c, bool dyn, DynPlanes d, Archive ar) {
    const uint32_t t = blockIdx.x * ARCH_BLOCK + threadIdx.x;
    bool stored = false, lost = false;
    if (t < strip_count(prm.nx, prm.nz, da, db)) {
        int32_t ga, gb;
        const uint32_t slot = strip_slot(prm, da, db, t, &ga, &gb);
        const Record r = window_record(c, dyn, d, slot);
        const int32_t pg = find_page(ar, cell_key(ga, gb));
        if (pg >= 0) {
            store_record(ar.pages, pg, tile_index(ga, gb), r);
            stored = true;
        } else {
            lost = !record_empty(r);
        }
    }
    wave_count(stored, &ar.ctl[AR_SAVED]);
    wave_count(lost, &ar.ctl[AR_LOST]);
    if (t == 0) {   // the call's claims are settled: k_grid_arch_assign has run, and no lane of this launch reads these words
        const unsigned long long claims = ar.ctl[AR_CLAIMS];
        if (claims_granted(ar, claims)) ar.ctl[AR_FREE] -= claims;
        else ar.ctl[AR_REFUSED] += 1ull;
        ar.ctl[AR_CLAIMS] = 0ull, ar.ctl[AR_OVERFLOW] = 0ull;
    }
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_enter(Params prm, int32_t da, int32_t db, Cells c, bool dyn, DynPlanes d, Archive ar) {
    const uint32_t t = blockIdx.x * ARCH_BLOCK + threadIdx.x;
    bool restored = false;
    if (t < strip_count(prm.nx, prm.nz, -(int64_t)da, -(int64_t)db)) {
        int32_t ga, gb;
        const uint32_t s = strip_slot(prm, -(int64_t)da, -(int64_t)db, t, &ga, &gb);
        const int32_t pg = find_page(ar, cell_key(ga, gb));
        restored = pg >= 0;
        const Record r = restored ? page_record(ar.pages, pg, tile_index(ga, gb)) : empty_record();
        c.kmin[s] = r.cell.kmin, c.kmax[s] = r.cell.kmax;
        c.count[s] = r.cell.count, c.overhead[s] = r.cell.overhead, c.pass[s] = r.pass;
        c.hsum[s] = (unsigned long long)r.cell.hsum, c.vsum[s] = (unsigned long long)r.cell.vsum;
        if (dyn) {
            d.body[s] = make_int2(0, 0);
            d.contra[s] = r.contra, d.last[s] = r.last, d.kept[s] = 0, d.event[s] = 0;
        }
    }
    wave_count(restored, &ar.ctl[AR_RESTORED]);
}

// the record of a global cell: the window's, a page's or the empty one
__device__ __forceinline__ Record region_record(const Params& prm, const Cells& c, const Archive& ar, int32_t ga, int32_t gb) {
    const int32_t ia = ga - prm.oa, ib = gb - prm.ob;
    if (ia >= 0 && ia < prm.nx && ib >= 0 && ib < prm.nz) return window_record(c, false, DynPlanes{}, slot_at(prm, ia, ib));
    const int32_t pg = find_page(ar, cell_key(ga, gb));
    return pg >= 0 ? page_record(ar.pages, pg, tile_index(ga, gb)) : empty_record();
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_region(Params prm, Cells c, Archive ar, int32_t kind, int32_t plane, int32_t ga0, int32_t gb0,
                                                                int32_t w, int32_t h, void* __restrict__ out) {
    const uint32_t i = blockIdx.x * ARCH_BLOCK + threadIdx.x;
    if (i >= (uint32_t)w * (uint32_t)h) return;
    const uint32_t y = i / (uint32_t)w, x = i - y * (uint32_t)w;
    const Record r = region_record(prm, c, ar, ga0 + (int32_t)x, gb0 + (int32_t)y);
    const Final f = finalise(prm, r.cell);
    if (kind == RK_LOCAL) {
        if (plane == L_PASS) ((int32_t*)out)[i] = r.pass;
        else ((uint8_t*)out)[i] = state_of(prm, f.cls, r.pass);
        return;
    }
    switch (plane) {
    case P_COUNT: ((int32_t*)out)[i] = r.cell.count; break;
    case P_OVERHEAD: ((int32_t*)out)[i] = r.cell.overhead; break;
    case P_HMIN: ((float*)out)[i] = f.hmin; break;
    case P_HMAX: ((float*)out)[i] = f.hmax; break;
    case P_HMEAN: ((float*)out)[i] = f.hmean; break;
    case P_INTENSITY: ((uint8_t*)out)[i] = f.intensity; break;
    default: ((uint8_t*)out)[i] = f.cls; break;
    }
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_render(Params prm, Cells c, Archive ar, int32_t mode, int32_t ga0, int32_t gb0, int32_t w,
                                                                int32_t h, uint8_t* __restrict__ rgb) {
    const uint32_t o = blockIdx.x * ARCH_BLOCK + threadIdx.x;
    if (o >= (uint32_t)w * (uint32_t)h) return;
    const uint32_t row = o / (uint32_t)w, col = o - row * (uint32_t)w;
    const Record r = region_record(prm, c, ar, ga0 + (int32_t)col, gb0 + (h - 1 - (int32_t)row));
    const Final f = finalise(prm, r.cell);
    uint8_t px[3];
    if (mode == M_LOCAL) colour_local(prm, r.cell.count, f, r.pass, px);
    else colour(prm, mode, r.cell.count, f, px);
    rgb[3 * (size_t)o] = px[0], rgb[3 * (size_t)o + 1] = px[1], rgb[3 * (size_t)o + 2] = px[2];
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_collect(Archive ar, int32_t ga0, int32_t gb0, int32_t ga1, int32_t gb1,
                                                                 unsigned long long* __restrict__ skeys, int32_t* __restrict__ spages) {
    const uint32_t s = blockIdx.x * ARCH_BLOCK + threadIdx.x;
    if (s >= ar.table) return;
    const unsigned long long k = ar.keys[s];
    if (k == TILE_NONE) return;
    const int32_t pg = ar.page[s];
    if (pg < 0 || pg >= ar.max_tiles) return;
    if (tile_meets(key_ta(k), key_tb(k), ga0, gb0, ga1, gb1)) {
        const unsigned long long at = atomicAdd(&ar.ctl[AR_CLAIMS], 1ull);
        if (at < (unsigned long long)ar.max_tiles) skeys[at] = k, spages[at] = pg;
    } else {
        const unsigned long long at = atomicAdd(&ar.ctl[AR_FREE], 1ull);
        if (at < (unsigned long long)ar.max_tiles) ar.stack[at] = pg;
    }
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_insert(Archive ar, const unsigned long long* __restrict__ skeys, const int32_t* __restrict__ spages) {
    const uint32_t t = blockIdx.x * ARCH_BLOCK + threadIdx.x;
    const unsigned long long kept = ar.ctl[AR_CLAIMS];
    if (t >= (uint32_t)ar.max_tiles || (unsigned long long)t >= kept) return;
    const unsigned long long key = skeys[t];
    const uint32_t mask = ar.table - 1u;
    uint32_t s = tile_home(key, mask);
    for (uint32_t step = 0; step < ar.table; step++) {   // the keys are distinct and fewer than half the slots
        if (atomicCAS(&ar.keys[s], TILE_NONE, key) == TILE_NONE) {
            ar.page[s] = spages[t];
            return;
        }
        s = (s + 1u) & mask;
    }
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_grid_arch_reset(Archive ar) {
    const uint32_t t = blockIdx.x * ARCH_BLOCK + threadIdx.x;
    if (t < (uint32_t)ar.max_tiles) ar.stack[t] = (int32_t)t;
    if (t < (uint32_t)AR_WORDS) ar.ctl[t] = t == (uint32_t)AR_FREE ? (unsigned long long)ar.max_tiles : 0ull;
}

unsigned blocks_for(uint64_t lanes) { return (unsigned)((lanes + ARCH_BLOCK - 1) / ARCH_BLOCK); }

// the distinct tiles the leaving cells of a scroll can touch: the most claims a call can make
uint64_t leaving_tiles(const Params& p, int32_t da, int32_t db) {
    if (strip_whole(p.nx, p.nz, da, db)) return (uint64_t)(tiles_spanned(p.oa, p.nx) * tiles_spanned(p.ob, p.nz));
    const int32_t cols = da < 0 ? -da : da, rows = db < 0 ? -db : db;
    uint64_t n = 0;
    if (cols > 0) n += (uint64_t)(tiles_spanned(da > 0 ? p.oa : p.oa + p.nx - cols, cols) * tiles_spanned(p.ob, p.nz));
    if (rows > 0) n += (uint64_t)(tiles_spanned(da > 0 ? p.oa + cols : p.oa, p.nx - cols) * tiles_spanned(db > 0 ? p.ob : p.ob + p.nz - rows, rows));
    return n;
}

}  // namespace

void launch_archive_reset(hipStream_t s, const Archive& ar) {
    const uint64_t lanes = (uint64_t)ar.max_tiles > (uint64_t)AR_WORDS ? (uint64_t)ar.max_tiles : (uint64_t)AR_WORDS;
    hipLaunchKernelGGL(k_grid_arch_reset, dim3(blocks_for(lanes)), dim3(ARCH_BLOCK), 0, s, ar);
}

void launch_archive_leave(hipStream_t s, const ArchScrollJob& j) {
    const unsigned blocks = blocks_for(strip_count(j.prm.nx, j.prm.nz, j.da, j.db));
    uint64_t claims = leaving_tiles(j.prm, j.da, j.db);
    claims = claims < (uint64_t)j.ar.table ? claims : (uint64_t)j.ar.table;
    hipLaunchKernelGGL(k_grid_arch_claim, dim3(blocks), dim3(ARCH_BLOCK), 0, s, j.prm, j.da, j.db, j.cells, j.dyn, j.planes, j.ar);
    hipLaunchKernelGGL(k_grid_arch_assign, dim3((unsigned)claims), dim3(ARCH_BLOCK), 0, s, j.ar);
    hipLaunchKernelGGL(k_grid_arch_store, dim3(blocks), dim3(ARCH_BLOCK), 0, s, j.prm, j.da, j.db, j.cells, j.dyn, j.planes, j.ar);
}

void launch_archive_enter(hipStream_t s, const ArchScrollJob& j) {
    const unsigned blocks = blocks_for(strip_count(j.prm.nx, j.prm.nz, -(int64_t)j.da, -(int64_t)j.db));
    hipLaunchKernelGGL(k_grid_arch_enter, dim3(blocks), dim3(ARCH_BLOCK), 0, s, j.prm, j.da, j.db, j.cells, j.dyn, j.planes, j.ar);
}

void launch_archive_region(hipStream_t s, const RegionJob& j, void* out) {
    hipLaunchKernelGGL(k_grid_arch_region, dim3(blocks_for((uint64_t)j.w * (uint64_t)j.h)), dim3(ARCH_BLOCK), 0, s, j.prm, j.cells, j.ar, j.kind, j.plane,
                       j.ga0, j.gb0, j.w, j.h, out);
}

void launch_archive_render_region(hipStream_t s, const RegionJob& j, int32_t mode, uint8_t* rgb) {
    hipLaunchKernelGGL(k_grid_arch_render, dim3(blocks_for((uint64_t)j.w * (uint64_t)j.h)), dim3(ARCH_BLOCK), 0, s, j.prm, j.cells, j.ar, mode, j.ga0,
                       j.gb0, j.w, j.h, rgb);
}

void launch_archive_trim_collect(hipStream_t s, const Archive& ar, int32_t ga0, int32_t gb0, int32_t ga1, int32_t gb1, unsigned long long* skeys,
                                 int32_t* spages) {
    hipLaunchKernelGGL(k_grid_arch_collect, dim3(blocks_for(ar.table)), dim3(ARCH_BLOCK), 0, s, ar, ga0, gb0, ga1, gb1, skeys, spages);
}

void launch_archive_trim_insert(hipStream_t s, const Archive& ar, const unsigned long long* skeys, const int32_t* spages) {
    hipLaunchKernelGGL(k_grid_arch_insert, dim3(blocks_for((uint64_t)ar.max_tiles)), dim3(ARCH_BLOCK), 0, s, ar, skeys, spages);
}

}  // namespace grid
}  // namespace svh

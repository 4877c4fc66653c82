// The objects of the ground grid and their tracks on the device (svh_grid_get_obj_plane, svh_grid_get_objects, svh_grid_objects_step,
// svh_grid_render_objects; include/svh_grid_obj.h, "OBJECTS").  The arithmetic is csrc/grid_obj_core.h: integer work on the finished
// STATE, HMAX and COUNT planes in logical order.  A label is the minimum of a set, every accumulator a commutative integer update and
// every choice the minimum or maximum of unique keys, so nothing here depends on the launch shape or the scheduling.  The number of
// launches is OBJ_LAUNCHES for the objects and 5 (7 with the gate) for a step, whatever the scene.
//
// The objects:
//   k_grid_obj_mask        FLAGS bit 0, LABEL = own index or -1, the object cells counted: the lanes stride, one atomic per wave.
//   (launch_front_label, launch_front_count, launch_front_roots of csrc/grid_front_kernels.hip: the tile and global union-find, the
//   roots compacted in ascending order)
//   k_grid_obj_accum       one lane per object cell: its component by a binary search of LABEL in the roots; size, the two sums, the
//                          box, the greatest HMAX bits and the sum of COUNT by atomics -- the lanes of a wave that share the component
//                          of its first object cell combined by shuffles first, as k_grid_front_accum does.
//   k_grid_obj_verdict     one lane per component: kept, large or low; the mark of the kept ones and the counts.
//   (launch_front_rank: the kept components ranked in order)
//   k_grid_obj_records     one lane per component: the record of a kept one at its rank.
//   k_grid_obj_flags       one lane per object cell: bits 1 and 2 of FLAGS.
// A step:
//   k_grid_obj_overlap     one lane per cell, at work on the kept cells: the pair (rank of the cell's object, index of the track the
//                          ID plane of the step before holds at the cell's global cell).  The lanes of a wave that share the pair
//                          of its first lane with one are combined, then the pair enters a lock-free open-addressing table (the scheme
//                          of view_thin_kernels.hip: atomicCAS on the 64-bit key, linear probing bounded by the capacity, a load
//                          factor of at most one half) and its count grows by atomicAdd.
//   k_grid_obj_claims      one lane per slot: a counting pair raises the claim of its object and of its track (64-bit atomicMax of
//                          overlap << 32 | ~index) and is counted for both.
//   k_grid_obj_match       one lane per object: mutual claims match.
//   k_grid_obj_gate        one lane per unmatched object, a loop over the tracks (at most 4096): its least key, and atomicMin of
//   k_grid_obj_gate_match  the key with its rank on each track within the gate; then mutual picks match.  Only when gate > 0.
//   k_grid_obj_update      one workgroup: the tracks updated and the survivors compacted in order by block scans, then the unmatched
//                          objects in ascending rank become new tracks while there is room; ASSIGN and the counts.
//   k_grid_obj_ids         one lane per cell: the new ID plane.
//
// A bound that is hit sets the unsettled word of the control block; the host returns SVH_ERR_HIP.  No kernel waits for another
// workgroup.
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "grid_comp_dev.h"
#include "grid_internal.h"
#include "grid_obj_core.h"

namespace svh {
namespace grid {
namespace {

constexpr unsigned long long EMPTY_PAIR = ~0ull;

// The lanes stride over the cells beyond OBJ_MASK_BLOCKS * OBJ_BLOCK of them and each wave adds its count once: one atomic per
// wave of cells on the one counter took 6.4 and 12.6 ms of a kernel trace at 8192 x 8192 (densities 0.01 and 0.3), where
// k_grid_finalise, which moves five times the bytes, takes 0.5 to 0.7 ms
__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_mask(uint32_t cells, const uint8_t* __restrict__ state, uint8_t* __restrict__ flags,
                                                             int32_t* __restrict__ label, unsigned long long* ctl) {
    int32_t n = 0;
    for (uint32_t i = blockIdx.x * OBJ_BLOCK + threadIdx.x; i < cells; i += gridDim.x * OBJ_BLOCK) {   // at most 128 rounds
        const bool f = obj_cell(state[i]);
        flags[i] = f ? (uint8_t)OF_OBJECT : (uint8_t)0;
        label[i] = f ? (int32_t)i : -1;
        n += f ? 1 : 0;
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&ctl[FC_CELLS], (unsigned long long)n);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int32_t)v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// The lanes of a wave whose component is that of the wave's first object cell are combined by shuffles and their leader issues the
// atomics; the other object cells of the wave issue their own.  A wave holds 64 consecutive cells of a row, so inside a solid object
// nearly every wave is of one component.  Sums, minima and maxima of integers: the grouping changes no byte.
__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_accum(int32_t nx, uint32_t cells, const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ roots, int32_t n_comp, const float* __restrict__ hmax,
                                                              const int32_t* __restrict__ count, ObjAcc acc) {
    const uint32_t i = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    int32_t k = -1, a = 0, b = 0, pts = 0;
    uint32_t hb = 0;
    if (i < cells && n_comp >= 1) {
        const int32_t l = label[i];
        if (l >= 0) {
            const int32_t r = rank_of(roots, n_comp, l);
            if (roots[r] == l) {                        // always: the roots are the labels that occur
                k = r;
                b = (int32_t)(i / (uint32_t)nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)nx);
                hb = bits_of(hmax[i]) ^ 0x80000000u, pts = count[i];
            }
        }
    }
    const unsigned long long live = __ballot(k >= 0);
    if (live == 0) return;                              // the whole wave
    const int32_t leader = __ffsll(live) - 1, k0 = __shfl(k, leader, 64);
    const bool mine = k == k0;
    const int32_t n = __popcll(__ballot(mine));
    const int32_t sa = wave_sum(mine ? a : 0), sb = wave_sum(mine ? b : 0);
    const int32_t a0 = wave_min(mine ? a : 0x7FFFFFFF), b0 = wave_min(mine ? b : 0x7FFFFFFF);
    const int32_t a1 = wave_max(mine ? a : -1), b1 = wave_max(mine ? b : -1);
    const uint32_t h1 = wave_max_u32(mine ? hb : 0u);
    // 64 counts of at most 2^31 - 1: the sum of a wave in two halves of 32 bits
    const long long ps = (long long)wave_sum(mine ? (pts & 0xFFFF) : 0) + ((long long)wave_sum(mine ? (pts >> 16) : 0) << 16);
    if (mine) {
        if ((int32_t)(threadIdx.x & 63u) != leader) return;
        atomicAdd(&acc.size[k], n);
        atomicAdd(&acc.sum[2 * k], (unsigned long long)sa);
        atomicAdd(&acc.sum[2 * k + 1], (unsigned long long)sb);
        atomicAdd(&acc.pts[k], (unsigned long long)ps);
        atomicMin(&acc.bmin[2 * k], a0), atomicMin(&acc.bmin[2 * k + 1], b0);
        atomicMax(&acc.bmax[2 * k], a1), atomicMax(&acc.bmax[2 * k + 1], b1);
        atomicMax(&acc.hbits[k], h1);
    } else if (k >= 0) {
        atomicAdd(&acc.size[k], 1);
        atomicAdd(&acc.sum[2 * k], (unsigned long long)a);
        atomicAdd(&acc.sum[2 * k + 1], (unsigned long long)b);
        atomicAdd(&acc.pts[k], (unsigned long long)(long long)pts);
        atomicMin(&acc.bmin[2 * k], a), atomicMin(&acc.bmin[2 * k + 1], b);
        atomicMax(&acc.bmax[2 * k], a), atomicMax(&acc.bmax[2 * k + 1], b);
        atomicMax(&acc.hbits[k], hb);
    }
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_verdict(ObjParams op, int32_t n_comp, ObjAcc acc, unsigned long long* ctl) {
    const uint32_t k = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    uint8_t v = 0;
    int32_t size = 0;
    if (k < (uint32_t)n_comp) {
        size = acc.size[k];
        v = size >= 1 ? obj_verdict(op, size, (int32_t)(acc.hbits[k] ^ 0x80000000u)) : (uint8_t)0;
        acc.mark[k] = v == OF_KEPT ? 1 : 0;
    }
    const unsigned long long large = __ballot(v == OF_LARGE), low = __ballot(v == OF_OBJECT);
    // the kept cells of the wave's 64 components, each at most 2^26: the sum in two halves of 32 bits, one atomic per wave
    const int32_t kept = v == OF_KEPT ? size : 0;
    const long long cells = (long long)wave_sum(kept & 0xFFFF) + ((long long)wave_sum(kept >> 16) << 16);
    if ((threadIdx.x & 63u) == 0) {
        if (large) atomicAdd(&ctl[OC_LARGE], (unsigned long long)__popcll(large));
        if (low) atomicAdd(&ctl[OC_LOW], (unsigned long long)__popcll(low));
        if (cells) atomicAdd(&ctl[FC_KEPT_CELLS], (unsigned long long)cells);
    }
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_records(int32_t oa, int32_t ob, int32_t n_comp, const int32_t* __restrict__ roots,
                                                                ObjAcc acc, const int32_t* __restrict__ slot, int32_t* __restrict__ recs) {
    const uint32_t k = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (k >= (uint32_t)n_comp) return;
    const int32_t at = slot[k];
    if (at < 0) return;
    const int64_t size = acc.size[k];
    int32_t* r = recs + (size_t)OBJ_REC * (size_t)at;
    r[OR_LABEL] = roots[k], r[OR_SIZE] = (int32_t)size;
    r[OR_GA_MIN] = oa + acc.bmin[2 * k], r[OR_GB_MIN] = ob + acc.bmin[2 * k + 1];
    r[OR_GA_MAX] = oa + acc.bmax[2 * k], r[OR_GB_MAX] = ob + acc.bmax[2 * k + 1];
    r[OR_C16_A] = obj_c16((int64_t)acc.sum[2 * k], size) + 16 * oa, r[OR_C16_B] = obj_c16((int64_t)acc.sum[2 * k + 1], size) + 16 * ob;
    r[OR_HMAX_BITS] = (int32_t)(acc.hbits[k] ^ 0x80000000u);
    r[OR_POINTS] = obj_points((int64_t)acc.pts[k]);
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_flags(ObjParams op, uint32_t cells, const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ roots, int32_t n_comp, ObjAcc acc,
                                                              uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (i >= cells || n_comp < 1) return;
    const int32_t l = label[i];
    if (l < 0) return;
    const int32_t k = rank_of(roots, n_comp, l);
    if (roots[k] != l) return;
    const uint8_t v = obj_verdict(op, acc.size[k], (int32_t)(acc.hbits[k] ^ 0x80000000u));
    if (v == OF_KEPT || v == OF_LARGE) flags[i] = (uint8_t)(OF_OBJECT | v);
}

// ---- a step ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t pair_home(unsigned long long key, uint32_t mask) {
    uint64_t x = key;                                   // the finaliser of splitmix64
    x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27, x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x & (uint64_t)mask;
}

// the index of track id among the n ascending records, -1 when it is not among them; at most 13 halvings
__device__ __forceinline__ int32_t track_index(const int32_t* __restrict__ tracks, int32_t n, int32_t id) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (tracks[(size_t)mid * TRACK_REC] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && tracks[(size_t)lo * TRACK_REC] == id ? lo : -1;
}

// the rank of the kept object that covers cell i, -1 when none does
__device__ __forceinline__ int32_t object_at(const ObjStepJob& j, uint32_t i) {
    if (!(j.flags[i] & OF_KEPT) || j.n_comp < 1) return -1;
    const int32_t l = j.label[i], k = rank_of(j.roots, j.n_comp, l);
    return j.roots[k] == l ? j.slot[k] : -1;
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_overlap(ObjStepJob j) {
    const uint32_t cells = (uint32_t)j.nx * (uint32_t)j.nz, i = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    unsigned long long key = EMPTY_PAIR;
    if (i < cells && j.n_prev >= 1) {
        const int32_t r = object_at(j, i);
        if (r >= 0 && r < j.n_obj) {
            const int32_t b = (int32_t)(i / (uint32_t)j.nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)j.nx);
            const int32_t pa = a + (j.oa - j.poa), pb = b + (j.ob - j.pob);   // offsets within +-2^20: no overflow
            if (pa >= 0 && pa < j.nx && pb >= 0 && pb < j.nz) {
                const int32_t tid = j.prev_id[(size_t)pb * (size_t)j.nx + (size_t)pa];
                const int32_t t = tid >= 0 ? track_index(j.prev, j.n_prev, tid) : -1;
                if (t >= 0) key = ((unsigned long long)(uint32_t)r << 32) | (unsigned long long)(uint32_t)t;
            }
        }
    }
    const bool has = key != EMPTY_PAIR;
    const unsigned long long live = __ballot(has);
    if (live == 0) return;                              // the whole wave
    const int32_t lane = (int32_t)(threadIdx.x & 63u), leader = __ffsll(live) - 1;
    const uint32_t hi0 = (uint32_t)__shfl((int32_t)(uint32_t)(key >> 32), leader, 64), lo0 = (uint32_t)__shfl((int32_t)(uint32_t)key, leader, 64);
    const bool mine = has && key == (((unsigned long long)hi0 << 32) | lo0);
    const unsigned long long same = __ballot(mine);
    const int32_t n = mine ? __popcll(same) : 1;
    if (!has || (mine && lane != leader)) return;
    const uint32_t mask = j.capacity - 1u;
    uint64_t s = pair_home(key, mask);
    for (uint32_t step = 0; step < j.capacity; step++) {
        const unsigned long long was = atomicCAS(&j.keys[s], EMPTY_PAIR, key);
        if (was == EMPTY_PAIR || was == key) {
            atomicAdd(&j.counts[s], n);
            return;
        }
        s = (s + 1) & (uint64_t)mask;
    }
    atomicMax(&j.ctl[SC_UNSETTLED], 1ull);              // never: the capacity is twice the pairs that can occur
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_claims(ObjStepJob j, ObjStepScratch w) {
    const uint32_t s = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (s >= j.capacity) return;
    const unsigned long long key = j.keys[s];
    if (key == EMPTY_PAIR) return;
    const int32_t o = j.counts[s], i = (int32_t)(key >> 32), t = (int32_t)(key & 0xFFFFFFFFull);
    if (o < j.op.min_overlap || i >= j.n_obj || t >= j.n_prev) return;
    atomicMax(&w.claim_obj[i], (unsigned long long)obj_claim_key(o, t));
    atomicMax(&w.claim_trk[t], (unsigned long long)obj_claim_key(o, i));
    atomicAdd(&w.cnt_obj[i], 1);
    atomicAdd(&w.cnt_trk[t], 1);
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_match(ObjStepJob j, ObjStepScratch w) {
    const uint32_t i = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (i >= (uint32_t)j.n_obj) return;
    const unsigned long long c = w.claim_obj[i];
    if (!c) return;
    const int32_t t = obj_claim_index(c);
    if (t < 0 || t >= j.n_prev || obj_claim_index(w.claim_trk[t]) != (int32_t)i) return;
    w.obj_trk[i] = t, w.trk_obj[t] = (int32_t)i, w.how[t] = TK_BY_OVERLAP;   // mutual: no other lane writes these
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_gate(ObjStepJob j, ObjStepScratch w) {
    const uint32_t i = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (i >= (uint32_t)j.n_obj || w.obj_trk[i] >= 0) return;
    const int32_t* obj = j.recs + (size_t)i * OBJ_REC;
    unsigned long long best = GATE_NONE;
    for (int32_t t = 0; t < j.n_prev; t++) {            // at most 4096
        if (w.how[t] == TK_BY_OVERLAP) continue;
        const unsigned long long d = obj_gate_key(j.op, j.prev + (size_t)t * TRACK_REC, obj, 0);
        if (d == GATE_NONE) continue;
        const unsigned long long mine = d | (unsigned long long)(uint32_t)t;
        best = mine < best ? mine : best;
        atomicMin(&w.pick_trk[t], d | (unsigned long long)i);
    }
    w.pick_obj[i] = best;
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_gate_match(ObjStepJob j, ObjStepScratch w) {
    const uint32_t i = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (i >= (uint32_t)j.n_obj) return;
    const unsigned long long c = w.pick_obj[i];
    if (c == GATE_NONE) return;
    const int32_t t = (int32_t)(c & 0xFFFFFFFFull);
    if (t >= j.n_prev || (uint32_t)(w.pick_trk[t] & 0xFFFFFFFFull) != i) return;
    w.obj_trk[i] = t, w.trk_obj[t] = (int32_t)i, w.how[t] = TK_BY_GATE;
}

__global__ __launch_bounds__(OBJ_UPDATE_BLOCK) void k_grid_obj_update(ObjStepJob j, ObjStepScratch w) {
    __shared__ int s_wave[OBJ_UPDATE_BLOCK / 64];
    __shared__ unsigned long long s_stat[SC_WORDS];
    constexpr int kBlock = (int)OBJ_UPDATE_BLOCK;
    if (threadIdx.x < SC_WORDS) s_stat[threadIdx.x] = 0;
    __syncthreads();
    int survivors = 0;
    for (int32_t base = 0; base < j.n_prev; base += kBlock) {
        const int32_t t = base + (int32_t)threadIdx.x;
        int32_t rec[TRACK_REC];
        int keep = 0, stat = -1;
        if (t < j.n_prev) {
            const int32_t* before = j.prev + (size_t)t * TRACK_REC;
            const int32_t i = w.trk_obj[t], split = w.cnt_trk[t] >= 2 ? (int32_t)TK_SPLIT : 0;
            if (i >= 0 && i < j.n_obj) {
                const int32_t how = w.how[t], won = how == TK_BY_OVERLAP ? obj_claim_overlap(w.claim_obj[i]) : 0;
                track_match(j.op, before, j.recs + (size_t)i * OBJ_REC, how, won, split | (w.cnt_obj[i] >= 2 ? (int32_t)TK_MERGED : 0), rec);
                j.assign[i] = before[TR_ID];
                keep = 1, stat = how == TK_BY_OVERLAP ? SC_BY_OVERLAP : SC_BY_GATE;
            } else {
                keep = track_miss(j.op, before, split, rec) ? 1 : 0;
                stat = keep ? SC_MISSED : SC_DROPPED;
            }
        }
        int chunk;
        const int at = survivors + block_exclusive_scan<kBlock>(keep, s_wave, &chunk);
        if (keep && at < j.op.max_tracks)
            for (int32_t k = 0; k < TRACK_REC; k++) j.tracks[(size_t)at * TRACK_REC + k] = rec[k];
        if (stat >= 0) atomicAdd(&s_stat[stat], 1ull);
        survivors += chunk;
    }
    const int room = track_room(j.op, survivors, j.next_id);
    int made = 0;
    for (int32_t base = 0; base < j.n_obj; base += kBlock) {
        const int32_t i = base + (int32_t)threadIdx.x;
        const int fresh = (i < j.n_obj && w.obj_trk[i] < 0) ? 1 : 0;
        int chunk;
        const int ord = made + block_exclusive_scan<kBlock>(fresh, s_wave, &chunk);
        if (fresh) {
            if (ord < room) {
                int32_t rec[TRACK_REC];
                track_new(j.op, j.next_id + ord, j.recs + (size_t)i * OBJ_REC, w.cnt_obj[i] >= 2 ? (int32_t)TK_MERGED : 0, rec);
                for (int32_t k = 0; k < TRACK_REC; k++) j.tracks[(size_t)(survivors + ord) * TRACK_REC + k] = rec[k];
                j.assign[i] = j.next_id + ord;
            } else {
                j.assign[i] = ASSIGN_UNTRACKED;
            }
        }
        made += chunk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int born = made < room ? made : room;
        j.ctl[SC_TRACKS] = (unsigned long long)(survivors + born);
        j.ctl[SC_NEW] = (unsigned long long)born, j.ctl[SC_UNTRACKED] = (unsigned long long)(made - born);
        j.ctl[SC_BY_OVERLAP] = s_stat[SC_BY_OVERLAP], j.ctl[SC_BY_GATE] = s_stat[SC_BY_GATE];
        j.ctl[SC_MISSED] = s_stat[SC_MISSED], j.ctl[SC_DROPPED] = s_stat[SC_DROPPED];
    }
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_ids(ObjStepJob j) {
    const uint32_t cells = (uint32_t)j.nx * (uint32_t)j.nz, i = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (i >= cells) return;
    const int32_t r = object_at(j, i);
    const int32_t a = (r >= 0 && r < j.n_obj) ? j.assign[r] : -1;
    j.id[i] = a >= 0 ? a : -1;
}

// ---- the image -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_overlay(int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* __restrict__ flags,
                                                                const int32_t* __restrict__ id, int32_t id_oa, int32_t id_ob,
                                                                const int32_t* __restrict__ tracks, int32_t n_tracks, uint8_t* rgb) {
    const uint32_t i = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (i >= (uint32_t)nx * (uint32_t)nz) return;
    const uint8_t f = flags[i];
    if (!(f & (OF_KEPT | OF_LARGE))) return;
    const int32_t b = (int32_t)(i / (uint32_t)nx), a = (int32_t)(i - (uint32_t)b * (uint32_t)nx);
    int32_t tid = -1;
    bool moving = false;
    if ((f & OF_KEPT) && id) {
        const int32_t pa = a + (oa - id_oa), pb = b + (ob - id_ob);
        if (pa >= 0 && pa < nx && pb >= 0 && pb < nz) tid = id[(size_t)pb * (size_t)nx + (size_t)pa];
        const int32_t t = tid >= 0 ? track_index(tracks, n_tracks, tid) : -1;
        if (t < 0) tid = -1;
        else moving = (tracks[(size_t)t * TRACK_REC + TR_FLAGS] & TK_MOVING) != 0;
    }
    uint8_t px[3];
    if (!colour_obj(f, tid, moving, px)) return;
    const size_t o = 3 * ((size_t)(nz - 1 - b) * (size_t)nx + (size_t)a);
    rgb[o] = px[0], rgb[o + 1] = px[1], rgb[o + 2] = px[2];
}

// one lane per track with a label: the cell ahead first, then the centroid's; two tracks on one cell write the same colour per mark,
// and the centroid of a track is drawn after every cell ahead by a launch of its own (mark 0, then mark 1)
__global__ __launch_bounds__(OBJ_BLOCK) void k_grid_obj_marks(int32_t nx, int32_t nz, int32_t oa, int32_t ob, const int32_t* __restrict__ tracks,
                                                              int32_t n_tracks, int32_t mark, uint8_t* rgb) {
    const uint32_t t = blockIdx.x * OBJ_BLOCK + threadIdx.x;
    if (t >= (uint32_t)n_tracks) return;
    const int32_t* r = tracks + (size_t)t * TRACK_REC;
    if (r[TR_LABEL] < 0) return;
    const int64_t ca = (int64_t)r[TR_C16_A] + (mark ? 0 : 8 * (int64_t)r[TR_V16_A]), cb = (int64_t)r[TR_C16_B] + (mark ? 0 : 8 * (int64_t)r[TR_V16_B]);
    const int64_t a = (int64_t)cell_of_c16(ca) - oa, b = (int64_t)cell_of_c16(cb) - ob;
    if (a < 0 || a >= nx || b < 0 || b >= nz) return;
    const size_t o = 3 * ((size_t)(nz - 1 - b) * (size_t)nx + (size_t)a);
    colour_mark(mark != 0, rgb + o);
}

inline unsigned blocks_of(size_t n, unsigned block) { return n ? (unsigned)((n + block - 1) / block) : 1u; }

FrontJob front_job(const ObjJob& j) {
    FrontJob f{};
    f.nx = j.nx, f.nz = j.nz, f.oa = j.oa, f.ob = j.ob;
    f.label = j.label, f.blockcnt = j.blockcnt, f.ctl = j.ctl;
    f.n_comp = j.n_comp, f.roots = j.roots;
    return f;
}

}  // namespace

int32_t launch_obj_mask(hipStream_t s, const ObjJob& j) {
    const uint32_t cells = (uint32_t)j.nx * (uint32_t)j.nz;
    hipLaunchKernelGGL(k_grid_obj_mask, dim3(std::min(blocks_of(cells, OBJ_BLOCK), OBJ_MASK_BLOCKS)), dim3(OBJ_BLOCK), 0, s, cells, j.state, j.flags,
                       j.label, j.ctl);
    return 1;
}

int32_t launch_obj_label(hipStream_t s, const ObjJob& j) {
    const FrontJob f = front_job(j);
    return launch_front_label(s, f) + launch_front_count(s, f);
}

int32_t launch_obj_table(hipStream_t s, const ObjJob& j) {
    const uint32_t cells = (uint32_t)j.nx * (uint32_t)j.nz, n = (uint32_t)j.n_comp;
    const ObjAcc acc = obj_acc(j.acc, n ? n : 1);
    const unsigned pc = blocks_of(cells, OBJ_BLOCK), cb = blocks_of(n, OBJ_BLOCK);
    int32_t launches = launch_front_roots(s, front_job(j));
    hipLaunchKernelGGL(k_grid_obj_accum, dim3(pc), dim3(OBJ_BLOCK), 0, s, j.nx, cells, (const int32_t*)j.label, (const int32_t*)j.roots, j.n_comp,
                       j.hmax, j.count, acc);
    hipLaunchKernelGGL(k_grid_obj_verdict, dim3(cb), dim3(OBJ_BLOCK), 0, s, j.op, j.n_comp, acc, j.ctl);
    // the block offsets of the cells are spent once the roots are scattered: the same counts serve the components
    launches += launch_front_rank(s, n, acc.mark, j.blockcnt, j.ctl + FC_KEPT, j.slot);
    hipLaunchKernelGGL(k_grid_obj_records, dim3(cb), dim3(OBJ_BLOCK), 0, s, j.oa, j.ob, j.n_comp, (const int32_t*)j.roots, acc,
                       (const int32_t*)j.slot, j.recs);
    hipLaunchKernelGGL(k_grid_obj_flags, dim3(pc), dim3(OBJ_BLOCK), 0, s, j.op, cells, (const int32_t*)j.label, (const int32_t*)j.roots, j.n_comp,
                       acc, j.flags);
    return launches + 4;
}

uint32_t obj_step_capacity(int64_t kept_cells, int64_t n_obj, int64_t n_prev) {
    const int64_t pairs = std::min(kept_cells, n_obj * n_prev);   // n_obj <= 2^26, n_prev <= 2^12
    uint32_t cap = 64;
    while ((int64_t)cap < 2 * pairs) cap <<= 1;                   // kept_cells <= 2^26: at most 2^27
    return cap;
}

int32_t launch_obj_step(hipStream_t s, const ObjStepJob& j) {
    const uint32_t cells = (uint32_t)j.nx * (uint32_t)j.nz;
    const ObjStepScratch w = obj_step_scratch(j);
    const unsigned pc = blocks_of(cells, OBJ_BLOCK), po = blocks_of((size_t)j.n_obj, OBJ_BLOCK);
    int32_t launches = 5;
    hipLaunchKernelGGL(k_grid_obj_overlap, dim3(pc), dim3(OBJ_BLOCK), 0, s, j);
    hipLaunchKernelGGL(k_grid_obj_claims, dim3(blocks_of(j.capacity, OBJ_BLOCK)), dim3(OBJ_BLOCK), 0, s, j, w);
    hipLaunchKernelGGL(k_grid_obj_match, dim3(po), dim3(OBJ_BLOCK), 0, s, j, w);
    if (j.op.gate > 0) {
        hipLaunchKernelGGL(k_grid_obj_gate, dim3(po), dim3(OBJ_BLOCK), 0, s, j, w);
        hipLaunchKernelGGL(k_grid_obj_gate_match, dim3(po), dim3(OBJ_BLOCK), 0, s, j, w);
        launches += 2;
    }
    hipLaunchKernelGGL(k_grid_obj_update, dim3(1), dim3(OBJ_UPDATE_BLOCK), 0, s, j, w);
    hipLaunchKernelGGL(k_grid_obj_ids, dim3(pc), dim3(OBJ_BLOCK), 0, s, j);
    return launches;
}

void launch_obj_overlay(hipStream_t s, int32_t nx, int32_t nz, int32_t oa, int32_t ob, const uint8_t* flags, const int32_t* id, int32_t id_oa,
                        int32_t id_ob, const int32_t* tracks, int32_t n_tracks, uint8_t* rgb) {
    const uint32_t cells = (uint32_t)nx * (uint32_t)nz;
    hipLaunchKernelGGL(k_grid_obj_overlay, dim3(blocks_of(cells, OBJ_BLOCK)), dim3(OBJ_BLOCK), 0, s, nx, nz, oa, ob, flags, id, id_oa, id_ob, tracks,
                       n_tracks, rgb);
    for (int32_t mark = 0; mark < 2; mark++)
        hipLaunchKernelGGL(k_grid_obj_marks, dim3(blocks_of((size_t)n_tracks, OBJ_BLOCK)), dim3(OBJ_BLOCK), 0, s, nx, nz, oa, ob, tracks, n_tracks, mark,
                           rgb);
}

}  // namespace grid
}  // namespace svh

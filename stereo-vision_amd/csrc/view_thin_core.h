// The arithmetic of the voxel-grid thinning of the map view (svh_view_thin, include/svh_view.h): which voxel a point
// falls into, which points fall into none, the 63-bit key of a voxel, where the key starts probing in the table and how
// large the table is.  THE CONTRACT IS THIS ARITHMETIC.  Compiled from this one header by
//   * hipcc into the kernels of csrc/view_thin_kernels.hip,
//   * the host compiler into csrc/view_engine.cpp (the capacity, and the test entry svh_test_thin_keys, which evaluates
//     every function below on the host),
// and restated in numpy by tests/view_thin_ref.py, which tests/test_view_thin.py pins against svh_test_thin_keys.
// Built like the rest of the library, without fast-math: the division below is IEEE's, rounded once, never a
// multiplication by a reciprocal, and denormal quotients are kept (-1e-45f / 0.5f lies in cell -1).
#pragma once
#include <math.h>
#include <stdint.h>

#include "mono_core.h"   // MC_FN

namespace svh {
namespace thin {

constexpr int32_t  CELL_LIMIT = 1 << 20;           // a cell index lies in [-2^20, 2^20)
constexpr uint64_t EMPTY_KEY = ~(uint64_t)0;       // the empty slot; the key of a point that falls into no voxel
constexpr uint32_t NO_WINNER = 0xFFFFFFFFu;        // a slot nobody has entered its index into
constexpr uint32_t NO_HOME = 0xFFFFFFFFu;          // svh_test_thin_keys' home of an unplaceable point
constexpr uint64_t MIN_CAPACITY = 1024;            // slots

// the cell of one coordinate, still a float: -0.0f -> -0.0f (cell 0), -0.5f * voxel -> -1
MC_FN float cell(float x, float voxel) { return floorf(x / voxel); }

// decided on the float, before any conversion (the device's conversions saturate, the host's are undefined out of
// range): NaN fails both comparisons, +-Inf one of them, and so does the cell of a coordinate too large for its quotient
MC_FN bool cell_ok(float c) { return c >= -(float)CELL_LIMIT && c < (float)CELL_LIMIT; }

// A point is placeable iff its three coordinates are finite and its three cells lie in [-2^20, 2^20).  x / voxel of a
// finite x can overflow to +-Inf or, for an Inf / NaN x, be Inf / NaN: cell_ok rejects all of them, the test of x itself
// is what the contract says and costs nothing.
MC_FN bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }

// the key of (x, y, z), EMPTY_KEY when the point is not placeable: (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20)
MC_FN uint64_t key_of(float x, float y, float z, float voxel) {
    const float cx = cell(x, voxel), cy = cell(y, voxel), cz = cell(z, voxel);
    if (!(finite_f(x) && finite_f(y) && finite_f(z) && cell_ok(cx) && cell_ok(cy) && cell_ok(cz))) return EMPTY_KEY;
    const uint64_t ix = (uint64_t)((int32_t)cx + CELL_LIMIT), iy = (uint64_t)((int32_t)cy + CELL_LIMIT),
                   iz = (uint64_t)((int32_t)cz + CELL_LIMIT);
    return (ix << 42) | (iy << 21) | iz;
}

// the finaliser of splitmix64: every bit of the key reaches the low bits the table index is taken from
MC_FN uint64_t hash(uint64_t key) {
    uint64_t h = key;
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h;
}

// The capacity rule: the smallest power of two that is at least twice the number of points, and at least MIN_CAPACITY.
// The load factor is therefore at most one half, and a probe of `capacity` steps meets an empty slot or its own key.
// (n <= 2^31 - 4096 points, so the capacity is at most 2^32 slots and a slot index fits 32 bits.)
MC_FN uint64_t capacity_for(int64_t n) {
    uint64_t cap = MIN_CAPACITY;
    while (cap < 2 * (uint64_t)n) cap <<= 1;
    return cap;
}

// where a key starts probing; the probe goes on to (slot + 1) & (capacity - 1)
MC_FN uint32_t home_of(uint64_t key, uint64_t capacity) { return (uint32_t)(hash(key) & (capacity - 1)); }

}  // namespace thin
}  // namespace svh

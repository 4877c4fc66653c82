// The arithmetic of the ground grid's archive (svh_grid_set_archive, svh_grid_get_region, include/svh_grid_archive.h): which cells
// a scroll takes out of the window and which it brings in, the tile and the record a cell is kept in while it is outside, and what
// a cell of a region says.  THE CONTRACT IS THIS ARITHMETIC, integers throughout.  Compiled from this one header by hipcc into the
// kernels of csrc/grid_archive_kernels.hip and by the host compiler into csrc/grid_engine.cpp (the test entries
// svh_test_grid_archive_key / _strip, which evaluate every function below on the host); restated in numpy by
// tests/grid_archive_ref.py, which tests/test_grid_archive.py pins by hand and against the test entries.
//
// Everything a cell holds is an integer under a commutative update, addressed by its GLOBAL cell (grid_core.h "THE WINDOW").  So a
// cell that is stored when it leaves the window and put back when its global cell enters again is exactly the cell that never
// left: a window that scrolled away and back equals, bit for bit, one that never moved.
#pragma once
#include "grid_core.h"
#include "grid_dyn_core.h"

namespace svh {
namespace grid {

// A TILE is a block of 16 x 16 global cells: tile (ga >> 4, gb >> 4), the shift arithmetic (floor), index (gb & 15) * 16 + (ga & 15)
constexpr int32_t TILE_SHIFT = 4, TILE_SIDE = 1 << TILE_SHIFT, TILE_MASK = TILE_SIDE - 1, TILE_CELLS = TILE_SIDE * TILE_SIDE;
static_assert((-17 >> TILE_SHIFT) == -2 && (-16 >> TILE_SHIFT) == -1 && (-1 >> TILE_SHIFT) == -1, "the shift of a negative cell must floor");
constexpr int32_t TILE_BIAS = 1 << 20;                 // |ga| < 2^20: a biased tile coordinate lies in 2^20 - 2^16 .. 2^20 + 2^16 - 1
constexpr unsigned long long TILE_NONE = ~0ull;        // the empty table slot; no key has it
constexpr int32_t ARCHIVE_MAX_TILES = 1 << 20, ARCHIVE_DEFAULT_TILES = 16384;
constexpr int32_t REGION_MAX_SIDE = 8192;              // w and h of a region lie in 1..8192
// A RECORD is what belongs to a cell and is not derived: the seven accumulators of Cells (kmin, kmax, count, overhead, hsum, vsum,
// pass: 4 + 4 + 4 + 4 + 8 + 8 + 4 bytes) and the dynamics' CONTRA and LAST (4 + 4).  A PAGE is the 256 records of a tile, a plane
// per field: 44 * 256 bytes
constexpr size_t RECORD_BYTES = 44, PAGE_BYTES = RECORD_BYTES * (size_t)TILE_CELLS;
enum ArchiveStat : int32_t { AS_PAGES = 0, AS_MAX_TILES, AS_SAVED, AS_RESTORED, AS_LOST, AS_REFUSED, AS_WORDS };
// planes of svh_grid_get_region by kind
enum RegionKind : int32_t { RK_GRID = 0, RK_LOCAL = 1, RK_KINDS };

struct Record {
    Cell cell;
    int32_t pass, contra, last;
};
MC_FN Record empty_record() { return Record{empty_cell(), 0, 0, 0}; }
// "not empty": what makes a tile need a page.  kmin, kmax, hsum and vsum are empty whenever count is 0
MC_FN bool record_empty(const Record& r) { return r.cell.count == 0 && r.cell.overhead == 0 && r.pass == 0 && r.contra == 0 && r.last == 0; }

MC_FN int32_t tile_of(int32_t g) { return g >> TILE_SHIFT; }
MC_FN uint32_t tile_index(int32_t ga, int32_t gb) { return (uint32_t)((gb & TILE_MASK) * TILE_SIDE + (ga & TILE_MASK)); }
// the key of tile (ta, tb): tb in the high word, so that keys ascend by (tb, ta)
MC_FN unsigned long long tile_key(int32_t ta, int32_t tb) {
    return ((unsigned long long)(uint32_t)(tb + TILE_BIAS) << 32) | (unsigned long long)(uint32_t)(ta + TILE_BIAS);
}
MC_FN int32_t key_ta(unsigned long long key) { return (int32_t)(uint32_t)(key & 0xFFFFFFFFull) - TILE_BIAS; }
MC_FN int32_t key_tb(unsigned long long key) { return (int32_t)(uint32_t)(key >> 32) - TILE_BIAS; }
MC_FN unsigned long long cell_key(int32_t ga, int32_t gb) { return tile_key(tile_of(ga), tile_of(gb)); }

// the table: a power of two of at least twice max_tiles slots, so the load factor stays at or below one half
MC_FN uint32_t archive_table_size(int32_t max_tiles) {
    uint32_t n = 2;
    while (n < 2u * (uint32_t)max_tiles) n <<= 1;
    return n;
}
// where the probe of a key starts: the finaliser of splitmix64
MC_FN uint32_t tile_home(unsigned long long key, uint32_t mask) {
    unsigned long long x = key;
    x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27, x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)x & mask;
}

// THE STRIPS.  The cells of a window of nx x nz that are NOT in the same window displaced by (da, db) cells, each exactly once: the
// |da| columns on the side the displacement leaves behind over all nz rows, then the |db| rows on that side over the other nx - |da|
// columns (the corner block belongs to the columns).  When |da| >= nx or |db| >= nz it is the whole window, row by row.
//   LEAVING a scroll by (da, db): strip_cell(.., da, db, ..) in the OLD window's cells.
//   ENTERING:                     strip_cell(.., -da, -db, ..) in the NEW window's cells.
MC_FN bool strip_whole(int32_t nx, int32_t nz, int64_t da, int64_t db) { return da >= nx || -da >= nx || db >= nz || -db >= nz; }
MC_FN uint32_t strip_count(int32_t nx, int32_t nz, int64_t da, int64_t db) {
    if (strip_whole(nx, nz, da, db)) return (uint32_t)nx * (uint32_t)nz;
    const uint32_t cols = (uint32_t)(da < 0 ? -da : da), rows = (uint32_t)(db < 0 ? -db : db);
    return cols * (uint32_t)nz + rows * ((uint32_t)nx - cols);
}
// lane t < strip_count -> window cell (ia, ib)
MC_FN void strip_cell(int32_t nx, int32_t nz, int64_t da, int64_t db, uint32_t t, int32_t* ia, int32_t* ib) {
    if (strip_whole(nx, nz, da, db)) {
        *ib = (int32_t)(t / (uint32_t)nx);
        *ia = (int32_t)(t - (uint32_t)*ib * (uint32_t)nx);
        return;
    }
    const uint32_t cols = (uint32_t)(da < 0 ? -da : da), rows = (uint32_t)(db < 0 ? -db : db);
    const uint32_t in_cols = cols * (uint32_t)nz;
    uint32_t a, b;
    if (t < in_cols) {   // the columns: the low side when the displacement is upwards
        b = t / cols;
        a = t - b * cols;
        if (da < 0) a += (uint32_t)nx - cols;
    } else {             // the rows, without the columns above
        const uint32_t w = (uint32_t)nx - cols;
        t -= in_cols;
        b = t / w;
        a = t - b * w;
        if (da > 0) a += cols;
        if (db < 0) b += (uint32_t)nz - rows;
    }
    *ia = (int32_t)a, *ib = (int32_t)b;
}

// the tiles a run of n >= 1 global cells from g0 touches along one axis
MC_FN int64_t tiles_spanned(int32_t g0, int32_t n) { return (int64_t)tile_of(g0 + n - 1) - (int64_t)tile_of(g0) + 1; }

// the checks behind SVH_ERR_BAD_ARG of svh_grid_get_region / svh_grid_render_region: every cell of the box is a global cell
MC_FN bool region_ok(int64_t ga0, int64_t gb0, int64_t w, int64_t h) {
    const int64_t lim = (int64_t)1 << 20;
    return w >= 1 && w <= REGION_MAX_SIDE && h >= 1 && h <= REGION_MAX_SIDE && ga0 > -lim && gb0 > -lim && ga0 + w - 1 < lim && gb0 + h - 1 < lim;
}
// ... of svh_grid_archive_trim
MC_FN bool trim_ok(int64_t ga0, int64_t gb0, int64_t ga1, int64_t gb1) {
    const int64_t lim = (int64_t)1 << 20;
    return ga0 <= ga1 && gb0 <= gb1 && ga0 > -lim && gb0 > -lim && ga1 < lim && gb1 < lim;
}
// a tile has a cell in the box of global cells ga0..ga1 x gb0..gb1
MC_FN bool tile_meets(int32_t ta, int32_t tb, int32_t ga0, int32_t gb0, int32_t ga1, int32_t gb1) {
    return ta >= tile_of(ga0) && ta <= tile_of(ga1) && tb >= tile_of(gb0) && tb <= tile_of(gb1);
}

}  // namespace grid
}  // namespace svh

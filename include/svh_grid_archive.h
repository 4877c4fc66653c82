/* ARCHIVE: the cells that scroll out of the window are kept and put back when the window returns, and the finished planes can be read
 * over any box of global cells.  Included by svh_grid.h; the entries are declared here, in a header of their own.  The arithmetic is
 * stereo-vision_amd/csrc/grid_archive_core.h (restated in tests/grid_archive_ref.py): integers throughout.
 *
 * Everything a cell holds is an integer under a commutative update, addressed by its global cell.  So a cell stored when it leaves the
 * window and put back when its global cell enters again is exactly the cell that never left: A WINDOW THAT SCROLLED AWAY AND BACK
 * EQUALS, BIT FOR BIT, A WINDOW THAT NEVER MOVED, in every plane of svh_grid_get and svh_grid_get_local (as long as no page was
 * refused, below).
 *
 * OFF BY DEFAULT.  Without svh_grid_set_archive every entry of svh_grid.h behaves as it always did, byte for byte and launch for launch.
 *
 * TILE.  A block of 16 x 16 global cells: tile (ga >> 4, gb >> 4), the shift arithmetic, so tile -1 holds the cells -16 .. -1.  The
 * cell's index inside its tile is (gb & 15) * 16 + (ga & 15).  A tile's key is 64 bits, (tb + 2^20) << 32 | (ta + 2^20); the word of
 * all ones is the empty slot of the table.
 * RECORD.  What belongs to a cell and is not derived: the seven accumulators (lowest and highest key, COUNT, OVERHEAD, the sums of
 * heights and intensities, PASS) and the dynamics' CONTRA and LAST, both 0 on a grid without the dynamics: 44 bytes.  The dynamics'
 * body, the kept THROUGH and the event byte are derived or belong to the last observation: they enter empty.
 * PAGE.  The 256 records of one tile, a plane per field: 11 264 bytes.
 * STORE.  A pool of max_tiles pages (max_tiles x 11 264 bytes: 176 MiB at the default 16 384) and a lock-free open-addressing table
 * from tile key to page of at least 2 max_tiles slots (12 bytes each, and 4 more for the bookkeeping of a scroll).  The pool is
 * allocated by the first scroll that needs it.
 *
 * A SCROLL by (da, db) with the layer on, in this order:
 *   LEAVING, with the old offsets: the cells of the old window that are not in the new one, each exactly once (the corner block of a
 *   diagonal scroll once; the whole window when |da| >= nx or |db| >= nz).  A leaving cell whose tile has a page is stored there, EVEN
 *   IF IT IS EMPTY: a cell that the dynamics cleared inside the window overwrites its older record.  A tile without a page NEEDS one
 *   when at least one leaving cell of it is not empty -- COUNT, OVERHEAD or PASS is not 0, or CONTRA or LAST is not 0.  Let `need` be
 *   the distinct tiles that need a page and `free` the unused pages.  If need <= free every such tile gets a page, its leaving cells are
 *   stored, and its cells that never left hold the empty record.  Otherwise NONE of them gets a page in this call: their leaving cells
 *   that are not empty are lost and counted, and the call is counted as refused; tiles that had a page before are stored as ever.  The
 *   decision is all or nothing per call, so what survives never depends on scheduling.
 *   ENTERING, with the new offsets: the cells of the new window that are not in the old one.  An entering cell whose tile has a page
 *   takes its record from the page; every other entering cell is the empty cell, as without the layer.  Restoring does not modify the
 *   page: the record of a cell that is inside the window is never visible, and is overwritten when the cell next leaves.
 * The scroll keeps its one host wait.  Which page number a tile gets may depend on scheduling; no byte that leaves the object does.
 *
 * WHAT FORGETS THE ARCHIVE.  svh_grid_clear and svh_grid_set_window (the stamp restarts there, and a new low corner renumbers the global
 * cells); svh_grid_archive_clear, alone; svh_grid_set_archive with another max_tiles; max_tiles = 0, which also turns the layer off and
 * frees the pool.  After SVH_ERR_HIP inside an add, an observation, a scroll or a follow the grid is EMPTY, as svh_grid.h says, and
 * so is the archive; after SVH_ERR_HIP inside svh_grid_archive_trim the archive is empty and the window untouched.
 *
 * DYNAMICS.  A restored LAST is the stamp it had: SVH_GRID_DYN_AGE of a restored cell counts the observations it spent outside.  Under
 * max_age > 0 a cell that comes back after more than max_age observations is therefore aged by the next observation -- what the
 * dynamics say about any cell without a point for that long.  A record keeps CONTRA and LAST only while the layer is set: a cell that
 * leaves while the dynamics are dropped stores 0 for both.
 *
 * CACHE.  Nothing is computed from the archive and kept: svh_grid_set_archive, svh_grid_archive_clear and svh_grid_archive_trim leave
 * every cached layer current.  A scroll makes stale what it always did.  The region entries change nothing and cache nothing.
 */
#ifndef SVH_GRID_ARCHIVE_H
#define SVH_GRID_ARCHIVE_H

#include "svh_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svh_grid_archive_params {
    int32_t max_tiles;         /* 16384: pages of the pool; 0 .. 2^20, 0 = the layer is off */
} svh_grid_archive_params;

void      svh_grid_archive_params_default(svh_grid_archive_params* p);
/* SVH_ERR_BAD_ARG, nothing changed: max_tiles out of range.  The value in force again changes nothing; another one empties the archive */
int32_t   svh_grid_set_archive(svh_grid* g, const svh_grid_archive_params* p);
/* max_tiles in force, 0 on a grid without the layer */
int32_t   svh_grid_get_archive(svh_grid* g, svh_grid_archive_params* p);
/* since the archive was last emptied: out[0] pages in use, out[1] max_tiles, out[2] cells stored into pages, out[3] cells restored from
 * pages (empty records count in both), out[4] cells that were not empty and lost, out[5] calls in which new tiles were refused */
int32_t   svh_grid_get_archive_stats(svh_grid* g, int64_t out[6]);
int32_t   svh_grid_archive_clear(svh_grid* g);
/* drops every tile that has no cell in the box of global cells ga0 .. ga1 x gb0 .. gb1, bounds inclusive, ga0 <= ga1, gb0 <= gb1, every
 * bound of magnitude below 2^20 (else SVH_ERR_BAD_ARG); their pages are unused again.  The window is untouched.  Without the layer, or
 * with an empty archive, there is nothing to do */
int32_t   svh_grid_archive_trim(svh_grid* g, int32_t ga0, int32_t gb0, int32_t ga1, int32_t gb1);
/* the tiles that have a page: *n their number, the first min(*n, cap) as pairs (ta, tb) to keys (host memory), ascending by (tb, ta) */
int32_t   svh_grid_archive_tiles(svh_grid* g, int32_t* keys, int64_t cap, int64_t* n);

/* kinds of svh_grid_get_region; mode 3 of svh_grid_render_region */
#define SVH_GRID_REGION_GRID   0   /* `plane` is a plane of svh_grid_get */
#define SVH_GRID_REGION_LOCAL  1   /* `plane` is a plane of svh_grid_get_local */
#define SVH_GRID_RENDER_LOCAL  3   /* the colours of svh_grid_render_local */
/* a plane over the box of w x h global cells from (ga0, gb0), w and h in 1 .. 8192, every cell of magnitude below 2^20: w * h elements of
 * the plane's type, row major, element [y * w + x] the cell (ga0 + x, gb0 + y).  A cell inside the window is read from the window; a
 * cell outside it whose tile has a page from that page; any other cell is the empty cell.  The finished value is the one svh_grid_get
 * computes: over the box (oa, ob, nx, nz) the result equals svh_grid_get bit for bit.  A device array of a 4-byte plane is 4-byte
 * aligned.  Without the layer the cells outside the window are empty */
int32_t   svh_grid_get_region(svh_grid* g, int32_t plane_kind, int32_t plane, int32_t ga0, int32_t gb0, int32_t w, int32_t h, void* out,
                              int32_t on_device);
/* the image of svh_grid_render (mode 0 .. 2) or svh_grid_render_local (mode 3) over the box: w * h * 3 bytes, row 0 the cells gb0 + h - 1 */
int32_t   svh_grid_render_region(svh_grid* g, int32_t mode, int32_t ga0, int32_t gb0, int32_t w, int32_t h, uint8_t* rgb, int32_t on_device);

#ifdef __cplusplus
}
#endif
#endif

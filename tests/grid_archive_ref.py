"""The ground grid's archive (stereo-vision_amd/csrc/grid_archive_core.h; include/svh_grid_archive.h) restated in numpy and plain
Python integers, on top of tests/grid_dyn_ref.py (and through it tests/grid_local_ref.py): a dictionary from tile to the records of its
256 global cells, the leaving and entering sets of a scroll, the all-or-nothing decision of a call, trim, and the planes over a box
of global cells.  This restatement keeps every plane of the window in logical order and has no torus, no table and no page numbers.
tests/test_grid_archive.py pins it by hand and compares the header with it; tests/test_grid_archive_gpu.py compares the device with
it, bit for bit."""
import numpy as np

import grid_dyn_ref as DR
import grid_local_ref as LR
import grid_ref as R

TILE = 16
BIAS = 2 ** 20
TILE_NONE = 2 ** 64 - 1
MAX_TILES, DEFAULT_TILES = 2 ** 20, 16384
RECORD_BYTES, PAGE_BYTES = 44, 44 * 256
REGION_MAX_SIDE = 8192
STATS = ("pages", "max_tiles", "stored", "restored", "lost", "refused")
# a record: the attribute of the window's plane, its type, its empty value
FIELDS = (("kmin", np.uint32, R.KMIN_EMPTY), ("kmax", np.uint32, R.KMAX_EMPTY), ("count", np.int32, 0), ("over", np.int32, 0),
          ("hsum", np.int64, 0), ("vsum", np.uint64, 0), ("passed", np.int32, 0), ("contra", np.int32, 0), ("last", np.int32, 0))
NOT_EMPTY = ("count", "over", "passed", "contra", "last")


def tile_of(g):
    """Python's >> floors, also below zero"""
    return g >> 4


def tile_index(ga, gb):
    return (gb & 15) * 16 + (ga & 15)


def tile_key(ta, tb):
    return ((tb + BIAS) << 32) | (ta + BIAS)


def table_size(max_tiles):
    n = 2
    while n < 2 * max_tiles:
        n *= 2
    return n


def strip(nx, nz, da, db):
    """the cells of a window of nx x nz that are not in the window displaced by (da, db), each once, in lane order: [n, 2] (ia, ib).
    The |da| columns on the side left behind over all rows, then the |db| rows over the other columns; the whole window, row by row,
    when |da| >= nx or |db| >= nz"""
    if abs(da) >= nx or abs(db) >= nz:
        ib, ia = np.divmod(np.arange(nx * nz), nx)
        return np.stack([ia, ib], 1).astype(np.int64)
    cols, rows = abs(da), abs(db)
    out = []
    if cols:
        b, a = np.divmod(np.arange(cols * nz), cols)
        out.append(np.stack([a + (nx - cols if da < 0 else 0), b], 1))
    if rows:
        w = nx - cols
        b, a = np.divmod(np.arange(rows * w), w)
        out.append(np.stack([a + (cols if da > 0 else 0), b + (nz - rows if db < 0 else 0)], 1))
    return np.concatenate(out).astype(np.int64)


def window_set(nx, nz, oa, ob):
    return {(oa + a, ob + b) for b in range(nz) for a in range(nx)}


def leaving_set(nx, nz, oa, ob, da, db):
    """by definition: the global cells of the old window that are not in the new one"""
    return window_set(nx, nz, oa, ob) - window_set(nx, nz, oa + da, ob + db)


def entering_set(nx, nz, oa, ob, da, db):
    return window_set(nx, nz, oa + da, ob + db) - window_set(nx, nz, oa, ob)


def empty_page():
    return {name: np.full(TILE * TILE, empty, t) for name, t, empty in FIELDS}


class Grid(DR.Grid):
    """grid_dyn_ref.Grid (the dynamics set or not) with the archive: set_archive, the scroll that stores and restores, trim, the tiles,
    the statistics, the planes and the image over a box of global cells"""

    def __init__(self, P, D=None, max_tiles=0):
        self.max_tiles = max_tiles
        self.pages = {}
        self.arch = dict.fromkeys(STATS[2:], 0)
        super().__init__(P, D)

    def archive_clear(self):
        self.pages = {}
        self.arch = dict.fromkeys(STATS[2:], 0)

    def clear(self):
        super().clear()
        self.archive_clear()

    def set_window(self, x0, z0):
        super().set_window(x0, z0)   # clears

    def set_archive(self, max_tiles):
        if not 0 <= max_tiles <= MAX_TILES:
            raise ValueError("max_tiles out of range")
        if max_tiles != self.max_tiles:
            self.archive_clear()
        self.max_tiles = max_tiles

    def archive_stats(self):
        return dict(self.arch, pages=len(self.pages), max_tiles=self.max_tiles)

    def archive_tiles(self):
        """[n, 2] (ta, tb), ascending by (tb, ta)"""
        return np.array(sorted(self.pages, key=lambda t: (t[1], t[0])), np.int32).reshape(-1, 2)

    def archive_trim(self, ga0, gb0, ga1, gb1):
        if not (ga0 <= ga1 and gb0 <= gb1 and max(abs(v) for v in (ga0, gb0, ga1, gb1)) < BIAS):
            raise ValueError("no such box")
        self.pages = {(ta, tb): p for (ta, tb), p in self.pages.items()
                      if tile_of(ga0) <= ta <= tile_of(ga1) and tile_of(gb0) <= tb <= tile_of(gb1)}

    def _record_planes(self):
        """the window's planes a record is taken from; without the dynamics CONTRA and LAST count as 0"""
        zero = np.zeros(self.P.nx * self.P.nz, np.int32)
        return {name: (zero if self.D is None and name in ("contra", "last") else getattr(self, name)) for name, _, _ in FIELDS}

    def scroll(self, da, db):
        if self.max_tiles == 0 or (da == 0 and db == 0):
            return super().scroll(da, db)
        if abs(self.oa + da) > LR.OFFSET_LIMIT or abs(self.ob + db) > LR.OFFSET_LIMIT:
            raise ValueError("offsets out of range")
        nx, nz = self.P.nx, self.P.nz
        # leaving, with the old offsets
        cells = strip(nx, nz, da, db)
        idx = cells[:, 1] * nx + cells[:, 0]
        ga, gb = cells[:, 0] + self.oa, cells[:, 1] + self.ob
        planes = self._record_planes()
        filled = np.zeros(len(idx), bool)
        for name in NOT_EMPTY:
            filled |= planes[name][idx] != 0
        tiles = [(int(a) >> 4, int(b) >> 4) for a, b in zip(ga, gb)]
        need = {t for t, f in zip(tiles, filled) if f and t not in self.pages}
        if len(need) <= self.max_tiles - len(self.pages):
            for t in need:
                self.pages[t] = empty_page()
        else:
            self.arch["refused"] += 1
        for k, t in enumerate(tiles):
            page = self.pages.get(t)
            if page is None:
                self.arch["lost"] += int(filled[k])
                continue
            at = tile_index(int(ga[k]), int(gb[k]))
            for name, _, _ in FIELDS:
                page[name][at] = planes[name][idx[k]]
            self.arch["stored"] += 1
        # the window moves: the strips that enter are empty
        super().scroll(da, db)
        # entering, with the new offsets
        cells = strip(nx, nz, -da, -db)
        for ia, ib in cells:
            g = (int(ia) + self.oa, int(ib) + self.ob)
            page = self.pages.get((g[0] >> 4, g[1] >> 4))
            if page is None:
                continue
            at, i = tile_index(*g), int(ib) * nx + int(ia)
            for name, _, _ in FIELDS:
                if self.D is None and name in ("contra", "last"):
                    continue
                getattr(self, name)[i] = page[name][at]
            self.arch["restored"] += 1
        return self

    def _region_records(self, ga0, gb0, w, h):
        if not (1 <= w <= REGION_MAX_SIDE and 1 <= h <= REGION_MAX_SIDE and -BIAS < ga0 and -BIAS < gb0 and ga0 + w - 1 < BIAS and gb0 + h - 1 < BIAS):
            raise ValueError("no such box")
        out = {name: np.full(w * h, empty, t) for name, t, empty in FIELDS}
        nx, nz = self.P.nx, self.P.nz
        for y in range(h):
            for x in range(w):
                ga, gb = ga0 + x, gb0 + y
                ia, ib = ga - self.oa, gb - self.ob
                if 0 <= ia < nx and 0 <= ib < nz:
                    for name, _, _ in FIELDS:
                        out[name][y * w + x] = getattr(self, name)[ib * nx + ia]
                    continue
                page = self.pages.get((ga >> 4, gb >> 4)) if self.max_tiles else None
                if page is not None:
                    for name, _, _ in FIELDS:
                        out[name][y * w + x] = page[name][tile_index(ga, gb)]
        return out

    def region(self, ga0, gb0, w, h):
        """dict of [h, w] arrays over the box of global cells: the planes of planes() and of local_planes()"""
        r = self._region_records(ga0, gb0, w, h)
        fin = R.finalise(self.P, r["count"], r["over"], r["kmin"], r["kmax"], r["hsum"], r["vsum"])
        out = dict(zip(R.PLANES, [a.reshape(h, w) for a in (r["count"], r["over"]) + tuple(fin)]))
        out["passed"] = r["passed"].reshape(h, w)
        out["state"] = (out["cls"] | np.where(out["passed"] >= self.P.min_points, LR.SEEN, 0)).astype(np.uint8)
        return out

    def render_region(self, ga0, gb0, w, h, mode=3):
        """[h, w, 3] uint8, row 0 = gb0 + h - 1: render(mode) for 0..2, render_local() for 3"""
        pl = self.region(ga0, gb0, w, h)
        rgb = R.colours(self.P, R.M_CLASS if mode == 3 else mode, pl["count"], pl["hmax"], pl["intensity"], pl["cls"])
        if mode == 3:
            seen_unknown = ((pl["cls"] & 3) == R.UNKNOWN) & ((pl["state"] & LR.SEEN) != 0)
            rgb[seen_unknown] = LR.SEEN_COLOUR
            rgb[..., 2] = np.where(seen_unknown & ((pl["cls"] & R.OVERHANG) != 0), 255, rgb[..., 2])
        return rgb[::-1].copy()

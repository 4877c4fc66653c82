"""The traversability layer of the ground grid (stereo-vision_amd/csrc/grid_core.h, "TRAVERSABILITY"; include/svh_grid.h)
restated in numpy on top of tests/grid_local_ref.py: the steep stencil with a loop over the eight neighbours, the lethal
mask, DIST2 as a BRUTE-FORCE minimum over all lethal cells of the window -- not the separable form of the header and the
kernels, so that it shares nothing with their method --, the cost table in float64, the unknown rule and the colours.
tests/test_grid_trav.py pins it by hand and compares the header with it; tests/test_grid_trav_gpu.py compares the device
with it, bit for bit."""
import numpy as np

import grid_local_ref as LR
import grid_ref as R

F = R.F
STEEP, LETHAL = 1, 2
L_OBSTACLE, L_DROP, L_STEEP, L_UNSEEN, L_UNKNOWN_SEEN = 1, 2, 4, 8, 16
L_ALL = 31
FAR = 0x7FFFFFFF
MAX_REACH = 256
SQRT2 = F(1.41421354)


class TravParams:
    """svh_grid_trav_params"""

    def __init__(self, max_slope=0.35, inscribed=0.4, inflate=1.5, lethal=L_OBSTACLE | L_DROP | L_STEEP):
        self.max_slope, self.inscribed, self.inflate, self.lethal = F(max_slope), F(inscribed), F(inflate), int(lethal)

    def ok(self):
        return bool(np.isfinite(self.max_slope) and self.max_slope > 0 and np.isfinite(self.inscribed) and self.inscribed >= 0
                    and np.isfinite(self.inflate) and self.inflate > self.inscribed and (self.lethal & ~L_ALL) == 0)


def reach_of(T, cell):
    """(int)ceil((double)inflate / (double)cell), or None where the parameters or the reach are out of range"""
    if not T.ok():
        return None
    with np.errstate(all="ignore"):
        r = np.ceil(np.float64(T.inflate) / np.float64(F(cell)))
    return int(r) if 1 <= r <= MAX_REACH else None


def rises(T, cell):
    with np.errstate(all="ignore"):
        rise4 = F(T.max_slope * F(cell))
        return rise4, F(rise4 * SQRT2)


def flags(T, cell, cls, hmean, state):
    """uint8 [nz, nx]: bit 0 steep, bit 1 lethal"""
    cls, hmean, state = np.asarray(cls, np.uint8), np.asarray(hmean, F), np.asarray(state, np.uint8)
    nz, nx = cls.shape
    rise4, rise8 = rises(T, cell)
    c = cls & 3
    free = c == R.FREE
    steep = np.zeros((nz, nx), bool)
    for db in (-1, 0, 1):
        for da in (-1, 0, 1):
            if da == 0 and db == 0:
                continue
            rise = rise8 if da != 0 and db != 0 else rise4
            for ib in range(max(0, -db), min(nz, nz - db)):          # the neighbour (ia + da, ib + db) is inside the window
                a0, a1 = max(0, -da), min(nx, nx - da)
                if a0 >= a1:
                    continue
                both = free[ib, a0:a1] & free[ib + db, a0 + da:a1 + da]
                with np.errstate(invalid="ignore"):
                    diff = np.abs(hmean[ib, a0:a1] - hmean[ib + db, a0 + da:a1 + da])
                assert diff.dtype == F
                steep[ib, a0:a1] |= both & (diff > rise)
    seen = (state & LR.SEEN) != 0
    is_ = (np.where(c == R.OBSTACLE, L_OBSTACLE, 0) | np.where(c == R.DROP, L_DROP, 0) | np.where(steep, L_STEEP, 0)
           | np.where((c == R.UNKNOWN) & ~seen, L_UNSEEN, 0) | np.where((c == R.UNKNOWN) & seen, L_UNKNOWN_SEEN, 0))
    lethal = (is_ & T.lethal) != 0
    return (np.where(steep, STEEP, 0) | np.where(lethal, LETHAL, 0)).astype(np.uint8)


def dist2(lethal, reach):
    """int32 [nz, nx]: the least (ia - ja)^2 + (ib - jb)^2 over ALL lethal cells (ja, jb), FAR where that exceeds reach^2"""
    lethal = np.asarray(lethal, bool)
    out = np.full(lethal.shape, FAR, np.int64)
    out[lethal] = 0
    lb, la = (v.astype(np.int32) for v in np.nonzero(lethal))   # a squared distance is below 2^27
    tb, ta = (v.astype(np.int32) for v in np.nonzero(~lethal))
    if len(la) and len(ta):
        step = max(1, (1 << 22) // len(la))
        best = np.empty(len(ta), np.int32)
        for at in range(0, len(ta), step):
            a, b = ta[at:at + step, None], tb[at:at + step, None]
            best[at:at + step] = ((a - la[None, :]) ** 2 + (b - lb[None, :]) ** 2).min(axis=1)
        out[tb, ta] = np.where(best <= reach * reach, best, FAR)
    return out.astype(np.int32)


def cost_table(T, cell):
    """uint8 [reach^2 + 1], float64 in the order of cost_of"""
    reach = reach_of(T, cell)
    d2 = np.arange(reach * reach + 1, dtype=np.int64)
    d = np.sqrt(d2.astype(np.float64)) * np.float64(F(cell))
    ins, inf = np.float64(T.inscribed), np.float64(T.inflate)
    ramp = 1 + np.floor(251.0 * (inf - d) / (inf - ins)).astype(np.int64)
    t = np.where(d2 == 0, 254, np.where(d <= ins, 253, np.where(d < inf, ramp, 0)))
    assert t.min() >= 0 and t.max() <= 254
    return t.astype(np.uint8)


def cost(T, cell, cls, fl, d2):
    table = cost_table(T, cell)
    far = d2 == FAR
    c = np.where(far, 0, table[np.where(far, 0, d2)]).astype(np.uint8)
    unknown = (np.asarray(cls, np.uint8) & 3) == R.UNKNOWN
    return np.where(unknown & ((fl & LETHAL) == 0) & (c == 0), 255, c).astype(np.uint8)


def colours(cost_, fl):
    """[..., 3] uint8 in cell order (no row flip)"""
    c = cost_.astype(np.int64)
    rgb = np.stack([c, np.zeros_like(c), 255 - c], -1)
    rgb[c == 254] = (255, 0, 0)
    rgb[c == 253] = (255, 128, 0)
    rgb[c == 0] = (0, 96, 0)
    rgb[c == 255] = (32, 32, 32)
    rgb[..., 1] = np.where(fl & STEEP, 255, rgb[..., 1])
    return rgb.astype(np.uint8)


def layer(T, cell, cls, hmean, state):
    """dict: flags, dist2, cost [nz, nx] and rgb [nz, nx, 3] in cell order"""
    fl = flags(T, cell, cls, hmean, state)
    d2 = dist2((fl & LETHAL) != 0, reach_of(T, cell))
    c = cost(T, cell, cls, fl, d2)
    return dict(flags=fl, dist2=d2, cost=c, rgb=colours(c, fl))


class Grid(LR.Grid):
    """grid_local_ref.Grid with the traversability layer on its finished planes"""

    def __init__(self, P, T=None):
        super().__init__(P)
        self.T = T if T is not None else TravParams()

    def trav(self):
        pl, lo = self.planes(), self.local_planes()
        return layer(self.T, self.P.cell, pl["cls"], pl["hmean"], lo["state"])

    def render_cost(self):
        return self.trav()["rgb"][::-1].copy()


def separable(lethal, reach):
    """the header's form, for the record that the two agree (test_grid_trav.py): column sweeps capped at reach + 1, then the
    row minimum"""
    lethal = np.asarray(lethal, bool)
    nz, nx = lethal.shape
    g = np.zeros((nz, nx), np.int64)
    for sweep in (range(nz), range(nz - 1, -1, -1)):
        d = np.full(nx, reach + 1, np.int64)
        for ib in sweep:
            d = np.where(lethal[ib], 0, np.minimum(d + 1, reach + 1))
            g[ib] = d if sweep.step == 1 else np.minimum(g[ib], d)
    out = np.full((nz, nx), FAR, np.int64)
    for k in range(-reach, reach + 1):
        a0, a1 = max(0, -k), min(nx, nx - k)
        if a0 >= a1:
            continue
        cand = np.where(g[:, a0 + k:a1 + k] <= reach, k * k + g[:, a0 + k:a1 + k] ** 2, FAR)
        out[:, a0:a1] = np.minimum(out[:, a0:a1], cand)
    return np.where(out <= reach * reach, out, FAR).astype(np.int32), g


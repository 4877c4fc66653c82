"""The time layer of the ground grid (include/svh_grid_time.h, "TIME") restated in numpy and plain Python from the text of
stereo-vision_amd/csrc/grid_time_core.h on top of tests/grid_plan_ref.py, tests/grid_pred_ref.py and tests/grid_trav_ref.py: the slot
of a layer, the BLOCK planes (one boolean plane per layer, read from PRED by global cell), the released cells and RCOST by the
brute-force obstacle distance, the backward sweep over the layers with Python integers and an explicit table of steps, TDIR by the
first-minimum rule with the wait last, the walk.  It shares no code with the header's functors or the kernels.  Planes are indexed
[ib, ia], fields [t, ib, ia]."""
import numpy as np

import grid_plan_ref as PL
import grid_pred_ref as PR
import grid_trav_ref as TR

FAR = PL.FAR
DIR_GOAL, DIR_NONE, DIR_WAIT = 8, 9, 10
STEPS = PL.STEPS
FOUND, UNREACHABLE, BLOCKED, OUTSIDE = range(4)
MAX_STATES = 1 << 28


class TimeParams:
    """svh_grid_time_params"""

    def __init__(self, layers=32, wait=100, release=1):
        self.layers, self.wait, self.release = int(layers), int(wait), int(release)

    def ok(self):
        return 1 <= self.layers <= 256 and (self.wait == -1 or 1 <= self.wait <= 65535) and self.release in (0, 1)


def slot_of_layer(pp, t):
    """layer 0 is now; layer t >= 1 is at the slot of pose t - 1"""
    return 0 if t == 0 else PR.slot_of_pose(pp, t - 1)


def blocks(pp, tp, pred, shape, off=(0, 0), pred_off=(0, 0)):
    """bool [L + 1, nz, nx]: BLOCK of every window cell at the layers 0 .. L (the last one is read by nobody's own rule)"""
    nz, nx = shape
    ga, gb = np.meshgrid(np.arange(nx, dtype=np.int64) + off[0], np.arange(nz, dtype=np.int64) + off[1])
    words = PR.read(np.asarray(pred, np.uint32), pred_off, ga, gb).astype(np.uint64)
    return np.stack([((words >> np.uint64(slot_of_layer(pp, t))) & np.uint64(1)) != 0 for t in range(tp.layers + 1)])


def released(pp, ids, tracks, shape, off=(0, 0), pred_off=(0, 0)):
    """bool [nz, nx]: the window cells whose global cell lies in the ID frame and holds the id of a predicting track"""
    nz, nx = shape
    out = np.zeros((nz, nx), bool)
    if ids is None:
        return out
    tracks = np.asarray(tracks, np.int64).reshape(-1, len(PR.OR.TRACK_FIELDS))
    who = {int(t[PR.T["id"]]) for t in tracks if PR.predicts(pp, t)}
    for b in range(nz):
        for a in range(nx):
            pa, pb = a + off[0] - pred_off[0], b + off[1] - pred_off[1]
            if 0 <= pa < nx and 0 <= pb < nz and int(ids[pb, pa]) in who:
                out[b, a] = True
    return out


def static_planes(plan, pp, tp, cost, flags, goals, off=(0, 0), pred_off=(0, 0), ids=None, tracks=(), cls=None, trav=None, cell=None):
    """(rcost uint8, rpot int32, rdir uint8 [nz, nx], released cells)"""
    cost = np.asarray(cost, np.uint8)
    rel = released(pp, ids, tracks, cost.shape, off, pred_off) if tp.release else np.zeros(cost.shape, bool)
    rcost = cost
    if rel.any():
        fl = np.where(rel, np.asarray(flags, np.uint8) & ~np.uint8(TR.LETHAL), flags).astype(np.uint8)
        d2 = TR.dist2((fl & TR.LETHAL) != 0, TR.reach_of(trav, cell))
        rcost = TR.cost(trav, cell, cls, fl, d2)
    rpot, rdir, _ = PL.field(plan, rcost, goals, off[0], off[1])
    return rcost, rpot, rdir, int(rel.sum())


def field(plan, pp, tp, rcost, rpot, rdir, pred, off=(0, 0), pred_off=(0, 0)):
    """(tpot int32 [L, nz, nx], tdir uint8 [L, nz, nx], (layers, reached, blocked, waits))"""
    price = PL.prices(plan, rcost)
    nz, nx = price.shape
    L = tp.layers
    blk = blocks(pp, tp, pred, (nz, nx), off, pred_off)
    tpot = [[[FAR] * nx for _ in range(nz)] for _ in range(L)]
    tdir = np.full((L, nz, nx), DIR_NONE, np.uint8)
    for b in range(nz):
        for a in range(nx):
            if not blk[L - 1, b, a]:
                tpot[L - 1][b][a], tdir[L - 1, b, a] = int(rpot[b, a]), rdir[b, a]
    for t in range(L - 2, -1, -1):
        nxt, now, after = tpot[t + 1], blk[t], blk[t + 1]
        for b in range(nz):
            for a in range(nx):
                if price[b, a] == 0 or now[b, a]:
                    continue
                if rpot[b, a] == 0:
                    tpot[t][b][a], tdir[t, b, a] = 0, DIR_GOAL
                    continue
                best, how = None, DIR_NONE
                for d, x, y, w in PL.steps_of(price, a, b):
                    if after[y, x] or (d % 2 == 1 and (after[b, x] or after[y, a])) or nxt[y][x] == FAR:
                        continue
                    c = nxt[y][x] + w
                    if c <= plan.max_cost and (best is None or c < best):
                        best, how = c, d
                if tp.wait >= 1 and not after[b, a] and nxt[b][a] != FAR:
                    c = nxt[b][a] + tp.wait
                    if c <= plan.max_cost and (best is None or c < best):
                        best, how = c, DIR_WAIT
                if best is not None:
                    tpot[t][b][a], tdir[t, b, a] = best, how
    tpot = np.array(tpot, np.int64).astype(np.int32)
    stats = (L, int((tpot != FAR).sum()), int(((price != 0)[None] & blk[:L]).sum()), int((tdir == DIR_WAIT).sum()))
    return tpot, tdir, stats


def path(plan, pp, tp, rcost, tpot, tdir, rdir, pred, a, b, off=(0, 0), pred_off=(0, 0)):
    """(status, triples int32 [n, 3], cost) from the window cell (a, b) at layer 0"""
    price = PL.prices(plan, rcost)
    nz, nx = price.shape
    none = np.zeros((0, 3), np.int32)
    if not (0 <= a < nx and 0 <= b < nz):
        return OUTSIDE, none, FAR
    cost = int(tpot[0, b, a])
    if price[b, a] == 0 or blocks(pp, tp, pred, (nz, nx), off, pred_off)[0, b, a]:
        return BLOCKED, none, cost
    if cost == FAR:
        return UNREACHABLE, none, cost
    L, t, out = tp.layers, 0, []
    while len(out) < L + nx * nz:
        d = int(tdir[t, b, a]) if t < L - 1 else int(rdir[b, a])
        if d == DIR_NONE or d > DIR_WAIT:
            break
        out.append((off[0] + a, off[1] + b, t))
        if d == DIR_GOAL:
            return FOUND, np.array(out, np.int32).reshape(-1, 3), cost
        if d != DIR_WAIT:
            a, b = a + STEPS[d][0], b + STEPS[d][1]
        t = min(t + 1, L - 1)
    return UNREACHABLE, none, cost


def path_cost(plan, tp, rcost, triples, off=(0, 0)):
    """the sum of the weights along a path's triples: a wait where the cell repeats below layer L - 1, else the step's weight"""
    price = PL.prices(plan, rcost)
    total = 0
    for (ga, gb, t), (ha, hb, _) in zip(triples[:-1], triples[1:]):
        a, b, x, y = int(ga) - off[0], int(gb) - off[1], int(ha) - off[0], int(hb) - off[1]
        if (a, b) == (x, y):
            total += tp.wait
        else:
            total += (7 if (a != x and b != y) else 5) * (int(price[b, a]) + int(price[y, x]))
    return total


def overlay(img, pp, tp, rcost, pred, goals, triples, t, plan, off=(0, 0), pred_off=(0, 0)):
    """on an image in cell order (no row flip): the cells blocked at layer t, the goals that count, the path's cells"""
    price = PL.prices(plan, rcost)
    nz, nx = price.shape
    out = img.copy()
    s = slot_of_layer(pp, t)
    out[blocks(pp, tp, pred, (nz, nx), off, pred_off)[t]] = (255, 8 * s, 255 - 8 * s)
    return PL.overlay(out, price, goals, np.asarray(triples, np.int64).reshape(-1, 3)[:, :2], off[0], off[1])

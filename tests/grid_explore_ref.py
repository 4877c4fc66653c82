"""The exploration layer of the ground grid (include/svh_grid.h, "EXPLORATION") restated in numpy and plain Python from the text
of stereo-vision_amd/csrc/grid_explore_core.h: the rays of a viewpoint, its VIEW plane and GAIN, the REACH field through
tests/grid_plan_ref.py with the start as the only goal, the records, the scores and the best.  The rays are advanced all at
once, step k for the 8 R of them, with numpy's floor division: the restatement shares no code with the header's loop over
single rays.  Planes are indexed [ib, ia]; a cell is (a, b) = (ia, ib)."""
import numpy as np

import grid_front_ref as FR
import grid_plan_ref as PR

OBSTACLE = 2
NONE, VISITED, COUNTED = 0, 1, 2
FAR = PR.FAR
INFEASIBLE = 2 ** 63 - 1
MAX_RECORDS = 65536
FIELDS = ("label", "rep_ga", "rep_gb", "gain", "reach")
VIEW_COLOUR, VIEWPOINT_COLOUR = (255, 0, 255), (255, 255, 255)


class ExploreParams:
    def __init__(self, range=10.0, min_gain=1, w_gain=500, w_reach=1):
        self.range, self.min_gain, self.w_gain, self.w_reach = np.float32(range), int(min_gain), int(w_gain), int(w_reach)

    def ok(self):
        return bool(np.isfinite(self.range) and self.range > 0 and 0 <= self.min_gain <= 2 ** 26 and 0 <= self.w_gain <= 65535 and
                    0 <= self.w_reach <= 65535)


def range_cells(range_, cell):
    """R, or 0 when it is outside 1..128: floorf of the fp32 quotient"""
    with np.errstate(all="ignore"):
        q = np.floor(np.float32(range_) / np.float32(cell))
    return int(q) if 1 <= q <= 128 else 0


def ray_ends(R):
    """int64 [8 R, 2]: the offsets (dx, dz) on the perimeter of [-R, R]^2, in the order of the ray index"""
    t = np.arange(2 * R)
    full = np.full(2 * R, R)
    return np.concatenate([np.stack([-R + t, -full], 1), np.stack([full, -R + t], 1), np.stack([R - t, full], 1), np.stack([-full, R - t], 1)]).astype(np.int64)


def view(front, R, state, va, vb):
    """(VIEW uint8 [nz, nx], GAIN) of the window viewpoint (va, vb), which is inside the window"""
    state = np.asarray(state, np.uint8)
    nz, nx = state.shape
    ends = ray_ends(R)
    alive = np.ones(len(ends), bool)
    visited = np.zeros((nz, nx), bool)
    for k in range(1, R + 1):
        sx, sz = (2 * k * ends[:, 0] + R) // (2 * R), (2 * k * ends[:, 1] + R) // (2 * R)     # floor division: rdiv
        a, b = va + sx, vb + sz
        alive &= (sx * sx + sz * sz <= R * R) & (a >= 0) & (a < nx) & (b >= 0) & (b < nz)
        alive[alive] = (state[b[alive], a[alive]] & 3) != OBSTACLE
        if not alive.any():
            break
        visited[b[alive], a[alive]] = True
    out = np.where(visited, np.where(FR.unexplored(front, state), COUNTED, VISITED), NONE).astype(np.uint8)
    return out, int((out == COUNTED).sum())


def gains(front, R, state, cells, oa=0, ob=0):
    """int32 [n]: GAIN of global cells, -1 outside the window"""
    state = np.asarray(state, np.uint8)
    nz, nx = state.shape
    out, known = [], {}
    for ga, gb in np.asarray(cells, np.int64).reshape(-1, 2):
        a, b = int(ga) - oa, int(gb) - ob
        if not (0 <= a < nx and 0 <= b < nz):
            out.append(-1)
            continue
        if (a, b) not in known:
            known[(a, b)] = view(front, R, state, a, b)[1]
        out.append(known[(a, b)])
    return np.array(out, np.int32).reshape(-1)


def score(p, gain, reach):
    if reach == FAR or gain < p.min_gain:
        return INFEASIBLE
    return p.w_reach * int(reach) - p.w_gain * int(gain)


def rank(front, plan, p, R, state, cost, start, oa=0, ob=0, front_recs=None, pot=None):
    """(records int32 [n, 5], scores int64 [n], best, feasible) from the global cell `start`; the frontier table and the reach field
    may be handed in"""
    if front_recs is None:
        front_recs = FR.frontiers(front, state, cost, oa, ob)[2]
    if pot is None:
        pot = PR.field(plan, cost, [start], oa, ob)[0]
    front_recs = front_recs[:MAX_RECORDS]
    g = gains(front, R, state, front_recs[:, 8:10], oa, ob)
    recs, scores = [], []
    for k, r in enumerate(front_recs):
        reach = int(pot[r[9] - ob, r[8] - oa])
        recs.append([int(r[0]), int(r[8]), int(r[9]), int(g[k]), reach])
        scores.append(score(p, int(g[k]), reach))
    feasible = [k for k, s in enumerate(scores) if s != INFEASIBLE]
    best = min(feasible, key=lambda k: (scores[k], k)) if feasible else -1
    return np.array(recs, np.int32).reshape(-1, 5), np.array(scores, np.int64).reshape(-1), best, len(feasible)


def overlay(img, mask, va, vb):
    """a VIEW plane and its viewpoint over an image [nz, nx, 3] whose row 0 is ib = nz - 1"""
    out = np.array(img, np.uint8)
    m = np.asarray(mask, np.uint8)[::-1]
    nz = m.shape[0]
    seen = m == VISITED
    out[seen] = (out[seen].astype(np.int64) + (255 - out[seen].astype(np.int64)) // 2).astype(np.uint8)
    out[m == COUNTED] = VIEW_COLOUR
    out[nz - 1 - vb, va] = VIEWPOINT_COLOUR
    return out

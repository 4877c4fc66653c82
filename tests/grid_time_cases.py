"""Scenes for the tests of the ground grid's time layer (tests/test_grid_time.py, tests/test_grid_time_gpu.py): planes made by hand
and at random, and one function that runs a case through tests/grid_time_ref.py and through a test entry of the library
(svh_test_grid_time or svh_test_grid_time_device) and compares every byte."""
import numpy as np

import grid_obj_ref as OR
import grid_plan_ref as PL
import grid_pred_ref as PR
import grid_time_ref as TM
import grid_trav_ref as TR

FREE, OBSTACLE = 1, 2          # CLASS
CELL = 0.5
TRAV = dict(max_slope=0.35, inscribed=0.4, inflate=1.5)   # reach 3 on cells of 0.5


def track(id_, moving=True, label=0, v16=(0, 0)):
    """one track record: an id, the MOVING flag, a label (-1: missed), a velocity in sixteenths of a cell per step"""
    t = np.zeros(len(OR.TRACK_FIELDS), np.int32)
    t[OR.T["id"]], t[OR.T["flags"]], t[OR.T["label"]] = id_, OR.MOVING if moving else 0, label
    t[OR.T["v16_a"]], t[OR.T["v16_b"]] = v16
    return t


def word(layers, pp):
    """the PRED word with the slots of the given layers set"""
    w = 0
    for t in layers:
        w |= 1 << TM.slot_of_layer(pp, t)
    return w


def random_cost(rng, nx, nz, lethal=0.08):
    c = rng.integers(0, 253, (nz, nx)).astype(np.uint8)
    c[rng.random((nz, nx)) < 0.6] = 0
    c[rng.random((nz, nx)) < 0.03] = 255
    c[rng.random((nz, nx)) < lethal] = rng.choice(np.array([253, 254], np.uint8))
    return c


def random_pred(rng, nx, nz, slots, share=0.15):
    """random words below 2^slots on a share of the cells; bit slots - 1 is set somewhere"""
    w = rng.integers(0, 1 << slots, (nz, nx), dtype=np.uint64).astype(np.uint32)
    w[rng.random((nz, nx)) >= share] = 0
    w[rng.integers(0, nz), rng.integers(0, nx)] |= np.uint32(1 << (slots - 1))
    return w


class Case:
    """everything a test entry takes; the planes of release = 1 are optional"""

    def __init__(self, cost, goals, pred=None, plan=None, pp=None, tp=None, off=(0, 0), pred_off=None, flags=None, cls=None, ids=None, tracks=(),
                 trav=None, cell=CELL, start=None):
        self.cost = np.ascontiguousarray(cost, np.uint8)
        self.goals = np.asarray(goals, np.int32).reshape(-1, 2)
        self.pred = np.zeros(self.cost.shape, np.uint32) if pred is None else np.ascontiguousarray(pred, np.uint32)
        self.plan, self.pp, self.tp = plan or {}, pp or {}, tp or {}
        self.off, self.pred_off = off, off if pred_off is None else pred_off
        self.flags = np.zeros(self.cost.shape, np.uint8) if flags is None else np.ascontiguousarray(flags, np.uint8)
        self.cls, self.ids = cls, ids
        self.tracks = np.asarray(tracks, np.int32).reshape(-1, len(OR.TRACK_FIELDS))
        self.trav, self.cell, self.start = trav, cell, start


def want(c):
    """the restatement's answer: a dict as svhip.grid.core_time returns (the rounds of RPOT are left out of the statistics)"""
    plan, pp, tp = PL.PlanParams(**c.plan), PR.PredParams(**c.pp), TM.TimeParams(**c.tp)
    trav = TR.TravParams(**c.trav) if c.trav is not None else None
    rcost, rpot, rdir, rel = TM.static_planes(plan, pp, tp, c.cost, c.flags, c.goals, c.off, c.pred_off, c.ids, c.tracks, c.cls, trav, c.cell)
    tpot, tdir, st = TM.field(plan, pp, tp, rcost, rpot, rdir, c.pred, c.off, c.pred_off)
    out = dict(rcost=rcost, rpot=rpot, rdir=rdir, tpot=tpot, tdir=tdir, stats=st + (rel,))
    if c.start is not None:
        status, triples, cost = TM.path(plan, pp, tp, rcost, tpot, tdir, rdir, c.pred, c.start[0], c.start[1], c.off, c.pred_off)
        out.update(status=status, path=triples, cost=cost, path_len=len(triples))
    return out


def got(G, entry, c, cap=None):
    """the library's answer through `entry`: G.core_time or G.device_time"""
    trav = G.default_trav(**c.trav) if c.trav is not None else None
    return entry(G.default_plan(**c.plan), G.default_pred(**c.pp), G.default_time(**c.tp), c.cost, c.flags, c.goals, c.pred, c.off[0], c.off[1], c.pred_off,
                 c.ids, c.tracks if len(c.tracks) else None, c.cls, trav, c.cell, c.start, cap)


def agree(G, entry, c, tag=""):
    """both on the same case, byte for byte; returns the restatement's answer"""
    w, g = want(c), got(G, entry, c)
    for name in ("rcost", "rpot", "rdir", "tpot", "tdir"):
        assert g[name].dtype == w[name].dtype and g[name].shape == w[name].shape, (tag, name, g[name].dtype, w[name].dtype)
        assert np.array_equal(g[name], w[name]), (tag, name, np.argwhere(g[name] != w[name])[:4])
    assert g["stats"][:5] == w["stats"], (tag, g["stats"], w["stats"])
    if c.start is not None:
        assert (g["status"], g["cost"], g["path_len"]) == (w["status"], w["cost"], w["path_len"]), (tag, g["status"], g["cost"], g["path_len"], w["status"], w["cost"], w["path_len"])
        assert np.array_equal(g["path"], w["path"]), (tag, g["path"][:6], w["path"][:6])
    return w


def random_case(seed, nx, nz, L, slots=8, wait=100, release=0, stride=1, pps=1, share=0.15, off=None, pred_off=None, with_tracks=False, **plan):
    """a random window with random PRED words, goals inside and outside, a start; with_tracks: random lethal objects with ids, some of
    them predicting, and the planes release = 1 needs"""
    rng = np.random.default_rng(seed)
    off = (int(rng.integers(-40, 40)), int(rng.integers(-40, 40))) if off is None else off
    pred_off = (off[0] + int(rng.integers(-3, 4)), off[1] + int(rng.integers(-3, 4))) if pred_off is None else pred_off
    cost = random_cost(rng, nx, nz)
    goals = np.stack([rng.integers(-2, nx + 2, 4) + off[0], rng.integers(-2, nz + 2, 4) + off[1]], 1).astype(np.int32)
    kw = dict(cost=cost, goals=goals, pred=random_pred(rng, nx, nz, slots, share), plan=plan, pp=dict(slots=slots, stride=stride, poses_per_step=pps),
              tp=dict(layers=L, wait=wait, release=release), off=off, pred_off=pred_off)
    if with_tracks:
        cls = np.where(rng.random((nz, nx)) < 0.1, 0, FREE).astype(np.uint8)      # some cells unknown
        flags = np.where(rng.random((nz, nx)) < 0.06, TR.LETHAL, 0).astype(np.uint8)
        ids = np.full((nz, nx), -1, np.int32)
        tracks = [track(3, True), track(5, False), track(9, True, label=-1), track(12, True)]
        for t in tracks:                                                          # a blob per track in the ID frame, lethal in the window
            a, b = int(rng.integers(0, nx)), int(rng.integers(0, nz))
            ids[max(0, b - 1):b + 1, max(0, a - 1):a + 1] = t[0]
        ids[rng.integers(0, nz), rng.integers(0, nx)] = 7                         # an id that is in no record
        wa, wb = np.meshgrid(np.arange(nx) + off[0] - pred_off[0], np.arange(nz) + off[1] - pred_off[1])
        inside = (wa >= 0) & (wa < nx) & (wb >= 0) & (wb < nz)
        held = np.where(inside, ids[np.clip(wb, 0, nz - 1), np.clip(wa, 0, nx - 1)], -1) >= 0
        flags[held] |= TR.LETHAL
        cls[held] = OBSTACLE
        trav = TR.TravParams(**TRAV)
        d2 = TR.dist2((flags & TR.LETHAL) != 0, TR.reach_of(trav, CELL))
        kw.update(cost=TR.cost(trav, CELL, cls, flags, d2), flags=flags, cls=cls, ids=ids, tracks=np.array(tracks), trav=TRAV)
        kw["pp"]["only_moving"] = int(rng.integers(0, 2))
    free = np.argwhere(kw["cost"] <= 252)                                         # a goal and the start on cells that are passable
    if len(free):
        goals[0] = (free[len(free) // 2][1] + off[0], free[len(free) // 2][0] + off[1])
    kw["start"] = (int(free[0][1]), int(free[0][0])) if len(free) else (0, 0)
    return Case(**kw)


# ---- an object of the library against the header on the object's own planes ------------------------------------------------------
def object_case(G, g, goals, start=None):
    """the Case that the header is to be given for the object as it stands: its own COST, FLAGS, CLASS, track table, ID plane and PRED"""
    ids, poff = g.track_plane()
    pred, poff2 = g.pred_plane()
    assert poff == poff2
    return Case(g.trav_plane(G.TRAV_COST), goals, pred, g.plan_params().asdict(), g.get_predict().asdict(), g.time_params().asdict(), g.window(), poff,
                g.trav_plane(G.TRAV_FLAGS), g.classes(), ids, g.tracks(), g.traversability()[0].asdict(), g.params.cell, start)


def check_object(G, g, goals, start_xyz, tag="", image_layers=()):
    """TPOT, TDIR, RCOST, RPOT, the statistics, the path with its status and cost and the image of the object against the header
    (svh_test_grid_time) on the object's own planes; returns (the header's answer, the case)"""
    (oa, ob), (ga, gb) = g.window(), g.cell_of(start_xyz)
    c = object_case(G, g, goals, (ga - oa, gb - ob))
    w = got(G, G.core_time, c)
    for which, name in ((G.TIME_TPOT, "tpot"), (G.TIME_TDIR, "tdir"), (G.TIME_RCOST, "rcost"), (G.TIME_RPOT, "rpot")):
        plane = g.time_plane(which)
        assert plane.dtype == w[name].dtype and np.array_equal(plane, w[name]), (tag, name, np.argwhere(plane != w[name])[:4])
    L = c.tp["layers"]
    if L > 2:
        assert np.array_equal(g.time_plane(G.TIME_TDIR, 1, L - 2), w["tdir"][1:L - 1]), (tag, "layers 1 .. L - 2")
    assert g.time_stats()[:5] == w["stats"][:5], (tag, g.time_stats(), w["stats"])
    status, triples, cost = g.time_path(start_xyz)
    assert (status, cost, g.time_path_len) == (w["status"], w["cost"], w["path_len"]), (tag, status, cost, w["status"], w["cost"])
    assert np.array_equal(triples, w["path"]), (tag, triples[:6], w["path"][:6])
    plan, pp, tp = PL.PlanParams(**c.plan), PR.PredParams(**c.pp), TM.TimeParams(**c.tp)
    for t in image_layers:
        want_img = TM.overlay(TR.colours(w["rcost"], c.flags), pp, tp, w["rcost"], c.pred, c.goals, triples, t, plan, c.off, c.pred_off)[::-1]
        assert np.array_equal(g.render_time(t, triples), want_img), (tag, "image", t)
    return w, c

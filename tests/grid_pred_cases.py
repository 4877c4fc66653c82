"""What tests/test_grid_pred_gpu.py and tests/test_grid_pred_cache_gpu.py share: a Grid object with objects, a vehicle and a prediction
set; frames of tests/grid_obj_cases.py played on it, a step each; and the comparisons of the device with the restatement
(tests/grid_pred_ref.py), which is given the device's own track table, ID plane, COST and POT -- so that a comparison here tests the
prediction and nothing before it.  Every comparison is of bytes."""
import numpy as np

import grid_obj_cases as OC
import grid_pred_ref as PR
import grid_roll_ref as RR

CELL = OC.CELL
OBJ_KW = dict(min_size=1, min_height=0.0, min_age=0, move_cells=1, gate=0, max_missed=0)
ROLL_KW = dict(unknown_cost=0, w_pot=0, w_cost=1, w_cut=10)        # unknown ground is free and no field is needed: the scenes are bare


def centre(ga, gb):
    """the map-frame position of the middle of a global cell (tests/grid_obj_cases.py: a = x, b = z, x0 = z0 = 0)"""
    return ((ga + 0.5) * CELL, 1.5, (gb + 0.5) * CELL)


def new_grid(G, nx, nz, obj=None, roll=None, pred=None):
    g = G.Grid(G.default_params(**OC.grid_kw(nx, nz)))
    g.set_objects(G.default_obj(**dict(OBJ_KW, **(obj or {}))))
    g.set_roll(G.default_roll(**dict(ROLL_KW, **(roll or {}))))
    if pred is not None:
        g.set_predict(G.default_pred(**pred))
    return g


def play(g, frames):
    """the grid rebuilt per frame, a step each, as tests/grid_obj_cases.run_device does"""
    for f in frames:
        g.clear()
        oa, ob = g.window()
        g.scroll(f.off[0] - oa, f.off[1] - ob)
        pts = OC.frame_points(f)
        if len(pts):
            g.add_points(pts)
        g.objects_step()


def moving_block(nx, nz, a0, b0, w, h, va, vb, steps=3, off=(0, 0)):
    """a block that moves (va, vb) cells per step; the part that leaves the window is cut off"""
    frames = []
    for k in range(steps):
        f = OC.Frame(nx, nz, off=off)
        for ib in range(b0 + k * vb, b0 + k * vb + h):
            for ia in range(a0 + k * va, a0 + k * va + w):
                if 0 <= ia < nx and 0 <= ib < nz:
                    f.put(ia, ib)
        frames.append(f)
    return frames


def merged(*histories):
    """several histories of equal length in one window"""
    out = []
    for fs in zip(*histories):
        f = OC.Frame(fs[0].state.shape[1], fs[0].state.shape[0], off=fs[0].off)
        for g in fs:
            m = g.state == 2
            f.state[m], f.hmax[m], f.count[m] = g.state[m], g.hmax[m], g.count[m]
        out.append(f)
    return out


def pred_params(g):
    return PR.PredParams(**g.get_predict().asdict())


def restated(g):
    """(PRED, its four statistics, the frame's offsets) by the restatement from the track state the object reports"""
    ids, off = g.track_plane()
    tracks = g.tracks()
    p = pred_params(g)
    stepped = g.track_stats()[0] > 0
    plane, stats = PR.plane(p, ids if stepped else None, tracks, ids.shape)
    return plane, stats + (PR.launches(p, len(tracks) if stepped else 0),), off


def check_pred(g, tag=""):
    want, wstats, woff = restated(g)
    got, off = g.pred_plane()
    assert got.dtype == np.uint32 and off == woff, (tag, off, woff)
    assert np.array_equal(got, want), (tag, "PRED", np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])
    assert g.pred_stats() == wstats, (tag, g.pred_stats(), wstats)
    return want, wstats, off


def roll_of(g):
    p = RR.RollParams(**g.roll_params()[0].asdict())
    return p, RR.table(p, g.params.cell)[1]


def check_score(G, g, tab, xyz, set_=0, tag="", image=True):
    """PRED, the footprint masks of the set's poses, best, records, scores and the image against the restatement on the object's own
    planes; returns (best, recs, scores)"""
    pred, _, poff = check_pred(g, tag)
    rp, lists = roll_of(g)
    cost = g.trav_plane(G.TRAV_COST)
    pot = g.plan_plane(G.PLAN_POT) if rp.w_pot else None
    (oa, ob), anchor = g.window(), g.cell_of(xyz)
    recs, scores, best = PR.score(rp, pred_params(g), lists, cost, pot, pred, poff, tab[set_], anchor, oa, ob)
    got = g.roll_score_pred(xyz, set_)
    assert got[0] == best, (tag, got[0], best)
    assert got[1].dtype == np.int32 and np.array_equal(got[1], recs), (tag, "records", got[1][(got[1] != recs).any(1)][:4], recs[(got[1] != recs).any(1)][:4])
    assert got[2].dtype == np.int64 and np.array_equal(got[2], scores), (tag, "scores")
    live = tab[set_][tab[set_][:, :, 2] >= 0]
    if len(live):
        poses = (live + np.array([anchor[0], anchor[1], 0])).astype(np.int32)[:2000]
        assert np.array_equal(g.footprint_pred(poses), PR.footprint_masks(lists, pred, poff, poses)), (tag, "footprint masks")
    if image:
        for mode in (G.RENDER_CLASS, G.RENDER_HEIGHT):
            assert np.array_equal(g.render_pred(mode), PR.overlay(g.render(mode), pred, poff, (oa, ob))), (tag, "image", mode)
    return best, recs, scores

"""The tables behind tests/test_grid_pred_cache.py and tests/test_grid_pred_cache_gpu.py: the outputs of the prediction
(include/svh_grid_pred.h) that pass through the engine's cache (READERS), every mutator of tests/grid_cache_cases.py and
tests/grid_obj_cache_cases.py with the layer's own (MUTATORS), and what the header says each does to each, written from the header's
text: PRED and its statistics are a function of the track state and the prediction parameters and of nothing else; they are dropped
by svh_grid_objects_step, svh_grid_objects_reset, svh_grid_set_objects, svh_grid_set_window and svh_grid_set_predict.

A scored record reads PRED and, beside it, what svh_grid_roll_score reads -- COST, POT, the vehicle, the candidates.  It is compared
with the restatement after every mutator; it is byte-equal to what it was where neither PRED is dropped nor the roll layer's own
table (tests/grid_cache_cases.py, reader "roll_score") says that a scoring changes.

The scene is that of tests/grid_obj_cache_cases.py (the composed restatement, the object parameters, two steps) with the prediction
parameters PRED_KW set: its objects stand, so only_moving is 0."""
import numpy as np

import grid_all_ref as ALL
import grid_cache_cases as CC
import grid_local_ref as LR
import grid_obj_cache_cases as OCC
import grid_pred_ref as PR

CHANGES, KEEPS = CC.CHANGES, CC.KEEPS
PRED_KW = dict(slots=6, stride=2, poses_per_step=1, margin=1, grow16=8, only_moving=0)
OTHER_KW = dict(PRED_KW, margin=0, grow16=0)                       # the skipped form
B = OCC.B


# ---- the restatement's side ------------------------------------------------------------------------------------------------------
def ref_pred(ref):
    """(PRED, the four statistics, the frame's offsets) of the composed restatement with its tracker"""
    nz, nx = ref.state().shape
    stepped = ref.trk.ids is not None
    plane, stats = PR.plane(ref.pred, ref.trk.ids, ref.trk.tracks if stepped else [], (nz, nx))
    off = tuple(ref.trk.off) if stepped else (ref.oa, ref.ob)
    return plane, stats + (PR.launches(ref.pred, len(ref.trk.tracks) if stepped else 0),), off


def ref_score(ref):
    if ref.cands is None:
        raise ALL.Refused("no candidates")
    plane, _, off = ref_pred(ref)
    anchor = LR.cell_of(ref.P, CC.ANCHOR)
    pot = ref.field()["pot"] if ref.roll.w_pot != 0 else None
    recs, scores, best = PR.score(ref.roll, ref.pred, ref.roll_lists(), ref.cost(), pot, plane, off, ref.cands[0], anchor, ref.oa, ref.ob)
    return B(recs, scores, np.array([best]))


def dev_score(g):
    best, recs, scores = g.roll_score_pred(CC.ANCHOR, 0)
    return B(recs, scores, np.array([best]))


def dev_plane(g):
    plane, off = g.pred_plane()
    return B(plane, np.array(off))


# ---- readers: name -> (group, device form, restated form) --------------------------------------------------------------------------
READERS = {
    "pred_plane": ("pred", dev_plane, lambda ref: B(ref_pred(ref)[0], np.array(ref_pred(ref)[2]))),
    "pred_stats": ("pred", lambda g: CC.ints(*g.pred_stats()), lambda ref: CC.ints(*ref_pred(ref)[1])),
    "pred_score": ("score", dev_score, ref_score),
}
CACHED = [n for n, r in READERS.items() if r[0] == "pred"]


# ---- the layer's own mutator -------------------------------------------------------------------------------------------------------
def set_predict(g, ref, rng):
    if g is not None:
        g.set_predict(g.G.default_pred(**OTHER_KW))
    if ref is not None:
        ref.pred = PR.PredParams(**OTHER_KW)


OWN = {"set_predict": set_predict}
MUTATORS = dict(OCC.MUTATORS, **OWN)
DROPS = ["set_window", "set_objects", "objects_step", "objects_reset", "set_predict"]      # what the header names, in the order of MUTATORS
# mutator -> the groups whose readers CHANGE (or are refused); every other reader KEEPS
RULES = {m: (({"pred", "score"} if m in DROPS else set()) | ({"score"} if m in CC.EXPECT and CC.EXPECT[m]["roll_score"] != KEEPS else set()))
         for m in MUTATORS}
EXPECT = {m: {n: (CHANGES if r[0] in RULES[m] else KEEPS) for n, r in READERS.items()} for m in MUTATORS}
# CHANGES pairs that the scene cannot show, each with its reason
UNSHOWN = {
    ("objects_step", "pred_plane"): "a step on a scene that has not changed leaves the ids and, the objects standing, the velocities: PRED is computed again to the same bytes",
    ("objects_step", "pred_stats"): "as pred_plane",
    ("objects_step", "pred_score"): "as pred_plane",
}


def served_from_cache(m, n):
    return READERS[n][0] == "pred" and m not in DROPS


def scene(g, ref):
    OCC.scene(g, ref)
    if g is not None:
        g.set_predict(g.G.default_pred(**PRED_KW))
    if ref is not None:
        ref.pred = PR.PredParams(**PRED_KW)


def read_ref(ref):
    out = {}
    with ref.frozen():
        for n, r in READERS.items():
            try:
                out[n] = r[2](ref)
            except ALL.Refused:
                out[n] = CC.REFUSED
    return out


def read_dev(g):
    out = {}
    for n, r in READERS.items():
        try:
            out[n] = r[1](g)
        except g.G.SvhError as e:
            assert e.code == -1, (n, e.code, str(e))
            out[n] = CC.REFUSED
    return out


class Rig(OCC.Rig):
    """tests/grid_obj_cache_cases.Rig with this file's scene and mutators"""

    def __init__(self, G, hip):
        self.G, self.hip, self.log = G, hip, []
        self.g, self.ref = self.make(), CC.new_ref()
        scene(self.g, self.ref)

    def apply(self, m):
        self.log.append(m)
        for g, ref, errors in ((self.g, None, (self.G.SvhError,)), (None, self.ref, (ALL.Refused, ValueError))):
            try:
                MUTATORS[m](g, ref, None)
            except errors:
                pass

    def fresh(self):
        g = self.make()
        scene(g, None)
        for m in self.log:
            try:
                MUTATORS[m](g, None, None)
            except self.G.SvhError:
                pass
        return g

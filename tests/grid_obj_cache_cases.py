"""The tables behind tests/test_grid_obj_cache.py and tests/test_grid_obj_cache_gpu.py: the outputs of the object layer
(include/svh_grid_obj.h) that pass through the engine's cache or are state of the tracks (READERS), every mutator of
tests/grid_cache_cases.py and the layer's own three (MUTATORS), and what the header says each does to each (EXPECT), written from the
header's text: the objects are a function of the accumulators, the window's offsets and the object parameters and of nothing else; the
tracks are advanced by svh_grid_objects_step alone and emptied by svh_grid_set_window, svh_grid_set_objects and
svh_grid_objects_reset.

The scene is that of tests/grid_cache_cases.py with the object parameters OBJ_KW set and two steps taken; the restatement is the
composed one (tests/grid_all_ref.py) with tests/grid_obj_ref.py on its finished planes and a Tracker beside it."""
import numpy as np

import grid_cache_cases as CC
import grid_obj_ref as OR

CHANGES, KEEPS = CC.CHANGES, CC.KEEPS
# the wall's two parts (12 and 3 cells) are kept, the room's ring of 20 cells is structure, single cells are too small
OBJ_KW = dict(min_size=2, max_size=16, min_height=0.5, max_tracks=8, min_overlap=1, gate=3, max_missed=1, min_age=1, move_cells=1, smooth_shift=1)
OTHER_KW = dict(OBJ_KW, max_size=32)                              # the ring becomes an object


def B(*arrays):
    return b"|".join(np.ascontiguousarray(a).tobytes() for a in arrays)


# ---- the restatement's side: the objects of the composed grid as it stands, a tracker beside it ------------------------------------
def ref_objects(ref):
    pl = ref.planes()
    return OR.objects(ref.obj, ref.state(), pl["hmax"], pl["count"], ref.oa, ref.ob)


def ref_step(ref):
    _, label, recs, _ = ref_objects(ref)
    return ref.trk.step(ref.obj, recs, label, (ref.oa, ref.ob))


def ref_track_plane(ref):
    nz, nx = ref.state().shape
    return (np.full((nz, nx), -1, np.int32), (ref.oa, ref.ob)) if ref.trk.ids is None else (ref.trk.ids, ref.trk.off)


# ---- readers: name -> (group, device form, restated form) --------------------------------------------------------------------------
READERS = {
    "obj:FLAGS": ("obj", lambda g: B(g.obj_plane(g.G.OBJ_FLAGS)), lambda ref: B(ref_objects(ref)[0])),
    "obj:LABEL": ("obj", lambda g: B(g.obj_plane(g.G.OBJ_LABEL)), lambda ref: B(ref_objects(ref)[1])),
    "objects": ("obj", lambda g: B(g.objects()), lambda ref: B(ref_objects(ref)[2])),
    "object_stats": ("obj", lambda g: CC.ints(*g.object_stats()[:6]), lambda ref: CC.ints(*ref_objects(ref)[3])),
    "tracks": ("tracks", lambda g: B(g.tracks()), lambda ref: B(ref.trk.tracks)),
    "track_plane": ("tracks", lambda g: B(g.track_plane()[0], np.array(g.track_plane()[1])), lambda ref: B(ref_track_plane(ref)[0], np.array(ref_track_plane(ref)[1]))),
    "track_stats": ("tracks", lambda g: CC.ints(*g.track_stats()), lambda ref: CC.ints(*ref.trk.track_stats())),
}
CACHED = [n for n, r in READERS.items() if r[0] == "obj"]


# ---- the layer's own mutators ------------------------------------------------------------------------------------------------------
def set_objects(g, ref, rng):
    if g is not None:
        g.set_objects(g.G.default_obj(**OTHER_KW))
    if ref is not None:
        ref.obj = OR.ObjParams(**OTHER_KW)
        ref.trk.reset()


def objects_step(g, ref, rng):
    if g is not None:
        g.last_assign = g.objects_step()
    if ref is not None:
        ref.last_assign = ref_step(ref)


def objects_reset(g, ref, rng):
    if g is not None:
        g.objects_reset()
    if ref is not None:
        ref.trk.reset()


def with_tracks(f):
    """a mutator of tests/grid_cache_cases.py with what the header says it does to the tracks"""
    def apply(g, ref, rng):
        f(g, ref, rng)
        if ref is not None and f is CC.MUTATORS["set_window"]:
            ref.trk.reset()
    return apply


OWN = {"set_objects": set_objects, "objects_step": objects_step, "objects_reset": objects_reset}
MUTATORS = dict({m: with_tracks(CC.MUTATORS[m]) for m in CC.MATRIX_MUTATORS}, **OWN)
# mutator -> the groups whose readers CHANGE; every other reader KEEPS
RULES = dict({m: ({"obj"} if "acc" in CC.RULES[m][0] else set()) for m in CC.MATRIX_MUTATORS}, set_objects={"obj", "tracks"}, objects_step={"tracks"},
             objects_reset={"tracks"})
RULES["set_window"] = {"obj", "tracks"}
EXPECT = {m: {n: (CHANGES if r[0] in RULES[m] else KEEPS) for n, r in READERS.items()} for m in MUTATORS}
# the mutators of other layers that the issue names: they leave the objects valid
OTHER_LAYERS = ["set_traversability", "set_plan", "plan_set_goals", "plan_set_goal", "plan_set_goals_frontiers", "plan_set_goal_explore", "set_frontier",
                "set_explore", "set_roll", "set_roll_headings", "roll_set_candidates", "set_align", "roll_score_elsewhere", "align_points_elsewhere",
                "align_view_lists", "explore_rank_elsewhere", "set_dynamics_change", "set_dynamics_drop", "set_dynamics_again"]
# CHANGES pairs that the scene cannot show, each with its reason
UNSHOWN = {
    ("observe_empty", "objects"): "what ages is the patch with its one obstacle cell, which is too small for the table",
    ("set_objects", "obj:LABEL"): "LABEL is a function of STATE alone; it is computed again with the rest all the same",
    ("objects_step", "track_plane"): "a step on a scene that has not changed writes the ids it found",
}


def served_from_cache(m, n):
    return READERS[n][0] == "obj" and "obj" not in RULES[m]


def scene(g, ref):
    """the scene of tests/grid_cache_cases.py, the object parameters, two steps"""
    CC.scene(g, ref)
    if g is not None:
        g.set_objects(g.G.default_obj(**OBJ_KW))
    if ref is not None:
        ref.obj, ref.trk = OR.ObjParams(**OBJ_KW), OR.Tracker()
    for _ in range(2):
        objects_step(g, ref, None)


def read_ref(ref):
    with ref.frozen():
        return {n: r[2](ref) for n, r in READERS.items()}


def read_dev(g):
    return {n: r[1](g) for n, r in READERS.items()}


class Rig:
    """an object and the restatement under one history of mutators; fresh() replays it on a new object that is never read in between"""

    def __init__(self, G, hip):
        self.G, self.hip, self.log = G, hip, []
        self.g, self.ref = self.make(), CC.new_ref()
        scene(self.g, self.ref)

    def make(self):
        g = CC.new_object(self.G)
        g.G, g.hip = self.G, self.hip
        return g

    def apply(self, m):
        self.log.append(m)
        MUTATORS[m](self.g, None, None)
        MUTATORS[m](None, self.ref, None)

    def fresh(self):
        g = self.make()
        scene(g, None)
        for m in self.log:
            MUTATORS[m](g, None, None)
        return g

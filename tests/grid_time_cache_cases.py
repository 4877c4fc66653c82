"""The tables behind tests/test_grid_time_cache.py and tests/test_grid_time_cache_gpu.py: the outputs of the time layer
(include/svh_grid_time.h) that pass through the engine's cache (READERS), every mutator of tests/grid_cache_cases.py,
tests/grid_obj_cache_cases.py, tests/grid_pred_cache_cases.py and tests/grid_pose_cache_cases.py, those of the archive, and the layer's
own setter in its three uses (MUTATORS), and what the header says about them: which mutators LEAVE the layer ALONE, so that its outputs
are served without a launch.

The scene is that of tests/grid_pose_cache_cases.py (objects, two steps, the prediction, the planner's goals) with the layer switched
on.  What a read must return is said twice: by a fresh object that replays the history and is read once, and by the header
(svh_test_grid_time) on the object's own COST, FLAGS, tracks and PRED (tests/grid_time_cases.check_object)."""
import numpy as np

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pose_cache_cases as QCC

B = OCC.B
TIME_KW = dict(layers=6, wait=100, release=1)

ARCHIVE = {
    "set_archive": lambda g, ref, rng: g.set_archive(max_tiles=32),
    "archive_trim": lambda g, ref, rng: g.archive_trim(0, 0, 5, 5),
    "archive_clear": lambda g, ref, rng: g.archive_clear(),
    "set_archive_off": lambda g, ref, rng: g.set_archive(max_tiles=0),
}
OWN = {
    "set_time_wait": lambda g, ref, rng: g.set_time(wait=7),
    "set_time_layers": lambda g, ref, rng: g.set_time(layers=9),
    "set_time_release": lambda g, ref, rng: g.set_time(release=0),
}
MUTATORS = dict(QCC.MUTATORS, **ARCHIVE, **OWN)


def dev_path(g):
    status, triples, cost = g.time_path(CC.ANCHOR)
    return B(triples, np.array([status, cost]))


# name -> (group, the read)
READERS = {
    "time:RCOST": ("static", lambda g: B(g.time_plane(g.G.TIME_RCOST))),
    "time:RPOT": ("static", lambda g: B(g.time_plane(g.G.TIME_RPOT))),
    "time:TPOT": ("field", lambda g: B(g.time_plane(g.G.TIME_TPOT))),
    "time:TDIR": ("field", lambda g: B(g.time_plane(g.G.TIME_TDIR))),
    "time_stats": ("field", lambda g: CC.ints(*g.time_stats()[:5])),
    "time_path": ("path", dev_path),
}
CACHED = [n for n, r in READERS.items() if r[0] in ("static", "field")]      # a path is walked per call: one launch

# what the header names as leaving the layer alone: the frontier, rollout, candidate, alignment and pose parameters and goals, the
# archive and its mutators
LEFT_ALONE = ["set_frontier", "set_roll", "set_roll_headings", "roll_set_candidates", "roll_score_elsewhere", "set_align", "align_points_elsewhere",
              "set_explore", "explore_rank_elsewhere", "set_pose", "pose_set_goals", "pose_set_goal"] + list(ARCHIVE)
# the layer's own setter keeps the static planes unless `release` changes
KEEPS_STATIC = ["set_time_wait", "set_time_layers"]


def scene(g):
    QCC.scene(g, None)
    g.set_time(g.G.default_time(**TIME_KW))


def read_dev(g):
    out = {}
    for n, r in READERS.items():
        try:
            out[n] = r[1](g)
        except g.G.SvhError as e:
            assert e.code == -1, (n, e.code, str(e))
            out[n] = CC.REFUSED
    return out


class Rig:
    """an object under one history of mutators; fresh() replays it on a new object that is never read in between"""

    def __init__(self, G, hip):
        self.G, self.hip, self.log = G, hip, []
        self.g = self.make()
        scene(self.g)

    def make(self):
        g = CC.new_object(self.G)
        g.G, g.hip = self.G, self.hip
        return g

    def apply(self, m, g=None):
        if g is None:
            self.log.append(m)
        try:
            MUTATORS[m](g if g is not None else self.g, None, None)
        except self.G.SvhError as e:
            assert e.code == -1, (m, e.code, str(e))

    def fresh(self):
        g = self.make()
        scene(g)
        for m in self.log:
            self.apply(m, g)
        return g

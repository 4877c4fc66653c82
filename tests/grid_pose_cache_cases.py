"""The tables behind tests/test_grid_pose_cache.py and tests/test_grid_pose_cache_gpu.py: the outputs of the pose planner
(include/svh_grid_pose.h) that pass through the engine's cache (READERS), every mutator of tests/grid_cache_cases.py,
tests/grid_obj_cache_cases.py and tests/grid_pred_cache_cases.py with the layer's own three (MUTATORS), and what the header says each
does to each, written from the header's text: CF is a function of COST and the rollout parameters -- the group `foot` of
tests/grid_cache_cases.py, whose reader is svh_grid_footprint_cost --; PPOT, PDIR, the statistics and a path are a function of CF, the
parameters of this layer and its goals; svh_grid_clear and svh_grid_set_window forget the goals.  svh_grid_set_plan, the planner's
goals, the candidates, the objects and the prediction leave all of it alone.

The scene is that of tests/grid_pred_cache_cases.py (the composed restatement, objects, two steps, the prediction) with the pose
parameters POSE_KW and the goals of the planner's scene as goal states; the restatement is tests/grid_pose_ref.py on the composed
grid's COST and footprint table."""
import numpy as np

import grid_all_ref as ALL
import grid_cache_cases as CC
import grid_local_ref as LR
import grid_obj_cache_cases as OCC
import grid_pose_ref as QR
import grid_pred_cache_cases as PCC

CHANGES, KEEPS = CC.CHANGES, CC.KEEPS
POSE_KW = dict(neutral=50, max_cost=0x7FFFFFFE, turn=100, reverse=120, spin=-1)
OTHER_KW = dict(POSE_KW, turn=40, spin=300)
START_D = 0                                                        # the path starts at the rollouts' anchor, facing the wall
B = OCC.B


def goals_of(L, off=(0, 0)):
    """the planner's three goals (the third outside the window) as goal states: every heading, one heading, every heading"""
    return np.array([(a + off[0], b + off[1], d) for (a, b), d in zip(L.goals.tolist(), (-1, 2, -1))], np.int32)


def other_goals(L, off=(0, 0)):
    return np.array([(L.start[0] + off[0], L.start[1] + off[1], -1), (L.start_b[0] + off[0], L.start_b[1] + off[1], 6)], np.int32)


# ---- the restatement's side ------------------------------------------------------------------------------------------------------
def ref_field(ref):
    """(cf, pot, dir, counted) of the composed restatement as it stands"""
    return QR.field(ref.roll, ref.pose, ref.roll_lists(), ref.cost(), ref.pose_goals, ref.oa, ref.ob)


def ref_stats(ref):
    _, pot, _, counted = ref_field(ref)
    return len(ref.pose_goals), counted, int((pot != QR.FAR).sum())


def ref_path(ref):
    cf, pot, dir_, _ = ref_field(ref)
    ga, gb = LR.cell_of(ref.P, CC.ANCHOR)
    a, b = ga - ref.oa, gb - ref.ob
    nz, nx = ref.cost().shape
    if not (0 <= a < nx and 0 <= b < nz):
        return B(np.zeros((0, 3), np.int32), np.array([QR.OUTSIDE, QR.FAR]))
    own = int(pot[START_D, b, a])
    if QR.prices(ref.pose, ref.roll.stop_cost, cf)[START_D, b, a] == 0:
        return B(np.zeros((0, 3), np.int32), np.array([QR.BLOCKED, own]))
    if own == QR.FAR:
        return B(np.zeros((0, 3), np.int32), np.array([QR.UNREACHABLE, own]))
    return B(QR.walk(dir_, a, b, START_D, ref.roll.headings_m, ref.oa, ref.ob), np.array([QR.FOUND, own]))


def dev_path(g):
    status, poses, cost = g.pose_path(CC.ANCHOR, START_D)
    return B(poses, np.array([status, cost]))


# ---- readers: name -> (group, device form, restated form) --------------------------------------------------------------------------
READERS = {
    "pose:CF": ("cf", lambda g: B(g.pose_plane(g.G.POSE_CF)), lambda ref: B(ref_field(ref)[0])),
    "pose:POT": ("pose", lambda g: B(g.pose_plane(g.G.POSE_POT)), lambda ref: B(ref_field(ref)[1])),
    "pose:DIR": ("pose", lambda g: B(g.pose_plane(g.G.POSE_DIR)), lambda ref: B(ref_field(ref)[2])),
    "pose_stats": ("pose", lambda g: CC.ints(*g.pose_stats()[:3]), lambda ref: CC.ints(*ref_stats(ref))),
    "pose_path": ("path", dev_path, ref_path),
}
CACHED = [n for n, r in READERS.items() if r[0] in ("cf", "pose")]     # a path is walked per call: one launch


# ---- the layer's own mutators ------------------------------------------------------------------------------------------------------
def set_pose(g, ref, rng):
    if g is not None:
        g.set_pose(g.G.default_pose(**OTHER_KW))
    if ref is not None:
        ref.pose = QR.PoseParams(**OTHER_KW)


def pose_set_goals(g, ref, rng):
    goals = other_goals((ref if ref is not None else g).L, CC.frame(g, ref)[2:])
    if g is not None:
        g.pose_set_goals(goals)
    if ref is not None:
        ref.pose_goals = goals


def pose_set_goal(g, ref, rng):
    """one goal: the cell of a position, here the rollouts' anchor, at heading 4"""
    if g is not None:
        g.pose_set_goal(CC.ANCHOR, 4)
    if ref is not None:
        ga, gb = LR.cell_of(ref.P, CC.ANCHOR)
        ref.pose_goals = np.array([(ga, gb, 4)], np.int32)


def with_goals(name, f):
    """a mutator of the other layers with what the header says it does to this layer's goals"""
    def apply(g, ref, rng):
        f(g, ref, rng)
        if ref is not None and name in ("clear", "set_window"):
            ref.pose_goals = np.zeros((0, 3), np.int32)
    return apply


OWN = {"set_pose": set_pose, "pose_set_goals": pose_set_goals, "pose_set_goal": pose_set_goal}
MUTATORS = dict({m: with_goals(m, f) for m, f in PCC.MUTATORS.items()}, **OWN)
# what makes CF stale: whatever the table of tests/grid_cache_cases.py says changes svh_grid_footprint_cost, the reader of group `foot`
CF_DROPS = [m for m in MUTATORS if m in CC.RULES and "foot" in CC.RULES[m][0]]
# mutator -> the groups whose readers CHANGE; every other reader KEEPS
RULES = {m: ({"cf", "pose", "path"} if m in CF_DROPS else {"pose", "path"} if m in OWN else set()) for m in MUTATORS}
EXPECT = {m: {n: (CHANGES if r[0] in RULES[m] else KEEPS) for n, r in READERS.items()} for m in MUTATORS}
# what the issue names as leaving the layer alone
LEFT_ALONE = ["set_plan", "plan_set_goals", "plan_set_goal", "plan_set_goals_frontiers", "plan_set_goal_explore", "roll_set_candidates", "set_objects",
              "objects_step", "objects_reset", "set_predict", "set_frontier", "set_explore", "set_align", "set_dynamics_change"]
# CHANGES pairs that the scene cannot show, each with its reason: filled in by tests/test_grid_pose_cache.py's own check, which fails,
# naming the pair, for one that is listed and shown or shown and not listed
SAME_BYTES = "the vectors of the 8 planning headings do not depend on headings_m: CF is computed again to the same bytes, and the field with it"
UNSHOWN = {
    ("set_roll_headings", "pose:CF"): SAME_BYTES,
    ("set_roll_headings", "pose:POT"): SAME_BYTES,
    ("set_roll_headings", "pose:DIR"): SAME_BYTES,
    ("set_roll_headings", "pose_stats"): SAME_BYTES,
    ("scroll", "pose_path"): "poses are global cells: the route lies inside the scrolled window and comes back as it was, at the same cost",
    ("set_traversability", "pose_stats"): "the other radii change prices, not which states are passable or reached: the three counts stay",
}


def served_from_cache(m, n):
    return n in CACHED and READERS[n][0] not in RULES[m]


def scene(g, ref):
    PCC.scene(g, ref)
    if g is not None:
        g.set_pose(g.G.default_pose(**POSE_KW))
        g.pose_set_goals(goals_of(g.L, CC.frame(g, None)[2:]))
    if ref is not None:
        ref.pose = QR.PoseParams(**POSE_KW)
        ref.pose_goals = goals_of(ref.L, CC.frame(None, ref)[2:])


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

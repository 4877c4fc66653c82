"""One restatement of the whole ground grid (include/svh_grid.h): the two branches of numpy restatements -- tests/grid_dyn_ref.py on
tests/grid_local_ref.py, and tests/grid_plan_ref.py on tests/grid_trav_ref.py on tests/grid_local_ref.py -- composed into one class
by cooperative super(), with thin methods that hand its own STATE, COST and POT planes to the stateless functions of
tests/grid_front_ref.py, tests/grid_explore_ref.py, tests/grid_roll_ref.py and tests/grid_align_ref.py.  No arithmetic is restated
here: every number comes out of one of those files.  What this file adds is what the engine keeps BETWEEN calls and the layers'
files do not model: the parameters of every layer in one object, the candidate table, the last scoring (svh_grid_render_roll) and
the last alignment (svh_grid_get_align_scan, svh_grid_get_align_volume, svh_grid_render_align), with the rules of the header for
when they are forgotten.  It caches nothing: every read is computed from the accumulators as they are, which is what a cache in
the engine must be indistinguishable from (tests/test_grid_cache.py, tests/test_grid_cache_gpu.py).

A refused call raises Refused, where the header says SVH_ERR_BAD_ARG."""
import numpy as np

import grid_align_ref as AR
import grid_dyn_ref as DR
import grid_explore_ref as ER
import grid_front_ref as FR
import grid_local_ref as LR
import grid_plan_ref as PR
import grid_roll_ref as RR


class Refused(Exception):
    """the header's SVH_ERR_BAD_ARG"""


class Grid(DR.Grid, PR.Grid):
    """grid_dyn_ref.Grid and grid_plan_ref.Grid on one set of accumulators, with the frontiers, the exploration layer, the rollouts
    and the alignment layer on its own planes"""

    def __init__(self, P, T=None, plan=None, D=None):
        self.D = D
        self._memo = None
        PR.Grid.__init__(self, P, T, plan)
        self.front = FR.FrontParams()
        self.explore = ER.ExploreParams()
        self.roll = RR.RollParams()
        self.cands = None                      # int32 [S, K, T, 3]
        self.roll_last = None                  # dict: set, anchor, recs, best
        self.align = None                      # AR.AlignParams; a grid is created without
        self.align_last = None                 # dict: Pa, Pb, scan, volume (None when FEW), rec
        self.rank_last = (0, 0)                # records and feasible records of the last ranking

    # ---- one read-out computes each plane once ---------------------------------------------------------------------------------
    def frozen(self):
        """a context in which nothing changes the accumulators or the parameters: planes(), local_planes(), trav(), field() and
        frontiers() are computed once in it.  It is a convenience of a read-out, not a cache: it ends with the read-out"""
        grid = self

        class Frozen:
            def __enter__(self):
                grid._memo = {}

            def __exit__(self, *exc):
                grid._memo = None
        return Frozen()

    def _once(self, key, f):
        if self._memo is None:
            return f()
        if key not in self._memo:
            self._memo[key] = f()
        return self._memo[key]

    def planes(self):
        return self._once("planes", super().planes)

    def local_planes(self):
        return self._once("local", super().local_planes)

    def trav(self):
        return self._once("trav", super().trav)

    def field(self):
        return self._once("field", super().field)

    # ---- the planes the layers read -------------------------------------------------------------------------------------------
    def state(self):
        return self.local_planes()["state"]

    def cost(self):
        return self.trav()["cost"]

    def observe(self, pts, origin):
        if self.D is None:
            raise Refused("the dynamics are not set")
        return super().observe(pts, origin)

    def dyn_planes(self):
        if self.D is None:
            raise Refused("the dynamics are not set")
        return super().dyn_planes()

    def render_dyn(self):
        if self.D is None:
            raise Refused("the dynamics are not set")
        return super().render_dyn()

    # ---- the frontiers --------------------------------------------------------------------------------------------------------
    def frontiers(self):
        """dict: flags, label, recs, stats (4)"""
        def compute():
            flags, label, recs, stats = FR.frontiers(self.front, self.state(), self.cost(), self.oa, self.ob)
            return dict(flags=flags, label=label, recs=recs, stats=stats)
        return self._once("frontiers", compute)

    def render_frontiers(self):
        return FR.overlay(self.render_cost(), self.frontiers()["flags"])

    def set_goals_frontiers(self):
        recs = self.frontiers()["recs"][:PR.MAX_GOALS]
        self.set_goals(recs[:, 8:10])
        return len(recs)

    # ---- the exploration layer ------------------------------------------------------------------------------------------------
    def range_cells(self):
        return ER.range_cells(self.explore.range, self.P.cell)

    def view_gain(self, cells):
        return ER.gains(self.front, self.range_cells(), self.state(), cells, self.oa, self.ob)

    def view_mask(self, ga, gb):
        a, b = ga - self.oa, gb - self.ob
        if not (0 <= a < self.P.nx and 0 <= b < self.P.nz):
            raise Refused("the viewpoint is outside the window")
        return ER.view(self.front, self.range_cells(), self.state(), a, b)[0]

    def render_view(self, ga, gb):
        return ER.overlay(self.render_frontiers(), self.view_mask(ga, gb), ga - self.oa, gb - self.ob)

    def explore_rank(self, start_xyz):
        """(best, recs, scores); the counts of svh_grid_get_explore_stats are kept"""
        recs, scores, best, feasible = ER.rank(self.front, self.plan, self.explore, self.range_cells(), self.state(), self.cost(),
                                               LR.cell_of(self.P, start_xyz), self.oa, self.ob)
        self.rank_last = (len(recs), feasible)
        return best, recs, scores

    def set_goal_explore(self, start_xyz):
        best, recs, _ = self.explore_rank(start_xyz)
        if best < 0:
            return 0
        self.set_goals(recs[best, 1:3])
        return 1

    # ---- the rollouts ---------------------------------------------------------------------------------------------------------
    def set_roll(self, roll):
        if roll.headings_m != self.roll.headings_m:
            self.cands = None
        self.roll, self.roll_last = roll, None

    def set_candidates(self, table):
        self.cands, self.roll_last = np.array(table, np.int32), None

    def roll_lists(self):
        return RR.table(self.roll, self.P.cell)[1]

    def footprint_cost(self, poses):
        return RR.footprint_costs(self.roll, self.roll_lists(), self.cost(), poses, self.oa, self.ob)

    def roll_score(self, anchor_xyz, set_=0):
        """(best, recs, scores); the scoring is kept for render_roll"""
        if self.cands is None:
            raise Refused("no candidates")
        anchor = LR.cell_of(self.P, anchor_xyz)
        pot = self.field()["pot"] if self.roll.w_pot != 0 else None
        recs, scores, best = RR.score(self.roll, self.roll_lists(), self.cost(), pot, self.cands[set_], anchor, self.oa, self.ob)
        self.roll_last = dict(set=set_, anchor=anchor, recs=recs, best=best)
        return best, recs, scores

    def render_roll(self):
        """the LAST scoring's cells over the cost planes as they are NOW"""
        w = self.roll_last
        if w is None:
            raise Refused("nothing was scored since the tables were set")
        return RR.overlay(self.render_cost(), self.cands[w["set"]], w["recs"], w["best"], w["anchor"], self.oa, self.ob)

    # ---- the alignment layer --------------------------------------------------------------------------------------------------
    def set_align(self, align):
        self.align, self.align_last = align, None

    def _aligned(self):
        if self.align is None:
            raise Refused("the align parameters are not set")
        return self.align.derive(self.P.cell)

    def align_field(self):
        return AR.field(self.state(), self._aligned()[0])

    def align_points(self, pts, pivot):
        _, Rg = self._aligned()
        Pa, Pb = AR.pivot_sub(self.P, pivot)
        scan, _ = AR.scan_points(self.P, Rg, Pa, Pb, pts)
        _, vol, rec = AR.align(self.align, self.P.cell, self.state(), self.oa, self.ob, Pa, Pb, scan)
        self.align_last = dict(Pa=Pa, Pb=Pb, scan=scan, volume=vol, rec=rec)
        return rec

    def align_scan(self):
        self._aligned()
        if self.align_last is None:
            raise Refused("there is no scan")
        return self.align_last["scan"]

    def align_volume(self):
        self._aligned()
        if self.align_last is None or self.align_last["volume"] is None:
            raise Refused("there is no volume")
        return self.align_last["volume"]

    def render_align(self):
        """the LAST alignment's scan over the local planes as they are NOW"""
        self._aligned()
        w = self.align_last
        if w is None:
            raise Refused("there is no alignment to draw")
        rec = w["rec"]
        at_best = AR.placed(self.align, w["Pa"], w["Pb"], w["scan"], int(rec[1]), int(rec[2]), int(rec[3]))
        return AR.overlay(self.render_local(), self.oa, self.ob, w["Pa"], w["Pb"], w["scan"], at_best)

"""The tables behind tests/test_grid_cache.py and tests/test_grid_cache_gpu.py: every call of include/svh_grid.h that changes what a
later read may return (MUTATORS), every output that passes through one of the engine's caches (READERS), and what the header says
each mutator does to each reader (EXPECT): CHANGES, KEEPS or REFUSES.  EXPECT is written from the header's text and the comment at
the top of stereo-vision_amd/csrc/grid_engine.cpp -- which state a reader is a function of (its GROUP) and which states a mutator
touches -- never from the engine's flag assignments: the tests exist to compare the two.

A mutator is a function (g, ref, rng): it applies the same change to the object `g` (svhip.grid.Grid, or None) and to the composed
restatement `ref` (tests/grid_all_ref.py, or None).  rng None is the canonical variant, the one EXPECT and the matrix speak about; a
numpy Generator draws another variant for the seeded walk.  All geometry is relative to the window as it stands, so a mutator
works after any scroll.  A reader has a device form g -> bytes and a restated form ref -> bytes.

Outputs WITHOUT a restatement, compared warm against fresh only: none of the readers below; the one figure left out everywhere is
out[3] of svh_grid_get_plan_stats (relaxation rounds), out[2] and out[3] of svh_grid_get_explore_stats (fields computed, launches) and
out[4] of svh_grid_get_frontier_stats (launches): the header says they depend on scheduling or on what was read before."""
import numpy as np

import grid_align_ref as AR
import grid_all_ref as ALL
import grid_dyn_ref as DR
import grid_explore_ref as ER
import grid_front_ref as FR
import grid_plan_ref as PR
import grid_ref as R
import grid_roll_ref as RR
import grid_trav_ref as TR

F = np.float32
CELL = 0.5
T = 16                                          # PLAN_TILE and FRONT_TILE of the build: the scene's window is (2 T + 1) x (T + 1)
NX, NZ = 2 * T + 1, T + 1
CHANGES, KEEPS, REFUSES = "CHANGES", "KEEPS", "REFUSES"
REFUSED = b"REFUSED"
BAD_ARG, HIP_ERR = -1, -2


# ---- parameters ---------------------------------------------------------------------------------------------------------------
def grid_kw(nx=NX, nz=NZ):
    """the window of the hand case of tests/test_grid_dyn.py: cells of 0.5, a camera 1.5 above the road (a = x, b = z, h = 1.5 - y)"""
    return dict(nx=nx, nz=nz, cell=CELL, x0=0.0, z0=0.0, T=R.frame_camera(1.5), min_points=2, step=0.2, drop=0.3, clearance=2.0)


DYN_KW = dict(clear_frames=2, min_through=1, margin=0.1, max_age=2)
ROLL_KW = dict(front=1.0, rear=0.5, half_width=0.2, headings_m=2, stop_cost=253, unknown_cost=254, w_pot=1, w_cost=1, w_cut=2)
EXPLORE_KW = dict(range=4.0, min_gain=1, w_gain=500, w_reach=1)
FRONT_KW = dict(max_cell_cost=235, min_size=8, unexplored=8, border=0)   # 235: between the costs beside an obstacle under the two inscribed radii
ALIGN_KW = dict(reach=0.6, range=8.0, rot_den=256, rot_n=2, trans_n=3, min_scan=8)


def frame(g, ref):
    """(x0, z0, oa, ob) of the window as it stands"""
    if ref is not None:
        return float(ref.P.x0), float(ref.P.z0), ref.oa, ref.ob
    oa, ob = g.window()
    return float(g.params.x0), float(g.params.z0), oa, ob


def pts(fr, ia, ib, h, val=0.5, rep=1):
    """`rep` points in the middle of each window cell (ia, ib) at height h (arrays broadcast): float32 [n, 4].  Cell centres are
    multiples of 0.25 and stay exact in fp32"""
    ia, ib, h, val = np.broadcast_arrays(np.asarray(ia), np.asarray(ib), np.asarray(h, np.float64), np.asarray(val, np.float64))
    p = np.zeros((ia.size, 4), F)
    p[:, 0], p[:, 1] = fr[0] + (fr[2] + ia.ravel() + 0.5) * CELL, 1.5 - h.ravel()
    p[:, 2], p[:, 3] = fr[1] + (fr[3] + ib.ravel() + 0.5) * CELL, val.ravel()
    return np.repeat(p, rep, axis=0)


def pos(fr, ia, ib, h=1.5):
    """the map-frame position in the middle of window cell (ia, ib) at height h, in double"""
    return [fr[0] + (fr[2] + ia + 0.5) * CELL, 1.5 - h, fr[1] + (fr[3] + ib + 0.5) * CELL]


ZERO = (0.0, 0.0, 0, 0)                         # the frame the readers' fixed positions are given in: they are GLOBAL


# ---- the scene ----------------------------------------------------------------------------------------------------------------
class Layout:
    """where the scene's things are, in window cells, for a window of nx x nz"""

    def __init__(self, nx=NX, nz=NZ):
        self.nx, self.nz = nx, nz
        self.wall = nx // 2                                              # a wall along this column ...
        self.gap = (nz - 5, nz - 4)                                      # ... with a gap of two cells
        self.room = (self.wall + 4, 2, self.wall + 9, 7)                 # a closed room: a0, b0, a1, b1, walls on the border
        self.block = (nx - 6, nz - 6)                                    # an unseen block from here to the far corner
        self.strip = 11                                                  # an unseen strip: the last row, columns below this
        self.patch = (4, nz - 4, 8, nz - 2)                              # ground seen by the first observation only: it ages
        self.origin = (1, 1)                                             # the rays come from here, 1.5 above the road
        self.goals = np.array([[nx - 3, nz // 2], [self.wall + 6, nz - 2], [nx + 5, 3]], np.int32)   # the third is outside
        self.start = (2, nz // 2)
        self.start_b = (self.wall + 1, nz - 3)                           # behind the wall, beside it
        self.relic = (6, nz - 3)                                         # an obstacle in the patch: it ages with it
        self.inside = (self.wall + 6, 4)                                 # a cell inside the room
        self.anchor = (self.wall - 8, nz - 5)                            # the rollouts start here, in front of the gap
        self.pivot = (self.wall - 8, nz // 2)

    def walls(self, wall=True):
        """(ia, ib) of every obstacle cell; without `wall` those of the room alone"""
        a0, b0, a1, b1 = self.room
        cells = [(self.wall, b) for b in range(self.nz) if b not in self.gap] if wall else []
        cells += [(a, b) for a in range(a0, a1 + 1) for b in range(b0, b1 + 1) if a in (a0, a1) or b in (b0, b1)]
        ia, ib = np.array(cells).T
        return ia, ib

    def ground(self, patch=True):
        ia, ib = np.meshgrid(np.arange(self.nx), np.arange(self.nz))
        ia, ib = ia.ravel(), ib.ravel()
        keep = ~((ia >= self.block[0]) & (ib >= self.block[1])) & ~((ib == self.nz - 1) & (ia < self.strip))
        if not patch:
            a0, b0, a1, b1 = self.patch
            keep &= ~((ia >= a0) & (ia <= a1) & (ib >= b0) & (ib <= b1))
        return ia[keep], ib[keep]

    def frame_points(self, fr, patch=True, wall=True):
        """one observation of the scene: two ground points in every seen cell, the wall's cells included, and two points 1.0 high in
        every wall cell"""
        ga, gb = self.ground(patch)
        wa, wb = self.walls(wall)
        p = [pts(fr, ga, gb, 0.0, 0.25 + 0.5 * ((ga + gb) % 2), rep=2), pts(fr, wa, wb, 1.0, 0.9, rep=2)]
        if patch:                                                        # in the patch: an obstacle, and a branch over its neighbour
            p += [pts(fr, *self.relic, 0.8, 0.7, rep=2), pts(fr, self.relic[0] - 1, self.relic[1], 2.5, 0.1, rep=2)]
        return np.concatenate(p)

    def behind(self, fr):
        """the ground behind the wall alone: its sight lines go through the wall"""
        ia, ib = np.meshgrid(np.arange(self.wall + 1, self.nx - 7), np.arange(self.nz - 7, self.nz - 1))
        return np.concatenate([pts(fr, ia.ravel(), ib.ravel(), 0.0, 0.6, rep=2), pts(fr, self.wall + 2, self.nz - 3, 2.5)])

    def plug(self, fr):
        """points that close the gap of the wall, fill a corner of the unseen block and put an obstacle before the second goal"""
        ia, ib = np.meshgrid(np.arange(self.block[0], self.block[0] + 3), np.arange(self.block[1], self.block[1] + 3))
        return np.concatenate([pts(fr, self.wall, np.array(self.gap), 1.2, 0.8, rep=2), pts(fr, ia.ravel(), ib.ravel(), 0.0, 0.4, rep=2),
                               pts(fr, self.wall + 5, self.nz - 2, 0.9, 0.3, rep=2), pts(fr, 3, 3, 2.5)])

    def align_frame(self, fr, shift=0.125):
        """the wall's cells and the patch's obstacle as a frame would see them a little to the side: two subs per cell"""
        wa, wb = self.walls()
        wa, wb = np.append(wa, self.relic[0]), np.append(wb, self.relic[1])
        p = np.concatenate([pts(fr, wa, wb, 1.0), pts(fr, wa, wb, 0.8)])
        p[len(wa):, 2] += F(0.25)
        p[:, 0] += F(shift)
        return p

    def candidates(self, other=False):
        """int32 [2, 3, 6, 3]: from the anchor towards and across the wall's column (heading 0 is +a with headings_m 2), along it
        (heading 4 is +b), and diagonally (heading 2); the second set runs the other way"""
        t = np.arange(1, 7)
        z = np.zeros(6, np.int64)
        step = 3 if other else 2
        fwd = [np.stack([step * t, z, z], 1), np.stack([z, t % 3, z + 4], 1), np.stack([t, t, z + 2], 1)]
        back = [np.stack([-step * t, z, z + 8], 1), np.stack([z, -(t % 3), z + 12], 1), np.stack([-t, -t, z + 10], 1)]
        tab = np.array([fwd, back], np.int32)
        tab[0, 1, 4:, 2] = -1                                            # a candidate that ends early
        return tab[:, :, :5].copy() if other else tab                    # the other table is a pose shorter


def new_ref(nx=NX, nz=NZ, dyn=DYN_KW):
    ref = ALL.Grid(R.Params(**grid_kw(nx, nz)), TR.TravParams(), PR.PlanParams(), DR.DynParams(**dyn) if dyn else None)
    ref.L = Layout(nx, nz)
    return ref


def new_object(G, nx=NX, nz=NZ):
    kw = grid_kw(nx, nz)
    g = G.Grid(G.default_params(**dict(kw, T=np.asarray(kw["T"], np.float64))))
    g.L = Layout(nx, nz)
    return g


def scene(g, ref):
    """the state every test starts from, applied to the object and to the restatement alike (either may be None): the layers'
    parameters, three observations from the corner (the patch is in the first alone and ages, the wall is not in the third), the goals, the candidates, one scoring, one ranking, one alignment"""
    L = (ref if ref is not None else g).L
    if g is not None:
        G = g.G
        g.set_dynamics(G.default_dyn(**DYN_KW))
        g.set_roll(G.default_roll(**ROLL_KW))
        g.set_explore(G.default_explore(**EXPLORE_KW))
        g.set_align(G.default_align(**ALIGN_KW))
        g.set_frontier(G.default_front(**FRONT_KW))
    if ref is not None:
        ref.set_roll(RR.RollParams(**ROLL_KW))
        ref.explore = ER.ExploreParams(**EXPLORE_KW)
        ref.set_align(AR.AlignParams(**ALIGN_KW))
        ref.front = FR.FrontParams(**FRONT_KW)
    fr = frame(g, ref)
    o = pos(fr, *L.origin)
    for k in range(3):                                   # the third frame misses the wall: its cells stand contradicted once
        p = L.frame_points(fr, patch=k == 0, wall=k < 2)
        if g is not None:
            g.observe_points(p, o)
        if ref is not None:
            ref.observe(p, o)
    goals = L.goals + np.array(fr[2:], np.int32)
    tab = L.candidates()
    if g is not None:
        g.set_goals(goals)
        g.set_candidates(tab)
    if ref is not None:
        ref.set_goals(goals)
        ref.set_candidates(tab)
    for name in ("roll_score", "explore_rank", "align_points"):
        MUTATORS[name](g, ref, None)


MUTATORS, MUTATOR_ENTRY = {}, {}


def mutator(entry, name=None):
    def deco(f):
        MUTATORS[name or f.__name__] = f
        MUTATOR_ENTRY[name or f.__name__] = entry
        return f
    return deco


# ---- the hand case: a cleared obstacle opens the route ---------------------------------------------------------------------------
HAND_DYN = dict(clear_frames=1, min_through=1)
HAND_ORIGIN, HAND_GOAL, HAND_START = (2, 8), (30, 8), (2, 8)
HAND = dict(reached=272, cleared=15, cost_bytes=75, reached_after=548, pot_after=19662)   # the restatement's values (tests/test_grid_cache.py)


def hand_scene(g, ref):
    """hand_kw(nx=33, nz=17) with default traversability and plan: the ground (h = 0) in every cell and a wall (h = 1.0) along column
    16, observed three times from the centre of cell (2, 8) at height 1.5; the goal is cell (30, 8).  The layers above the planner are
    set as in the scene, so that every reader can be asked"""
    L = (ref if ref is not None else g).L
    if g is not None:
        G = g.G
        g.set_dynamics(G.default_dyn(**HAND_DYN))
        g.set_roll(G.default_roll(**ROLL_KW))
        g.set_explore(G.default_explore(**EXPLORE_KW))
        g.set_align(G.default_align(**ALIGN_KW))
    if ref is not None:
        ref.set_dynamics(DR.DynParams(**HAND_DYN))
        ref.set_roll(RR.RollParams(**ROLL_KW))
        ref.explore = ER.ExploreParams(**EXPLORE_KW)
        ref.set_align(AR.AlignParams(**ALIGN_KW))
    ia, ib = (a.ravel() for a in np.meshgrid(np.arange(L.nx), np.arange(L.nz)))
    p = np.concatenate([pts(ZERO, ia, ib, 0.0), pts(ZERO, 16, np.arange(L.nz), 1.0)])
    o = pos(ZERO, *HAND_ORIGIN)
    tab = hand_candidates()
    for k in range(3):
        if g is not None:
            g.observe_points(p, o)
        if ref is not None:
            ref.observe(p, o)
    if g is not None:
        g.set_goals([HAND_GOAL])
        g.set_candidates(tab)
    if ref is not None:
        ref.set_goals([HAND_GOAL])
        ref.set_candidates(tab)


def hand_candidates():
    """int32 [1, 3, 8, 3]: three candidates from cell (8, 8) along +a in steps of 1, 2 and 3 cells: the first ends after four poses, before
    the wall; the last two cross column 16"""
    t, z = np.arange(1, 9), np.zeros(8, np.int64)
    tab = np.array([[np.stack([s * t, z, z], 1) for s in (1, 2, 3)]], np.int32)
    tab[0, 0, 4:, 2] = -1
    return tab


HAND_ANCHOR = pos(ZERO, 8, 8, h=0.0)


@mutator("svh_grid_observe_points", "hand_clearing")
def hand_clearing(g, ref, rng):
    """one further observation of the ground alone, without the wall's cells"""
    L = (ref if ref is not None else g).L
    ia, ib = (a.ravel() for a in np.meshgrid(np.arange(L.nx), np.arange(L.nz)))
    p, o = pts(ZERO, ia[ia != 16], ib[ia != 16], 0.0), pos(ZERO, *HAND_ORIGIN)
    if g is not None:
        g.observe_points(p, o)
    if ref is not None:
        ref.observe(p, o)


# ---- mutators -----------------------------------------------------------------------------------------------------------------

def pick(rng, canonical, others):
    return canonical if rng is None else others[int(rng.integers(len(others)))]


def device_copy(g, a):
    from test_view_gpu import Dev
    return Dev(g.hip, np.ascontiguousarray(a, F))


def with_view(lists, call):
    """call(v) on a view that holds the lists; the view is closed when the call has consumed it"""
    from svhip import view
    v = view.View(64, 48)
    try:
        for a in lists:
            v.add_points([np.ascontiguousarray(a, F)])
        return call(v)
    finally:
        v.close()


@mutator("svh_grid_clear")
def clear(g, ref, rng):
    if g is not None:
        g.clear()
    if ref is not None:
        ref.clear()


@mutator("svh_grid_set_window")
def set_window(g, ref, rng):
    x0, z0 = pick(rng, (1.0, -0.5), [(1.0, -0.5), (-2.0, 0.0), (0.0, 0.0)])
    if g is not None:
        g.set_window(x0, z0)
    if ref is not None:
        ref.set_window(x0, z0)


@mutator("svh_grid_scroll")
def scroll(g, ref, rng):
    da, db = pick(rng, (3, -2), [(3, -2), (-1, 0), (0, 2), (-2, -1), (1, 1), (-T - 1, 3)])
    if g is not None:
        g.scroll(da, db)
    if ref is not None:
        ref.scroll(da, db)


@mutator("svh_grid_follow")
def follow(g, ref, rng):
    fr = frame(g, ref)
    ia, ib = pick(rng, (0, 7), [(0, 7), (6, 3), (2, 2), (3, 5)])
    p = pos(fr, 4, 4, 0.0)
    if g is not None:
        g.follow(p, ia, ib)
    if ref is not None:
        ref.follow(p, ia, ib)


def _more(g, ref, rng):
    """the points of an add: the canonical ones close the gap and fill a corner of the block"""
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    if rng is None:
        return L.plug(fr)
    n = int(rng.integers(1, 40))
    ia, ib = rng.integers(0, L.nx, n), rng.integers(0, L.nz, n)
    return pts(fr, ia, ib, np.where(rng.random(n) < 0.4, rng.uniform(0.3, 1.8, n), 0.0), rng.random(n), rep=2)


def _origin(g, ref, rng):
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    return pos(fr, *pick(rng, L.origin, [L.origin, (L.nx - 2, 1), L.start]))


@mutator("svh_grid_add_points")
def add_points(g, ref, rng):
    p = _more(g, ref, rng)
    if g is not None:
        g.add_points(p)
    if ref is not None:
        ref.add(p)


@mutator("svh_grid_add_points", "add_points_device")
def add_points_device(g, ref, rng):
    p = _more(g, ref, rng)
    if g is not None:
        d = device_copy(g, p)
        g.add_points_device(d.addr, len(p))
    if ref is not None:
        ref.add(p)


@mutator("svh_grid_add_points_from")
def add_points_from(g, ref, rng):
    p, o = _more(g, ref, rng), _origin(g, ref, rng)
    if g is not None:
        g.add_points_from(p, o)
    if ref is not None:
        ref.add_from(p, o)


@mutator("svh_grid_add_view")
def add_view(g, ref, rng):
    p = _more(g, ref, rng)
    if g is not None:
        with_view([p[:1], p[1:]] if len(p) > 1 else [p], g.add_view)
    if ref is not None:
        ref.add(p)


@mutator("svh_grid_add_view_lists_from")
def add_view_lists_from(g, ref, rng):
    p, o = _more(g, ref, rng), _origin(g, ref, rng)
    if g is not None:
        with_view([p[:1], p, p[:1]], lambda v: g.add_view_lists_from(v, 1, 1, o))
    if ref is not None:
        ref.add_from(p, o)


def _frame(g, ref, rng):
    """the points of an observation: the canonical ones are the ground behind the wall, seen through it"""
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    if rng is None or rng.random() < 0.5:
        return L.behind(fr)
    return L.frame_points(fr, patch=bool(rng.integers(2)))


@mutator("svh_grid_observe_points")
def observe_points(g, ref, rng):
    p, o = _frame(g, ref, rng), _origin(g, ref, rng)
    if g is not None:
        g.observe_points(p, o)
    if ref is not None:
        ref.observe(p, o)


@mutator("svh_grid_observe_points", "observe_empty")
def observe_empty(g, ref, rng):
    """n == 0: the stamp advances and the cells that were not seen for long are aged"""
    o = _origin(g, ref, rng)
    if g is not None:
        g.observe_points(np.zeros((0, 4), F), o)
    if ref is not None:
        ref.observe(np.zeros((0, 4), F), o)


@mutator("svh_grid_observe_view_lists")
def observe_view_lists(g, ref, rng):
    p, o = _frame(g, ref, rng), _origin(g, ref, rng)
    if g is not None:
        with_view([p[:1], p[1:], p[:1]], lambda v: g.observe_view_lists(v, 0, 2, o))
    if ref is not None:
        ref.observe(p, o)


def _dyn_of(ref, **kw):
    D = ref.D
    old = dict(DYN_KW) if D is None else dict(clear_frames=D.clear_frames, min_through=D.min_through, margin=D.margin, max_age=D.max_age)
    return DR.DynParams(**dict(old, **kw))


@mutator("svh_grid_set_dynamics", "set_dynamics_change")
def set_dynamics_change(g, ref, rng):
    """new parameters keep CONTRA and LAST (and set the layer where it was dropped)"""
    kw = pick(rng, dict(clear_frames=3, margin=0.3), [dict(clear_frames=3, margin=0.3), dict(clear_frames=1, margin=0.1), dict(max_age=0), dict(max_age=2)])
    if g is not None:
        if _has_dyn(g):
            g.set_dynamics(**kw)
        else:
            g.set_dynamics(g.G.default_dyn(**dict(DYN_KW, **kw)))
    if ref is not None:
        ref.set_dynamics(_dyn_of(ref, **kw))


@mutator("svh_grid_set_dynamics", "set_dynamics_drop")
def set_dynamics_drop(g, ref, rng):
    if g is not None:
        g.drop_dynamics()
    if ref is not None:
        ref.set_dynamics(None)


@mutator("svh_grid_set_dynamics", "set_dynamics_again")
def set_dynamics_again(g, ref, rng):
    """dropped and set again: the planes start empty, the stamp goes on"""
    if g is not None:
        p = g.dynamics() if _has_dyn(g) else g.G.default_dyn(**DYN_KW)
        g.drop_dynamics()
        g.set_dynamics(p)
    if ref is not None:
        D = _dyn_of(ref)
        ref.set_dynamics(None)
        ref.set_dynamics(D)


def _has_dyn(g):
    try:
        g.dynamics()
        return True
    except g.G.SvhError:
        return False


@mutator("svh_grid_set_traversability")
def set_traversability(g, ref, rng):
    """the canonical variant keeps inflate, so the cost table keeps its size"""
    kw = pick(rng, dict(inscribed=0.45), [dict(inscribed=0.45), dict(inscribed=0.9), dict(inscribed=0.4), dict(inflate=2.0), dict(inflate=1.5), dict(lethal=15), dict(lethal=7)])
    if g is not None:
        g.set_traversability(**kw)
    if ref is not None:
        for k, v in kw.items():
            setattr(ref.T, k, int(v) if k == "lethal" else F(v))


@mutator("svh_grid_set_plan")
def set_plan(g, ref, rng):
    kw = pick(rng, dict(neutral=20, max_cost=9000), [dict(neutral=20, max_cost=9000), dict(neutral=50), dict(unknown=30), dict(unknown=-1), dict(max_cost=9000), dict(max_cost=0x7FFFFFFE)])
    if g is not None:
        g.set_plan(**kw)
    if ref is not None:
        for k, v in kw.items():
            setattr(ref.plan, k, v)


@mutator("svh_grid_plan_set_goals")
def plan_set_goals(g, ref, rng):
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    cells = pick(rng, [[3, 3], [L.nx - 2, 2], [3, 3], [3, 3]], [[[3, 3], [L.nx - 2, 2], [3, 3], [3, 3]], [], [[L.inside[0], L.inside[1]]], L.goals.tolist()])
    cells = np.asarray(cells, np.int32).reshape(-1, 2) + np.array(fr[2:], np.int32)
    if g is not None:
        g.set_goals(cells)
    if ref is not None:
        ref.set_goals(cells)


@mutator("svh_grid_plan_set_goal")
def plan_set_goal(g, ref, rng):
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    p = pos(fr, *pick(rng, (L.nx - 4, 3), [(L.nx - 4, 3), (5, 5), L.inside]), h=0.0)
    if g is not None:
        g.set_goal(p)
    if ref is not None:
        ref.set_goals([ALL.LR.cell_of(ref.P, p)])


@mutator("svh_grid_plan_set_goals_frontiers")
def plan_set_goals_frontiers(g, ref, rng):
    n = []
    if g is not None:
        n.append(g.set_goals_frontiers())
    if ref is not None:
        n.append(ref.set_goals_frontiers())
    assert len(set(n)) == 1, n


@mutator("svh_grid_plan_set_goal_explore")
def plan_set_goal_explore(g, ref, rng):
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    p = pos(fr, *pick(rng, L.start, [L.start, L.inside, (L.nx - 3, 2)]), h=0.0)
    n = []
    if g is not None:
        n.append(g.set_goal_explore(p))
    if ref is not None:
        n.append(ref.set_goal_explore(p))
    assert len(set(n)) == 1, n


@mutator("svh_grid_set_frontier")
def set_frontier(g, ref, rng):
    kw = pick(rng, dict(border=1, min_size=5), [dict(border=1, min_size=5), dict(border=0, min_size=8), dict(unexplored=24), dict(unexplored=8), dict(max_cell_cost=100),
                                                dict(max_cell_cost=235)])
    if g is not None:
        g.set_frontier(**kw)
    if ref is not None:
        for k, v in kw.items():
            setattr(ref.front, k, v)


@mutator("svh_grid_set_explore")
def set_explore(g, ref, rng):
    kw = pick(rng, dict(range=3.0, w_gain=100), [dict(range=3.0, w_gain=100), dict(range=4.0, w_gain=500), dict(min_gain=30), dict(min_gain=1), dict(w_reach=0)])
    if g is not None:
        g.set_explore(**kw)
    if ref is not None:
        for k, v in kw.items():
            setattr(ref.explore, k, F(v) if k == "range" else v)


@mutator("svh_grid_set_roll")
def set_roll(g, ref, rng):
    """the same headings_m: the candidates stay"""
    kw = pick(rng, dict(half_width=0.7, w_cost=3), [dict(half_width=0.7, w_cost=3), dict(half_width=0.2, w_cost=1), dict(w_pot=0), dict(w_pot=1), dict(stop_cost=200),
                                                    dict(stop_cost=253)])
    if g is not None:
        g.set_roll(**kw)
    if ref is not None:
        q = ref.roll
        old = dict(front=q.front, rear=q.rear, half_width=q.half_width, headings_m=q.headings_m, stop_cost=q.stop_cost, unknown_cost=q.unknown_cost,
                   w_pot=q.w_pot, w_cost=q.w_cost, w_cut=q.w_cut)
        ref.set_roll(RR.RollParams(**dict(old, **kw)))


@mutator("svh_grid_set_roll", "set_roll_headings")
def set_roll_headings(g, ref, rng):
    """another headings_m: "svh_grid_set_roll with another headings_m forgets the candidates, whose headings it renumbers".  The
    tables of the cases name headings below 16, so they stay valid under either enumeration"""
    m = pick(rng, 4, [4, 2])
    if g is not None:
        g.set_roll(headings_m=m)
    if ref is not None:
        q = ref.roll
        ref.set_roll(RR.RollParams(front=q.front, rear=q.rear, half_width=q.half_width, headings_m=m, stop_cost=q.stop_cost, unknown_cost=q.unknown_cost,
                                   w_pot=q.w_pot, w_cost=q.w_cost, w_cut=q.w_cut))


@mutator("svh_grid_roll_set_candidates")
def roll_set_candidates(g, ref, rng):
    L = (ref if ref is not None else g).L
    tab = L.candidates(other=pick(rng, True, [True, False]))
    if g is not None:
        g.set_candidates(tab)
    if ref is not None:
        ref.set_candidates(tab)


@mutator("svh_grid_set_align")
def set_align(g, ref, rng):
    kw = pick(rng, dict(reach=1.1, trans_n=2), [dict(reach=1.1, trans_n=2), dict(), dict(min_scan=500), dict(rot_n=0)])
    kw = dict(ALIGN_KW, **kw)
    if g is not None:
        g.set_align(g.G.default_align(**kw))
    if ref is not None:
        ref.set_align(AR.AlignParams(**kw))


def _outcome(calls):
    """runs the device call and the restated one: both refuse or neither; returns their results"""
    out, refused = [], []
    for f, errors in calls:
        try:
            out.append(f())
            refused.append(False)
        except errors:
            refused.append(True)
    assert len(set(refused)) <= 1, refused
    return out, bool(refused and refused[0])


def _errors(g):
    return (g.G.SvhError,)


@mutator("svh_grid_roll_score")
def roll_score(g, ref, rng):
    """a scoring is kept for svh_grid_render_roll: the canonical one is the scene's own, the other variants anchor elsewhere"""
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    (ia, ib), s = pick(rng, (L.anchor, 0), [(L.anchor, 0), ((L.wall + 3, 12), 1), ((4, 4), 0)])
    p = pos(fr, ia, ib, 0.0)
    calls = ([(lambda: g.roll_score(p, s), _errors(g))] if g is not None else []) + ([(lambda: ref.roll_score(p, s), (ALL.Refused,))] if ref is not None else [])
    out, _ = _outcome(calls)
    if len(out) == 2:
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2]), "roll_score"


@mutator("svh_grid_roll_score", "roll_score_elsewhere")
def roll_score_elsewhere(g, ref, rng):
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    p = pos(fr, L.wall + 3, L.nz - 5, 0.0)
    calls = ([(lambda: g.roll_score(p, 1), _errors(g))] if g is not None else []) + ([(lambda: ref.roll_score(p, 1), (ALL.Refused,))] if ref is not None else [])
    _outcome(calls)


def _align_args(g, ref, rng, elsewhere=False):
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    if elsewhere:
        return L.align_frame(fr, shift=-0.25)[::2], pos(fr, L.wall - 3, L.nz // 2 + 2)
    return L.align_frame(fr, shift=pick(rng, 0.125, [0.125, 0.25, -0.125])), pos(fr, *L.pivot)


@mutator("svh_grid_align_points")
def align_points(g, ref, rng):
    p, pivot = _align_args(g, ref, rng)
    calls = ([(lambda: g.align_points(p, pivot), _errors(g))] if g is not None else []) + ([(lambda: ref.align_points(p, pivot), (ALL.Refused,))] if ref is not None else [])
    out, _ = _outcome(calls)
    if len(out) == 2:
        assert np.array_equal(out[0], out[1]), ("align_points", out)


@mutator("svh_grid_align_points", "align_points_elsewhere")
def align_points_elsewhere(g, ref, rng):
    p, pivot = _align_args(g, ref, rng, elsewhere=True)
    calls = ([(lambda: g.align_points(p, pivot), _errors(g))] if g is not None else []) + ([(lambda: ref.align_points(p, pivot), (ALL.Refused,))] if ref is not None else [])
    _outcome(calls)


@mutator("svh_grid_align_view_lists")
def align_view_lists(g, ref, rng):
    p, pivot = _align_args(g, ref, rng, elsewhere=True)
    calls = ([(lambda: with_view([p[:4], p[4:]], lambda v: g.align_view_lists(v, 0, 2, pivot)), _errors(g))] if g is not None else [])
    calls += [(lambda: ref.align_points(p, pivot), (ALL.Refused,))] if ref is not None else []
    _outcome(calls)


@mutator("svh_grid_explore_rank")
def explore_rank(g, ref, rng):
    """a ranking leaves its counts (svh_grid_get_explore_stats) and the reach field of its start: the canonical one is the scene's"""
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    p = pos(fr, *pick(rng, L.start, [L.start, L.inside, (L.nx - 3, 3)]), h=0.0)
    if g is not None:
        g.explore_rank(p)
    if ref is not None:
        ref.explore_rank(p)


@mutator("svh_grid_explore_rank", "explore_rank_elsewhere")
def explore_rank_elsewhere(g, ref, rng):
    """from inside the closed room: nothing is reachable, no record is feasible"""
    L, fr = (ref if ref is not None else g).L, frame(g, ref)
    p = pos(fr, *L.inside, h=0.0)
    if g is not None:
        g.explore_rank(p)
    if ref is not None:
        ref.explore_rank(p)


# the calls that make up the scene itself are canonical no-ops of the matrix: it applies the *_elsewhere forms
@mutator("svh_grid_roll_score", "hand_roll")
def hand_roll(g, ref, rng):
    """the hand case's scoring: candidates that cross column 16"""
    if g is not None:
        g.roll_score(HAND_ANCHOR, 0)
    if ref is not None:
        ref.roll_score(HAND_ANCHOR, 0)


@mutator("svh_grid_clear", "emptied_with_the_goals")
def emptied_with_the_goals(g, ref, rng):
    """where the header says a failed add, observation or scroll leaves the object: the empty grid, the goals as they were"""
    L = (ref if ref is not None else g).L
    for o in (g, ref):
        if o is not None:
            o.clear()
            o.set_goals(L.goals)


SCENE_CALLS = ("roll_score", "align_points", "explore_rank")
HELPERS = ("hand_clearing", "hand_roll", "emptied_with_the_goals")
MATRIX_MUTATORS = [m for m in MUTATORS if m not in SCENE_CALLS + HELPERS]
WALK_MUTATORS = [m for m in MUTATORS if m not in HELPERS]


# ---- readers ------------------------------------------------------------------------------------------------------------------
class Reader:
    def __init__(self, name, entry, group, dev, ref, cached=False, bearing=False):
        self.name, self.entry, self.group, self.dev, self.ref, self.cached, self.bearing = name, entry, group, dev, ref, cached, bearing


READERS = {}


def reader(name, entry, group, dev, ref, **kw):
    READERS[name] = Reader(name, entry, group, dev, ref, **kw)


def B(*arrays):
    return b"|".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def ints(*values):
    return np.array(values, np.int64).tobytes()


L0 = Layout()
START_A, START_B = pos(ZERO, L0.relic[0] - 1, L0.relic[1] - 2, h=0.0), pos(ZERO, *L0.start_b, h=0.0)
RANK_START = pos(ZERO, *L0.start, h=0.0)
ANCHOR = pos(ZERO, *L0.anchor, h=0.0)
VIEWPOINT = (L0.wall - 4, L0.nz - 4)
VIEW_CELLS = np.array([VIEWPOINT, (L0.nx - 8, L0.nz - 8), (3, L0.nz - 3), (-5, 2)], np.int32)
POSES = np.array([(L0.anchor[0], L0.anchor[1], 0), (L0.wall - 2, L0.gap[0], 0), (L0.wall + 2, 10, 4), (5, 5, 7), (2, 3, 4), (L0.relic[0], L0.relic[1] - 2, 4), (0, 0, 8), (L0.nx + 3, 2, 1)], np.int32)
PATH_CELLS = np.array([(3, 3), (4, 4), (5, 4), (L0.nx + 4, 1)], np.int32)
ALIGN_PTS, ALIGN_PIVOT = L0.align_frame(ZERO, shift=0.25), pos(ZERO, L0.wall - 5, L0.nz // 2 - 1)

# the last results first: they show what the history left, before the state-bearing readers below overwrite it
reader("render_roll", "svh_grid_render_roll", "roll_last", lambda g: B(g.render_roll()), lambda r: B(r.render_roll()))
reader("render_align", "svh_grid_render_align", "align_image", lambda g: B(g.render_align()), lambda r: B(r.render_align()))
reader("align_scan", "svh_grid_get_align_scan", "align_last", lambda g: B(g.align_scan()), lambda r: B(r.align_scan()))
reader("align_volume", "svh_grid_get_align_volume", "align_last", lambda g: B(g.align_volume()), lambda r: B(r.align_volume()))
reader("explore_stats", "svh_grid_get_explore_stats", "rank_last", lambda g: ints(*g.explore_stats()[:2]), lambda r: ints(*r.rank_last))
for _k, _name in enumerate(R.PLANES):
    reader("get:" + _name, "svh_grid_get", "acc", lambda g, k=_k: B(g.plane(k)), lambda r, n=_name: B(r.planes()[n]), cached=True)
for _k in range(3):
    reader("render:%d" % _k, "svh_grid_render", "acc", lambda g, k=_k: B(g.render(k)), lambda r, k=_k: B(r.render(k)))
reader("local:PASS", "svh_grid_get_local", "pass", lambda g: B(g.local_plane(0)), lambda r: B(r.local_planes()["passed"]), cached="acc")   # a finished plane: its bytes follow the rays, its cache the accumulators
reader("local:STATE", "svh_grid_get_local", "acc", lambda g: B(g.local_plane(1)), lambda r: B(r.local_planes()["state"]), cached=True)
reader("render_local", "svh_grid_render_local", "acc", lambda g: B(g.render_local()), lambda r: B(r.render_local()))
reader("stats", "svh_grid_get_stats", "stats", lambda g: ints(*g.stats().asdict().values()), lambda r: ints(*[r.stats[k] for k in ("added", "binned", "overhead", "outside", "unplaced")]))
reader("ray_stats", "svh_grid_get_ray_stats", "rays", lambda g: ints(*g.ray_stats()), lambda r: ints(r.rays, r.ray_cells))
for _k, _name in enumerate(("flags", "dist2", "cost")):
    reader("trav:" + _name, "svh_grid_get_trav", "trav", lambda g, k=_k: B(g.trav_plane(k)), lambda r, n=_name: B(r.trav()[n]), cached=True)
reader("render_cost", "svh_grid_render_cost", "trav", lambda g: B(g.render_cost()), lambda r: B(r.render_cost()))
reader("plan:POT", "svh_grid_get_plan_plane", "plan", lambda g: B(g.plan_plane(0)), lambda r: B(r.field()["pot"]), cached=True)
reader("plan:DIR", "svh_grid_get_plan_plane", "plan", lambda g: B(g.plan_plane(1)), lambda r: B(r.field()["dir"]), cached=True)
reader("plan_stats", "svh_grid_get_plan_stats", "plan", lambda g: ints(*g.plan_stats()[:3]),
       lambda r: (lambda f: ints(len(r.goals), f["counted"], f["reached"]))(r.field()), cached=True)


def _dev_path(g, start):
    st, cells, cost = g.path(start)
    return ints(st, cost, g.path_len) + B(cells)


def _ref_path(r, start):
    st, cells, cost = r.path(start, r.field())
    return ints(st, cost, len(cells)) + B(cells)


reader("path:a", "svh_grid_plan_path", "plan", lambda g: _dev_path(g, START_A), lambda r: _ref_path(r, START_A))
reader("path:b", "svh_grid_plan_path", "plan", lambda g: _dev_path(g, START_B), lambda r: _ref_path(r, START_B))
reader("render_plan", "svh_grid_render_plan", "plan", lambda g: B(g.render_plan(PATH_CELLS)), lambda r: B(r.render_plan(PATH_CELLS, r.field())))
reader("front:FLAGS", "svh_grid_get_front_plane", "front", lambda g: B(g.front_plane(0)), lambda r: B(r.frontiers()["flags"]), cached=True)
reader("front:LABEL", "svh_grid_get_front_plane", "front", lambda g: B(g.front_plane(1)), lambda r: B(r.frontiers()["label"]), cached=True)
reader("frontiers", "svh_grid_get_frontiers", "front", lambda g: B(g.frontiers()), lambda r: B(r.frontiers()["recs"]), cached=True)
reader("frontier_stats", "svh_grid_get_frontier_stats", "front", lambda g: ints(*g.frontier_stats()[:4]), lambda r: ints(*r.frontiers()["stats"]), cached=True)
reader("render_frontiers", "svh_grid_render_frontiers", "front", lambda g: B(g.render_frontiers()), lambda r: B(r.render_frontiers()))
reader("candidates", "svh_grid_roll_get_candidates", "cands", lambda g: ints(*g.candidates()), lambda r: ints(*(r.cands.shape[:3] if r.cands is not None else (0, 0, 0))))
reader("footprint_cost", "svh_grid_footprint_cost", "foot", lambda g: B(g.footprint_cost(POSES)), lambda r: B(r.footprint_cost(POSES)))
reader("view_gain", "svh_grid_view_gain", "view", lambda g: B(g.view_gain(VIEW_CELLS)), lambda r: B(r.view_gain(VIEW_CELLS)))
reader("view_mask", "svh_grid_view_mask", "view", lambda g: B(g.view_mask(*VIEWPOINT)), lambda r: B(r.view_mask(*VIEWPOINT)))
reader("render_view", "svh_grid_render_view", "front_view", lambda g: B(g.render_view(*VIEWPOINT)), lambda r: B(r.render_view(*VIEWPOINT)))
reader("align_field", "svh_grid_get_align_field", "afield", lambda g: B(g.align_field()), lambda r: B(r.align_field()), cached=True)
for _k, _name in enumerate(("age", "contra", "through")):
    reader("dyn:" + _name, "svh_grid_get_dyn", "dyn", lambda g, k=_k: B(g.dyn_plane(k)), lambda r, n=_name: B(r.dyn_planes()[n]))
reader("dyn_stats", "svh_grid_get_dyn_stats", "dyn_stats", lambda g: ints(*g.dyn_stats().values()), lambda r: ints(*[r.dyn_stats[k] for k in DR.STATS]))
reader("render_dyn", "svh_grid_render_dyn", "dyn_image", lambda g: B(g.render_dyn()), lambda r: B(r.render_dyn()))


def _triple(t):
    best, recs, scores = t
    return ints(best) + B(recs, scores)


# the state-bearing readers last: each leaves a last result, so the harness logs them as part of the history
reader("roll_score", "svh_grid_roll_score", "score", lambda g: _triple(g.roll_score(ANCHOR, 0)), lambda r: _triple(r.roll_score(ANCHOR, 0)), bearing=True)
reader("explore_rank", "svh_grid_explore_rank", "rank", lambda g: _triple(g.explore_rank(RANK_START)), lambda r: _triple(r.explore_rank(RANK_START)), bearing=True)


def _dev_align(g):
    rec = g.align_points(ALIGN_PTS, ALIGN_PIVOT)
    return B(rec, g.align_scan()) + (B(g.align_volume()) if rec[0] != AR.FEW else b"")


def _ref_align(r):
    rec = r.align_points(ALIGN_PTS, ALIGN_PIVOT)
    return B(rec, r.align_scan()) + (B(r.align_volume()) if rec[0] != AR.FEW else b"")


reader("align_points", "svh_grid_align_points", "align", _dev_align, _ref_align, bearing=True)


def served_from_cache(m, name):
    """whether the documented rule says that mutator m leaves the cache that reader `name` is served from: such a read needs no launch"""
    r = READERS[name]
    cache = r.group if r.cached is True else r.cached
    return bool(cache) and cache not in RULES[m][0] | RULES[m][1]


def read_dev(g, name):
    try:
        return READERS[name].dev(g)
    except g.G.SvhError as e:
        assert e.code == BAD_ARG, (name, e.code, str(e))
        return REFUSED


def read_ref(ref, name):
    try:
        return READERS[name].ref(ref)
    except ALL.Refused:
        return REFUSED


# ---- what the header says -----------------------------------------------------------------------------------------------------
# the state a group of readers is a function of
GROUPS = {
    "acc": "the accumulators and the window's offsets",
    "pass": "the PASS plane: the rays of the _from entries and of the observations",
    "stats": "the point statistics since the last clear",
    "rays": "the ray statistics since the last clear",
    "trav": "acc, the traversability parameters",
    "plan": "trav, the plan parameters, the goals",
    "front": "trav, the frontier parameters",
    "view": "acc, the frontier parameters' unexplored mask, the exploration range",
    "front_view": "front, view",
    "rank": "front, view, the reach field (trav, the plan parameters, the start), the exploration parameters",
    "rank_last": "the counts of the last ranking",
    "foot": "trav, the rollout parameters",
    "cands": "the sizes of the candidate table",
    "score": "foot, plan (w_pot > 0), the candidates",
    "roll_last": "trav drawn under the cells of the last scoring",
    "afield": "acc, the align parameters",
    "align": "afield, the align parameters, the frame",
    "align_last": "the scan and the volume of the last alignment",
    "align_image": "acc drawn under the scan of the last alignment",
    "dyn": "CONTRA, LAST and THROUGH of the cells, the stamp",
    "dyn_stats": "the statistics of the layer since the last clear",
    "dyn_image": "acc, dyn, the events of the last observation",
}
_ACC = {"acc", "trav", "plan", "front", "view", "front_view", "rank", "foot", "score", "roll_last", "afield", "align", "align_image", "dyn_image"}
_TRAV = {"trav", "plan", "front", "front_view", "rank", "foot", "score", "roll_last"}
_PLAN = {"plan", "score"}
_ADD = _ACC | {"stats"}
_RAYS = {"pass", "rays"}
_EMPTY = _ACC | _RAYS | {"stats", "dyn", "dyn_stats"}
# mutator -> (groups whose readers CHANGE, groups whose readers REFUSE); every other group KEEPS
RULES = {
    "clear": (_EMPTY, set()),                         # "forgotten by svh_grid_clear"; the last scan and the roll tables survive
    "set_window": (_EMPTY, set()),
    "scroll": (_ACC | {"pass", "dyn"}, set()),                # "the statistics go on counting"; CONTRA and LAST travel with their cells
    "follow": (_ACC | {"pass", "dyn"}, set()),
    "add_points": (_ADD, set()),                      # "leave CONTRA and LAST alone"
    "add_points_device": (_ADD, set()),
    "add_view": (_ADD, set()),
    "add_points_from": (_ADD | _RAYS, set()),
    "add_view_lists_from": (_ADD | _RAYS, set()),
    "observe_points": (_ADD | _RAYS | {"dyn", "dyn_stats"}, set()),   # "an observation invalidates what an add invalidates"
    "observe_view_lists": (_ADD | _RAYS | {"dyn", "dyn_stats"}, set()),
    "observe_empty": (_ACC | {"dyn", "dyn_stats"}, set()),            # no point, no ray: it ages
    "set_dynamics_change": (set(), set()),            # "new parameters keep CONTRA and LAST"
    "set_dynamics_drop": (set(), {"dyn", "dyn_image"}),
    "set_dynamics_again": ({"dyn", "dyn_image"}, set()),              # "starts from empty planes (the stamp goes on)"
    "set_traversability": (_TRAV, set()),
    "set_plan": (_PLAN | {"rank"}, set()),            # the reach field shares the plan parameters; the frontiers do not
    "plan_set_goals": (_PLAN, set()),
    "plan_set_goal": (_PLAN, set()),
    "plan_set_goals_frontiers": (_PLAN, set()),
    "plan_set_goal_explore": (_PLAN, set()),          # "the planner's goals": a ranking from the scene's start leaves the scene's counts
    "set_frontier": ({"front", "front_view", "rank"}, set()),         # border and min_size: the unexplored mask stays
    "set_explore": ({"view", "front_view", "rank"}, set()),           # nothing cached depends on them; the per-call outputs do
    "set_roll": ({"foot", "score"}, {"roll_last"}),   # "nothing was scored since the tables were set"
    "set_roll_headings": ({"foot", "cands"}, {"score", "roll_last"}),   # "forgets the candidates": "SVH_ERR_BAD_ARG: no candidates"
    "roll_set_candidates": ({"cands", "score"}, {"roll_last"}),
    "set_align": ({"afield", "align"}, {"align_last", "align_image"}),   # "a success forgets the last alignment"
    "roll_score_elsewhere": ({"roll_last"}, set()),
    "align_points_elsewhere": ({"align_last", "align_image"}, set()),
    "align_view_lists": ({"align_last", "align_image"}, set()),
    "explore_rank_elsewhere": ({"rank_last"}, set()),
}
EXPECT = {m: {r: (REFUSES if READERS[r].group in RULES[m][1] else CHANGES if READERS[r].group in RULES[m][0] else KEEPS) for r in READERS}
          for m in MATRIX_MUTATORS}
# CHANGES pairs the scene cannot show at this size, each with its reason; at most 5 % of the CHANGES pairs
UNSHOWN = {
    ("observe_empty", "dyn:contra"): "a frame without points casts no line, and the cells it ages stood at CONTRA 0",
    ("observe_empty", "path:b"): "what ages lies on the other side of the wall from this start and its goals",
    ("set_traversability", "trav:flags"): "the canonical change is the inscribed radius: it moves the cost table alone (and keeps its size)",
    ("set_traversability", "trav:dist2"): "as above",
    ("set_traversability", "plan:DIR"): "the costs beside the obstacles rise and no cheapest step turns",
    ("set_traversability", "plan_stats"): "no cell becomes impassable: the same goals count and the same cells are reached",
    ("set_plan", "render_plan"): "the image draws the goals that count and the given cells over COST: no goal lies on a cell of COST 255",
}

# ---- every entry of the header --------------------------------------------------------------------------------------------------
NEITHER = {
    "svh_grid_params_default", "svh_grid_trav_params_default", "svh_grid_plan_params_default", "svh_grid_front_params_default",
    "svh_grid_roll_params_default", "svh_grid_explore_params_default", "svh_grid_align_params_default", "svh_grid_dyn_params_default",
    "svh_grid_create", "svh_grid_destroy", "svh_grid_frame_camera", "svh_grid_frame_plane", "svh_grid_cell_of", "svh_grid_heading_of",
    # getters of parameters and of what is derived from them alone
    "svh_grid_get_window", "svh_grid_get_traversability", "svh_grid_get_plan", "svh_grid_get_frontier", "svh_grid_get_roll", "svh_grid_roll_footprint",
    "svh_grid_get_explore", "svh_grid_get_dynamics", "svh_grid_align_correction",
}


def classified():
    """entry -> set of roles"""
    out = {e: {"neither"} for e in NEITHER}
    for e in MUTATOR_ENTRY.values():
        out.setdefault(e, set()).add("mutator")
    for r in READERS.values():
        out.setdefault(r.entry, set()).add("reader")
    return out


def matrix_table():
    """the EXPECT matrix as the lines of a markdown table: a row per mutator, a column per group of readers"""
    groups = list(GROUPS)
    mark = {CHANGES: "C", KEEPS: "·", REFUSES: "R"}
    lines = ["| mutator | " + " | ".join(groups) + " |", "|---|" + "---|" * len(groups)]
    for m in MATRIX_MUTATORS:
        cells = []
        for gname in groups:
            kinds = {EXPECT[m][r] for r in READERS if READERS[r].group == gname}
            assert len(kinds) == 1, (m, gname, kinds)
            cells.append(mark[kinds.pop()])
        lines.append("| `%s` | " % m + " | ".join(cells) + " |")
    return lines


# ---- the harness --------------------------------------------------------------------------------------------------------------
class Rig:
    """an object and the restatement under one history: every state-bearing call is logged, so that `fresh` can replay it on a
    new object that is never read in between"""

    def __init__(self, G, hip, nx=NX, nz=NZ, setup=scene):
        self.G, self.hip, self.nx, self.nz, self.setup = G, hip, nx, nz, setup
        self.g, self.ref, self.log = self.make(), new_ref(nx, nz), []
        setup(self.g, self.ref)

    def make(self):
        g = new_object(self.G, self.nx, self.nz)
        g.G, g.hip = self.G, self.hip
        return g

    def apply(self, name, seed=None):
        """the mutator on the object, then on the restatement: both take it or both refuse it"""
        self.log.append(("mutate", name, seed))
        refused = []
        for g, ref, errors in ((self.g, None, (self.G.SvhError,)), (None, self.ref, (ALL.Refused, ValueError))):
            try:
                MUTATORS[name](g, ref, None if seed is None else np.random.default_rng(seed))
                refused.append(False)
            except errors as e:
                assert ref is not None or e.code == BAD_ARG, (name, e.code, str(e))
                refused.append(True)
        assert refused[0] == refused[1], (name, seed, refused)
        return refused[0]

    def read(self, name):
        """(the object's bytes, the restatement's)"""
        if READERS[name].bearing:
            self.log.append(("read", name, None))
        return read_dev(self.g, name), read_ref(self.ref, name)

    def read_all(self, names=None):
        """a read-out: every reader in the order of READERS (or `names`); `fresh` replays the history up to its beginning"""
        self.upto = len(self.log)
        with self.ref.frozen():
            return {n: self.read(n) for n in (names or READERS)}

    def fresh(self):
        """a new object with the history up to the last read-out and no other read: it is to be read as that read-out read"""
        g = self.make()
        self.setup(g, None)
        for kind, name, seed in self.log[:self.upto]:
            if kind == "mutate":
                try:
                    MUTATORS[name](g, None, None if seed is None else np.random.default_rng(seed))
                except self.G.SvhError as e:               # the same refusal the warm object gave
                    assert e.code == BAD_ARG, (name, e.code)
            else:
                read_dev(g, name)
        return g

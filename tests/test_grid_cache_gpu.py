"""GPU: the part of the ground grid's engine that decides whether a kernel runs at all (stereo-vision_amd/csrc/grid_engine.cpp: the
`valid` mask of six derived layers, four uploads and two last results with its table of needs and drops, and `body_valid`) pinned
from outside, against the tables of tests/grid_cache_cases.py, which tests/test_grid_cache.py pins on the CPU.

The rule under test: a read through a cache is indistinguishable from a read computed from the state as it is.  So every test keeps
three things under one history of state-changing calls: `warm`, an object that was read in between; `fresh`, a new object that
replays the history and is read once, at the end; and the composed restatement tests/grid_all_ref.py, which caches nothing.  Every
comparison is of bytes and exact.  A stale read returns plausible bytes and no error: warm differs from fresh.

Every window is the scene's (2 T + 1) x (T + 1) = 33 x 17, T = PLAN_TILE = FRONT_TILE = 16 -- a partial tile and a tile border in every
tiled layer -- but for the second seeded walk on 65 x 65."""
import ctypes as C

import numpy as np
import pytest

import grid_cache_cases as CC
import helpers as H   # puts the package on the path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import svhip
    from svhip import grid
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    grid._bind()
    assert grid.PLAN_TILE == grid.FRONT_TILE == CC.T
    return grid


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(autouse=True)
def restore(G):
    yield
    G.lib().svh_test_fail_at(None)


def agree(tag, reads):
    """every reader: the object's bytes are the restatement's"""
    bad = [n for n, (dev, ref) in reads.items() if dev != ref]
    assert not bad, "%s: the object and the restatement differ on %s" % (tag, bad)


def same_as_fresh(tag, rig, reads):
    """a new object with the same history, read once: byte for byte what the warm one returned"""
    fresh = rig.fresh()
    got = {n: CC.read_dev(fresh, n) for n in reads}
    bad = [n for n in reads if got[n] != reads[n][0]]
    assert not bad, "%s: the object that was read in between and a fresh one with the same history differ on %s" % (tag, bad)
    fresh.close()


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", CC.MATRIX_MUTATORS)
def test_matrix(G, hip, m):
    rig = CC.Rig(G, hip)
    agree("the scene", rig.read_all())
    before = rig.read_all()                                             # every cache is valid; the last results are the readers' own
    agree("the scene, read again", before)
    assert not rig.apply(m), "the scene takes every canonical mutator"
    # KEEPS: the documented rule says this cache survives, so the read is served without a launch
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n, r in CC.READERS.items():
        if CC.served_from_cache(m, n):
            try:
                got = r.dev(rig.g)
            except G.SvhError as e:
                raise AssertionError("%s keeps %s by the documented rule, yet the read launched a kernel (%s)" % (m, n, e))
            assert got == before[n][0], (m, n, "kept, but other bytes")
    G.lib().svh_test_fail_at(None)
    after = rig.read_all()
    agree("after " + m, after)
    same_as_fresh("after " + m, rig, after)
    for n in CC.READERS:
        want = CC.EXPECT[m][n]
        if want == CC.REFUSES:
            assert after[n][0] == CC.REFUSED, (m, n)                    # read_dev has checked the code: SVH_ERR_BAD_ARG
        elif want == CC.KEEPS:
            assert after[n][0] == before[n][0], (m, n, "the documented rule says this output stays")
        elif (m, n) not in CC.UNSHOWN:
            assert after[n][0] != before[n][0] and after[n][0] != CC.REFUSED, (m, n, "this output was to change")
    rig.g.close()


@pytest.mark.parametrize("n", [n for n, r in CC.READERS.items() if r.cached])
def test_a_getter_keeps_what_it_computed(G, hip, n):
    """After a plain add every derived plane is stale and this getter is the first entry to find it so: it computes what it returns.
    The same read again, under the simulated error launch:1:0, must then be served without a launch, with the same bytes.  The
    matrix cannot see a getter that computes and forgets to say so: every read-out of it starts with svh_grid_render_roll, which
    makes COST and the finished planes valid for all that follow, and a second computation returns the same bytes."""
    rig = CC.Rig(G, hip)
    assert not rig.apply("add_points")
    first = CC.READERS[n].dev(rig.g)
    G.lib().svh_test_fail_at(b"launch:1:0")
    try:
        again = CC.READERS[n].dev(rig.g)
    except G.SvhError as e:
        raise AssertionError("%s computed its planes and did not keep them: the second read launched a kernel (%s)" % (n, e))
    G.lib().svh_test_fail_at(None)
    assert again == first, n
    rig.g.close()


# ---- read order ------------------------------------------------------------------------------------------------------------------
LAST = [n for n in CC.READERS][:5]
REST = [n for n in CC.READERS if n not in LAST]


def orders():
    """The FIRST read after the mutator finds every derived plane stale, so it is what differs between the orders: lowest layer
    first; svh_grid_explore_rank first, which needs the frontiers, the reach field, COST and the finished planes at once; the
    planner, the frontiers, a scoring and the alignment field first, each of which settles several layers in one call; three seeded
    permutations.  The readers of a last result (svh_grid_render_roll and svh_grid_render_align among them, which would make COST
    and the finished planes valid before anything else ran) come LAST in every order, after the three state-bearing readers have
    all run: then they show the same scoring, ranking and alignment whatever the order was"""
    low = ["local:STATE", "local:PASS", "trav:cost", "plan:POT", "front:LABEL", "explore_rank", "align_field"]
    high = ["explore_rank", "roll_score", "align_points", "render_view", "front:LABEL", "plan:POT", "trav:cost", "local:STATE"]
    out = [("lowest first", low + [n for n in REST if n not in low]), ("highest first", high + [n for n in reversed(REST) if n not in high])]
    for head in ("plan:POT", "frontiers", "roll_score", "align_field"):
        out.append((head + " first", [head] + [n for n in REST if n != head]))
    for seed in (1, 2, 3):
        out.append(("permutation %d" % seed, [REST[k] for k in np.random.default_rng(seed).permutation(len(REST))]))
    for tag, names in out:
        assert names[0] not in LAST and not set(names) & set(LAST)
    assert out[1][1][0] == "explore_rank" and len({names[0] for _, names in out}) >= 7
    return [(tag, names + LAST) for tag, names in out]


@pytest.mark.parametrize("m", ["observe_points", "scroll", "set_traversability", "add_points_from"])
def test_read_order(G, hip, m):
    first = None
    for tag, names in orders():
        assert sorted(names) == sorted(CC.READERS)
        rig = CC.Rig(G, hip)
        rig.read_all()
        rig.apply(m)
        if first is None:                                               # once against the restatement
            reads = rig.read_all(names)
            agree("%s, %s" % (m, tag), reads)
            first = {n: reads[n][0] for n in names}
        else:
            got = {n: CC.read_dev(rig.g, n) for n in names}
            bad = [n for n in names if got[n] != first[n]]
            assert not bad, "%s, read %s: %s differ from the first order" % (m, tag, bad)
        rig.g.close()


# ---- the hand case ---------------------------------------------------------------------------------------------------------------
def test_a_cleared_obstacle_opens_the_route(G, hip):
    rig = CC.Rig(G, hip, setup=CC.hand_scene)
    g, ref = rig.g, rig.ref
    start = CC.pos(CC.ZERO, *CC.HAND_START, h=0.0)
    before = rig.read_all()                                             # COST, POT, DIR, the frontier table, the ranking, the alignment field
    agree("before the clearing observation", before)
    cost = g.trav_plane(G.TRAV_COST)
    assert g.plan_stats()[2] == CC.HAND["reached"] and g.path(start)[::2] == (G.PATH_UNREACHABLE, G.PLAN_FAR)
    assert g.plan_plane(G.PLAN_POT)[CC.HAND_START[1], CC.HAND_START[0]] == G.PLAN_FAR
    rig.apply("hand_roll")                                              # candidates that cross column 16; the scoring is part of the history
    _, recs, _ = g.roll_score(CC.HAND_ANCHOR, 0)
    assert np.array_equal(recs, ref.roll_score(CC.HAND_ANCHOR, 0)[1]) and recs[:, 1].tolist() == [0, 1, 1] and (recs[:, 4] == G.PLAN_FAR).all()
    rig.apply("hand_clearing")
    after = rig.read_all()
    agree("after the clearing observation", after)
    same_as_fresh("after the clearing observation", rig, after)
    assert g.dyn_stats()["cleared"] == CC.HAND["cleared"]
    assert int((g.trav_plane(G.TRAV_COST) != cost).sum()) == CC.HAND["cost_bytes"]
    st, cells, c = g.path(start)
    assert st == G.PATH_FOUND and c == CC.HAND["pot_after"] == 19662 and tuple(cells[-1]) == CC.HAND_GOAL and g.plan_stats()[2] == CC.HAND["reached_after"]
    assert np.array_equal(cells, ref.path(start)[1])
    for n in ("trav:cost", "plan:POT", "plan:DIR", "plan_stats", "path:a", "roll_score", "align_field", "render_cost"):
        assert after[n][0] != before[n][0], (n, "the cleared obstacle does not show")
    _, recs, _ = g.roll_score(CC.HAND_ANCHOR, 0)
    assert np.array_equal(recs, ref.roll_score(CC.HAND_ANCHOR, 0)[1]) and (recs[:, 4] != G.PLAN_FAR).all()
    g.close()


# ---- a seeded walk ---------------------------------------------------------------------------------------------------------------
WALK = [m for m in CC.WALK_MUTATORS for _ in range(1 if m in ("clear", "set_window") else 4)]   # an empty grid shows little: seldom


@pytest.mark.parametrize("seed,nx,nz,steps", [(11, CC.NX, CC.NZ, 40), (12, 65, 65, 25)])
def test_a_seeded_walk(G, hip, seed, nx, nz, steps):
    rng = np.random.default_rng(seed)
    rig = CC.Rig(G, hip, nx, nz)
    names = list(CC.READERS)
    checkpoints = set(int(k) for k in np.linspace(steps // 6, steps - 1, 6))
    for step in range(steps):
        m, s = WALK[int(rng.integers(len(WALK)))], int(rng.integers(2 ** 31))
        tag = "seed %d, step %d (%s, %d)" % (seed, step, m, s)
        try:
            rig.apply(m, s)
            for k in rng.permutation(len(names))[:int(rng.integers(0, 7))]:   # a random subset, possibly empty, in a random order
                dev, ref = rig.read(names[k])
                assert dev == ref, "the object and the restatement differ on %s" % names[k]
            if step in checkpoints:
                reads = rig.read_all()
                agree("checkpoint", reads)
                same_as_fresh("checkpoint", rig, reads)
        except Exception as e:                                          # whatever fails, an error code of the library included
            raise AssertionError("%s: %s: %s" % (tag, type(e).__name__, e)) from e
    rig.g.close()


# ---- the last results --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ["scroll", "add_points", "observe_points", "set_traversability", "set_plan", "set_roll", "roll_set_candidates", "set_align", "clear"])
def test_last_results_after_a_mutator(G, hip, m):
    """svh_grid_render_roll, svh_grid_render_align, svh_grid_get_align_scan and svh_grid_get_align_volume show the scene's own scoring and
    alignment over the planes as the mutator left them, or refuse as the header says"""
    rig = CC.Rig(G, hip)
    quiet = [n for n in CC.READERS if not CC.READERS[n].bearing]
    before = rig.read_all(quiet)                                        # every cache warm; the last results are the history's
    agree("the scene", before)
    rig.apply(m)
    reads = rig.read_all(LAST)
    agree("after " + m, reads)
    same_as_fresh("after " + m, rig, reads)
    for n in LAST:
        want = CC.EXPECT[m][n]
        assert (reads[n][0] == CC.REFUSED) == (want == CC.REFUSES), (m, n)
        if want == CC.KEEPS:
            assert reads[n][0] == before[n][0], (m, n)
    if m in ("scroll", "add_points", "observe_points", "set_traversability", "clear"):
        assert reads["render_roll"][0] != before["render_roll"][0]      # the old cells over the new cost planes
    rig.g.close()


# ---- failures with every cache warm ----------------------------------------------------------------------------------------------
# mutator -> (the guarded call that fails, what a fresh object does to reach the documented state after the failure)
FAILURES = {
    "scroll": (b"launch:1", ["emptied_with_the_goals", "scroll"]),            # "the grid is EMPTY ... the window stands at its new offsets"
    "add_points": (b"launch:1", ["emptied_with_the_goals"]),                  # "the grid is EMPTY ... all statistics are zero"
    "observe_points": (b"launch:1", ["emptied_with_the_goals"]),              # "EMPTY as after a failed add: statistics, stamp, CONTRA and LAST included"
    "set_traversability": (b"copy:1", ["set_traversability"]),                # "the parameters are set and the next svh_grid_get_trav ... uploads the table again"
    "set_roll": (b"copy:1", ["set_roll"]),                                    # "the parameters are set and the next call that needs the table uploads it again"
    "roll_set_candidates": (b"copy:1", ["roll_set_candidates"]),              # "the table is set and the next svh_grid_roll_score uploads it again"
}


@pytest.mark.parametrize("m", list(FAILURES))
def test_a_failed_mutator_with_every_cache_warm(G, hip, m):
    spec, then = FAILURES[m]
    rig = CC.Rig(G, hip)
    agree("the scene", rig.read_all())
    G.lib().svh_test_fail_at(spec)
    with pytest.raises(G.SvhError) as e:
        CC.MUTATORS[m](rig.g, None, None)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == CC.HIP_ERR
    for name in then:                                                   # the restatement and the log go where the header says the object is
        CC.MUTATORS[name](None, rig.ref, None)
        rig.log.append(("mutate", name, None))
    reads = rig.read_all()
    agree("after a failed " + m, reads)
    same_as_fresh("after a failed " + m, rig, reads)
    rig.g.close()

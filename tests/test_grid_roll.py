"""CPU: the contract of the ground grid's rollouts (include/svh_grid.h, "ROLLOUT": svh_grid_set_roll, svh_grid_heading_of,
svh_grid_roll_footprint, svh_grid_footprint_cost, svh_grid_roll_set_candidates, svh_grid_roll_score, svh_grid_render_roll).
tests/grid_roll_ref.py restates stereo-vision_amd/csrc/grid_roll_core.h in numpy and plain Python; this file pins the restatement
with cases derived by hand, compares the header itself with it -- evaluated on the host by the library's test entries
svh_test_grid_roll, svh_test_grid_roll_table and svh_test_grid_roll_heading, and once more as a program of its own under the
address and undefined-behaviour sanitizers --, and checks what needs no device: the refusals, the exports, the C99 header and the
candidate builder arc_candidates.  Every comparison is exact.

tests/test_grid_roll_gpu.py compares the device with the same header and restatement.

Planes are indexed [ib, ia]; a pose is (ga, gb, k)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_roll_ref as RR
import helpers as H

FAR, INF = RR.FAR, RR.INFEASIBLE
POINT = dict(front=0.0, rear=0.0, half_width=0.0)


@pytest.fixture(scope="module")
def G():
    from svhip import grid
    grid._bind()
    return grid


def both(G, **kw):
    """the restatement's parameters and the library's"""
    return RR.RollParams(**kw), G.default_roll(**kw)


def same_lists(got, want, tag=""):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == np.int32 and np.array_equal(g, w), (tag, k, g.tolist()[:6], w.tolist()[:6])


def agree(G, cost, table, anchor=(0, 0), pot=None, cell=1.0, oa=0, ob=0, set_=0, poses=None, tag="", **kw):
    """the restatement and the header on the same planes and table: records, scores, best and F; returns the restatement's"""
    p, q = both(G, **kw)
    cost = np.asarray(cost, np.uint8)
    table = np.asarray(table, np.int32)
    R, lists = RR.table(p, cell)
    want = RR.score(p, lists, cost, pot, table[set_], anchor, oa, ob)
    got = G.core_roll(q, cell, cost, pot, table, set_, anchor, oa, ob, poses)
    for name, w in zip(("recs", "scores"), want):
        assert got[name].dtype == w.dtype and np.array_equal(got[name], w), (tag, name, got[name].tolist()[:8], w.tolist()[:8])
    assert got["best"] == want[2], (tag, got["best"], want[2])
    if poses is not None:
        f = RR.footprint_costs(p, lists, cost, poses, oa, ob)
        assert np.array_equal(got["f"], f), (tag, got["f"].tolist()[:8], f.tolist()[:8])
        return want + (f,)
    return want


# ---- the headings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 8, 32])
def test_the_enumeration_of_the_headings(G, m):
    seen = set()
    for k in range(8 * m):
        ux, uz = RR.heading_vec(m, k)
        assert max(abs(ux), abs(uz)) == m and (ux, uz) not in seen                   # on the perimeter, each once
        seen.add((ux, uz))
        for scale in (1.0, 0.37, 1e-20, 3e30):                                       # every perimeter vector maps to its own k
            assert RR.heading_of(m, ux * scale, uz * scale) == k, (k, scale)
            assert G.core_heading(m, ux * scale, uz * scale) == (k, (ux, uz)), (k, scale)
        nxt = RR.heading_vec(m, (k + 1) % (8 * m))                                   # counter-clockwise: the cross product is positive
        assert ux * nxt[1] - uz * nxt[0] > 0
    assert RR.heading_vec(m, 0) == (m, 0) and RR.heading_vec(m, 2 * m) == (0, m)      # straight ahead is 2 m
    assert RR.heading_of(m, m, m) == m and RR.heading_of(m, -m, m) == 3 * m           # the corners
    assert RR.heading_of(m, -m, -m) == 5 * m and RR.heading_of(m, m, -m) == 7 * m
    assert np.array_equal(G.heading_vectors(m), np.array([RR.heading_vec(m, k) for k in range(8 * m)]))
    ks = np.arange(8 * m)
    v = G.heading_vectors(m)
    assert np.array_equal(G.headings_of(m, v[:, 0], v[:, 1]), ks)


@pytest.mark.parametrize("m", [1, 2, 8, 32])
def test_a_direction_halfway_between_two_headings_follows_rintf(G, m):
    H8 = 8 * m
    for j in range(m):                                                               # (m, j + 0.5): the quotient is exactly j + 0.5
        even = j if j % 2 == 0 else j + 1                                            # rintf rounds a half to the even integer
        for (ua, ub), want in (((m, j + 0.5), even), ((m, -(j + 0.5)), (H8 - even) % H8), ((-m, j + 0.5), 4 * m - even), ((-m, -(j + 0.5)), 4 * m + even),
                               ((j + 0.5, m), 2 * m - even), ((-(j + 0.5), m), 2 * m + even), ((j + 0.5, -m), 6 * m + even), ((-(j + 0.5), -m), 6 * m - even)):
            assert RR.heading_of(m, ua, ub) == want, (ua, ub)
            assert G.core_heading(m, ua, ub)[0] == want, (ua, ub)
            assert G.headings_of(m, ua, ub) == want, (ua, ub)


def test_directions_without_a_heading(G):
    nan, inf = float("nan"), float("inf")
    for m in (1, 8, 32):
        for ua, ub in ((0.0, 0.0), (-0.0, 0.0), (nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, -inf), (inf, inf)) + (((3e38, 3e38),) if m > 1 else ()):   # the last: ub * m overflows
            assert RR.heading_of(m, ua, ub) == -1 and G.core_heading(m, ua, ub) == (-1, None) and G.headings_of(m, ua, ub) == -1, (m, ua, ub)
    assert RR.heading_of(1, 3e38, 3e38) == 1 and G.core_heading(1, 3e38, 3e38) == (1, (1, 1))
    rng = np.random.default_rng(3)
    for m in (1, 2, 8, 32):                                                          # random directions, denormals and huge values among them
        d = (rng.standard_normal((300, 2)) * 10.0 ** rng.integers(-44, 38, (300, 1))).astype(np.float32)
        want = [RR.heading_of(m, a, b) for a, b in d]
        assert [G.core_heading(m, a, b)[0] for a, b in d] == want and G.headings_of(m, d[:, 0], d[:, 1]).tolist() == want
    L = G._bind()
    k = C.c_int32(-7)
    for m in (0, 33, -1):
        assert L.svh_test_grid_roll_heading(m, 1.0, 0.0, C.addressof(k), None) == -1 and k.value == -7


# ---- the footprint table -------------------------------------------------------------------------------------------------
def test_a_point_vehicle_is_one_cell_at_every_heading(G):
    for m in (1, 8, 32):
        for cell in (0.05, 0.2, 1.0, 7.5):
            p, q = both(G, headings_m=m, **POINT)
            R, lists = G.core_roll_table(cell, q)
            assert R == 1 == RR.reach_of(p, cell) and len(lists) == 8 * m and all(l.tolist() == [[0, 0]] for l in lists)
            same_lists(lists, RR.table(p, cell)[1])


def test_a_vehicle_of_no_width_and_one_cell(G):
    """cells of 1 m, m = 1: headings 0, 1, 2 are (1, 0), (1, 1), (0, 1).  h = 0.5.  front 1: along (1, 0) l = da <= 1.5, -l <= 0.5,
    |db| <= 0.5: (0, 0), (1, 0).  Along (1, 1), rt = sqrt 2: l = da + db in 0..2 (2.12), t = db - da = 0 (0.707): (0, 0), (1, 1).  front
    0.5: l <= 1 along (1, 0) -- da = 1 lies exactly on the bound and is in; along (1, 1) l <= 1.41 with t = 0 leaves (0, 0) alone"""
    for front, want in ((1.0, {0: [[0, 0], [1, 0]], 1: [[0, 0], [1, 1]], 2: [[0, 0], [0, 1]], 3: [[0, 0], [-1, 1]], 4: [[-1, 0], [0, 0]], 5: [[-1, -1], [0, 0]],
                               6: [[0, -1], [0, 0]], 7: [[1, -1], [0, 0]]}),
                        (0.5, {0: [[0, 0], [1, 0]], 1: [[0, 0]], 2: [[0, 0], [0, 1]], 3: [[0, 0]], 4: [[-1, 0], [0, 0]], 5: [[0, 0]], 6: [[0, -1], [0, 0]], 7: [[0, 0]]})):
        p, q = both(G, front=front, rear=0.0, half_width=0.0, headings_m=1)
        R, lists = G.core_roll_table(1.0, q)
        assert R == 2 and {k: l.tolist() for k, l in enumerate(lists)} == want, front
        same_lists(lists, RR.table(p, 1.0)[1])
    # the bound of the rear and of the width, exactly: rear 0.5 admits l = -1, half_width 0.5 admits |t| = 1
    p, q = both(G, front=0.0, rear=0.5, half_width=0.5, headings_m=1)
    R, lists = G.core_roll_table(1.0, q)
    assert lists[0].tolist() == [[-1, -1], [0, -1], [-1, 0], [0, 0], [-1, 1], [0, 1]] and lists[2].tolist() == [[-1, -1], [0, -1], [1, -1], [-1, 0], [0, 0], [1, 0]]
    same_lists(lists, RR.table(p, 1.0)[1])


def test_the_symmetry_of_the_table(G):
    """heading k + 4 m is the vehicle turned round: its list is the negated list of k, and it is the list of k itself once front and
    rear are swapped"""
    for m, cell, front, rear, hw in ((1, 0.2, 1.3, 0.4, 0.5), (8, 0.2, 3.5, 1.0, 0.9), (2, 0.5, 0.0, 2.2, 0.3), (32, 0.3, 1.0, 0.2, 0.6)):
        _, a = G.core_roll_table(cell, G.default_roll(front=front, rear=rear, half_width=hw, headings_m=m))
        _, b = G.core_roll_table(cell, G.default_roll(front=rear, rear=front, half_width=hw, headings_m=m))
        for k in range(8 * m):
            neg = -a[k]
            neg = neg[np.lexsort((neg[:, 0], neg[:, 1]))]
            assert np.array_equal(a[(k + 4 * m) % (8 * m)], neg), (m, k)
            assert np.array_equal(b[(k + 4 * m) % (8 * m)], a[k]), (m, k)
            assert [0, 0] in a[k].tolist()
            assert np.array_equal(a[k], a[k][np.lexsort((a[k][:, 0], a[k][:, 1]))]) and len(np.unique(a[k], axis=0)) == len(a[k])


def test_the_reach_at_its_limits(G):
    """R = ceil((max(front, rear) + half_width + c) / c): 1 for the point vehicle, 128 for 127 cells of length, 129 for half a cell more.
    R = 0 cannot be reached through the parameters -- (0 + c) / c is 1 -- so the refusal below 1 is that of a cell side that is not
    positive"""
    L = G._bind()
    R = C.c_int32(-7)

    def table(cell, **kw):
        q = G.default_roll(headings_m=1, **kw)
        return L.svh_test_grid_roll_table(cell, C.byref(q), C.addressof(R), None, -1, None, 0, None)
    assert table(1.0, **POINT) == 0 and R.value == 1
    assert table(1.0, front=127.0, rear=0.0, half_width=0.0) == 0 and R.value == 128
    assert table(0.5, front=3.0, rear=60.0, half_width=3.5) == 0 and R.value == 128
    R.value = -7
    for cell, kw in ((1.0, dict(front=127.5, rear=0.0, half_width=0.0)), (1.0, dict(front=0.0, rear=127.0, half_width=0.5)), (0.0, POINT), (-1.0, POINT),
                     (float("nan"), POINT), (float("inf"), POINT), (0.01, dict(front=3.5, rear=1.0, half_width=0.9))):
        assert table(cell, **kw) == -1 and R.value == -7, (cell, kw)
        assert RR.table(RR.RollParams(headings_m=1, **kw), cell) is None
    p, q = both(G, front=127.0, rear=0.0, half_width=0.0, headings_m=1)
    got, want = G.core_roll_table(1.0, q), RR.table(p, 1.0)
    assert got[0] == want[0] == 128
    same_lists(got[1], want[1])
    assert got[1][0].tolist() == [[a, 0] for a in range(0, 128)]


def test_the_table_against_the_restatement_for_random_parameters(G):
    rng = np.random.default_rng(11)
    for n in range(10):
        m = int(rng.choice([1, 2, 3, 8, 32 if n == 0 else 5]))
        cell = float(rng.choice([0.1, 0.2, 0.25, 0.33, 1.0]))
        kw = dict(front=float(rng.random() * 12 * cell), rear=float(rng.random() * 6 * cell), half_width=float(rng.random() * 5 * cell), headings_m=m)
        p, q = both(G, **kw)
        got, want = G.core_roll_table(cell, q), RR.table(p, cell)
        assert got[0] == want[0], kw
        same_lists(got[1], want[1], repr(kw))
    p, q = both(G)                                                                    # the default car on cells of 0.2 m
    got, want = G.core_roll_table(0.2, q), RR.table(p, 0.2)
    same_lists(got[1], want[1])
    assert got[0] == 23 and 200 < len(got[1][16]) < 260                              # about 4.7 m x 2 m of cells straight ahead


# ---- scoring by hand -----------------------------------------------------------------------------------------------------
AHEAD = [[0, 1, 2], [0, 2, 2], [0, 3, 2], [0, 4, 2]]              # m = 1: heading 2 is straight ahead; from the anchor (2, 0) up column 2


def plane(**cells):
    c = np.zeros((5, 5), np.uint8)
    c[:, 2] = (10, 11, 12, 13, 14)
    for k, v in cells.items():
        c[int(k[1]), 2] = v                                        # b3=200: the cell (2, 3)
    return c


HAND = dict(headings_m=1, w_pot=0, **POINT)


def test_hand_no_cut_a_cut_at_pose_0_and_at_the_last_pose(G):
    recs, scores, best = agree(G, plane(), [[AHEAD]], (2, 0), **HAND)
    assert recs.tolist() == [[4, 0, 14, 11 + 12 + 13 + 14, FAR]] and scores.tolist() == [50] and best == 0
    recs, scores, best = agree(G, plane(b1=253), [[AHEAD]], (2, 0), **HAND)
    assert recs.tolist() == [[0, 1, -1, 0, FAR]] and scores.tolist() == [INF] and best == -1
    recs, scores, best = agree(G, plane(b4=254), [[AHEAD]], (2, 0), w_cut=7, **HAND)
    assert recs.tolist() == [[3, 1, 13, 36, FAR]] and scores.tolist() == [36 + 7] and best == 0


def test_hand_the_window_s_edge(G):
    recs, scores, best = agree(G, plane(), [[AHEAD + [[0, 5, 2]]]], (2, 0), w_cut=3, **HAND)
    assert recs.tolist() == [[4, 2, 14, 50, FAR]] and scores.tolist() == [53]
    recs, _, best = agree(G, plane(), [[AHEAD]], (5, 0), **HAND)                     # an anchor outside the window: cut at pose 0
    assert recs.tolist() == [[0, 2, -1, 0, FAR]] and best == -1
    recs, _, _ = agree(G, plane(), [[[[-3, 1, 2]], [[2, 1, 2]], [[3, 1, 2]], [[0, -1, 2]]]], (2, 0), **HAND)
    assert recs[:, :2].tolist() == [[0, 2], [1, 0], [0, 2], [0, 2]]
    # a vehicle one cell long: at (2, 3) it covers (2, 4) too, at (2, 4) it leaves the window
    recs, _, _ = agree(G, plane(), [[AHEAD]], (2, 0), headings_m=1, w_pot=0, front=1.0, rear=0.0, half_width=0.0)
    assert recs.tolist() == [[3, 2, 14, 12 + 13 + 14, FAR]]
    # under the offsets of a scrolled window
    recs, _, _ = agree(G, plane(), [[AHEAD]], (2 - 1000, 0 + 77), oa=-1000, ob=77, **HAND)
    assert recs.tolist() == [[4, 0, 14, 50, FAR]]


def test_hand_stop_cost_equal_to_f_and_one_more(G):
    recs, _, _ = agree(G, plane(b2=100), [[AHEAD]], (2, 0), stop_cost=100, **HAND)
    assert recs.tolist() == [[1, 1, 11, 11, FAR]]
    recs, _, _ = agree(G, plane(b2=100), [[AHEAD]], (2, 0), stop_cost=101, **HAND)
    assert recs.tolist() == [[4, 0, 100, 11 + 100 + 13 + 14, FAR]]
    recs, _, _ = agree(G, plane(b2=254), [[AHEAD]], (2, 0), stop_cost=255, **HAND)   # 255 never cuts
    assert recs.tolist() == [[4, 0, 254, 11 + 254 + 13 + 14, FAR]]
    recs, _, _ = agree(G, plane(), [[AHEAD]], (2, 0), stop_cost=1, **HAND)
    assert recs.tolist() == [[0, 1, -1, 0, FAR]]


def test_hand_no_information_under_unknown_cost(G):
    recs, _, _ = agree(G, plane(b3=255), [[AHEAD]], (2, 0), unknown_cost=254, **HAND)
    assert recs.tolist() == [[2, 1, 12, 23, FAR]]
    recs, _, _ = agree(G, plane(b3=255), [[AHEAD]], (2, 0), unknown_cost=0, **HAND)
    assert recs.tolist() == [[4, 0, 14, 11 + 12 + 0 + 14, FAR]]
    recs, _, _ = agree(G, plane(b3=255), [[AHEAD]], (2, 0), unknown_cost=254, stop_cost=255, **HAND)
    assert recs.tolist() == [[4, 0, 254, 11 + 12 + 254 + 14, FAR]]


def test_hand_the_field(G):
    pot = np.full((5, 5), FAR, np.int32)
    hand = dict(HAND, w_pot=3, w_cost=2)
    recs, scores, best = agree(G, plane(), [[AHEAD]], (2, 0), pot=pot, **hand)        # no goals: FAR everywhere, infeasible
    assert recs.tolist() == [[4, 0, 14, 50, FAR]] and scores.tolist() == [INF] and best == -1
    pot[4, 2], pot[3, 2] = 70, 900
    recs, scores, best = agree(G, plane(), [[AHEAD]], (2, 0), pot=pot, **hand)
    assert recs.tolist() == [[4, 0, 14, 50, 70]] and scores.tolist() == [3 * 70 + 2 * 50] and best == 0
    recs, scores, best = agree(G, plane(b4=253), [[AHEAD]], (2, 0), pot=pot, **hand)  # the field where the cut leaves the vehicle
    assert recs.tolist() == [[3, 1, 13, 36, 900]] and scores.tolist() == [3 * 900 + 2 * 36]
    recs, scores, best = agree(G, plane(), [[AHEAD]], (2, 0), pot=None, **HAND)       # w_pot = 0: no field is needed, FAR is no obstacle
    assert recs[0, 4] == FAR and scores.tolist() == [50] and best == 0


def test_hand_ties_the_lower_index_wins_and_none_feasible(G):
    worse = [[1, 1, 2], [1, 2, 2], [1, 3, 2], [1, 4, 2]]
    c = plane()
    c[:, 3] = 20
    recs, scores, best = agree(G, c, [[worse, AHEAD, AHEAD, worse]], (2, 0), **HAND)
    assert scores.tolist() == [80, 50, 50, 80] and best == 1
    recs, scores, best = agree(G, c, [[AHEAD, AHEAD]], (2, 0), stop_cost=5, **HAND)
    assert scores.tolist() == [INF, INF] and best == -1
    # the second set of a table
    recs, scores, best = agree(G, c, [[[AHEAD[0]]], [[worse[0]]]], (2, 0), set_=1, **HAND)
    assert recs.tolist() == [[1, 0, 20, 20, FAR]]


def test_hand_empty_candidates_and_a_sentinel_in_the_middle(G):
    lethal = [0, 9, 2]
    tab = [[[[0, 0, -1]] * 4, AHEAD[:2] + [[0, 0, -1], lethal], [[0, 1, 2], [7, 7, -1], [0, 2, 2], [0, 3, 2]]]]
    recs, scores, best = agree(G, plane(), tab, (2, 0), w_cut=100, **HAND)
    assert recs.tolist() == [[0, 3, -1, 0, FAR], [2, 0, 12, 23, FAR], [1, 0, 11, 11, FAR]] and scores.tolist() == [INF, 23, 11] and best == 2


def test_hand_int64_scores_at_the_largest_weights(G):
    T = 1024
    pot = np.full((5, 5), FAR - 1, np.int32)
    c = np.full((5, 5), 252, np.uint8)
    tab = np.zeros((1, 2, T, 3), np.int32)
    tab[..., 2] = 2
    tab[0, 1, 1000:, 1] = 9                                                          # the second leaves the window at pose 1000
    recs, scores, best = agree(G, c, tab, (2, 2), pot=pot, headings_m=1, w_pot=65535, w_cost=65535, w_cut=65535, **POINT)
    assert recs.tolist() == [[T, 0, 252, T * 252, FAR - 1], [1000, 2, 252, 1000 * 252, FAR - 1]]
    assert scores.tolist() == [65535 * (FAR - 1) + 65535 * T * 252, 65535 * (FAR - 1) + 65535 * 1000 * 252 + 65535 * 24] and best == 1
    assert scores[0] > 2 ** 46


# ---- random windows ------------------------------------------------------------------------------------------------------
def random_case(rng, nx, nz, K=12, T=9, S=2, m=None):
    """planes over their whole range, a table of random walks with sentinels, free poses in and round the window"""
    m = int(rng.choice([1, 2, 8])) if m is None else m
    cost = rng.integers(0, 256, (nz, nx)).astype(np.uint8)
    cost[rng.random((nz, nx)) < 0.6] = 0
    cost[rng.random((nz, nx)) < 0.05] = 255
    pot = rng.integers(0, 10 ** 6, (nz, nx)).astype(np.int32)
    pot[rng.random((nz, nx)) < 0.2] = FAR
    tab = np.zeros((S, K, T, 3), np.int32)
    tab[..., :2] = np.cumsum(rng.integers(-1, 3, (S, K, T, 2)), axis=2)
    tab[..., 2] = rng.integers(0, 8 * m, (S, K, T))
    end = rng.integers(0, 2 * T, (S, K))                                             # about half of the candidates end early
    for s in range(S):
        for c in range(K):
            if end[s, c] < T:
                tab[s, c, end[s, c], 2] = -1
    poses = np.stack([rng.integers(-3, nx + 3, 40), rng.integers(-3, nz + 3, 40), rng.integers(-1, 8 * m + 1, 40)], axis=1).astype(np.int32)
    kw = dict(front=float(rng.random() * 3), rear=float(rng.random() * 2), half_width=float(rng.random() * 1.5), headings_m=m,
              stop_cost=int(rng.choice([1, 100, 253, 255])), unknown_cost=int(rng.choice([0, 50, 254])), w_pot=int(rng.choice([0, 1, 65535])),
              w_cost=int(rng.integers(0, 65536)), w_cut=int(rng.integers(0, 65536)))
    return cost, pot, tab, poses, kw


WINDOWS = [(1, 1), (1, 9), (9, 1), (3, 3), (40, 7), (33, 65), (65, 65)]


@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_the_header_against_the_restatement_on_random_windows(G, nx, nz):
    rng = np.random.default_rng(100 * nx + nz)
    statuses = set()
    for k, (oa, ob) in enumerate(((0, 0), (5, -7), (-(2 ** 20 - 8192), 2 ** 20 - 8192 - nz))):
        cost, pot, tab, poses, kw = random_case(rng, nx, nz)
        poses[:, 0] += oa
        poses[:, 1] += ob
        anchor = (oa + int(rng.integers(-1, nx + 1)), ob + int(rng.integers(-1, nz + 1)))
        for cell in (1.0, 0.5):
            recs, scores, best, f = agree(G, cost, tab, anchor, pot=pot, cell=cell, oa=oa, ob=ob, set_=k % 2, poses=poses, tag="case %d" % k, **kw)
            statuses |= set(recs[:, 1].tolist())
            assert ((recs[:, 0] == 0) == (recs[:, 2] == -1)).all() and (scores[recs[:, 0] == 0] == INF).all()
            assert best == -1 or scores[best] == scores.min()
    if nx * nz >= 200:
        assert statuses == {0, 1, 2, 3}


# ---- refusals and exports ------------------------------------------------------------------------------------------------
nan, inf = float("nan"), float("inf")
BAD = [dict(front=-0.1), dict(front=nan), dict(rear=inf), dict(rear=-1.0), dict(half_width=nan), dict(half_width=-0.5), dict(headings_m=0),
       dict(headings_m=33), dict(stop_cost=0), dict(stop_cost=256), dict(unknown_cost=-1), dict(unknown_cost=255), dict(w_pot=-1), dict(w_pot=65536),
       dict(w_cost=-1), dict(w_cost=65536), dict(w_cut=-1), dict(w_cut=65536)]
GOOD = [dict(front=0.0, rear=0.0, half_width=0.0), dict(headings_m=1), dict(headings_m=32), dict(stop_cost=1), dict(stop_cost=255), dict(unknown_cost=0),
        dict(unknown_cost=254), dict(w_pot=0, w_cost=0, w_cut=0), dict(w_pot=65535, w_cost=65535, w_cut=65535)]


def test_refusals(G):
    import svhip
    L = G._bind()
    cost, pot = np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.int32)
    tab = np.zeros((1, 1, 1, 3), np.int32)
    recs, scores, best = np.full((1, 5), 0x55, np.int32), np.full(1, 0x55, np.int64), C.c_int32(-7)
    poses, f = np.zeros((1, 3), np.int32), np.full(1, 0x55, np.int32)

    def call(p, cell=1.0, nx=2, nz=2, oa=0, ob=0, cost_=cost, pot_=pot, tab_=tab, S=1, K=1, T=1, set_=0, ga=0, gb=0, poses_=poses, n=1, f_=f, best_=best):
        return L.svh_test_grid_roll(C.byref(p) if p is not None else None, cell, nx, nz, oa, ob, cost_.ctypes.data if cost_ is not None else None,
                                    pot_.ctypes.data if pot_ is not None else None, tab_.ctypes.data if tab_ is not None else None, S, K, T, set_, ga, gb,
                                    poses_.ctypes.data if poses_ is not None else None, n, f_.ctypes.data if f_ is not None else None,
                                    recs.ctypes.data, scores.ctypes.data, C.addressof(best_) if best_ is not None else None)
    good = G.default_roll()
    assert good.asdict() == dict(front=3.5, rear=1.0, half_width=np.float32(0.9), headings_m=8, stop_cost=253, unknown_cost=254, w_pot=1, w_cost=1, w_cut=0)
    assert C.sizeof(G.RollParams) == 36
    for kw in BAD:
        assert not RR.RollParams(**kw).ok(), kw
        assert call(G.default_roll(**kw)) == svhip.ERR_BAD_ARG and "svh_test_grid_roll" in svhip.last_error(), kw
    big = np.zeros((1, 1, 1, 3), np.int32)
    cases = [dict(p=None), dict(cell=0.0), dict(cell=nan), dict(nx=0), dict(nz=8193), dict(oa=2 ** 20), dict(cost_=None), dict(pot_=None), dict(tab_=None),
             dict(S=0), dict(K=0), dict(T=0), dict(T=1025), dict(K=65537), dict(S=2 ** 22 + 1), dict(S=2 ** 21, K=2, T=2), dict(set_=1), dict(set_=-1),
             dict(ga=2 ** 20), dict(gb=-2 ** 20), dict(poses_=None), dict(f_=None), dict(n=-1), dict(best_=None), dict(cell=0.01)]
    for field, v in ((2, 64), (2, -2), (0, 16385), (1, -16385)):                      # a heading that does not exist, an offset too far
        t = big.copy()
        t[0, 0, 0, field] = v
        cases.append(dict(tab_=t))
    for bad in cases:
        assert call(**dict(dict(p=good), **bad)) == svhip.ERR_BAD_ARG, bad
    assert (recs == 0x55).all() and (scores == 0x55).all() and best.value == -7 and (f == 0x55).all()
    for kw in GOOD:
        assert RR.RollParams(**kw).ok() and call(G.default_roll(**kw)) == 0, kw
    t = big.copy()
    t[0, 0, 0] = (16384, -16384, 63)
    assert call(good, tab_=t) == 0 and call(G.default_roll(w_pot=0), pot_=None) == 0
    assert call(good, tab_=None, S=0, K=0, T=0, best_=None) == 0                      # the poses alone
    assert call(good, poses_=None, n=0, f_=None) == 0                                 # the table alone
    t = np.zeros((1, 1, 2, 3), np.int32)
    t[0, 0, 0, 2], t[0, 0, 1] = -1, (99999, 0, 999)                                   # what follows the first -1 is not looked at
    assert call(good, tab_=t, T=2) == 0
    # the entries refuse a null grid before anything else
    buf = np.full(64, 0xAB, np.uint8)
    for fn in (lambda: L.svh_grid_set_roll(None, C.byref(good)), lambda: L.svh_grid_get_roll(None, C.byref(good), buf.ctypes.data, buf.ctypes.data),
               lambda: L.svh_grid_heading_of(None, buf.ctypes.data, buf.ctypes.data), lambda: L.svh_grid_roll_footprint(None, 0, buf.ctypes.data, 1, buf.ctypes.data),
               lambda: L.svh_grid_footprint_cost(None, buf.ctypes.data, 1, 0, buf.ctypes.data), lambda: L.svh_grid_roll_set_candidates(None, big.ctypes.data, 1, 1, 1),
               lambda: L.svh_grid_roll_get_candidates(None, buf.ctypes.data),
               lambda: L.svh_grid_roll_score(None, buf.ctypes.data, 0, buf.ctypes.data, buf.ctypes.data, 0, buf.ctypes.data),
               lambda: L.svh_grid_render_roll(None, buf.ctypes.data, 0)):
        assert fn() == svhip.ERR_BAD_ARG and "svh_grid" in svhip.last_error()
    L.svh_grid_roll_params_default(None)
    assert (buf == 0xAB).all()
    for tab_, m, ok in ((big, 8, True), (np.zeros((1, 1, 1, 3), np.int32) + [0, 0, 8], 1, False), (np.zeros((2, 3, 1025, 3), np.int32), 8, False)):
        assert RR.table_ok(tab_, m) == ok


ENTRIES = ("svh_grid_roll_params_default", "svh_grid_set_roll", "svh_grid_get_roll", "svh_grid_heading_of", "svh_grid_roll_footprint",
           "svh_grid_footprint_cost", "svh_grid_roll_set_candidates", "svh_grid_roll_get_candidates", "svh_grid_roll_score", "svh_grid_render_roll")


def test_entries_are_declared_and_exported(G):
    import svhip
    text = open(os.path.join(H.ROOT, "include", "svh_grid.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(svhip.lib(), name), name
    for name in ("svh_test_grid_roll", "svh_test_grid_roll_device", "svh_test_grid_roll_table", "svh_test_grid_roll_heading", "svh_test_grid_roll_group"):
        assert hasattr(svhip.lib(), name) and name not in text, name                 # test entries: exported, not in the public header
    for name, value in (("SVH_GRID_ROLL_RECORD", "5"), ("SVH_GRID_ROLL_COMPLETE", "0"), ("SVH_GRID_ROLL_CUT_COST", "1"), ("SVH_GRID_ROLL_CUT_WINDOW", "2"),
                        ("SVH_GRID_ROLL_EMPTY", "3")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), hdr), name
    assert "ROLLOUT" in text and "svh_grid_roll_params" in hdr
    assert (G.ROLL_RECORD, G.ROLL_FIELDS, G.ROLL_INFEASIBLE) == (5, RR.FIELDS, RR.INFEASIBLE)
    assert (G.ROLL_COMPLETE, G.ROLL_CUT_COST, G.ROLL_CUT_WINDOW, G.ROLL_EMPTY) == (RR.COMPLETE, RR.CUT_COST, RR.CUT_WINDOW, RR.EMPTY)
    assert (G.ROLL_COLOUR, G.ROLL_BEST_COLOUR) == (RR.COLOUR, RR.BEST_COLOUR) == ((0, 192, 255), (255, 255, 255))
    assert [G.roll_group(n) for n in (0, 1, 2, 3, 4, 5, 33, 64, 65, 257, 66049)] == [1, 1, 2, 4, 4, 8, 64, 64, 64, 64, 64]


def test_header_is_c99(tmp_path):
    exe = str(tmp_path / "grid_roll_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "cxx", "grid_roll_c99.c"), "-L", H.PKG, "-lsvhip", "-Wl,-rpath," + H.PKG])
    out = subprocess.check_output([exe]).decode()
    assert "rollouts C99 ok, records of 5, statuses 0..3" in out


# ---- the header once more, as a program of its own under the sanitizers --------------------------------------------------
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_roll")
    exe = str(d / "grid_roll_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.PKG, "csrc"), "-o", exe, os.path.join(H.ROOT, "tests", "cxx", "grid_roll_check.cpp")])

    def run(p, cell, cost, pot=None, tab=None, set_=0, anchor=(0, 0), oa=0, ob=0, poses=None):
        cost = np.asarray(cost, np.uint8)
        nz, nx = cost.shape
        S, K, T = tab.shape[:3] if tab is not None else (0, 0, 0)
        q = np.zeros((0, 3), np.int32) if poses is None else np.ascontiguousarray(poses, np.int32)
        head = np.array([nx, nz, oa, ob, p.headings_m, p.stop_cost, p.unknown_cost, p.w_pot, p.w_cost, p.w_cut, S, K, T, set_, anchor[0], anchor[1], len(q),
                         pot is not None], np.int64).astype(np.int32)
        job = str(d / "job.bin")
        with open(job, "wb") as f:
            f.write(head.tobytes() + np.array([cell, p.front, p.rear, p.half_width], np.float32).tobytes() + cost.tobytes())
            f.write((b"" if pot is None else np.ascontiguousarray(pot, np.int32).tobytes()) + (b"" if tab is None else np.ascontiguousarray(tab, np.int32).tobytes()))
            f.write(q.tobytes())
        r = subprocess.run([exe, job], capture_output=True)
        if r.returncode == 3:
            assert not r.stdout and not r.stderr
            return None
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out, at = r.stdout, 4
        R, lists = int(np.frombuffer(out[:4], np.int32)[0]), []
        for k in range(8 * p.headings_m):
            n = int(np.frombuffer(out[at:at + 8], np.int64)[0])
            lists.append(np.frombuffer(out[at + 8:at + 8 + 8 * n], np.int32).reshape(n, 2))
            at += 8 + 8 * n
        res = dict(R=R, lists=lists, f=np.frombuffer(out[at:at + 4 * len(q)], np.int32))
        at += 4 * len(q)
        if tab is not None:
            res.update(recs=np.frombuffer(out[at:at + 20 * K], np.int32).reshape(K, 5), scores=np.frombuffer(out[at + 20 * K:at + 28 * K], np.int64),
                       best=int(np.frombuffer(out[at + 28 * K:at + 28 * K + 4], np.int32)[0]))
            at += 28 * K + 4
        assert at == len(out)
        return res
    return run


def san_check(core, p, cell, cost, pot, tab, set_, anchor, oa, ob, poses):
    got = core(p, cell, cost, pot, tab, set_, anchor, oa, ob, poses)
    R, lists = RR.table(p, cell)
    assert got["R"] == R
    same_lists(got["lists"], lists)
    assert np.array_equal(got["f"], RR.footprint_costs(p, lists, cost, poses, oa, ob))
    recs, scores, best = RR.score(p, lists, cost, pot, tab[set_], anchor, oa, ob)
    assert np.array_equal(got["recs"], recs) and np.array_equal(got["scores"], scores) and got["best"] == best
    return recs


@pytest.mark.parametrize("nx,nz,oa,ob", [(33, 9, 0, 0), (1, 40, -5, 9), (40, 1, 2 ** 20 - 8192, -(2 ** 20 - 8192)), (17, 17, 0, 0), (1, 1, 0, 0)])
def test_the_header_under_the_sanitizers(core, nx, nz, oa, ob):
    rng = np.random.default_rng(60 + nx)
    cost, pot, tab, poses, kw = random_case(rng, nx, nz)
    poses[:, 0] += oa
    poses[:, 1] += ob
    san_check(core, RR.RollParams(**kw), 0.5, cost, pot, tab, 1, (oa + nx // 2, ob + nz // 3), oa, ob, poses)


def test_the_program_at_the_reach_and_the_table_limits(core):
    rng = np.random.default_rng(70)
    cost = rng.integers(0, 253, (9, 9)).astype(np.uint8)
    pot = rng.integers(0, 1000, (9, 9)).astype(np.int32)
    poses = np.array([[4, 4, 0], [0, 0, 1], [8, 8, 7], [4, 4, 8], [4, 4, -1]], np.int32)
    point = RR.RollParams(headings_m=1, **POINT)                                     # R = 1
    # T at its limit: 1024 poses that walk round the window; K at its limit: 65536 candidates of one pose, S K T = 2^22
    walk = np.zeros((1, 1, 1024, 3), np.int32)
    walk[0, 0, :, 0], walk[0, 0, :, 1], walk[0, 0, :, 2] = np.arange(1024) % 4, (np.arange(1024) // 4) % 4, np.arange(1024) % 8
    recs = san_check(core, point, 1.0, cost, pot, walk, 0, (2, 2), 0, 0, poses)
    assert recs[0, 0] == 1024
    many = np.zeros((64, 65536, 1, 3), np.int32)
    many[..., 0], many[..., 1] = rng.integers(-6, 7, (64, 65536, 1)), rng.integers(-6, 7, (64, 65536, 1))
    many[63, 5::7, 0, 2] = -1
    recs = san_check(core, point, 1.0, cost, pot, many, 63, (4, 4), 0, 0, poses)
    assert set(recs[:, 1].tolist()) == {0, 2, 3}
    long_ = RR.RollParams(front=127.0, rear=0.0, half_width=0.0, headings_m=1, w_pot=0)   # R = 128: every pose leaves a window of 9 x 9 ...
    recs = san_check(core, long_, 1.0, cost, None, walk[:, :, :8], 0, (2, 2), 0, 0, poses)
    assert recs.tolist() == [[0, 2, -1, 0, FAR]]
    wide = np.zeros((3, 200), np.uint8)                                              # ... and fits one of 200 x 3 along the row
    wide[1, 147], wide[1, 148], wide[1, 149] = 77, 88, 99                            # the vehicle covers 20 .. 147, then 21 .. 148, then leaves
    recs = san_check(core, long_, 1.0, wide, None, np.array([[[[0, 0, 0], [1, 0, 0], [60, 0, 0], [0, 0, 4]]]], np.int32), 0, (20, 1), 0, 0, poses)
    assert recs.tolist() == [[2, 2, 88, 77 + 88, FAR]]
    assert core(RR.RollParams(front=127.5, rear=0.0, half_width=0.0, headings_m=1), 1.0, cost, pot, walk, 0, (2, 2), 0, 0, poses) is None   # R = 129


def test_the_program_refuses_what_the_library_refuses(core):
    tab = np.zeros((1, 1, 1, 3), np.int32)
    for kw in BAD:
        assert core(RR.RollParams(**kw), 1.0, np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.int32), tab) is None, kw
    bad = tab.copy()
    bad[0, 0, 0, 2] = 64
    assert core(RR.RollParams(), 1.0, np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.int32), bad) is None


# ---- arc_candidates: plumbing, by its properties -------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 8])
def test_arc_candidates(G, m):
    cell, step, T = 0.2, 0.35, 24
    kap = [-0.3, -0.11, 0.0, 0.11, 0.3]
    tab = G.arc_candidates(cell, m, kap, step, T)
    assert tab.shape == (8 * m, 5, T, 3) and tab.dtype == np.int32 and RR.table_ok(tab, m)
    u = G.heading_vectors(m)
    for s in range(8 * m):
        straight = tab[s, 2]
        assert (straight[:, 2] == s).all()                                           # the straight arc keeps the set's heading ...
        d = straight[:, :2].astype(np.float64) * cell
        along = (d @ u[s]) / np.sqrt((u[s] ** 2).sum())
        across = (d[:, 0] * u[s, 1] - d[:, 1] * u[s, 0]) / np.sqrt((u[s] ** 2).sum())
        assert np.abs(along - step * (np.arange(T) + 1)).max() <= cell and np.abs(across).max() <= cell      # ... and advances along its vector
        assert (np.diff(along) > 0).all()
        for c in (0, 1):                                                             # a left and a right turn leave the heading to either side
            right, left = tab[s, c, :, 2].astype(np.int64), tab[s, 4 - c, :, 2].astype(np.int64)
            assert (((left - s) % (8 * m)) <= 4 * m).all() and (((s - right) % (8 * m)) <= 4 * m).all()
    ahead = tab[2 * m]                                                               # mirrored curvatures, straight ahead: mirrored offsets
    for c in (0, 1):
        assert np.array_equal(ahead[c, :, 0], -ahead[4 - c, :, 0]) and np.array_equal(ahead[c, :, 1], ahead[4 - c, :, 1])
        assert ((ahead[c, :, 2].astype(np.int64) + ahead[4 - c, :, 2]) % (8 * m) == 4 * m % (8 * m)).all()   # k and 4 m - k mirror each other
    # sentinels: an arc that would leave +-16384 cells ends there and stays ended
    far = G.arc_candidates(0.01, m, [0.0, 0.001], 20.0, 16)
    assert RR.table_ok(far, m)
    n = RR.lengths(far.reshape(-1, 16, 3))
    assert (n < 16).all() and (n >= 7).all()
    for cand, n_c in zip(far.reshape(-1, 16, 3), n):
        assert (cand[n_c:, 2] == -1).all() and (cand[n_c:, :2] == 0).all() and (cand[:n_c, 2] >= 0).all()

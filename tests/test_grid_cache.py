"""CPU: the tables of tests/grid_cache_cases.py against the header and against the composed restatement tests/grid_all_ref.py.

tests/test_grid_cache_gpu.py asks the device, after every mutator, for every output that passes through one of the engine's caches
and compares it with a fresh object and with the restatement.  That comparison is only as good as its tables, so this file pins the
tables without a device: no entry of include/svh_grid.h is left unclassified, every CHANGES cell of the matrix does change the
restatement's output on the scene (or is listed, with its reason, among the few that the scene cannot show), every KEEPS cell keeps
it, every REFUSES cell refuses, the hand case has the values the restatement gives, and the table in DESIGN.md is the one the
cases file generates."""
import os
import re

import numpy as np
import pytest

import grid_all_ref as ALL
import grid_cache_cases as CC
import grid_plan_ref as PR
import helpers as H

ROOT = H.ROOT


def read_all(ref):
    with ref.frozen():
        return {n: CC.read_ref(ref, n) for n in CC.READERS}


@pytest.fixture(scope="module")
def baseline():
    """the scene on the restatement, read twice: the second read-out shows the last results the state-bearing readers leave"""
    ref = CC.new_ref()
    CC.scene(None, ref)
    read_all(ref)
    return read_all(ref)


# ---- nothing forgotten -----------------------------------------------------------------------------------------------------------
def header_entries():
    text = open(os.path.join(ROOT, "include", "svh_grid.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text[text.index("#ifndef SVH_GRID_H"):], flags=re.S)
    return sorted(set(re.findall(r"\b(svh_grid_[a-z0-9_]+)\s*\(", text)))


def test_every_entry_of_the_header_is_classified():
    entries, roles = header_entries(), CC.classified()
    assert "svh_grid_observe_view_lists" in entries and "svh_grid_create" in entries and "svh_grid_params" not in entries
    missing = [e for e in entries if e not in roles]
    assert not missing, "entries of include/svh_grid.h that tests/grid_cache_cases.py does not classify: %s" % missing
    gone = [e for e in roles if e not in entries]
    assert not gone, "classified, but not in the header: %s" % gone
    for e, r in roles.items():
        assert r == {"neither"} or "neither" not in r, (e, r)
    # what the issue names as "neither", and the four entries that are both a mutator and a reader: they leave a last result
    for e in ("svh_grid_create", "svh_grid_destroy", "svh_grid_cell_of", "svh_grid_heading_of", "svh_grid_frame_camera", "svh_grid_get_plan"):
        assert roles[e] == {"neither"}
    both = sorted(e for e, r in roles.items() if r == {"mutator", "reader"})
    assert both == ["svh_grid_align_points", "svh_grid_explore_rank", "svh_grid_roll_score"], both


def test_the_tables_are_whole():
    assert set(CC.EXPECT) == set(CC.MATRIX_MUTATORS) and all(set(row) == set(CC.READERS) for row in CC.EXPECT.values())
    assert set(CC.RULES) == set(CC.MATRIX_MUTATORS)
    assert {r.group for r in CC.READERS.values()} == set(CC.GROUPS)
    for m, (changed, refused) in CC.RULES.items():
        assert changed <= set(CC.GROUPS) and refused <= set(CC.GROUPS) and not changed & refused, m
    # the state-bearing readers come last and the last results first: a read-out shows what the history left
    names = list(CC.READERS)
    bearing = [n for n in names if CC.READERS[n].bearing]
    assert names[-len(bearing):] == bearing == ["roll_score", "explore_rank", "align_points"]
    assert names[:5] == ["render_roll", "render_align", "align_scan", "align_volume", "explore_stats"]
    # the examples of the documented rule
    for m, r in (("plan_set_goals", "front:LABEL"), ("set_plan", "frontiers"), ("set_frontier", "plan:POT"), ("set_align", "trav:cost"), ("set_roll", "plan:POT")):
        assert CC.EXPECT[m][r] == CC.KEEPS, (m, r)
    assert all(CC.served_from_cache("set_explore", r) for r in CC.READERS if CC.READERS[r].cached)
    assert all(CC.EXPECT[m][r] == CC.KEEPS for m in CC.EXPECT for r in CC.READERS if CC.served_from_cache(m, r))


def test_the_scene_has_what_the_issue_asks_for(baseline):
    ref = CC.new_ref()
    CC.scene(None, ref)
    L, f, fr = ref.L, ref.field(), ref.frontiers()
    assert (L.nx, L.nz) == (2 * CC.T + 1, CC.T + 1) == (33, 17)
    cls = ref.planes()["cls"] & 3
    assert (cls[:, L.wall] == 2).sum() == L.nz - 2 and (cls[list(L.gap), L.wall] == 1).all()                  # a wall with one gap
    assert f["pot"][L.inside[1], L.inside[0]] == PR.FAR and f["price"][L.inside[1], L.inside[0]] > 0           # a closed room
    state = ref.state()
    assert (state[L.block[1]:, L.block[0]:] == 0).all() and (state[L.nz - 1, :L.strip] == 0).all()             # unseen: unknown, no ray
    assert len(fr["recs"]) == 2 and fr["stats"][1] >= 2                                                        # so that frontiers exist
    assert ref.rays > 0 and f["counted"] == 2 and len(ref.goals) == 3
    assert f["pot"][L.start[1], L.start[0]] != PR.FAR                                                          # through the gap
    assert ref.roll_last["recs"][0, 0] == 6 and ref.cands.shape == (2, 3, 6, 3) and ref.L.candidates(other=True).shape == (2, 3, 5, 3)
    assert ref.align_last["rec"][0] == 0 and ref.align_last["rec"][6] >= CC.ALIGN_KW["min_scan"]
    assert (ref.dyn_planes()["contra"] > 0).sum() > 0 and ref.dyn_stats["observations"] == 3
    assert all(b != CC.REFUSED for b in baseline.values())


# ---- not vacuous -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", CC.MATRIX_MUTATORS)
def test_the_matrix_on_the_restatement(baseline, m):
    ref = CC.new_ref()
    CC.scene(None, ref)
    read_all(ref)
    CC.MUTATORS[m](None, ref, None)
    after = read_all(ref)
    for r in CC.READERS:
        want = CC.EXPECT[m][r]
        if want == CC.REFUSES:
            assert after[r] == CC.REFUSED, (m, r)
        elif want == CC.KEEPS:
            assert after[r] == baseline[r], (m, r, "the documented rule says this output stays")
        elif (m, r) in CC.UNSHOWN:
            assert after[r] == baseline[r], (m, r, "listed as UNSHOWN, yet the scene shows it: take it off the list")
        else:
            assert after[r] != baseline[r] and after[r] != CC.REFUSED, (m, r, "the scene does not show this change")


def test_unshown_is_within_its_cap():
    pairs = [(m, r) for m in CC.EXPECT for r in CC.READERS if CC.EXPECT[m][r] == CC.CHANGES]
    assert all(p in pairs and reason for p, reason in CC.UNSHOWN.items())
    assert len(CC.UNSHOWN) <= 0.05 * len(pairs), (len(CC.UNSHOWN), len(pairs))


# ---- the composed class ----------------------------------------------------------------------------------------------------------
def test_the_composition_reaches_every_branch():
    ref = CC.new_ref()
    CC.scene(None, ref)
    assert [c.__module__ for c in type(ref).__mro__[:6]] == ["grid_all_ref", "grid_dyn_ref", "grid_plan_ref", "grid_trav_ref", "grid_local_ref", "grid_ref"]
    ref.scroll(2, 1)
    assert ref.window() == (2, 1) and (ref.dyn_planes()["age"][:, -2:] == -1).all() and (ref.local_planes()["passed"][:, -2:] == 0).all()
    ref.set_window(1.0, 0.0)
    assert ref.window() == (0, 0) and len(ref.goals) == 0 and ref.stamp == 0 and ref.stats["added"] == 0 and (ref.contra == 0).all()
    assert ref.roll_last is not None and ref.align_last is not None           # the last results survive a clear
    with pytest.raises(ALL.Refused):
        ALL.Grid(ref.P).observe(np.zeros((0, 4), np.float32), CC.pos(CC.ZERO, 1, 1))


# ---- the hand case ---------------------------------------------------------------------------------------------------------------
def test_a_cleared_obstacle_opens_the_route_on_the_restatement():
    ref = CC.new_ref(dyn=None)
    CC.hand_scene(None, ref)
    assert ref.D.min_through == 1 and ref.D.clear_frames == 1 and ref.T.lethal == 7 and ref.plan.neutral == 50
    f, cost = ref.field(), ref.cost().copy()
    sa, sb = CC.HAND_START
    assert f["reached"] == CC.HAND["reached"] == 272 and f["pot"][sb, sa] == PR.FAR
    assert ref.path(CC.pos(CC.ZERO, sa, sb, 0.0))[0] == PR.UNREACHABLE
    _, recs, _ = ref.roll_score(CC.HAND_ANCHOR, 0)
    assert recs[:, 1].tolist() == [0, 1, 1] and (recs[:, 4] == PR.FAR).all()             # two are cut at the wall, none has a way on
    CC.hand_clearing(None, ref, None)
    f = ref.field()
    assert ref.dyn_stats["cleared"] == CC.HAND["cleared"] == 15
    assert int((ref.cost() != cost).sum()) == CC.HAND["cost_bytes"] == 75
    assert f["reached"] == CC.HAND["reached_after"] == 548 and f["pot"][sb, sa] == CC.HAND["pot_after"] == 19662
    st, cells, c = ref.path(CC.pos(CC.ZERO, sa, sb, 0.0))
    assert st == PR.FOUND and c == 19662 and tuple(cells[-1]) == CC.HAND_GOAL
    _, recs, _ = ref.roll_score(CC.HAND_ANCHOR, 0)
    assert (recs[:, 4] != PR.FAR).all()                                                # the cleared cells are unknown: they still cut, but the way on exists


# ---- the document ----------------------------------------------------------------------------------------------------------------
def test_the_matrix_in_the_design_document_is_current():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    begin, end = "<!-- cache-matrix:begin -->", "<!-- cache-matrix:end -->"
    assert text.count(begin) == 1 and text.count(end) == 1
    got = [line for line in text[text.index(begin) + len(begin):text.index(end)].strip().splitlines()]
    want = CC.matrix_table()
    assert got == want, "DESIGN.md, 'Caches: who invalidates what': the table is not the one tests/grid_cache_cases.py generates (CC.matrix_table())"

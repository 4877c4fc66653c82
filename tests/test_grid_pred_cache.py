"""CPU: the tables of tests/grid_pred_cache_cases.py against the composed restatement.  tests/test_grid_pred_cache_gpu.py asks the
device, after every mutator of the grid, for PRED, its statistics and a scored record and compares them with a fresh object and with
the restatement; that comparison is only as good as its tables, so this file pins them without a device: every entry of
include/svh_grid_pred.h is classified, every mutator of tests/grid_cache_cases.py and tests/grid_obj_cache_cases.py is in the matrix,
the five mutators the header names -- and no other -- drop PRED, every CHANGES cell does change the restatement's output on the scene
(or is listed, with its reason, among the few the scene cannot show), every KEEPS cell keeps it, and the scene predicts something
and cuts a candidate by it."""
import os
import re

import numpy as np
import pytest

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pred_cache_cases as PCC
import grid_pred_ref as PR
import helpers as H


def rig():
    ref = CC.new_ref()
    PCC.scene(None, ref)
    return ref


@pytest.fixture(scope="module")
def baseline():
    return PCC.read_ref(rig())


def test_every_entry_of_the_header_is_classified():
    text = open(os.path.join(H.ROOT, "include", "svh_grid_pred.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    entries = set(re.findall(r"\b(svh_grid_[a-z0-9_]+)\s*\(", text))
    readers = {"svh_grid_get_pred_plane", "svh_grid_get_pred_stats", "svh_grid_roll_score_pred"}
    mutators = {"svh_grid_set_predict"}
    neither = {"svh_grid_pred_params_default", "svh_grid_get_predict"}
    elsewhere = {"svh_grid_footprint_pred", "svh_grid_render_pred"}       # reads of PRED, compared with the restatement in tests/test_grid_pred_gpu.py
    assert entries == readers | mutators | neither | elsewhere
    assert {"svh_grid_" + m for m in PCC.OWN} == mutators and len(PCC.READERS) == 3


def test_the_tables_are_whole():
    assert set(PCC.MUTATORS) == set(CC.MATRIX_MUTATORS) | set(OCC.OWN) | set(PCC.OWN) == set(PCC.EXPECT) == set(PCC.RULES)
    dropping = [m for m in PCC.MUTATORS if "pred" in PCC.RULES[m]]
    assert dropping == PCC.DROPS == ["set_window", "set_objects", "objects_step", "objects_reset", "set_predict"]
    for m in PCC.MUTATORS:                                        # no add, observation, scroll, follow or clear, and no other layer's parameters
        if m not in PCC.DROPS:
            assert all(PCC.EXPECT[m][n] == PCC.KEEPS and PCC.served_from_cache(m, n) for n in PCC.CACHED), m
    for m in ("clear", "scroll", "follow", "add_points", "observe_points", "set_traversability", "set_plan", "set_roll", "roll_set_candidates", "set_frontier",
              "set_explore", "set_align", "set_dynamics_change"):
        assert m in PCC.MUTATORS and m not in PCC.DROPS, m
    pairs = [(m, n) for m in PCC.EXPECT for n in PCC.READERS if PCC.EXPECT[m][n] == PCC.CHANGES]
    assert all(p in pairs and reason for p, reason in PCC.UNSHOWN.items()) and len(PCC.UNSHOWN) <= 0.1 * len(pairs), (len(PCC.UNSHOWN), len(pairs))


def test_the_scene_predicts_and_cuts(baseline):
    ref = rig()
    plane, stats, off = PCC.ref_pred(ref)
    assert stats[0] >= 2 and stats[1] >= 15 and stats[2] > stats[1] and stats[3] == 4 and off == tuple(ref.trk.off)
    assert (plane >> np.uint32(PCC.PRED_KW["slots"]) == 0).all() and (plane == (1 << PCC.PRED_KW["slots"]) - 1).any()
    recs = np.frombuffer(baseline["pred_score"].split(b"|")[0], np.int32).reshape(-1, 6)
    assert (recs[:, 1] == PR.CUT_OBJECT).any() and (recs[recs[:, 1] == PR.CUT_OBJECT, 5] >= 0).all(), recs


@pytest.mark.parametrize("m", list(PCC.MUTATORS))
def test_the_matrix_on_the_restatement(baseline, m):
    ref = rig()
    try:
        PCC.MUTATORS[m](None, ref, None)
    except Exception as e:                                        # a refusal of the restatement leaves it as it was
        assert type(e).__name__ in ("Refused", "ValueError"), e
    after = PCC.read_ref(ref)
    for n in PCC.READERS:
        if PCC.EXPECT[m][n] == PCC.KEEPS:
            assert after[n] == baseline[n], (m, n, "the documented rule says this output stays")
        elif (m, n) in PCC.UNSHOWN:
            assert after[n] == baseline[n], (m, n, "listed as UNSHOWN, yet the scene shows it: take it off the list")
        elif PCC.READERS[n][0] == "pred":
            assert after[n] != baseline[n], (m, n, "the scene does not show this change")


def test_what_empties_the_tracks_resets_pred():
    for m in ("set_window", "set_objects", "objects_reset"):
        ref = rig()
        PCC.MUTATORS[m](None, ref, None)
        plane, stats, off = PCC.ref_pred(ref)
        assert not plane.any() and stats == (0, 0, 0, 0) and off == (ref.oa, ref.ob), m
    ref = rig()
    PCC.MUTATORS["set_predict"](None, ref, None)
    assert PCC.ref_pred(ref)[1][3] == 2                           # the skipped form

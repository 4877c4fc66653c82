"""CPU: the tables of tests/grid_pose_cache_cases.py against the composed restatement.  tests/test_grid_pose_cache_gpu.py asks the
device, after every mutator of the grid, for CF, PPOT, PDIR, the statistics and a path and compares them with a fresh object and with
the restatement; that comparison is only as good as its tables, so this file pins them without a device: every entry of
include/svh_grid_pose.h is classified, every mutator of the three existing case files is in the matrix, what drops CF is what the
table of tests/grid_cache_cases.py says changes svh_grid_footprint_cost, the mutators the issue names leave the layer alone, every
CHANGES cell does change the restatement's output on the scene (or is listed, with its reason, among the few the scene cannot show),
every KEEPS cell keeps it, and the scene has a field and a path."""
import os
import re

import numpy as np
import pytest

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pose_cache_cases as QCC
import grid_pose_ref as QR
import grid_pred_cache_cases as PCC
import helpers as H


def rig():
    ref = CC.new_ref()
    QCC.scene(None, ref)
    return ref


@pytest.fixture(scope="module")
def baseline():
    return QCC.read_ref(rig())


def test_every_entry_of_the_header_is_classified():
    text = open(os.path.join(H.ROOT, "include", "svh_grid_pose.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    entries = set(re.findall(r"\b(svh_grid_[a-z0-9_]+)\s*\(", text))
    readers = {"svh_grid_get_pose_plane", "svh_grid_get_pose_stats", "svh_grid_pose_path"}
    mutators = {"svh_grid_set_pose", "svh_grid_pose_set_goals", "svh_grid_pose_set_goal"}
    neither = {"svh_grid_pose_params_default", "svh_grid_get_pose", "svh_grid_pose_heading_of"}
    elsewhere = {"svh_grid_render_pose"}                          # a read of the field, compared in tests/test_grid_pose_gpu.py
    assert entries == readers | mutators | neither | elsewhere
    assert {"svh_grid_" + m for m in QCC.OWN} == mutators and len(QCC.READERS) == 5


def test_the_tables_are_whole():
    assert set(QCC.MUTATORS) == set(CC.MATRIX_MUTATORS) | set(OCC.OWN) | set(PCC.OWN) | set(QCC.OWN) == set(QCC.EXPECT) == set(QCC.RULES)
    assert QCC.CF_DROPS == [m for m in CC.MATRIX_MUTATORS if CC.EXPECT[m]["footprint_cost"] == CC.CHANGES]
    for m in ("clear", "set_window", "scroll", "follow", "add_points", "observe_points", "observe_empty", "set_traversability", "set_roll",
              "set_roll_headings"):
        assert m in QCC.CF_DROPS, m
    for m in QCC.LEFT_ALONE:                                      # the planner, the candidates, the objects, the prediction: nothing
        assert m in QCC.MUTATORS and not QCC.RULES[m] and all(QCC.served_from_cache(m, n) for n in QCC.CACHED), m
    for m in QCC.OWN:                                             # the layer's own: the field, not CF
        assert QCC.RULES[m] == {"pose", "path"} and QCC.served_from_cache(m, "pose:CF") and not QCC.served_from_cache(m, "pose:POT")
    pairs = [(m, n) for m in QCC.EXPECT for n in QCC.READERS if QCC.EXPECT[m][n] == QCC.CHANGES]
    assert all(p in pairs and reason for p, reason in QCC.UNSHOWN.items()) and len(QCC.UNSHOWN) <= 0.1 * len(pairs), (len(QCC.UNSHOWN), len(pairs))


def test_the_scene_has_a_field_and_a_path(baseline):
    ref = rig()
    cf, pot, dir_, counted = QCC.ref_field(ref)
    given, counted2, reached = QCC.ref_stats(ref)
    assert given == 3 and counted == counted2 >= 2 and reached > 200 and (pot == QR.FAR).any() and (cf == 255).any() and (cf >= 253).sum() > 100
    path = np.frombuffer(baseline["pose_path"].split(b"|")[0], np.int32).reshape(-1, 3)
    tail = np.frombuffer(baseline["pose_path"].split(b"|")[1], np.int64)
    assert tail[0] == QR.FOUND and len(path) >= 5 and tail[1] < QR.FAR
    assert len(set(path[:, 2].tolist())) >= 2                     # it turns on its way through the gap


@pytest.mark.parametrize("m", list(QCC.MUTATORS))
def test_the_matrix_on_the_restatement(baseline, m):
    ref = rig()
    try:
        QCC.MUTATORS[m](None, ref, None)
    except Exception as e:                                        # a refusal of the restatement leaves it as it was
        assert type(e).__name__ in ("Refused", "ValueError"), e
    after = QCC.read_ref(ref)
    for n in QCC.READERS:
        if QCC.EXPECT[m][n] == QCC.KEEPS:
            assert after[n] == baseline[n], (m, n, "the documented rule says this output stays")
        elif (m, n) in QCC.UNSHOWN:
            assert after[n] == baseline[n], (m, n, "listed as UNSHOWN, yet the scene shows it: take it off the list")
        else:
            assert after[n] != baseline[n], (m, n, "the scene does not show this change")


def test_clear_and_set_window_forget_the_goals():
    for m in ("clear", "set_window"):
        ref = rig()
        QCC.MUTATORS[m](None, ref, None)
        assert QCC.ref_stats(ref) == (0, 0, 0), m
    ref = rig()
    QCC.MUTATORS["scroll"](None, ref, None)
    assert QCC.ref_stats(ref)[0] == 3                             # they survive a scroll

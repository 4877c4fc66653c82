"""CPU: the tables of tests/grid_obj_cache_cases.py against the composed restatement.  tests/test_grid_obj_cache_gpu.py asks the
device, after every mutator of the grid, for every output of the object layer and compares it with a fresh object and with the
restatement; that comparison is only as good as its tables, so this file pins them without a device: every entry of
include/svh_grid_obj.h is classified, every mutator of tests/grid_cache_cases.py is in the matrix, every CHANGES cell does change
the restatement's output on the scene (or is listed, with its reason, among the few the scene cannot show), every KEEPS cell keeps
it, and the scene has objects of every kind and tracks with a history."""
import os
import re

import numpy as np
import pytest

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_obj_ref as OR
import helpers as H


def rig():
    ref = CC.new_ref()
    OCC.scene(None, ref)
    return ref


@pytest.fixture(scope="module")
def baseline():
    return OCC.read_ref(rig())


def test_every_entry_of_the_header_is_classified():
    text = open(os.path.join(H.ROOT, "include", "svh_grid_obj.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    entries = set(re.findall(r"\b(svh_grid_[a-z0-9_]+)\s*\(", text))
    readers = {"svh_grid_get_obj_plane", "svh_grid_get_objects", "svh_grid_get_object_stats", "svh_grid_get_tracks", "svh_grid_get_track_plane",
               "svh_grid_get_track_stats"}
    mutators = {"svh_grid_set_objects", "svh_grid_objects_step", "svh_grid_objects_reset"}
    neither = {"svh_grid_obj_params_default", "svh_grid_get_objects_params"}
    image = {"svh_grid_render_objects"}                           # compared with the restatement per frame in tests/test_grid_obj_gpu.py
    assert entries == readers | mutators | neither | image
    assert {"svh_grid_" + m for m in OCC.OWN} == mutators and len(OCC.READERS) == 7


def test_the_tables_are_whole():
    assert set(OCC.MUTATORS) == set(CC.MATRIX_MUTATORS) | set(OCC.OWN) == set(OCC.EXPECT) == set(OCC.RULES)
    assert set(OCC.OTHER_LAYERS) <= set(CC.MATRIX_MUTATORS)
    for m in OCC.OTHER_LAYERS:                                    # goals, roll parameters, align parameters ...: the objects stay valid
        assert all(OCC.EXPECT[m][n] == OCC.KEEPS for n in OCC.READERS) and all(OCC.served_from_cache(m, n) for n in OCC.CACHED), m
    changing = [m for m in CC.MATRIX_MUTATORS if "obj" in OCC.RULES[m]]
    assert sorted(changing) == sorted(["clear", "set_window", "scroll", "follow", "add_points", "add_points_device", "add_view", "add_points_from",
                                       "add_view_lists_from", "observe_points", "observe_view_lists", "observe_empty"])
    assert [m for m in OCC.MUTATORS if "tracks" in OCC.RULES[m]] == ["set_window", "set_objects", "objects_step", "objects_reset"]
    pairs = [(m, n) for m in OCC.EXPECT for n in OCC.READERS if OCC.EXPECT[m][n] == OCC.CHANGES]
    assert all(p in pairs and reason for p, reason in OCC.UNSHOWN.items()) and len(OCC.UNSHOWN) <= 0.1 * len(pairs), (len(OCC.UNSHOWN), len(pairs))


def test_the_scene_has_objects_of_every_kind_and_tracks_with_a_history(baseline):
    ref = rig()
    flags, label, recs, stats = OCC.ref_objects(ref)
    assert stats[2] >= 2 and stats[4] >= 1 and stats[1] > stats[2] + stats[4]          # kept, structure, and some too small or too low
    assert (flags & OR.KEPT).any() and (flags & OR.LARGE).any() and ((flags & 7) == OR.OBJECT).any()
    t = ref.trk.tracks
    assert len(t) == stats[2] and (t[:, OR.T["age"]] == 1).all() and (t[:, OR.T["flags"]] & OR.BY_OVERLAP).all() and ref.trk.steps == 2
    assert (ref.trk.ids >= 0).sum() == stats[3] and ref.last_assign.tolist() == t[:, 0].tolist()


@pytest.mark.parametrize("m", list(OCC.MUTATORS))
def test_the_matrix_on_the_restatement(baseline, m):
    ref = rig()
    OCC.MUTATORS[m](None, ref, None)
    after = OCC.read_ref(ref)
    for n in OCC.READERS:
        if OCC.EXPECT[m][n] == OCC.KEEPS:
            assert after[n] == baseline[n], (m, n, "the documented rule says this output stays")
        elif (m, n) in OCC.UNSHOWN:
            assert after[n] == baseline[n], (m, n, "listed as UNSHOWN, yet the scene shows it: take it off the list")
        else:
            assert after[n] != baseline[n], (m, n, "the scene does not show this change")


def test_a_step_after_each_mutator_goes_on_from_the_tracks_that_are(baseline):
    """the tracks survive what the header says they survive: after a clear and the scene again the ids are the same"""
    ref = rig()
    ids = ref.trk.tracks[:, 0].tolist()
    CC.MUTATORS["clear"](None, ref, None)
    assert OCC.read_ref(ref)["tracks"] == baseline["tracks"]
    OCC.objects_step(None, ref, None)                             # nothing there: every track is missed
    assert (ref.trk.tracks[:, OR.T["flags"]] & OR.MISSED).all() and ref.trk.tracks[:, 0].tolist() == ids
    CC.MUTATORS["set_window"](None, ref, None)
    OCC.MUTATORS["set_window"](None, ref, None)
    assert len(ref.trk.tracks) == 0 and ref.trk.next_id == 0

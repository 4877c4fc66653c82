"""CPU: the tables of tests/grid_time_cache_cases.py against the text they were written from: every entry of
include/svh_grid_time.h is classified, the mutators of the four existing case files and of the archive are all in the matrix, and
what the head comment of the header names as leaving the layer alone is what the table lists.  tests/test_grid_time_cache_gpu.py
runs the matrix on the device."""
import os
import re

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pose_cache_cases as QCC
import grid_pred_cache_cases as PCC
import grid_time_cache_cases as TCC
import helpers as H


def test_every_entry_of_the_header_is_classified():
    text = open(os.path.join(H.ROOT, "include", "svh_grid_time.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    entries = set(re.findall(r"\b(svh_grid_[a-z0-9_]+)\s*\(", hdr))
    readers = {"svh_grid_get_time_plane", "svh_grid_get_time_stats", "svh_grid_time_path", "svh_grid_render_time"}
    mutators = {"svh_grid_set_time"}
    neither = {"svh_grid_time_params_default", "svh_grid_get_time"}
    assert entries == readers | mutators | neither
    assert {r[0] for r in TCC.READERS.values()} == {"static", "field", "path"} and len(TCC.CACHED) == 5
    assert set(TCC.OWN) == {"set_time_wait", "set_time_layers", "set_time_release"}


def test_every_mutator_of_the_existing_case_files_is_in_the_matrix():
    for table in (CC.MATRIX_MUTATORS, OCC.MUTATORS, PCC.MUTATORS, QCC.MUTATORS, TCC.ARCHIVE, TCC.OWN):     # the matrix of tests/grid_cache_cases.py
        assert set(table) <= set(TCC.MUTATORS)
    assert set(TCC.LEFT_ALONE) <= set(TCC.MUTATORS) and set(TCC.KEEPS_STATIC) <= set(TCC.OWN)
    from svhip import grid as G                                                 # what the layer's own mutators and readers call exists
    for method in ("set_time", "time_plane", "time_stats", "time_path"):
        assert callable(getattr(G.Grid, method)), method


def test_what_the_header_names_as_leaving_the_layer_alone_is_listed():
    text = " ".join(open(os.path.join(H.ROOT, "include", "svh_grid_time.h")).read().split())
    assert "The * frontier, rollout, candidate, alignment and pose parameters and goals, and svh_grid_set_archive with its mutators, leave them * alone" in text
    for word, m in (("frontier", "set_frontier"), ("rollout", "set_roll"), ("candidate", "roll_set_candidates"), ("alignment", "set_align"),
                    ("pose", "set_pose"), ("pose", "pose_set_goals"), ("archive", "set_archive")):
        assert m in TCC.LEFT_ALONE, (word, m)
    # what must not be there: everything the header says the layer follows
    for m in ("add_points", "scroll", "clear", "set_window", "set_traversability", "set_plan", "plan_set_goals", "objects_step", "objects_reset",
              "set_objects", "set_predict") + tuple(TCC.OWN):
        assert m not in TCC.LEFT_ALONE, m
    assert "svh_grid_set_time makes no other layer stale" in text

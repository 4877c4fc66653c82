"""CPU: what tests/test_grid_archive_cache_gpu.py relies on, pinned without a device.  That file asks the device for every cached
output after the archive's mutators and after a scroll that restores; it is only as good as its lists, so this file checks that
every entry of include/svh_grid_archive.h is classified, that the mutators it applies are the header's, that the case files it
imports still offer the cached readers it counts on, and -- on the restatement -- that the archive's mutators change no plane of the
window while a scroll away and back restores every one of them."""
import os
import re

import numpy as np

import grid_archive_ref as AR
import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pose_cache_cases as QCC
import grid_pred_cache_cases as PCC
import helpers as H
import test_grid_archive as TA
import test_grid_archive_cache_gpu as ACG


def test_every_entry_of_the_header_is_classified():
    text = open(os.path.join(H.ROOT, "include", "svh_grid_archive.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    entries = set(re.findall(r"\b(svh_grid_[a-z0-9_]+)\s*\(", text))
    mutators = {"svh_grid_set_archive", "svh_grid_archive_clear", "svh_grid_archive_trim"}          # of the archive; of no cache
    readers = {"svh_grid_get_region", "svh_grid_render_region", "svh_grid_archive_tiles", "svh_grid_get_archive_stats"}   # cache nothing
    neither = {"svh_grid_archive_params_default", "svh_grid_get_archive"}
    assert entries == mutators | readers | neither
    applied = {"svh_grid_" + re.sub(r"_(same|off)$", "", m) for m in ACG.MUTATORS}
    assert applied == mutators
    assert '#include "svh_grid_archive.h"' in open(os.path.join(H.ROOT, "include", "svh_grid.h")).read()


def test_the_case_files_offer_the_cached_readers():
    cached = [n for n, r in CC.READERS.items() if r.cached is True]
    assert len(cached) >= 15 and {"get:count", "local:STATE", "trav:cost", "plan:POT", "front:LABEL", "align_field"} <= set(cached)
    assert OCC.CACHED and PCC.CACHED and QCC.CACHED and "pose:CF" in QCC.CACHED
    assert "scroll" in CC.MATRIX_MUTATORS and CC.EXPECT["scroll"]["get:count"] == CC.CHANGES      # a scroll drops the accumulators' layers


def test_the_mutators_and_the_restoring_scroll_on_the_restatement():
    from svhip import grid
    grid._bind()
    ref = TA.filled(grid, 33, 17, (-20, 9), 64)
    want = TA.everything(ref)
    ref.scroll(5, 3)
    assert not TA.same(TA.everything(ref), want)
    ref.scroll(-5, -3)
    assert TA.same(TA.everything(ref), want) and ref.archive_stats()["restored"] > 0
    for m in (lambda r: r.set_archive(64), lambda r: r.archive_trim(0, 0, 5, 5), lambda r: r.archive_clear(), lambda r: r.set_archive(32),
              lambda r: r.set_archive(0)):
        m(ref)
        assert TA.same(TA.everything(ref), want)
    assert np.array_equal(ref.region(-20, 9, 33, 17)["count"], want["count"])

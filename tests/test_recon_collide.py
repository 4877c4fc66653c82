"""CPU: scene `collide` of Reconstruction (tests/golden/recon_collide.npz, make_goldens_recon_collide.py;
recon_ref.collide_scene): the sizes and collisions at which the kernels of the resident track table
(recon_track_kernels.hip) can go wrong, which the realistic drives of recon.npz and recon_shared.npz do not contain.

What the scene is there for is asserted here on the STORED matches, with the parallel form of the association
(test_recon_resident.parallel_update) and with the reference's sequential rule (recon_ref.sequential_update): the exact
n / n_old sequence with 0, 1, 1023, 1024, 1025, 2048, 2049 and 3000 in both, a large update that loses nothing, an
empty one that loses 3000 tracks, at least 50 feature indices shared by tracks of different blocks of 256 and asked for
by a match (10 of them by tracks of three blocks), at least 50 i1p values named by two to four matches of different
blocks (some of them shared indices), and an index table that is about n in some updates and far above n in others.
These are conditions: a fixture that loses one fails here.

Then: the live reference equals the record, recon_core.h reproduces it bit for bit with its SVD scratch contiguous and
interleaved, and the parallel form reproduces its counts and too-short codes -- while the same form with either rule
turned round (the LOWEST track owns a shared index; the LAST match claims a track) does not, so the scene tells both
rules apart.  The GPU runs are in tests/test_recon_collide_gpu.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import recon_ref as R
from test_recon import CORE_CHECK, same_run
from test_recon_resident import model_matches, parallel_update


@pytest.fixture(scope="module")
def Z():
    with np.load(R.COLLIDE_GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_is_small_and_complete(Z):
    assert os.path.getsize(R.COLLIDE_GOLDEN) <= 1024 * 1024
    assert list(Z["scene_names"]) == ["collide"] and tuple(Z["calib"]) == R.CALIB
    assert [tuple(s) for s in Z["collide_settings"]] == [tuple(float(x) for x in s) for s in R.COLLIDE_SETTINGS]
    assert 3.0 in Z["collide_settings"][:, 1]                 # a setting under which lengths 2 and 3 differ
    assert list(Z["collide_n"]) == R.COLLIDE_N
    for j in range(len(R.COLLIDE_SETTINGS)):
        res = R.unpack_result(Z, "collide_%d" % j)
        assert [r[0] for r in res] == R.COLLIDE_N             # active tracks after an update = its matches
        seen = np.bincount(np.concatenate([r[2] for r in res]), minlength=7)
        assert seen[R.ACCEPTED] >= 500, seen                  # a good share of the lost tracks gives a point
        k = R.COLLIDE_QUIET + 1
        assert len(res[k][2]) == 3000 and (res[k][2] == R.ACCEPTED).sum() > 256   # accepted beyond a round of 256
        last = np.flatnonzero(res[k][2] == R.ACCEPTED).max()
        # ... in the twelfth round too where two frames are enough (the last 951 tracks have two)
        assert last >= (11 * 256 if Z["collide_settings"][j][1] == 2 else 7 * 256), (j, last)


@pytest.mark.parametrize("rule", ["parallel", "sequential"])
def test_scene_has_the_sizes_and_collisions_it_is_there_for(Z, rule):
    scene = R.unpack_scene(Z, "collide")
    p = R.collide_properties(scene, parallel_update if rule == "parallel" else R.sequential_update)
    R.check_collide_properties(p)
    # the record agrees with the replay: lost tracks per update
    assert p["lost"] == list(Z["collide_0_nlost"])
    # the shared indices are spread over the updates they were built into, those named twice follow them
    assert {k for k, _ in p["shared"]} == {k + 1 for k in R.COLLIDE_SHARE_AT}
    assert {k for k, _ in p["named"]} == {k + 1 for k in R.COLLIDE_SHARE_AT}


def test_parallel_association_reproduces_collide_and_turned_rules_do_not(Z):
    assert model_matches(Z, "collide", max) is None
    assert model_matches(Z, "collide", min) is not None                 # the lowest track owns a shared index
    assert model_matches(Z, "collide", max, claim=max) is not None      # the last match claims a track


def test_recon_core_reproduces_collide(Z, tmp_path):
    exe = str(tmp_path / "recon_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, CORE_CHECK])
    scene = R.unpack_scene(Z, "collide")
    path = str(tmp_path / "collide.bin")
    R.write_scene(path, scene)
    for j, s in enumerate(Z["collide_settings"]):
        for S in (1, 64):
            b = subprocess.run([exe, path] + [repr(float(c)) for c in Z["calib"]] + R.setting_args(s) + [str(S)],
                               check=True, capture_output=True).stdout
            same_run(R.parse_run(b, len(scene)), R.unpack_result(Z, "collide_%d" % j), ("collide", j, S))


@pytest.mark.skipif(not R.have_ref(), reason="the reference's sources are not on this machine")
def test_live_reference_equals_collide(Z):
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        scene = R.unpack_scene(Z, "collide")
        path = os.path.join(tmp, "collide.bin")
        R.write_scene(path, scene)
        for j, s in enumerate(Z["collide_settings"]):
            got = R.run_scene(exe, path, len(scene), s, tuple(Z["calib"]))
            same_run(got, R.unpack_result(Z, "collide_%d" % j), ("collide", j))

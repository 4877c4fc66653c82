"""CPU: the estimate-only cases of tests/golden/vo_mono_edges.npz (make_goldens_mono_edges.py, mono_ref.edge_cases):
N and ransac_iters at the sizes the kernels of vo_mono_kernels.hip stride by, and cases in which several hypotheses
reach the largest inlier count.

The fixture's claims are asserted on what it stores: every size is present with that many matches and votes, and in
every tie case the reference's own votes reach their maximum first at h0 and again at an h1 > h0 with
h1 % 256 < h0 % 256 -- the only arrangement in which a reduction over 256 lanes that prefers the lower lane to the
lower index picks another hypothesis than the reference (which keeps a set only when it is strictly larger).  One
case has h0 >= 256, so the lane's own loop has passed a round before it meets its maximum.  The winner's inlier set
must differ from the later one's, or the wrong choice would not show: that is asserted with mono_core.h.

Then the live reference against the stored matches, and mono_core.h against the votes and inliers, as
tests/test_vo_mono.py does for vo_mono.npz.  The GPU runs are in tests/test_vo_mono_edges_gpu.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mono_ref as R
from test_vo_mono import CORE_CHECK, run_core_check


@pytest.fixture(scope="module")
def Z():
    with np.load(R.EDGE_GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_size(Z):
    assert os.path.getsize(R.EDGE_GOLDEN) <= 1024 * 1024
    names = list(Z["est_names"])
    assert names == ["n%d" % n for n in R.EDGE_N] + ["iters%d" % i for i in R.EDGE_ITERS] + [t[0] for t in R.EDGE_TIES]
    assert set(R.EDGE_N) == {63, 64, 65, 255, 256, 257, 1024}
    assert set(R.EDGE_ITERS) == {0, 1, 31, 32, 33, 255, 256, 257}
    demo = R.param_vector(R.DEMO)
    for n in R.EDGE_N:
        assert len(Z["est_n%d_matches" % n]) == n and np.array_equal(Z["est_n%d_params" % n], demo)
        assert len(Z["est_n%d_votes" % n]) == 2000 and int(Z["est_n%d_ok" % n]) == 1
    for it in R.EDGE_ITERS:
        p = Z["est_iters%d_params" % it]
        assert int(p[5]) == it == len(Z["est_iters%d_votes" % it]) and np.array_equal(np.delete(p, 5), np.delete(demo, 5))
        assert len(Z["est_iters%d_matches" % it]) == R.EDGE_ITERS_N
        assert int(Z["est_iters%d_ok" % it]) == (it > 0)
    assert len(Z["est_iters0_inliers"]) == 0 and np.array_equal(Z["est_iters0_motion"], np.eye(4))
    for name in names:
        v = Z["est_%s_votes" % name]
        if len(v):
            assert len(Z["est_%s_inliers" % name]) == v.max(), name


def test_tie_cases_have_a_later_maximum_in_a_lower_lane(Z, tmp_path):
    exe = str(tmp_path / "mono_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, CORE_CHECK])
    first = []
    for name, n, _, thr in R.EDGE_TIES:
        votes, m, p = Z["est_%s_votes" % name], Z["est_%s_matches" % name], Z["est_%s_params" % name]
        assert len(m) == n and p[6] == thr
        tie = R.tie_of(votes)
        assert tie is not None, name
        h0, h1, most, reach = tie
        assert h0 == int(np.argmax(votes)) and h0 < h1 and h1 % 256 < h0 % 256 and votes[h0] == votes[h1] == most
        assert reach >= 2 and most == len(Z["est_%s_inliers" % name])
        first.append(h0)
        # choosing by lane would show: the hypothesis a reduction returns that prefers the lower lane, and the one it
        # returns that prefers the higher, each have another inlier set than h0 (mono_core.h's, with the winner looked
        # for from that hypothesis on)
        for other in R.lane_winners(votes):
            assert other > h0 and votes[other] == most, name
            cut = np.concatenate([p[:5], [other + 1], p[6:]])
            a = run_core_check(exe, str(tmp_path), m, cut, 1)
            b = run_core_check(exe, str(tmp_path), m, cut, 1, first=other)
            assert np.array_equal(a[0], votes[:other + 1]) and np.array_equal(a[1], Z["est_%s_inliers" % name]), name
            assert len(b[1]) == most and not np.array_equal(a[1], b[1]), (name, other)
    assert any(h >= 256 for h in first) and any(h < 256 for h in first), first


def test_mono_core_reproduces_votes_and_inliers(Z, tmp_path):
    exe = str(tmp_path / "mono_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, CORE_CHECK])
    for name in Z["est_names"]:
        for S in (1, 32):
            votes, inl = run_core_check(exe, str(tmp_path), Z["est_%s_matches" % name], Z["est_%s_params" % name], S)
            assert np.array_equal(votes, Z["est_%s_votes" % name]), (name, S)
            if len(votes):
                assert np.array_equal(inl, Z["est_%s_inliers" % name]), (name, S)


@pytest.mark.skipif(not R.have_ref(), reason="the reference's sources are not on this machine")
def test_live_reference_equals_edges(Z):
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        for name in Z["est_names"]:
            ok, inl, T, votes = R.run_estimate(exe, tmp, Z["est_%s_params" % name], Z["est_%s_matches" % name])
            assert ok == Z["est_%s_ok" % name] and np.array_equal(inl, Z["est_%s_inliers" % name]), name
            assert T.tobytes() == Z["est_%s_motion" % name].tobytes(), name
            assert np.array_equal(votes, Z["est_%s_votes" % name]), name

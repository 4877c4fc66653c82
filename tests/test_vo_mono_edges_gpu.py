"""GPU: the estimate-only cases of tests/golden/vo_mono_edges.npz (what they contain is asserted in
tests/test_vo_mono_edges.py) through svh_vo_mono_process_matches and the lockstep entry
svh_vo_mono_process_matches_batch, against the reference's record.  Only committed fixtures are read.

As in tests/test_vo_mono_gpu.py: the return value, the votes of EVERY hypothesis and the inlier indices must be
identical, the motion within that file's TOL.  In the tie cases several hypotheses have the winner's count and another
inlier set: k_mono_select has to return the first of them.

Objects run in lockstep only with equal parameters.  The cases n<N> have the parameters of syn9 and identical of
vo_mono.npz, which leave before RANSAC: they run side by side with them, N from 9 to 1024 in one call, forwards and
backwards (grid x is the largest job's; the largest job is not always job 0).  The other cases differ in
ransac_iters or threshold; each runs in lockstep beside copies of itself and beside syn9 and identical given ITS
parameters -- what those two return (false, no vote, no inlier, the identity) does not depend on them."""
import ctypes as C

import numpy as np
import pytest

import mono_ref as R
from test_vo_mono_gpu import TOL, params

pytestmark = pytest.mark.gpu
EARLY = ["syn9", "identical"]


@pytest.fixture(scope="module")
def Z():
    out = {}
    for path in (R.GOLDEN, R.EDGE_GOLDEN):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files if k != "est_names"})
            out.setdefault("edge_names", [])
            if path == R.EDGE_GOLDEN:
                out["edge_names"] = [str(n) for n in z["est_names"]]
    return out


@pytest.fixture(scope="module")
def S():
    import svhip
    return svhip


def check(Z, vo, ok, name):
    assert int(ok) == int(Z["est_%s_ok" % name]), name
    assert np.array_equal(vo.votes(), Z["est_%s_votes" % name]), (name, "votes")
    assert np.array_equal(vo.inliers(), Z["est_%s_inliers" % name]), (name, "inliers")
    err = np.abs(vo.motion() - Z["est_%s_motion" % name]).max()
    assert err < TOL, (name, "motion", err)


def test_early_cases_do_not_depend_on_parameters(Z):
    for name in EARLY:
        assert int(Z["est_%s_ok" % name]) == 0 and len(Z["est_%s_votes" % name]) == 0
        assert len(Z["est_%s_inliers" % name]) == 0 and np.array_equal(Z["est_%s_motion" % name], np.eye(4))


def test_every_case_alone(S, Z):
    for name in Z["edge_names"]:
        vo = S.VoMono(params(S, Z["est_%s_params" % name]))
        ok = vo.process_matches(Z["est_%s_matches" % name])
        check(Z, vo, ok, name)
        vo.close()


def run_batch(S, Z, jobs):
    """jobs: (case, case whose parameters the object gets); one call, every object against its own record"""
    vos = [S.VoMono(params(S, Z["est_%s_params" % p]), private_rand=0) for _, p in jobs]
    ok = S.VoMono.process_matches_batch(vos, [Z["est_%s_matches" % n] for n, _ in jobs])
    for vo, o, (name, _) in zip(vos, ok, jobs):
        check(Z, vo, o, name)
        vo.close()


@pytest.mark.parametrize("order", ["forwards", "backwards"])
def test_sizes_side_by_side_in_lockstep(S, Z, order):
    names = ["n%d" % n for n in R.EDGE_N]
    for n in names + EARLY:
        assert np.array_equal(Z["est_%s_params" % n], Z["est_syn9_params"]), n     # equal parameters: lockstep
    jobs = [(n, n) for n in names[:3] + EARLY[:1] + names[3:] + EARLY[1:]]
    run_batch(S, Z, jobs if order == "forwards" else jobs[::-1])


@pytest.mark.parametrize("order", ["forwards", "backwards"])
def test_every_case_in_one_call(S, Z, order):
    """all new cases with syn9 and identical in ONE call: the parameters differ, so the entry runs the groups it can"""
    jobs = [(n, n) for n in Z["edge_names"] + EARLY]
    run_batch(S, Z, jobs if order == "forwards" else jobs[::-1])


@pytest.mark.parametrize("order", ["forwards", "backwards"])
def test_iteration_counts_and_ties_in_lockstep(S, Z, order):
    for name in Z["edge_names"]:
        if name.startswith("n"):
            continue
        jobs = [(name, name), ("syn9", name), (name, name), ("identical", name)]
        run_batch(S, Z, jobs if order == "forwards" else jobs[::-1])

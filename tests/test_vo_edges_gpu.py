"""k_vo_ransac / k_vo_refine against the oracle at their structural switches, under ties and on degenerate matches
(tests/vo_edge_cases.py lists the cases and says why each is a fair one; tests/test_vo_edges.py checks that on the CPU).

Per admitted case, product and oracle both from srand(0): status, inlier list and the winner's index identical, the
motion within TOL; and through svh_vo_get_hypotheses EVERY hypothesis, not only the winner -- votes identical, vectors
within TOL -- on the hypotheses that the oracle's own four trig modes leave in place (a FAILED one: the vote only).
One object walked through sizes on both sides of the LDS limit; three objects in one lockstep launch that holds jobs
of both memory forms."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import vo_edge_cases as E

pytestmark = pytest.mark.gpu
TOL = E.TOL
LIBC = C.CDLL(None)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def check_final(tag, a, b, winner=True):
    """a: oracle (exact trig), b: product"""
    dev = float(np.abs(a.tr - b.tr).max()) if a.ok and b.ok else 0.0
    print("%s: status %d / %d, inliers %d / %d, winner %d / %d, motion differs by %.2e" % (
        tag, a.ok, b.ok, len(a.inliers), len(b.inliers), a.winner(), b.winner(), dev))
    assert b.ok == a.ok
    assert np.array_equal(a.inliers, b.inliers)
    if winner:
        assert b.winner() == a.winner()
    if a.ok:
        assert dev < TOL


def check_hypotheses(tag, a, b, mask):
    assert len(b.votes) == len(a.votes) == len(mask)
    live = mask & (a.votes >= 0)
    dev = float(np.abs(a.hyp[live] - b.hyp[live]).max()) if live.any() else 0.0
    print("%s: %d hypotheses, %d compared (%d of them FAILED), votes differ on %d, vectors by %.2e; masked: votes "
          "differ on %d" % (tag, len(mask), int(mask.sum()), int((mask & (a.votes < 0)).sum()),
                            int((a.votes[mask] != b.votes[mask]).sum()), dev, int((a.votes[~mask] != b.votes[~mask]).sum())))
    assert np.array_equal(a.votes[mask], b.votes[mask])
    assert np.isfinite(b.hyp[live]).all() and dev < TOL


@pytest.mark.parametrize("case", E.PARITY_CASES, ids=repr)
def test_edge_case_matches_oracle(case):
    rs = E.oracle_modes(case.name)            # (before the product object exists: its constructor is the srand(0))
    assert E.admitted(rs)
    vo = H.ProductVo(case.prm())
    b = E.run_steps(vo, [case.matches()])[0]
    check_final(case.name, rs[0], b, winner=case.hypotheses or all(r.winner() == rs[0].winner() for r in rs))
    if b.winner() >= 0:
        assert b.votes[b.winner()] == len(b.inliers)
    if case.hypotheses:
        check_hypotheses(case.name, rs[0], b, E.stable_mask(rs))
    else:   # nearly every hypothesis moves with the last bit: the count, and FAILED where all four modes say FAILED
        assert len(b.votes) == len(rs[0].votes)
        sure = np.all([r.votes < 0 for r in rs], axis=0)
        assert (b.votes[sure] < 0).all()


def test_single_match_leaves_the_object_usable():
    """40 copies of one match is no parity case (the oracle's own inlier list depends on the last bit of a sine):
    status 0, no error, and the next estimate on the same object is the oracle's"""
    c = E.BY_NAME["one_match_x40"]
    nxt = E.BY_NAME["n64"]
    o = E.new_oracle(c.prm())
    o.estimate_motion(c.matches())
    a = E.run_steps(o, [nxt.matches()])[0]
    assert E.admitted(E.oracle_modes(nxt.name))
    import svhip as S
    vo = H.ProductVo(c.prm())
    ok, _ = vo.estimate_motion(c.matches())
    assert ok == 0, S.last_error()
    votes, hyp = vo.hypotheses()
    assert len(votes) == 200 and len(vo.inliers()) in (0, 40)
    b = E.run_steps(vo, [nxt.matches()])[0]
    check_final("after the single match", a, b)


def test_one_object_through_small_and_large_sets():
    """N = 657, 64, 656, 3000, 6, 5, 257 on ONE object (d_flags, d_J, the pinned inlier list are grown, never shrunk;
    the refinement changes between LDS and global scratch from call to call); at N = 5 the reference returns before
    it clears the inliers, so those of the N = 6 call stay"""
    seq = E.oracle_modes("sequence")
    vo = H.ProductVo(H.vo_defaults())
    got = E.run_steps(vo, E.sequence_matches())
    for i, n in enumerate(E.SEQUENCE):
        rs = [s[i] for s in seq]
        assert E.admitted(rs)
        check_final("step %d (N = %d)" % (i, n), rs[0], got[i])
        check_hypotheses("step %d (N = %d)" % (i, n), rs[0], got[i], E.stable_mask(rs))
    i5 = E.SEQUENCE.index(5)
    assert len(got[i5].votes) == 0 and len(got[i5].inliers) > 0
    assert np.array_equal(got[i5].inliers, got[i5 - 1].inliers)


def run_trio(batched):
    import svhip.resident as RS
    fr = E.trio_frames()
    vos = [H.ProductVo(H.vo_defaults(**E.TRIO_PARAMS)) for _ in fr]
    LIBC.srand(E.TRIO_SRAND)
    log = []
    for call in range(4):
        a = [q[0] if call % 2 == 0 else q[2] for q in fr]
        b = [q[1] if call % 2 == 0 else q[3] for q in fr]
        before = RS.lockstep_counts()
        if batched:
            _, ok = H.product_vo_process_batch(vos, a, b)
            ok = list(ok)
        else:
            ok = [vo.process(a[k], b[k]) for k, vo in enumerate(vos)]
        after = RS.lockstep_counts()
        log.append(dict(ok=ok, n=[vo.num_matches() for vo in vos], motion=[vo.motion().copy() for vo in vos],
                        inliers=[vo.inliers().copy() for vo in vos], matches=[vo.matches().copy() for vo in vos],
                        hyp=[vo.hypotheses() for vo in vos], batched_phases=after[0] - before[0]))
    return log


def test_lockstep_launch_with_jobs_of_both_forms():
    """k_vo_refine_b with K = 3 jobs under one dynamic-LDS size, the largest: one job keeps its rows in LDS, two in
    global scratch.  The batch call equals three single calls in the same order, every hypothesis bit for bit."""
    loop = run_trio(False)
    bat = run_trio(True)
    for call in range(4):
        l, b = loop[call], bat[call]
        print("call %d: ok %s / %s, N %s / %s, batched phases %d" % (call, l["ok"], b["ok"], l["n"], b["n"],
                                                                     b["batched_phases"]))
        assert l["ok"] == b["ok"] and l["n"] == b["n"]
        for k in range(3):
            assert np.array_equal(l["motion"][k], b["motion"][k]), ("motion", call, k)
            assert np.array_equal(l["inliers"][k], b["inliers"][k]), ("inliers", call, k)
            assert l["matches"][k].tobytes() == b["matches"][k].tobytes(), ("matches", call, k)
            assert np.array_equal(l["hyp"][k][0], b["hyp"][k][0]), ("votes", call, k)
            assert l["hyp"][k][1].tobytes() == b["hyp"][k][1].tobytes(), ("hypothesis vectors", call, k)
        if call >= 2:   # (calls 0 and 1 bootstrap: the batch entry runs them one by one)
            assert b["ok"] == [1, 1, 1]
            assert b["batched_phases"] > 0
            assert sum(n <= E.LDS_MAX_N for n in b["n"]) == 1 and sum(n > E.LDS_MAX_N for n in b["n"]) == 2, b["n"]
            assert all(len(h[0]) == 200 and (h[0] > 0).any() for h in b["hyp"])

"""Which edge cases of VisualOdometryStereo::estimateMotion are fair parity cases (tests/vo_edge_cases.py)?

CPU only, oracle only.  The device's sine / cosine may differ from glibc's in the last bit, so a case may be held
against the oracle within TOL only if the ORACLE's own answer survives such a change: every case is run with the
linearisation's sines and cosines exact, one ulp up, one ulp down and in a seeded mix (orc_vo_set_trig_mode), and

  admission   status and inlier list identical in the four modes, motion moved by < 1e-10 (a tenth of TOL)
  mask        a hypothesis is compared on the device only if its vote is identical in the four modes and its vector
              stays finite and within 1e-10; the mask may hide at most 5 % of the hypotheses of a size or parameter
              case and at most 20 % of a degenerate one.  The caps are conditions of the cases, not results.

Measured (hidden hypotheses of 200; motion moved by at most 5.4e-15 in every admitted case):
  sizes        n6 0, n7 7, n63 7, n64 5, n65 2, n255 3, n256 3, n257 4, n511 5, n512 3, n513 5, n655 7, n656 8,
               n657 3, n658 4, n1025 4, all-inlier 656 / 657: 0
  parameters   N = 257: 2 (0 with 1 or 3 iterations and with cu = 0); N = 657: 3-4 (0 likewise)
  degenerate   copy of first half 8, zero disparity on every second 31, one row 0, 97 % outliers 19, noise 3.0: 5,
               exact 0, zero motion 0, large motion 13
  final only   negative disparity, two matches x 20 (nearly every hypothesis moves), one match x 40 (not admitted by
               rule: a measurement found its inlier list empty in one mode and full in the others)
  sequence     657, 64, 656, 3000, 6, 5, 257 on one object: 5, 4, 5, 4, 0, -, 7"""
import numpy as np
import pytest

import helpers as H
import vo_edge_cases as E


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def hidden(rs):
    m = E.stable_mask(rs)
    return int((~m).sum()), len(m)


@pytest.mark.parametrize("case", E.PARITY_CASES, ids=repr)
def test_final_answer_survives_the_last_bit_of_sine_and_cosine(case):
    rs = E.oracle_modes(case.name)
    same, move = E.final_shift(rs)
    print("%s: N %d, status %d, %d inliers, motion moved %.2e" % (case, len(case.matches()), rs[0].ok,
                                                                   len(rs[0].inliers), move))
    assert same, "status or inlier list depends on the last bit"
    assert move < E.ADMIT, move
    for r in rs[1:]:   # the winner is part of what the device is held to
        assert r.winner() == rs[0].winner()


@pytest.mark.parametrize("case", E.HYP_CASES, ids=repr)
def test_mask_hides_no_more_than_its_cap(case):
    rs = E.oracle_modes(case.name)
    h, n = hidden(rs)
    print("%s: %d of %d hypotheses hidden (cap %.0f %%)" % (case, h, n, 100 * case.cap))
    assert n == max(case.prm().ransac_iters, 0)
    assert h <= case.cap * n, (h, n)


def test_sequence_steps_are_admitted_and_within_the_plain_cap():
    seq = E.oracle_modes("sequence")
    left = None
    for i, n in enumerate(E.SEQUENCE):
        rs = [s[i] for s in seq]
        assert E.admitted(rs), (i, n, E.final_shift(rs))
        h, cnt = hidden(rs)
        print("step %d: N %d, status %d, %d inliers, %d of %d hidden" % (i, n, rs[0].ok, len(rs[0].inliers), h, cnt))
        if n < 6:   # the early return: no hypotheses, the previous call's inliers stay (viso_stereo.cpp:91-94)
            assert cnt == 0 and rs[0].ok == 0
            assert len(left) > 0 and np.array_equal(rs[0].inliers, left)
        else:
            assert cnt == 200 and h <= E.CAP_PLAIN * cnt, (i, n, h)
        left = rs[0].inliers
    ns = [n for n in E.SEQUENCE if n >= 6]
    assert any(E.uses_lds(a) != E.uses_lds(b) for a, b in zip(ns, ns[1:]))     # the forms alternate on one object
    assert any(a > 4 * b for a, b in zip(E.SEQUENCE, E.SEQUENCE[1:]))          # a small N after a large one


def test_single_match_is_not_a_parity_case():
    """40 copies of one match: an earlier measurement found status 0 in every mode but the inlier list empty in one
    and full in the others, so the case keeps only 'status 0, no error, object usable afterwards'"""
    c = E.BY_NAME["one_match_x40"]
    assert not c.parity and not c.hypotheses
    for r in E.oracle_modes(c.name):
        assert r.ok == 0
        assert len(r.inliers) in (0, 40)


def test_both_memory_forms_see_both_row_parities():
    """wave_gn_step takes 4 nin rows in turns of 8: an odd inlier count leaves half a turn.  Both parities occur among
    the admitted cases whose refinement runs (nin >= 6) in LDS, and among those in global scratch."""
    seen = set()
    for c in E.PARITY_CASES:
        r = E.oracle_modes(c.name)[0]
        if len(r.inliers) >= 6:
            seen.add((E.uses_lds(len(c.matches())), len(r.inliers) % 2))
    assert seen == {(True, 0), (True, 1), (False, 0), (False, 1)}
    # ... and the row count reaches the last LDS row, and an odd count the global tail, with every match an inlier
    assert len(E.oracle_modes("all_inliers_n656")[0].inliers) == 656 == E.LDS_MAX_N
    assert len(E.oracle_modes("all_inliers_n657")[0].inliers) == 657


def test_lds_limit_is_where_the_cases_put_it():
    """vlaunch_estimate: lds_rows = roundup8(4 N) + 8 rows of 7 doubles, dropped to 0 above 144 KB"""
    fits = lambda n: (((4 * n + 7) & ~7) + 8) * 7 * 8 <= 144 * 1024
    assert fits(E.LDS_MAX_N) and not fits(E.LDS_MAX_N + 1)
    assert {655, 656, 657, 658} <= set(E.SIZES)


@pytest.mark.parametrize("n", E.PARAM_SIZES)
def test_parameter_cases_do_what_they_are_there_for(n):
    r = E.oracle_modes("thr1e6_n%d" % n)[0]
    assert len(r.votes) == 200 and (r.votes == n).all()          # 200 equal votes: the FIRST must win
    assert r.winner() == 0 and len(r.inliers) == n
    r = E.oracle_modes("thr1e-6_n%d" % n)[0]
    assert len(r.votes) == 200 and (r.votes <= 0).all() and (r.votes == 0).any()
    assert r.winner() == -1 and r.ok == 0 and len(r.inliers) == 0  # no winner
    r = E.oracle_modes("cu0_n%d" % n)[0]
    assert len(r.votes) == 200 and (r.votes == -1).all()         # every hypothesis FAILED
    assert r.ok == 0 and len(r.inliers) == 0
    assert len(E.oracle_modes("iters0_n%d" % n)[0].votes) == 0
    assert len(E.oracle_modes("iters1_n%d" % n)[0].votes) == 1
    assert len(E.oracle_modes("iters3_n%d" % n)[0].votes) == 3


def test_degenerate_cases_do_what_they_are_there_for():
    r = E.oracle_modes("exact_n80")[0]
    assert (r.votes == 80).all() and r.winner() == 0             # all 200 votes tie
    m = E.BY_NAME["zero_disparity_every_second"].matches()
    assert (m["u1p"][::2] == m["u2p"][::2]).all()
    m = E.BY_NAME["negative_disparity"].matches()
    assert (m["u1p"] - m["u2p"] < 0).all()
    m = E.BY_NAME["two_matches_x20"].matches()
    assert len(m) == 40 and len(np.unique(m)) == 2
    m = E.BY_NAME["one_match_x40"].matches()
    assert len(m) == 40 and len(np.unique(m)) == 1
    # no case makes a hypothesis non-finite in the oracle: the NaN branch of the pivot search (wave_solve6: pos
    # stays -1; the reference carries irow / icol over) is read, not measured -- see DESIGN.md
    for c in E.CASES:
        for r in E.oracle_modes(c.name):
            assert np.isfinite(r.hyp).all(), c


@pytest.mark.skipif(not H.have_ref_viso(), reason="process() needs the real Triangle (oracle/_ref) for removeOutliers")
def test_lockstep_trio_straddles_the_lds_limit():
    """three objects, three frame variants.  The first two calls bootstrap (run one by one: 1126, 730, 636 matches at
    the second); the third and fourth are lockstep calls, and each holds one N <= 656 and two N >= 657"""
    import ctypes as C
    fr = E.trio_frames()
    vos = [H.OracleVo(H.vo_defaults(**E.TRIO_PARAMS)) for _ in fr]
    C.CDLL(None).srand(E.TRIO_SRAND)
    for call in range(4):
        oks = [vo.process(*(q[0:2] if call % 2 == 0 else q[2:4])) for vo, q in zip(vos, fr)]
        ns = [vo.num_matches() for vo in vos]
        print("call %d: ok %s, N %s" % (call, oks, ns))
        if call >= 1:
            assert oks == [1, 1, 1]
            assert sum(n <= E.LDS_MAX_N for n in ns) == 1 and sum(n > E.LDS_MAX_N for n in ns) == 2, ns

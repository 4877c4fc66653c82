"""Pin the CPU restatement (oracle/) to the reference on the reference's own images at full size:
the seven stereo pairs of libelas/src/main.cpp's demo (1344x391 urban1-4, 900x750 cones,
1282x1110 aloe, 1342x1110 raindeer) under the demo, ROBOTICS and MIDDLEBURY settings, and the
mono sequence I1_000000..6 through the Matcher.  Goldens: tests/golden/make_goldens_full.py.

Every tapped stage is compared by its sha256 (float stages with -0.0 taken as +0.0, the value
semantics of the float compares elsewhere); support and triangle lists exactly.
"""
import numpy as np
import pytest

import helpers as H

ELAS_CASES = ["urban1_demo", "urban2_demo", "urban3_demo", "urban4_demo", "cones_demo", "aloe_demo",
              "raindeer_demo", "urban1_robotics", "urban2_robotics", "urban3_robotics", "urban4_robotics",
              "cones_middlebury", "aloe_middlebury", "raindeer_middlebury", "urban1_robotics_sub"]
MONO_SETS = ["default", "full_res", "refine2"]
T1P1, T1C1 = H.M_TABLES.index("1p1"), H.M_TABLES.index("1c1")


def first_bad_stage(z, run):
    """name of the first hashed stage whose sha256 differs from the golden (None: all equal)"""
    for name in z["hashed"]:
        s = next(k for k, v in H.STAGE_NAMES.items() if v == str(name))
        if s not in run or H.stage_sha256(run[s]) != str(z[str(name) + "_sha256"]):
            return str(name)
    return None


def assert_lists(z, run):
    """support list (u, v, d) and both triangle lists exact, order included; a difference names its first entry"""
    for s in (H.SUPPORT, H.TRI1, H.TRI2):
        a, b = run[s].reshape(-1, 3), z[H.STAGE_NAMES[s]].astype(np.int32).reshape(-1, 3)
        assert a.shape == b.shape, (H.STAGE_NAMES[s], "entries", len(a), "golden", len(b))
        bad = np.flatnonzero((a != b).any(axis=1))
        assert not len(bad), (H.STAGE_NAMES[s], "first differing entry", int(bad[0]), a[bad[0]], "golden", b[bad[0]])


def assert_matches_golden(z, run):
    assert run.status == 0
    assert_lists(z, run)
    bad = first_bad_stage(z, run)
    assert bad is None, "first stage differing from the reference: " + bad
    assert int((run[H.D1_FINAL] >= 0).sum()) == int(z["d1_valid"])
    assert int((run[H.D2_FINAL] >= 0).sum()) == int(z["d2_valid"])


@pytest.mark.parametrize("case", ELAS_CASES)
def test_oracle_matches_full_golden(case, oracle_lib):
    z, prm, l, r = H.full_case(case)
    # the real Triangle when oracle/_ref is there (triangle lists checked too), else the golden lists replayed
    tri = None if H.have_ref_elas() else H.fixture_triangulator([z["tri1"], z["tri2"]])
    assert_matches_golden(z, H.oracle_elas_run(prm, l, r, tri))


def test_known_answer_urban1_full():
    """full-size urban1 under ROBOTICS gives 1590 support points and 3118 / 3118 triangles"""
    for case in ("urban1_robotics", "urban1_demo"):
        z, prm, l, r = H.full_case(case)
        assert l.shape == r.shape == (391, 1344)
        assert (len(z["support"]) // 3, len(z["tri1"]) // 3, len(z["tri2"]) // 3) == (1590, 3118, 3118)


def test_hash_names_the_stage():
    """the golden hashes are sharp: one changed pixel of one stage is reported as that stage"""
    z, prm, l, r = H.full_case("urban1_robotics_sub")
    run = H.oracle_elas_run(prm, l, r, H.fixture_triangulator([z["tri1"], z["tri2"]]))
    assert first_bad_stage(z, run) is None
    seg = run[H.D1_SEG]
    d = seg.copy()
    d[len(d) // 2] += 1
    run.stages[H.D1_SEG] = d
    assert first_bad_stage(z, run) == "d1_seg"
    neg = run[H.PLANES1].copy()
    assert (neg == 0).any()
    neg[neg == 0] = -0.0                      # -0.0 and +0.0 hash alike
    run.stages[H.D1_SEG] = seg
    run.stages[H.PLANES1] = neg
    assert first_bad_stage(z, run) is None


@pytest.mark.skipif(not H.have_ref_elas(), reason="oracle/_ref not built")
@pytest.mark.parametrize("case", ELAS_CASES)
def test_reference_reproduces_full_golden(case):
    """the compiled reference still gives the committed goldens"""
    z, prm, l, r = H.full_case(case)
    assert_matches_golden(z, H.ref_elas_run(prm, l, r))


def mono_params(name):
    z = np.load("%s/full/mono_%s.npz" % (H.GOLDEN, name))
    return z, H.MatcherParams.from_buffer_copy(z["params"].tobytes())


def check_mono_step(z, m, k, got):
    """step k (frames k-1, k) of a mono run against the golden record"""
    i = k - 1
    assert len(got) == int(z["n"][i]), ("step", k, "count")
    assert H.stage_sha256(got) == str(z["sha256"][i]), ("step", k, "matches")
    if "matches_%d" % k in z:
        assert (got == z["matches_%d" % k]).all(), ("step", k, "matches")
    assert H.stage_sha256(m.features(T1P1)) == str(z["t1p1_sha256"][i]), ("step", k, "table 1p1")
    assert H.stage_sha256(m.features(T1C1)) == str(z["t1c1_sha256"][i]), ("step", k, "table 1c1")


@pytest.mark.skipif(not H.have_ref_viso(), reason="oracle needs the real Triangle (oracle/_ref) for removeOutliers")
@pytest.mark.parametrize("name", MONO_SETS)
@pytest.mark.parametrize("impl", ["oracle", "reference"])
def test_mono_sequence_matches_golden(name, impl, oracle_lib):
    """pushBack(I1_k) + matchFeatures(0) over the seven frames: the ring buffer advances six times"""
    z, prm = mono_params(name)
    m = H.OracleMatcher(prm) if impl == "oracle" else H.RefMatcher(prm)
    for k, img in enumerate(H.mono_frames()):
        m.push_back(img)
        if k:
            m.match(0)
            check_mono_step(z, m, k, m.matches())

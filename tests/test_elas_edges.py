"""CPU: the scenes of elas_scenes.py are what test_elas_edges_gpu.py takes them for.

Admission -- on every case the oracle equals the live reference on every stage, the reference is deterministic, and the
status is the one the case lists -- and coverage: the tie, starvation and empty-triangulation counts that make the
scenes worth running are asserted on the reference side (orc_elas_tie_stats counts beside the oracle's two arg-min
searches without touching them).  The collinear support lists also go through the device triangulation core on the CPU
(tests/cxx/dt_core_check --points), which has to end with an empty list there before any kernel sees them.
"""
import os
import subprocess

import numpy as np
import pytest

import elas_scenes as E
import helpers as H

ALL = sorted(E.CASES)
live = pytest.mark.skipif(not H.have_ref_elas(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def counts(oracle_lib):
    return lambda name: E.oracle_run(E.CASES[name])[1]


@live
@pytest.mark.parametrize("name", ALL)
def test_oracle_equals_reference_and_reference_repeats(name, oracle_lib):
    """(every compared image is at least 60 rows high: the reference's staged harness does not run below that)"""
    case = E.CASES[name]
    l, r = case.pair()
    assert l.shape[0] >= 60
    a, a2 = H.ref_elas_run(case.params(), l, r), H.ref_elas_run(case.params(), l, r)
    b = E.oracle_run(case)[0]
    assert a.status == a2.status == b.status == case.status
    assert not [(n, c) for n, c in H.compare_runs(a, a2) if c != 0]
    assert not [(n, c) for n, c in H.compare_runs(a, b) if c != 0]
    assert set(a.stages) <= set(b.stages)          # (the reference's harness has no DCAN_RAW)


@pytest.mark.parametrize("name", ALL)
def test_status_and_kernel_forms(name, counts):
    case = E.CASES[name]
    assert counts(name).status == case.status
    assert E.forms(case.params(), case.w, case.h) == case.kernels


def test_every_form_of_both_matchers_meets_ties(counts):
    seen = {}
    for name, case in E.CASES.items():
        n = counts(name)
        for kernel, ties in zip(case.kernels, (n.support_ties, n.dense_not_lowest)):
            seen[kernel] = max(seen.get(kernel, 0), ties)
    assert set(seen) == {"k_support_lds", "k_support", "k_match_list", "k_match_keyed", "k_match<true>", "k_match<false>"}
    assert all(v >= 10 for v in seen.values()), seen
    assert min(seen[k] for k in ("k_support_lds", "k_support", "k_match_list", "k_match_keyed", "k_match<true>")) >= 500


@pytest.mark.parametrize("scene", E.TIE)
def test_tie_scenes(scene, counts):
    n = counts(scene)
    assert n.dense_ties >= 1000 and n.dense_not_lowest >= 100, n.row()


@pytest.mark.parametrize("scene", E.SUPPORT_TIE + ("binary8",))
def test_support_tie_scenes(scene, counts):
    assert counts(scene).support_ties >= 1000


@pytest.mark.parametrize("scene", E.STARVED)
def test_starved_scenes(scene, counts):
    n = counts(scene)
    assert 3 <= n.support <= 40 and n.valid <= 0.10, n.row()


def test_tiny_scene(counts):
    assert 3 <= counts("tiny").support <= 8


def test_saturated_descriptor_bytes(oracle_lib):
    """0 / 255 cells clamp the Sobel bytes at both ends"""
    for scene in ("binary3", "binary8", "levels2c4"):
        d = E.oracle_run(E.CASES[scene])[0][H.DESC1]
        assert (d == 0).mean() > 0.01 and (d == 255).mean() > 0.01, scene


@pytest.mark.parametrize("name", ["collinear", "collinear-sub_both"])
def test_collinear_scene_has_no_triangle(name, counts):
    run, n = E.oracle_run(E.CASES[name])
    sup = run[H.SUPPORT].reshape(-1, 3)
    assert n.status == 0 and n.support >= 3 and n.tri == (0, 0)
    assert len(set(sup[:, 1])) == 1
    for s in (H.D1_RAW, H.D2_RAW, H.D1_FINAL, H.D2_FINAL):
        assert (run[s] < 0).all()


def test_collinear_scene_with_corner_points(counts):
    n = counts("collinear-corners")
    assert n.status == 0 and min(n.tri) > 0 and n.dense_unevaluated >= 500, n.row()


@pytest.mark.parametrize("name", ALL)
def test_recorded_counts(name, counts):
    """elas_scenes.REACHED is what the cases reach: at least half of every recorded tie count is there (the record itself
    is exact on the machine that wrote it), and the sizes of the support and triangle lists are the recorded ones"""
    got, want = counts(name).row(), E.REACHED[name]
    assert got[:3] == want[:3] and abs(got[3] - want[3]) <= 0.02, (got, want)
    for g, w in zip(got[4:], want[4:]):
        assert g >= w // 2, (got, want)


# ----------------------------------------------------------------------------------------------- triangulations
def _point_sets(name):
    sup = E.oracle_run(E.CASES[name])[0][H.SUPPORT].reshape(-1, 3)
    return {"left": np.stack([sup[:, 0], sup[:, 1]], 1), "right": np.stack([sup[:, 0] - sup[:, 2], sup[:, 1]], 1)}


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", ["collinear", "collinear-corners", "collinear-sub_both", "tiny"])
def test_device_triangulation_core_on_the_cpu(name, side, tmp_path, oracle_lib):
    """the support list of the collinear scene (and, with corner points, of the same scene as a fan of sliver triangles
    over one dense row) through dt_core.h on the CPU, as k_delaunay drives it: it terminates, and its list -- empty for
    the collinear sets -- is the host triangulation's, which in turn is the real Triangle's where that is built"""
    cxx = os.path.join(H.ROOT, "tests", "cxx")
    subprocess.check_call(["make", "-C", cxx, "dt_core_check"], stdout=subprocess.DEVNULL)
    pts = _point_sets(name)[side]
    assert len(np.unique(pts, axis=0)) == len(pts)
    path = tmp_path / "pts.txt"
    path.write_text("%d\n" % len(pts) + "".join("%d %d\n" % (x, y) for x, y in pts))
    xoff = E.CASES[name].params().disp_max
    r = subprocess.run([os.path.join(cxx, "dt_core_check"), "--points", str(path), str(xoff)], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    want = E.oracle_run(E.CASES[name])[1].tri[side == "right"]
    assert "points %d, triangles %d, mismatches 0, shortcuts wrong 0" % (len(pts), want) in r.stdout, r.stdout
    if "corners" not in name and name != "tiny":
        assert want == 0
    import svhip
    mine = svhip.delaunay(pts)
    assert len(mine) == want
    if H.have_ref_elas():
        assert np.array_equal(mine, H.ref_triangulate(pts))

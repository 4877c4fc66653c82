"""GPU parity of the ELAS kernels on the scenes of elas_scenes.py: ties of both arg-min searches in every kernel form
(k_support_lds / k_support; k_match_list, k_match_keyed, k_match<true>, k_match<false>), saturated Sobel bytes, starved
frames, and support sets that Triangle answers with no triangle at all.  test_elas_edges.py shows on the CPU that the
scenes reach what they are here for and that the oracle is the reference on them.

Every case runs three times: with taps through the host form and the device form of the middle stages, every stage
bit-exact against the oracle, and without taps (the production path: fused tiles, descriptors on the fly).
"""
import numpy as np
import pytest

import elas_scenes as E
import helpers as H
from test_elas_gpu import product_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def svhip():
    import svhip as S
    S.lib()
    assert S.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return S


def assert_all_stages(want, got):
    """every stage of both runs, absent == empty (a triangulation without triangles has empty lists and planes)"""
    none = np.zeros(0, np.uint8)
    for s, name in sorted(H.STAGE_NAMES.items()):
        w, g = want.stages.get(s, none), got.stages.get(s, none)
        assert w.size == g.size, (name, w.size, g.size)
        assert np.array_equal(w, g), (name, int((w != g).sum()))


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_every_stage_and_the_production_path(name, svhip, oracle_lib):
    case = E.CASES[name]
    prm = case.params()
    l, r = case.pair()
    want = E.oracle_run(case)[0]
    assert want.status == case.status
    for stage in (0, 1):
        svhip.set_stage(stage)
        try:
            got = product_run(svhip, prm, l, r)
        finally:
            svhip.set_stage(-1)
        assert got.status == case.status, stage
        if case.status == 0:
            assert_all_stages(want, got)
    dh, dw = (l.shape[0] // 2, l.shape[1] // 2) if prm.subsampling else l.shape
    D1, D2 = np.full((dh, dw), -7.0, np.float32), np.full((dh, dw), -7.0, np.float32)
    rc, D1, D2 = svhip.Elas(prm).process(l, r, D1, D2)          # no taps
    assert rc == case.status
    if rc == 0:
        # (== the taps-on maps, which assert_all_stages has just compared with the same arrays)
        assert np.array_equal(D1.ravel(), want[H.D1_FINAL]) and np.array_equal(D2.ravel(), want[H.D2_FINAL])
        assert np.array_equal(D1.ravel(), got[H.D1_FINAL]) and np.array_equal(D2.ravel(), got[H.D2_FINAL])
    else:
        assert (D1 == -7.0).all() and (D2 == -7.0).all()         # elas.cpp:69-75: outputs untouched


@pytest.mark.parametrize("name", ["collinear", "collinear-sub_both"])
def test_empty_triangulation_leaves_all_invalid_maps(name, svhip, oracle_lib):
    """status 0, empty triangle lists and planes, and maps that are invalid everywhere -- written, not left alone"""
    case = E.CASES[name]
    l, r = case.pair()
    for stage in (0, 1):
        svhip.set_stage(stage)
        try:
            got = product_run(svhip, case.params(), l, r)
        finally:
            svhip.set_stage(-1)
        assert got.status == 0
        assert len(got[H.SUPPORT]) >= 9
        for s in (H.TRI1, H.TRI2, H.PLANES1, H.PLANES2):
            assert got[s].size == 0
        for s in (H.D1_RAW, H.D2_RAW, H.D1_FINAL, H.D2_FINAL):
            assert (got[s] < 0).all()


@pytest.mark.parametrize("group,lanes", [(1, 1), (4, 1), (1, 8), (4, 8)])
def test_lockstep_groups_with_an_empty_triangulation(group, lanes, svhip, oracle_lib):
    """process_batch over two tie scenes, a starved one, the collinear one and a constant pair: the pair without triangles
    shares its group's launches (its two slots end where the previous slot ended) or, at group size 1 on one lane, is a
    whole group with no triangle whose launches are sized from the lane's earlier groups.  Then groups without it, and
    with it in the first and a middle slot, on the same object."""
    names = ["binary3", "hstripes", "flat0_5", "collinear", "constant"]
    prm = H.robotics()
    pairs = {n: E.pair(n) for n in names}
    want = {n: E.oracle_run(E.CASES[n])[0] for n in names}
    single = {}
    for n in names[:4]:
        rc, a, b = svhip.Elas(prm).process(*pairs[n])
        assert rc == 0 and np.array_equal(a.ravel(), want[n][H.D1_FINAL]) and np.array_equal(b.ravel(), want[n][H.D2_FINAL])
        single[n] = (a, b)
    assert (single["collinear"][0] < 0).all() and (single["collinear"][1] < 0).all()

    def batch(e, order):
        st, D1, D2 = e.process_batch(np.stack([pairs[n][0] for n in order]), np.stack([pairs[n][1] for n in order]))
        assert st == [1 if n == "constant" else 0 for n in order]
        for i, n in enumerate(order):
            if n == "constant":
                assert (D1[i] == 0).all() and (D2[i] == 0).all()      # process_batch hands in zeroed maps: untouched
            else:
                assert np.array_equal(D1[i], single[n][0]) and np.array_equal(D2[i], single[n][1]), (order, i)

    svhip.set_group(group)
    svhip.set_lanes(lanes)
    try:
        e = svhip.Elas(prm)
        batch(e, names)
        batch(e, ["binary3", "hstripes", "flat0_5", "binary3"])
        batch(e, ["collinear", "binary3", "collinear", "hstripes", "collinear"])
        batch(e, ["collinear"])
    finally:
        svhip.set_group(4)
        svhip.set_lanes(8)

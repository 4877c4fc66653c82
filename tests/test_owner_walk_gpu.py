"""GPU: k_owner walks the columns [uA, uC) of a triangle once, every lane taking the edge (AB below uB, BC from uB on)
of the part its column lies in, where the reference has two loops with a guard each (uA != uB, uB != uC).  Both passes
-- plain stores, then the fix pass at the span ends, or over every pixel with SVH_OWNER_FIX_ALL=1 -- use the walk, so
every case runs with the variable at 0 and at 1: D1_RAW, D2_RAW and the final maps agree bit for bit, and in the
device-stage cases every tap equals the CPU oracle's (the real Triangle from oracle/_ref where it is built, else the
triangle lists of the product's host-stage run).  process_batch has no taps: there the final maps are compared, with
each other and with the oracle's.

The cases are small on purpose and still hold what the walk can get wrong: triangles with two corners in one column
(an empty part on either side), subsampling (odd rows and columns are skipped), multiply covered pixels (counted in
numpy from the TRI taps with the reference's float operations: at least 20 in all), and a launch shared by the
triangles of several (pair, side) slots on a lane with and without history (stride loop, XCD order of the blocks)."""
import numpy as np
import pytest

import helpers as H
from test_elas_gpu import product_run
from test_phase_b_sizing_gpu import assert_bits, edge_pair

pytestmark = pytest.mark.gpu


@pytest.fixture()
def S():
    import svhip as S
    S.lib()
    assert S.device_count() > 0, "no HIP device: the product has no CPU fallback"
    S.set_stage(1)
    S.trim()            # fresh lanes: no history, no leftovers in their buffers
    yield S
    S.set_stage(-1)


_want = {}


def want_for(S, key, l, r, prm):
    """the oracle's run of the pair, computed once per module"""
    if key not in _want:
        if H.have_ref_elas():
            _want[key] = H.oracle_elas_run(prm, l, r)
        else:
            S.set_stage(0)
            try:
                host = product_run(S, prm, l, r)
            finally:
                S.set_stage(1)
            _want[key] = H.oracle_elas_run(prm, l, r, H.fixture_triangulator([host[H.TRI1], host[H.TRI2]]))
    return _want[key]


def f2u2i(x):
    """(int32)(uint32)x of the reference (elas.cpp:1081-1082) for the float32 values of an edge line"""
    return x.astype(np.int64).astype(np.uint32).astype(np.int32)


def contested_pixels(run, w, h):
    """pixels more than one triangle covers, both sides, by the reference's rasteriser in float32"""
    sup = run[H.SUPPORT].reshape(-1, 3)
    total = 0
    f = np.float32
    for side, stage in ((0, H.TRI1), (1, H.TRI2)):
        cnt = np.zeros((h, w), np.int32)
        for tri in run[stage].reshape(-1, 3):
            c = sup[tri]
            tu = [f(c[k, 0] - (c[k, 2] if side else 0)) for k in range(3)]
            tv = [f(c[k, 1]) for k in range(3)]
            for j in range(3):                      # the reference's exchange loop (elas.cpp:1044-1053)
                for k in range(j):
                    if tu[k] > tu[j]:
                        tu[j], tu[k] = tu[k], tu[j]
                        tv[j], tv[k] = tv[k], tv[j]
            (Au, Bu, Cu), (Av, Bv, Cv) = tu, tv
            uA, uB, uC = int(Au), int(Bu), int(Cu)
            ABa = (Av - Bv) / (Au - Bu) if uA != uB else f(0)
            ACa = (Av - Cv) / (Au - Cu) if uA != uC else f(0)
            BCa = (Bv - Cv) / (Bu - Cu) if uB != uC else f(0)
            ABb, ACb, BCb = Av - ABa * Au, Av - ACa * Au, Bv - BCa * Bu
            for lo, hi, ea, eb in ((uA, uB, ABa, ABb), (uB, uC, BCa, BCb)):
                us = np.arange(max(lo, 2), min(hi, w - 2))
                if lo == hi or not len(us):
                    continue
                fu = us.astype(f)
                v1, v2 = f2u2i(ACa * fu + ACb), f2u2i(ea * fu + eb)
                va, vb = np.maximum(np.minimum(v1, v2), 0), np.minimum(np.maximum(v1, v2), h)
                for u, a, b in zip(us, va, vb):
                    cnt[a:b, u] += 1
        total += int((cnt > 1).sum())
    return total


def both_forms(S, monkeypatch, key, l, r, prm):
    """the pair through the device stage with the span-end and the exhaustive fix pass: all taps of both"""
    runs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("SVH_OWNER_FIX_ALL", mode)
        runs.append(product_run(S, prm, l, r))
    ends, full = runs
    assert ends.status == full.status == 0, key
    for s in (H.D1_RAW, H.D2_RAW, H.D1_FINAL, H.D2_FINAL):
        assert np.array_equal(ends[s].view(np.uint32), full[s].view(np.uint32)), (key, H.STAGE_NAMES[s])
    want = want_for(S, key, l, r, prm)
    assert_bits(want, ends, key + ": span ends")
    assert_bits(want, full, key + ": exhaustive")


CASES = {
    "edge_320x120": lambda: (edge_pair(), H.robotics()),
    "synth_320x200": lambda: (H.synth_pair(320, 200, 61, dmax=48, planes=12), H.robotics()),
    "synth_401x177_sub": lambda: (H.synth_pair(401, 177, 62, dmax=48, planes=12), H.robotics(subsampling=1)),
    "urban3_640x240": lambda: (H.golden_pair("urban3_640x240"), H.robotics()),
}


@pytest.mark.parametrize("key", list(CASES))
def test_both_fix_passes_equal_the_oracle(S, monkeypatch, key):
    (l, r), prm = CASES[key]()
    both_forms(S, monkeypatch, key, l, r, prm)
    if key == "edge_320x120":       # the case with two corners in one column
        want = _want[key]
        u = want[H.SUPPORT].reshape(-1, 3)[want[H.TRI1].reshape(-1, 3)][..., 0]
        assert int(((u[:, 0] == u[:, 1]) | (u[:, 0] == u[:, 2]) | (u[:, 1] == u[:, 2])).sum()) > 0


def group_pairs():
    l, r = H.golden_pair("urban3_640x240")
    return [(l, r), (np.ascontiguousarray(l[::-1]), np.ascontiguousarray(r[::-1])),      # upside down: other content
            H.synth_pair(640, 240, 63, dmax=48, planes=12)]


@pytest.mark.parametrize("history", [False, True])
def test_group_of_three_pairs_shares_one_launch(S, monkeypatch, history):
    """three different pairs in one process_batch group: triangles of six slots in one k_owner launch, sized by the
    bound on a fresh lane and by the lane's last group on one with history"""
    pairs, prm = group_pairs(), H.robotics()
    wants = [want_for(S, "group%d" % k, a, b, prm) for k, (a, b) in enumerate(pairs)]
    assert [w.status for w in wants] == [0, 0, 0]
    L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    e = S.Elas(prm)
    if history:
        monkeypatch.setenv("SVH_OWNER_FIX_ALL", "0")
        assert e.process_batch(L, R)[0] == [0, 0, 0]
    outs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("SVH_OWNER_FIX_ALL", mode)
        st, D1, D2 = e.process_batch(L, R)
        assert st == [0, 0, 0]
        outs.append((D1, D2))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    for k, w in enumerate(wants):
        assert np.array_equal(outs[0][0][k].ravel(), w[H.D1_FINAL]), k
        assert np.array_equal(outs[0][1][k].ravel(), w[H.D2_FINAL]), k


def test_the_cases_hold_contested_pixels(S):
    """the comparisons above are about multiply covered pixels: the four single pairs and the group's three hold at
    least 20 of them (the urban crops do; the synthetic pairs exercise corner columns, subsampling and ragged sizes)"""
    seen = {}
    for key, make in CASES.items():
        (l, r), prm = make()
        seen[key] = contested_pixels(want_for(S, key, l, r, prm), l.shape[1], l.shape[0])
    for k, (l, r) in enumerate(group_pairs()):
        seen["group%d" % k] = contested_pixels(want_for(S, "group%d" % k, l, r, H.robotics()), 640, 240)
    print(seen)
    assert sum(seen.values()) >= 20, seen

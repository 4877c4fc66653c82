"""GPU: the corner form of the ownership fix pass (k_owner_corner, SVH_OWNER_FIX_ALL=0: eight lanes per triangle
re-check the span-end rows of the columns uA and uB only) against the span-end walk (2) and the exhaustive form (1):
D1_RAW, D2_RAW and the final maps agree bit for bit across the three, and every tap equals the CPU oracle's.  The same
with SVH_OWNER_FORCE_WALK=1, which has the plain pass set every slot's flag word and so sends the corner kernel down
its fallback path (all columns, two per step).

The cases are those of test_owner_walk_gpu.py -- two corners in one column, corner columns on odd u under subsampling
with ragged sizes, an urban crop, a synthetic pair -- and its group of three 640x240 pairs in one process_batch call:
six slots in one launch, the stride loop, the XCD order, on a fresh lane and on one with history.  On the lane with
history a forced-walk group is followed by an ordinary one, which must equal the oracle as well: the flag words are
cleared with every group.  Together the cases hold at least 20 multiply covered pixels (counted in numpy from the
oracle's triangle lists).  The oracle's runs are shared with test_owner_walk_gpu.py (its cache, same keys)."""
import numpy as np
import pytest

import helpers as H
import test_owner_walk_gpu as W
from test_elas_gpu import product_run
from test_phase_b_sizing_gpu import assert_bits, edge_pair  # noqa: F401  (edge_pair: behind CASES["edge_320x120"])

pytestmark = pytest.mark.gpu

S = W.S     # the fixture: device stage, fresh lanes

KEYS = ["edge_320x120", "synth_401x177_sub", "urban3_640x240", "synth_320x200"]
RAW_AND_FINAL = (H.D1_RAW, H.D2_RAW, H.D1_FINAL, H.D2_FINAL)


@pytest.mark.parametrize("key", KEYS)
def test_three_forms_and_the_fallback_equal_the_oracle(S, monkeypatch, key):
    (l, r), prm = W.CASES[key]()
    assert prm.subsampling == (1 if key == "synth_401x177_sub" else 0)
    want = W.want_for(S, key, l, r, prm)
    runs = {}
    for name, mode, force in (("corner", "0", "0"), ("span ends", "2", "0"), ("exhaustive", "1", "0"),
                              ("corner, forced walk", "0", "1")):
        monkeypatch.setenv("SVH_OWNER_FIX_ALL", mode)
        monkeypatch.setenv("SVH_OWNER_FORCE_WALK", force)
        runs[name] = product_run(S, prm, l, r)
        assert runs[name].status == 0, (key, name)
    first = runs["corner"]
    for name, run in runs.items():
        for s in RAW_AND_FINAL:
            assert np.array_equal(first[s].view(np.uint32), run[s].view(np.uint32)), (key, name, H.STAGE_NAMES[s])
        assert_bits(want, run, key + ": " + name)


@pytest.mark.parametrize("history", [False, True])
def test_group_of_three_pairs_in_one_launch(S, monkeypatch, history):
    pairs, prm = W.group_pairs(), H.robotics()
    wants = [W.want_for(S, "group%d" % k, a, b, prm) for k, (a, b) in enumerate(pairs)]
    assert [w.status for w in wants] == [0, 0, 0]
    L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    e = S.Elas(prm)

    def run(mode, force):
        monkeypatch.setenv("SVH_OWNER_FIX_ALL", mode)
        monkeypatch.setenv("SVH_OWNER_FORCE_WALK", force)
        st, D1, D2 = e.process_batch(L, R)
        assert st == [0, 0, 0], (mode, force)
        return D1, D2

    def equals_oracle(out, what):
        for k, w in enumerate(wants):
            assert np.array_equal(out[0][k].ravel(), w[H.D1_FINAL]), (what, k)
            assert np.array_equal(out[1][k].ravel(), w[H.D2_FINAL]), (what, k)

    if history:
        run("0", "0")
    corner, full = run("0", "0"), run("1", "0")
    assert np.array_equal(corner[0].view(np.uint32), full[0].view(np.uint32))
    assert np.array_equal(corner[1].view(np.uint32), full[1].view(np.uint32))
    equals_oracle(corner, "corner")
    equals_oracle(full, "exhaustive")
    if history:
        equals_oracle(run("0", "1"), "corner, forced walk")
        equals_oracle(run("0", "0"), "corner, after a forced walk on the same lane")   # the flags were cleared


def test_the_cases_hold_contested_pixels(S):
    seen = {}
    for key in KEYS:
        (l, r), prm = W.CASES[key]()
        seen[key] = W.contested_pixels(W.want_for(S, key, l, r, prm), l.shape[1], l.shape[0])
    for k, (l, r) in enumerate(W.group_pairs()):
        seen["group%d" % k] = W.contested_pixels(W.want_for(S, "group%d" % k, l, r, H.robotics()), 640, 240)
    print(seen)
    assert sum(seen.values()) >= 20, seen

"""GPU: the launches behind the device-side triangulations (k_prior, k_grid_seed, the two k_owner passes) are
enqueued before the group's counts exist.  They are sized by what the lane's last groups held (plus 1/8) and stride
over whatever the header says, so the size must never show in a result; k_stage_pack clears the grid bit sets of the
group and writes the counts to pinned memory itself; k_prior solves its 3x3 systems with prior_core.h.

Every case runs single calls (or one group of three) through the device stage on ONE lane -- svhip.trim() first, then
calls from this thread only: the pool hands out the lane released last -- and compares every tap, or the final maps of
a group, bit for bit with the CPU oracle (the real Triangle from oracle/_ref where it is built, else the triangle
lists of the product's host-stage run).  svh_elas_sizing_stats tells which launches were sized by the bound, which by
history, and which of the latter came up short (the stride loops ran)."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from test_elas_gpu import product_run

pytestmark = pytest.mark.gpu

PRM = H.robotics()


@pytest.fixture()
def S():
    import svhip as S
    S.lib()
    assert S.device_count() > 0, "no HIP device: the product has no CPU fallback"
    S.set_stage(1)
    S.trim()            # fresh lanes: no history, no leftovers in their buffers
    yield S
    S.set_stage(-1)


def sizing(S):
    """(sized by the bound, sized by history, history short of triangles, history short of support points)"""
    out = (C.c_int64 * 4)()
    S.lib().svh_elas_sizing_stats(out)
    return np.array(list(out))


def poor_of(l, r):
    """the pair with everything but a window of 150 x 100 pixels flattened: a few dozen support points"""
    pl, pr = np.full_like(l, 90), np.full_like(r, 90)
    pl[60:160, 250:400] = l[60:160, 250:400]
    pr[60:160, 150:400] = r[60:160, 150:400]
    return pl, pr


def edge_pair(w=320, h=120):
    """a textured wall at disparity 10 with a block at disparity 20 in front of it: support points on either side
    of the block's edges are 10 columns and 10 disparities apart, so triangles across an edge collapse to a line in
    the other image's coordinates -- a singular plane fit, which Gauss-Jordan in doubles either detects (zero plane,
    elas.cpp:640-650) or carries through a pivot of rounding-error size (planes of 1e14 and more: every bit of
    those depends on the order of the operations) -- and the lattice gives every second triangle two corners in one
    column"""
    rng = np.random.default_rng(5)
    wide = w + 40
    tex = np.kron(rng.integers(40, 216, (h // 2 + 1, wide // 2 + 1)), np.ones((2, 2), np.int64))[:h, :wide]
    tex = (tex + rng.integers(-12, 13, tex.shape)).clip(0, 255)
    disp = np.full((h, w), 10, np.int64)
    disp[30:90, 100:220] = 20
    xx = np.arange(w)[None, :] + disp
    left = tex[:, :w]
    right = np.take_along_axis(tex, xx, axis=1)      # right(x) = left(x + d)
    return left.astype(np.uint8), right.astype(np.uint8)


_want = {}


def want_for(S, key, l, r, prm=PRM):
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


def assert_bits(want, got, what):
    assert got.status == want.status == 0, what
    bad = [(n, c) for n, c in H.compare_runs(want, got) if c != 0]
    assert not bad, (what, bad)
    for s in (H.PLANES1, H.PLANES2):      # (compare_runs takes floats by value: +0 == -0)
        assert np.array_equal(want[s].view(np.uint32), got[s].view(np.uint32)), (what, H.STAGE_NAMES[s])


@pytest.fixture(scope="module")
def urban():
    return H.golden_pair("urban3_640x240")


def test_first_group_without_history_then_a_second_on_the_same_object(S, urban):
    l, r = urban
    l2, r2 = np.ascontiguousarray(l[::-1]), np.ascontiguousarray(r[::-1])     # upside down: as dense, other content
    e = S.Elas(PRM)
    e.set_taps(True)
    before = sizing(S)
    for n, (a, b, key) in enumerate(((l, r, "urban"), (l2, r2, "urban_flipped"))):
        rc, D1, D2 = e.process(a, b)
        st = {s: e.stage(s, H.stage_dtype(s)) for s in range(H.STAGE_COUNT)}
        st[H.D1_FINAL], st[H.D2_FINAL] = D1.ravel(), D2.ravel()
        assert_bits(want_for(S, key, a, b), H.StageRun(rc, st), key)
        assert list(sizing(S) - before)[:2] == [1, n], "first group by the bound, second by the first one's counts"


def test_grow_a_dense_pair_behind_a_poor_one_strides(S, urban):
    l, r = urban
    pl, pr = poor_of(l, r)
    before = sizing(S)
    poor = product_run(S, PRM, pl, pr)
    dense = product_run(S, PRM, l, r)
    assert_bits(want_for(S, "poor", pl, pr), poor, "poor")
    assert_bits(want_for(S, "urban", l, r), dense, "dense behind poor")
    ntri = lambda run: (len(run[H.TRI1]) + len(run[H.TRI2])) // 3
    assert ntri(dense) > 8 * ntri(poor) > 0 and len(dense[H.SUPPORT]) > 8 * len(poor[H.SUPPORT])
    # the dense group was sized by the poor one's counts and held more of both: the stride loops ran
    assert list(sizing(S) - before) == [1, 1, 1, 1]


def test_shrink_a_poor_pair_behind_a_dense_one(S, urban):
    l, r = urban
    pl, pr = poor_of(l, r)
    before = sizing(S)
    dense = product_run(S, PRM, l, r)
    poor = product_run(S, PRM, pl, pr)
    assert_bits(want_for(S, "urban", l, r), dense, "dense")
    assert_bits(want_for(S, "poor", pl, pr), poor, "poor behind dense")
    assert list(sizing(S) - before) == [1, 1, 0, 0]


def test_seed_words_of_the_group_before_do_not_show(S, urban):
    """k_stage_pack clears the grid bit sets k_grid_seed ORs into: the grids of a pair with few support points,
    run right behind a dense one on the same lane, hold that pair's disparities only"""
    l, r = urban
    pl, pr = poor_of(l, r)
    dense = product_run(S, PRM, l, r)
    poor = product_run(S, PRM, pl, pr)
    want = want_for(S, "poor", pl, pr)
    for s in (H.GRID1, H.GRID2):
        assert np.array_equal(poor[s], want[s]), H.STAGE_NAMES[s]
        assert not np.array_equal(poor[s], dense[s])          # (the dense pair's grids are fuller)
        assert np.count_nonzero(poor[s]) < np.count_nonzero(dense[s]) // 2


def test_group_of_three_with_a_pair_without_support_points(S, urban, capfd):
    l, r = urban
    l2, r2 = np.ascontiguousarray(l[::-1]), np.ascontiguousarray(r[::-1])
    flat = np.full_like(l, 77)
    wa, wb = want_for(S, "urban", l, r), want_for(S, "urban_flipped", l2, r2)
    e = S.Elas(PRM)
    before = sizing(S)
    for n in range(2):      # the lane's first group (bound), then one sized by it
        st, D1, D2 = e.process_batch(np.stack([l, flat, l2]), np.stack([r, flat, r2]))
        assert st == [0, 1, 0]
        assert np.all(D1[1] == 0) and np.all(D2[1] == 0)      # untouched (process_batch hands in zeroed maps)
        for k, w in ((0, wa), (2, wb)):
            assert np.array_equal(D1[k].ravel(), w[H.D1_FINAL]) and np.array_equal(D2[k].ravel(), w[H.D2_FINAL]), (n, k)
        assert list(sizing(S) - before)[:2] == [1, n]
    assert capfd.readouterr().out.count("Need at least 3 support points") == 2


def test_history_does_not_cross_a_change_of_image_size(S, urban):
    l, r = urban
    sl, sr = H.synth_pair(320, 120, 91, dmax=40)
    e = S.Elas(PRM)
    e.set_taps(True)
    before = sizing(S)
    for n, (a, b, key) in enumerate(((l, r, "urban"), (sl, sr, "synth_320x120"), (l, r, "urban"))):
        rc, D1, D2 = e.process(a, b)
        st = {s: e.stage(s, H.stage_dtype(s)) for s in range(H.STAGE_COUNT)}
        st[H.D1_FINAL], st[H.D2_FINAL] = D1.ravel(), D2.ravel()
        assert_bits(want_for(S, key, a, b), H.StageRun(rc, st), key)
        assert list(sizing(S) - before) == [n + 1, 0, 0, 0], "new buffers, no history: the bound every time"


def test_history_does_not_cross_a_change_of_parameters(S, urban):
    l, r = urban
    before = sizing(S)
    assert product_run(S, PRM, l, r).status == 0
    other = H.robotics(support_threshold=0.9)
    assert_bits(want_for(S, "urban_thr0.9", l, r, other), product_run(S, other, l, r), "other parameters")
    assert list(sizing(S) - before) == [2, 0, 0, 0]


def test_planes_of_collinear_and_same_column_triangles(S):
    l, r = edge_pair()
    want = want_for(S, "edge", l, r)
    assert want.status == 0
    sup = want[H.SUPPORT].reshape(-1, 3).astype(np.int64)
    seen = {"collinear": 0, "detected": 0, "carried": 0, "same_u": 0}
    for tri_s, planes_s, other in ((H.TRI1, H.PLANES1, slice(3, 6)), (H.TRI2, H.PLANES2, slice(0, 3))):
        t = sup[want[tri_s].reshape(-1, 3)]                   # [triangles][corner][u, v, d]
        u, v, d = t[..., 0], t[..., 1], t[..., 2]
        x = u - d if tri_s == H.TRI1 else u                   # the OTHER image's column of the corners
        det = (x[:, 1] - x[:, 0]) * (v[:, 2] - v[:, 0]) - (x[:, 2] - x[:, 0]) * (v[:, 1] - v[:, 0])
        flatp = want[planes_s].reshape(-1, 6)[:, other]
        zero = np.all(flatp[det == 0] == 0, axis=1)
        seen["collinear"] += int((det == 0).sum())
        seen["detected"] += int(zero.sum())
        seen["carried"] += int((np.abs(flatp[det == 0][~zero]).max(axis=1) > 1e9).sum()) if (~zero).any() else 0
        seen["same_u"] += int(((u[:, 0] == u[:, 1]) | (u[:, 0] == u[:, 2]) | (u[:, 1] == u[:, 2])).sum())
    assert min(seen.values()) > 0, seen
    assert_bits(want, product_run(S, PRM, l, r), "edge pair")

"""CPU: the contract of the map view's voxel-grid thinning (svh_view_thin, include/svh_view.h).  tests/view_thin_ref.py
restates the arithmetic of stereo-vision_amd/csrc/view_thin_core.h in numpy; this file pins that restatement with cases
derived by hand, compares the header itself -- evaluated on the host by the library's test entry svh_test_thin_keys --
with it, and checks what needs no device: the exports, the argument checks, the algebra the contract promises.

tests/test_view_thin_gpu.py thins the same cases (HAND, EXAMPLE) on the device and demands the same bytes.

The hand cases use voxel = 0.5, a power of two: x / 0.5 = 2 x is exact, so every cell below can be checked in the
head.  Cells are biased by 2^20 in the key: cell c of x sits at bits 42.., of y at bits 21.., of z at bits 0..."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers as H
import view_thin_ref as TR

F = np.float32
B = 1 << 20
NA = lambda x, to: np.nextafter(F(x), F(to))
HALF = F(0.5)

# (x, the cell of x at voxel 0.5, or None where x has none)
HAND = [
    (F(0.0), 0), (F(-0.0), 0),                         # -0.0f / 0.5f = -0.0f, floorf -> -0.0f, (int) -> 0
    (F(0.5), 1), (F(-0.5), -1),                        # +-voxel
    (F(-0.25), -1),                                    # -0.5 voxel: floor(-0.5) = -1
    (NA(0.5, 0), 0), (NA(0.5, 1), 1),                  # either side of the boundary between cells 0 and 1
    (NA(-0.5, 0), -1), (NA(-0.5, -1), -2),             # ... between -1 and -2: -0.5 itself is the first of cell -1
    (NA(0, 1), 0), (NA(0, -1), -1),                    # the smallest denormals: -1.4e-45 / 0.5 = -2.8e-45, floor -1
    (F(1.75), 3), (F(-1.75), -4),
    (F(524287.5), B - 1),                              # (2^20 - 1) / 2: the last cell
    (NA(524288, 0), B - 1),                            # 524287.97: 2 x = 1048575.94, floor 2^20 - 1
    (F(524288.0), None),                               # cell 2^20: out of range
    (F(-524288.0), -B),                                # cell -2^20: the first cell
    (NA(-524288, -1e9), None),                         # -524288.06: 2 x = -1048576.1, floor -2^20 - 1
    (F(3e38), None),                                   # finite, the quotient overflows to +Inf
    (F(np.nan), None), (F(np.inf), None), (F(-np.inf), None),
]

# Twelve points in four lists at voxel 1.0: the written-out example.  Voxels: a = (0,0,0), b = (1,0,0), c = (-1,0,0),
# d = (2,2,2).  Store index, voxel, fate:
#   list 0:  0 a keep | 1 a gone (0) | 2 b keep | 3 NaN: no voxel, keep
#   list 1:  empty
#   list 2:  4 c keep | 5 a gone (0) | 6 b gone (2) | 7 -0.0 is a, gone (0) | 8 NaN: no voxel, keep (never a duplicate)
#   list 3:  9 c gone (4): -1.0 is the first coordinate of cell -1 | 10 d keep | 11 d gone (10)
EXAMPLE = [
    np.array([[0.5, 0.5, 0.5, 0.10], [0.9, 0.1, 0.2, 0.11], [1.5, 0, 0, 0.12], [np.nan, 0, 0, 0.13]], F),
    np.zeros((0, 4), F),
    np.array([[-0.5, 0, 0, 0.20], [0.1, 0.1, 0.1, 0.21], [1.0, 0.9, 0.9, 0.22], [-0.0, 0, 0, 0.23], [np.nan, 0, 0, 0.24]], F),
    np.array([[-1.0, 0, 0, 0.30], [2, 2, 2, 0.31], [2.5, 2.5, 2.5, 0.32]], F),
]
EXAMPLE_KEEP = [[0, 2, 3], [], [0, 4], [1]]
EXAMPLE_STATS = dict(before=12, after=6, unplaced=2)


def hand_points():
    """every hand case on each axis in turn, the other two coordinates in cell 0: (points [3 * len(HAND), 4], keys)"""
    pts, keys = [], []
    for axis in range(3):
        for k, (x, c) in enumerate(HAND):
            p = [F(0.125), F(0.125), F(0.125), F(k) / F(64)]
            p[axis] = x
            pts.append(p)
            idx = [B, B, B]
            if c is not None:
                idx[axis] = c + B
            keys.append((1 << 64) - 1 if c is None else (idx[0] << 42) | (idx[1] << 21) | idx[2])
    return np.array(pts, F), np.array(keys, np.uint64)


def seeded(n, seed, spread=4.0):
    """random points, negative coordinates included, with a sprinkling of unplaceable ones"""
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-spread, spread, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(F)
    if n >= 16:
        bad = rng.choice(n, n // 16, replace=False)
        p[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -1e9], F), len(bad))
    return p


def split(pts, cuts):
    return [pts[a:b] for a, b in zip([0] + list(cuts), list(cuts) + [len(pts)])]


# ---- 1: the restatement, by hand ---------------------------------------------------------------------------------------
def test_cells_of_the_hand_cases():
    for x, c in HAND:
        got = TR.cells(np.array([x], F), HALF)[0]
        ok = bool(TR.placeable(np.array([[x, 0, 0, 0]], F), HALF)[0])
        assert ok == (c is not None), (x, c)
        if c is not None:
            assert got == c and got.dtype == np.float32, (x, got, c)
    assert np.signbit(TR.cells(np.array([-0.0], F), HALF)[0])   # -0.0f stays -0.0f until the conversion: cell 0


def test_keys_of_the_hand_cases():
    pts, want = hand_points()
    assert np.array_equal(TR.keys(pts, HALF), want)
    # one written out: (-0.0, 0.5, -0.5) at voxel 0.5 lies in (0, 1, -1)
    k = TR.keys(np.array([[-0.0, 0.5, -0.5, 1.0]], F), HALF)[0]
    assert int(k) == (B << 42) | ((B + 1) << 21) | (B - 1) and int(k) < (1 << 63)
    # the largest key is 63 bits and not the empty slot
    top = TR.keys(np.array([[524287.5] * 3 + [0]], F), HALF)[0]
    assert int(top) == (1 << 63) - 1 and top != TR.EMPTY


def test_capacity_rule_and_hash():
    assert [TR.capacity_for(n) for n in (0, 1, 512, 513, 1024, 1025, 4096, (1 << 31) - 4096)] == \
        [1024, 1024, 1024, 2048, 2048, 4096, 8192, 1 << 32]
    # splitmix64's finaliser: 0 is its fixed point; 1 by hand-run of the five steps in Python integers
    h, M = 1, (1 << 64) - 1
    h ^= h >> 30
    h = h * 0xbf58476d1ce4e5b9 & M
    h ^= h >> 27
    h = h * 0x94d049bb133111eb & M
    h ^= h >> 31
    assert [int(v) for v in TR.hash64(np.array([0, 1], np.uint64))] == [0, h]
    assert int(TR.homes(np.array([1], np.uint64), 1024)[0]) == h & 1023
    assert TR.homes(np.array([TR.EMPTY]), 1024)[0] == TR.NO_HOME


def test_the_written_out_example():
    got, stats = TR.thin(EXAMPLE, 1.0)
    want = [a[idx] if len(idx) else np.zeros((0, 4), F) for a, idx in zip(EXAMPLE, EXAMPLE_KEEP)]
    assert [len(a) for a in got] == [3, 0, 2, 1]
    assert TR.same_lists(got, want) and stats == EXAMPLE_STATS
    assert got[0][0, 3] == F(0.10) and got[3][0, 3] == F(0.31)          # the winner's val is the one kept


# ---- 2: the header itself (host code of the library) -------------------------------------------------------------------
@pytest.fixture(scope="module")
def V():
    from svhip import view
    view._bind()
    return view


def test_header_equals_the_restatement_on_the_hand_cases(V):
    pts, want = hand_points()
    key, home, cap = V.thin_keys(pts, HALF)
    assert cap == TR.capacity_for(len(pts)) == 1024
    assert np.array_equal(key, want)
    assert np.array_equal(home, TR.homes(want, cap))
    key, _, _ = V.thin_keys(np.concatenate(EXAMPLE), 1.0)
    assert np.array_equal(key, TR.keys(np.concatenate(EXAMPLE), 1.0))


@pytest.mark.parametrize("n,voxel,seed", [(0, 0.05, 1), (1, 0.05, 2), (513, 0.05, 3), (5000, 0.05, 4), (5000, 0.3, 5),
                                          (20000, 2e-6, 6), (20000, 7.0, 7)])
def test_header_equals_the_restatement_on_seeded_points(V, n, voxel, seed):
    """voxel 0.05 is no power of two: the quotients round.  2e-6 pushes most of the cloud out of the cell range"""
    pts = seeded(n, seed)
    key, home, cap = V.thin_keys(pts, voxel)
    want = TR.keys(pts, voxel)
    assert cap == TR.capacity_for(n)
    assert np.array_equal(key, want) and np.array_equal(home, TR.homes(want, cap))
    if n >= 5000:
        assert 0 < (want == TR.EMPTY).sum() < n


def test_new_entries_are_declared_and_exported(V):
    import svhip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "svh_view.h")).read(), flags=re.S)
    for name in ("svh_view_thin", "svh_view_get_points", "svh_view_list_len"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(svhip.lib(), name), name
    assert "svh_view_thin_stats" in hdr
    assert hasattr(svhip.lib(), "svh_test_thin_keys") and "svh_test_thin_keys" not in hdr
    drop_in = open(os.path.join(H.ROOT, "include", "view3d.h")).read()
    assert "thin(float voxel)" in drop_in and "getPoints()" in drop_in


def test_bad_arguments_need_no_device(V):
    import svhip
    L = V._bind()
    st = V.ThinStats(7, 7, 7)
    for voxel in (0.05, 0.0, -1.0, float("nan"), float("inf")):
        assert L.svh_view_thin(None, voxel, C.byref(st)) == svhip.ERR_BAD_ARG
        assert "svh_view_thin" in svhip.last_error()
    assert (st.before, st.after, st.unplaced) == (7, 7, 7)
    assert L.svh_view_get_points(None, -1, None, 0, 0) == svhip.ERR_BAD_ARG
    assert L.svh_view_list_len(None, 0) == svhip.ERR_BAD_ARG
    pts = seeded(4, 1)
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        assert L.svh_test_thin_keys(pts.ctypes.data, 4, voxel, None, None, None) == svhip.ERR_BAD_ARG


# ---- 3: the algebra, on the restatement ---------------------------------------------------------------------------------
CLOUDS = [(seeded(3000, 11), [700, 700, 1900], 1.0), (seeded(3000, 12), [1, 2999], 2.0), (seeded(2000, 13), [1000], 0.05)]


@pytest.mark.parametrize("k", range(len(CLOUDS)))
def test_algebra_of_the_restatement(k):
    pts, cuts, voxel = CLOUDS[k]
    lists = split(pts, cuts)
    once, st = TR.thin(lists, voxel)
    assert st["before"] == len(pts) and st["after"] == sum(len(a) for a in once) and st["unplaced"] > 0
    if voxel >= 0.5:
        assert st["after"] < st["before"] // 2                       # the cloud is dense at this voxel: most points go
    # idempotence
    twice, st2 = TR.thin(once, voxel)
    assert TR.same_lists(twice, once) and st2["after"] == st2["before"] == st["after"]
    # thin(thin(A) ++ B) == thin(A ++ B), for every split point between lists
    for cut in range(1, len(lists)):
        head, _ = TR.thin(lists[:cut], voxel)
        both, _ = TR.thin(head + lists[cut:], voxel)
        assert TR.same_lists(both, once), cut
    # dropping the newest list commutes with thinning: the lowest index wins and the newest list is the tail
    assert TR.same_lists(TR.thin(lists[:-1], voxel)[0], once[:-1])
    # survivors are a subsequence, bit for bit, and no two placeable survivors share a voxel
    flat = np.concatenate(once)
    keys = TR.keys(flat, voxel)
    placed = keys[keys != TR.EMPTY]
    assert len(np.unique(placed)) == len(placed)
    assert set(np.unique(TR.keys(pts, voxel))) == set(np.unique(keys))

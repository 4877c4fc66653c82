"""GPU: the map view's voxel-grid thinning and read-back (svh_view_thin, svh_view_get_points, svh_view_list_len;
csrc/view_thin_kernels.hip, csrc/view_engine.cpp) against the numpy restatement tests/view_thin_ref.py, which
tests/test_view_thin.py pins on the CPU.  Every comparison is exact: np.array_equal on the raw bits of the floats and
on the list lengths.  The winner of a voxel is the lowest store index, whatever the schedule.

Shapes: the insert kernel runs 256 points per workgroup, flag / scatter 1024 (the compaction's block, 16 waves), the
scan takes 1024 block counts per round with a carry, so 1024 * 1024 + 1 points need a second round."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import test_view as T
import test_view_thin as TT
import view_ref as R
import view_thin_ref as TR
from test_view_gpu import Dev, same

pytestmark = pytest.mark.gpu

F = np.float32
BAD_ARG, HIP_ERR = -1, -2
EMPTY = np.zeros((0, 4), F)


@pytest.fixture(scope="module")
def V():
    import svhip
    from svhip import view
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    return view


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(autouse=True)
def disarm(V):
    yield
    V.lib().svh_test_fail_at(None)


def held(V, lists):
    """a view that holds exactly these lists: one array per call appends and drops nothing"""
    v = V.View(64, 48)
    for a in lists:
        v.add_points([a])
    return v


def lists_of(v, V):
    n = v.count(V.LISTS)
    out = [v.points(i) for i in range(n)]
    assert [v.list_len(i) for i in range(n)] == [len(a) for a in out]
    assert v.count(V.POINTS) == sum(len(a) for a in out)
    return out


def check(V, v, want, tag=""):
    """the view holds `want`, list by list and as a whole, bit for bit"""
    got = lists_of(v, V)
    assert [len(a) for a in got] == [len(a) for a in want], tag
    assert TR.same_lists(got, want), tag
    whole = v.points()
    flat = np.concatenate(want) if want else EMPTY
    assert whole.shape == flat.shape and np.array_equal(whole.view(np.uint32), flat.view(np.uint32)), tag


def thin_and_check(V, lists, voxel, tag=""):
    want, stats = TR.thin(lists, voxel)
    v = held(V, lists)
    st = v.thin(voxel)
    assert dict(before=st.before, after=st.after, unplaced=st.unplaced) == stats, (tag, st, stats)
    check(V, v, want, tag)
    return v, want


def layouts(pts):
    """one list; two; five with an empty list at the front, in the middle and at the end"""
    n = len(pts)
    return {1: [pts], 2: [pts[:n // 2], pts[n // 2:]], 5: [EMPTY, pts[:n // 3], EMPTY, pts[n // 3:], EMPTY]}


# ---- sizes --------------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 1024 * 1024 + 1]
_clouds = {}


def cloud_and_voxel(n):
    """computed once per count and left unchanged; the large one at a fine voxel so that most points survive and the
    second round of the scan carries a large number"""
    if n not in _clouds:
        _clouds[n] = TT.seeded(n, 1000 + n % 997)
    return _clouds[n], (0.5 if n <= 4096 else 0.05)


@pytest.mark.parametrize("nlists", [1, 2, 5])
@pytest.mark.parametrize("n", COUNTS)
def test_sizes(V, n, nlists):
    """the counts around a wave, the insert's workgroup, the compaction's block and twice it, and one that needs a second
    round of the scan; n = 2048 in two lists puts a list boundary on a block boundary, the last list's end always is
    the store's end"""
    pts, voxel = cloud_and_voxel(n)
    lists = layouts(pts)[nlists]
    v, want = thin_and_check(V, lists, voxel, "%d points in %d lists" % (n, nlists))
    if n >= 1024:
        assert 0 < sum(len(a) for a in want) < n          # something went and something stayed
    if n == 0:
        assert v.count(V.LISTS) == nlists


# ---- contention ---------------------------------------------------------------------------------------------------------
def test_one_voxel_4096_points(V):
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(0.01, 0.99, (4096, 3)), np.arange(4096)[:, None] / 4096.0], 1).astype(F)
    v, want = thin_and_check(V, [pts[:1000], pts[1000:]], 1.0, "one voxel")
    assert [len(a) for a in want] == [1, 0] and np.array_equal(v.points()[0], pts[0])


def test_all_distinct_voxels(V):
    i = np.arange(5000)
    pts = np.stack([i % 17 - 8 + 0.5, i // 17 % 17 - 8 + 0.5, i // 289 + 0.5, i / 5000.0], 1).astype(F)
    v, want = thin_and_check(V, layouts(pts)[5], 1.0, "distinct")
    assert sum(len(a) for a in want) == 5000


def test_every_voxel_twice_a_workgroup_apart(V):
    """point i and point i + 2048 share a voxel: the two hits are in different workgroups of every kernel, and the
    earlier one survives with its own val"""
    i = np.arange(2048)
    a = np.stack([i % 16 + 0.25, i // 16 % 16 + 0.25, i // 256 + 0.25, np.full(2048, 0.25)], 1).astype(F)
    b = a + F(0.5)
    v, want = thin_and_check(V, [np.concatenate([a, b])], 1.0, "twice")
    assert np.array_equal(v.points().view(np.uint32), a.view(np.uint32))


# ---- probing -------------------------------------------------------------------------------------------------------------
def test_probe_chains_and_wrap_around(V):
    """a store of 4096 points has 8192 slots.  Built with svh_test_thin_keys: 256 distinct voxels homed at slot 1000 (a
    chain of 256), 64 homed at slot 1100 inside that chain, 64 homed at the last slot, so their probes wrap to slot 0;
    every one of them twice or three times, interleaved by a seeded shuffle, the rest of the store filled from voxels
    homed elsewhere"""
    N, CAP = 4096, 8192
    i = np.arange(1 << 22)
    cand = np.stack([i % 256 - 128 + 0.5, i // 256 % 256 - 128 + 0.5, i // 65536 + 0.5, np.zeros(len(i))], 1).astype(F)
    _, home_big, cap_big = V.thin_keys(cand, 1.0)
    assert cap_big == 1 << 23
    home = home_big & np.uint32(CAP - 1)          # the capacity is a power of two: the low bits are the smaller table's home
    g1, g2, g3 = (np.flatnonzero(home == h)[:k] for h, k in ((1000, 256), (1100, 64), (CAP - 1, 64)))
    assert (len(g1), len(g2), len(g3)) == (256, 64, 64)
    fill = np.flatnonzero((home >= 3000) & (home < 7000))
    rng = np.random.default_rng(9)
    picks = np.concatenate([g1, g1, g2, g2, g2, g3, g3])
    picks = np.concatenate([picks, rng.choice(fill, N - len(picks), replace=True)])
    rng.shuffle(picks)
    pts = cand[picks].copy()
    pts[:, :3] += rng.uniform(-0.4, 0.4, (N, 3)).astype(F)       # another place in the same voxel
    pts[:, 3] = np.arange(N) / F(N)
    key, got_home, cap = V.thin_keys(pts, 1.0)
    assert cap == CAP and np.array_equal(key, V.thin_keys(cand[picks], 1.0)[0])
    assert (got_home == 1000).sum() == 512 and (got_home == 1100).sum() == 192 and (got_home == CAP - 1).sum() == 128
    v, want = thin_and_check(V, [pts[:1500], pts[1500:]], 1.0, "probing")
    assert len(np.unique(key)) == sum(len(a) for a in want) < N


# ---- arithmetic on the device -----------------------------------------------------------------------------------------
def test_hand_cases_on_the_device(V):
    """negative coordinates, -0.0, the cell boundaries, the denormals, the range limits, NaN and Inf: the device puts
    them where the hand derivation does"""
    pts, keys = TT.hand_points()
    assert np.array_equal(TR.keys(pts, TT.HALF), keys)
    nowhere = int((keys == TR.EMPTY).sum())
    assert nowhere == 3 * sum(c is None for _, c in TT.HAND)
    # each hand point once more at the end, val changed: the placeable copies go, the unplaceable ones stay in place
    again = pts.copy()
    again[:, 3] += F(0.5)
    v, want = thin_and_check(V, [pts, again], TT.HALF, "hand")
    st = TR.thin([pts, again], TT.HALF)[1]
    assert st["unplaced"] == 2 * nowhere
    assert len(want[1]) == nowhere and np.array_equal(want[1].view(np.uint32), again[keys == TR.EMPTY].view(np.uint32))
    assert len(want[0]) == nowhere + len(np.unique(keys[keys != TR.EMPTY]))


def test_the_written_out_example_on_the_device(V):
    v, want = thin_and_check(V, TT.EXAMPLE, 1.0, "example")
    assert [list(np.flatnonzero([any(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for q in w) for p in a]))
            for a, w in zip(TT.EXAMPLE, want)] == TT.EXAMPLE_KEEP
    assert v.points(0)[0, 3] == F(0.10) and v.points(3)[0, 3] == F(0.31)     # the winner's val


@pytest.mark.parametrize("voxel", [0.05, 0.3, 2e-6, 7.0])
def test_seeded_points_at_rounding_voxels(V, voxel):
    """voxels that are no power of two: the device's division must round as IEEE's does"""
    thin_and_check(V, TT.split(TT.seeded(20000, 77), [5000, 5001]), voxel, "voxel %g" % voxel)


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------
def test_read_back_host_and_device(V, hip):
    lists = TT.split(TT.seeded(3000, 21), [1000, 1000, 2500])
    v, want = thin_and_check(V, lists, 0.5)
    flat = np.concatenate(want)
    for i, a in list(enumerate(want)) + [(-1, flat)]:
        assert np.array_equal(v.points(i, cap=3).view(np.uint32), a[:3].view(np.uint32))
        d = Dev(hip, len(a) * 16 + 16)
        assert v.points(i, device_ptr=d.addr) == len(a)
        got = d.get()
        assert np.array_equal(got[:len(a) * 16], a.view(np.uint8).ravel()) and (got[len(a) * 16:] == 0xEE).all()
        d = Dev(hip, 64)
        assert v.points(i, cap=2, device_ptr=d.addr) == len(a)
        assert np.array_equal(d.get()[:min(len(a), 2) * 16], a[:2].view(np.uint8).ravel())
        assert (d.get()[min(len(a), 2) * 16:] == 0xEE).all()
    L = v._L
    assert L.svh_view_get_points(v._h, -1, None, 0, 0) == len(flat)
    for bad in (4, 5, -2):
        assert L.svh_view_get_points(v._h, bad, None, 0, 0) == BAD_ARG
        assert L.svh_view_list_len(v._h, bad) == BAD_ARG
    assert L.svh_view_list_len(v._h, -1) == BAD_ARG
    assert L.svh_view_get_points(v._h, 0, None, 1, 0) == BAD_ARG and L.svh_view_get_points(v._h, 0, None, -1, 0) == BAD_ARG
    check(V, v, want)


def test_bad_voxel_changes_nothing(V):
    lists = TT.split(TT.seeded(500, 22), [200])
    v = held(V, lists)
    st = V.ThinStats(7, 7, 7)
    for voxel in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert v._L.svh_view_thin(v._h, voxel, C.byref(st)) == BAD_ARG
    assert (st.before, st.after, st.unplaced) == (7, 7, 7)
    check(V, v, lists)
    assert v._L.svh_view_thin(v._h, 0.5, None) == 0           # the statistics are optional
    check(V, v, TR.thin(lists, 0.5)[0])


def test_empty_stores(V):
    v = V.View(64, 48)
    st = v.thin(0.5)
    assert (st.before, st.after, st.unplaced) == (0, 0, 0) and v.count(V.LISTS) == 0 and len(v.points()) == 0
    v = held(V, [EMPTY, EMPTY])
    st = v.thin(0.5)
    assert (st.before, st.after, st.unplaced) == (0, 0, 0)
    check(V, v, [EMPTY, EMPTY])


def test_add_points_after_a_thinning(V):
    """two arrays drop exactly the thinned newest list; the store grows past its capacity on the way"""
    a, b, c, d = (TT.seeded(n, s) for n, s in ((900, 31), (700, 32), (300, 33), (6000, 34)))
    v, want = thin_and_check(V, [a, b], 0.5)
    v.add_points([c, d])
    want = TR.add_points(want, [c, d])
    assert len(want) == 3
    check(V, v, want, "after add_points")
    v.thin(0.5)
    check(V, v, TR.thin(want, 0.5)[0], "thinned again")
    check(V, v, TR.thin([a, c, d], 0.5)[0], "as if thinned once")


def test_add_map_after_a_thinning(V):
    """a 640 x 240 crop of two consecutive golden urban frames through svh_map_add: thin after the first, let the
    second drop the thinned list and append its two, thin again"""
    from svhip import mapper
    m = mapper.Mapper(721.5377, 609.5593, 172.854, 0.5371657, 12.0)
    v = V.View(64, 48)
    want = []
    for k, name in enumerate(("urban2", "urban3")):
        z = np.load(os.path.join(H.GOLDEN, name + "_kitti.npz"))
        l, _ = H.golden_pair(str(z["crop"]))
        d = np.ascontiguousarray(z["d1"].reshape(l.shape)[60:300, 300:940])
        Ht = np.eye(4)
        Ht[2, 3] = 0.3 * k
        m.add(d, np.ascontiguousarray(l[60:300, 300:940]), Ht, 0.0)
        p0, p1 = m.points(0), m.points(1)
        assert len(p1) > 1000 and (len(p0) > 0) == (k == 1)
        v.add_map(m)
        want = TR.add_points(want, [p0, p1] if k == 1 else [p1])
        check(V, v, want, "frame %d" % k)
        st = v.thin(0.05)
        want, stats = TR.thin(want, 0.05)
        assert (st.before, st.after, st.unplaced) == (stats["before"], stats["after"], stats["unplaced"])
        assert st.after < st.before
        check(V, v, want, "frame %d thinned" % k)


def test_render_after_a_thinning(V):
    """the render of a thinned store is view_ref's render of the restatement's thinned lists"""
    lists = [T.cloud(150, 41), T.cloud(0, 42), T.cloud(150, 43)]
    v, want = thin_and_check(V, lists, 1.0)
    assert sum(len(a) for a in want) < 300
    ref = R.View(64, 48)
    ref.lists = [a.copy() for a in want]
    same(v.render(), ref.render(), "thinned render")


# ---- properties on the device ---------------------------------------------------------------------------------------------
def test_idempotence_and_incremental_thinning(V):
    a, b, c = TT.split(TT.seeded(6000, 51), [2500, 2600])
    v, once = thin_and_check(V, [a, b], 0.5)
    st = v.thin(0.5)
    assert st.before == st.after
    check(V, v, once, "thinned twice")
    v.add_points([c])
    v.thin(0.5)
    check(V, v, TR.thin([a, b, c], 0.5)[0], "thin, append, thin")


def test_fresh_objects_give_identical_bytes(V):
    lists = TT.split(TT.seeded(50000, 61), [20000])
    got = []
    for _ in range(2):
        v = held(V, lists)
        v.thin(0.3)
        got.append((v.points().tobytes(), [v.list_len(0), v.list_len(1)]))
    assert got[0] == got[1]


@pytest.mark.parametrize("spec", ["malloc:1", "malloc:3", "copy:1", "copy:4", "launch:1", "wait:1"])
def test_a_failed_thinning_leaves_the_object_as_it_was(V, spec):
    import svhip
    lists = TT.split(TT.seeded(3000, 71), [1000])
    v = held(V, lists)
    before = v.render()
    V.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(V.SvhError) as e:
        v.thin(0.5)
    V.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR
    check(V, v, lists, spec)
    same(v.render(), before, spec)
    v.thin(0.5)
    check(V, v, TR.thin(lists, 0.5)[0], spec + ", then thinned")


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------
def read_ply(path):
    raw = open(path, "rb").read()
    head, _, body = raw.partition(b"end_header\n")
    lines = head.decode().split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    assert lines[3:7] == ["property float " + n for n in ("x", "y", "z", "val")]
    n = int(lines[2].split()[-1])
    assert lines[2] == "element vertex %d" % n and len(body) == 16 * n
    return np.frombuffer(body, "<f4").reshape(n, 4)


@pytest.fixture()
def tool(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    import test_rectify
    from test_view_gpu import two_frame_drive
    drive = two_frame_drive(tmp_path / "drive")
    calib = tmp_path / "calib_cam_to_cam.txt"
    calib.write_text(test_rectify.rig_calib_text())
    return SP, str(drive), str(calib)


def test_pipeline_thin_and_ply(V, tool, tmp_path, monkeypatch, capsys):
    """--thin 0.05 --ply FILE: the file holds View.points() of the thinned map, which is the restatement's thinning of
    the lists the pipeline accumulates without the flag; thinning every second append gives the same file, and the
    per-frame lines do not change"""
    import sys
    from svhip import kitti
    SP, drive, calib = tool
    c = kitti.read_cam_to_cam(calib)
    p = SP.Pipeline(c.f, c.cu, c.cv, c.base)
    for I1, I2, _ in kitti.Sequence(drive):
        p.push(I1, I2)
    raw = lists_of(p.view, V)
    want, stats = TR.thin(raw, 0.05)
    assert stats["after"] < stats["before"]
    plain, files = None, []
    for k, extra in enumerate(([], ["--thin", "0.05"], ["--thin", "0.05", "--thin-every", "2"])):
        ply = str(tmp_path / ("map%d.ply" % k))
        monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py"] + extra + ["--ply", ply, drive, calib])
        SP.main()
        out = capsys.readouterr().out.splitlines()
        frames = [l for l in out if l.startswith("frame ")]
        plain = plain or frames
        assert frames == plain and len(frames) == 2
        pts = read_ply(ply)
        assert ("map of %d points in 2 lists written to %s" % (len(pts), ply)) in out
        flat = np.concatenate(want if extra else raw)
        assert np.array_equal(pts.view(np.uint32), flat.view(np.uint32)), extra
        if extra:
            assert any(l.startswith("map thinned at 0.05: %d points of" % stats["after"]) for l in out)


def test_pipeline_thin_in_lockstep(V, tool, tmp_path, monkeypatch, capsys):
    """--lockstep 2 --thin: one view and one file per drive"""
    import sys
    SP, drive, calib = tool
    ply = str(tmp_path / "map.ply")
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--lockstep", "2", "--thin", "0.05", "--ply", ply, drive, calib])
    SP.main()
    out = capsys.readouterr().out
    for i in range(2):
        pts = read_ply(str(tmp_path / ("map_%d.ply" % i)))
        assert len(pts) > 1000 and "[%d] map of %d points in 1 lists" % (i, len(pts)) in out
        assert len(np.unique(TR.keys(pts, 0.05))) == len(pts)


# ---- the drop-in class -----------------------------------------------------------------------------------------------------
def test_view3d_dropin_thin_and_get_points(tmp_path):
    """include/view3d.h, compiled with only include/ on the path: thin(voxel) returns the number of points left and
    getPoints() the held lists, empty ones included; a bad voxel comes back as SVH_ERR_BAD_ARG"""
    import subprocess
    exe, lib_dir = str(tmp_path / "view3d_thin_dropin"), os.path.join(H.ROOT, "stereo-vision_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "view", "view3d_thin_dropin.cpp"), "-L", lib_dir, "-lsvhip",
                           "-Wl,-rpath," + lib_dir])
    lists = TT.split(TT.seeded(3000, 91), [1200, 1200, 2900])
    want, stats = TR.thin(lists, 0.5)
    (tmp_path / "points.bin").write_bytes(np.array([len(lists)] + [len(a) for a in lists], np.int32).tobytes() +
                                          b"".join(a.tobytes() for a in lists))
    subprocess.check_call([exe, str(tmp_path / "points.bin"), "0.5", str(tmp_path / "out.bin")])
    raw = (tmp_path / "out.bin").read_bytes()
    assert int(np.frombuffer(raw[:8], np.int64)[0]) == stats["after"]
    nl = int(np.frombuffer(raw[8:12], np.int32)[0])
    lens = np.frombuffer(raw[12:12 + 4 * nl], np.int32).tolist()
    assert nl == 4 and lens == [len(a) for a in want]
    pts = np.frombuffer(raw[12 + 4 * nl:], np.float32).reshape(-1, 4)
    assert np.array_equal(pts.view(np.uint32), np.concatenate(want).view(np.uint32))

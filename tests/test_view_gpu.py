"""GPU: the map view (include/svh_view.h, csrc/view_kernels.hip, csrc/view_engine.cpp) against the numpy restatement
tests/view_ref.py, which tests/test_view.py pins on the CPU.  Every image comparison is exact (np.array_equal on the
RGB bytes): the render has no tolerance, the winner of a pixel does not depend on scheduling."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import test_view as T
import view_ref as R

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR, UNSUPPORTED = -1, -2, -3


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


class Dev:
    """device memory through the HIP runtime the library links: a copy of a host array, or `a` bytes of 0xEE"""

    def __init__(self, hip, a):
        self.hip, self.p = hip, C.c_void_p()
        host = np.full(a, 0xEE, np.uint8) if isinstance(a, int) else np.ascontiguousarray(a)
        self.nbytes = max(host.nbytes, 16)
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(self.nbytes)) == 0
        if host.nbytes:
            assert hip.hipMemcpy(self.p, C.c_void_p(host.ctypes.data), C.c_size_t(host.nbytes), 1) == 0

    @property
    def addr(self):
        return self.p.value

    def get(self, n=None):
        out = np.zeros(self.nbytes if n is None else n, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out

    def __del__(self):
        if self.p:
            self.hip.hipFree(self.p)


def product(V, sc):
    v = V.View(sc.W, sc.H)
    v.set_pose(sc.pose)
    v.set_flags(sc.cams, sc.grid, sc.white)
    for Ht, s, key in sc.cameras:
        v.add_camera(Ht, s, key)
    for lists in sc.adds:
        v.add_points(lists)
    return v


def same(got, want, tag=""):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        raise AssertionError("%s: %d pixels differ, first at row %d column %d: got %s, wanted %s" % (
            tag, len(bad), bad[0][0], bad[0][1], got[bad[0][0], bad[0][1]], want[bad[0][0], bad[0][1]]))


def render_to_device(v, hip):
    d = Dev(hip, v.width * v.height * 3)
    v.render(device_ptr=d.addr)
    return d.get(v.width * v.height * 3).reshape(v.height, v.width, 3)


# ---- the scenes of tests/test_view.py ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", T.SCENES, ids=[s.name for s in T.SCENES])
def test_scene(V, hip, sc):
    """items 1-5 of the CPU file: through the host pointer and through a device pointer"""
    want = sc.ref().render()
    if sc.want is not None:
        assert np.array_equal(want, sc.want)
    v = product(V, sc)
    same(v.render(), want, sc.name + " (host)")
    same(render_to_device(v, hip), want, sc.name + " (device)")


# ---- block edges of the point kernel ---------------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize("n", COUNTS)
def test_block_edges(V, n):
    """256 points per workgroup, 64 per wave: the counts around both, as one list and split over three"""
    pts = T.cloud(n, 100 + n)
    ref = R.View(64, 48)
    ref.add_points([pts])
    want = ref.render()
    a = V.View(64, 48)
    a.add_points([pts])
    assert a.count(V.LISTS) == 1 and a.count(V.POINTS) == n
    same(a.render(), want, "one list")
    b = V.View(64, 48)
    cut = [0, n // 3, (2 * n) // 3, n]
    for k in range(3):
        b.add_points([pts[cut[k]:cut[k + 1]]])
    assert b.count(V.LISTS) == 3 and b.count(V.POINTS) == n
    same(b.render(), want, "three lists")


# ---- contention and ties across workgroups ---------------------------------------------------------------------------
def test_one_block_of_pixels_under_65536_points(V):
    """every footprint is the same 2 x 2 block, seven distinct depths: the first point of the nearest depth shows,
    whichever workgroup gets there first; a second render is the same image"""
    rng = np.random.default_rng(7)
    n = 65536
    depths = np.array([3.0, 2.5, 9.0, 2.0, 4.0, 2.25, 7.5], np.float32)
    pts = np.zeros((n, 4), np.float32)
    pts[:, 2] = depths[rng.integers(0, 7, n)]
    pts[:, 3] = rng.uniform(0, 1, n)
    pts[:100, 2] = 3.0          # the nearest depth does not come first
    first = int(np.flatnonzero(pts[:, 2] == 2.0)[0])
    assert first >= 100
    sc = T.Scene("contention", 64, 48, cams=False, grid=False, adds=[[pts]])
    want = sc.ref().render()
    g = int(R.grey_of(pts[first, 3]))
    assert (want[23:25, 31:33] == g).all() and int((want != 0).any(axis=2).sum()) <= 4
    v = product(V, sc)
    one = v.render()
    same(one, want, "contention")
    same(v.render(), one, "second render")


def test_4096_points_of_equal_depth(V):
    """a tie across sixteen workgroups: the first point's grey shows"""
    rng = np.random.default_rng(8)
    pts = np.zeros((4096, 4), np.float32)
    pts[:, 2] = 5.0
    pts[:, 3] = rng.uniform(0.1, 1, 4096)
    pts[0, 3] = 0.6
    sc = T.Scene("tie", 64, 48, cams=False, grid=False, adds=[[pts]])
    want = sc.ref().render()
    assert (want[23:25, 31:33] == 153).all()       # floor(0.6f * 255 + 0.5) = 153
    v = product(V, sc)
    one = v.render()
    same(one, want, "tie")
    same(v.render(), one, "second render")


# ---- sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Ht", [(1, 1), (1, 7), (7, 1), (320, 480), (1242, 375)])
def test_sizes(V, hip, W, Ht):
    """the smallest images, the reference's recording size and a KITTI frame: 20 k points, three cameras, default flags"""
    sc = T.Scene("size", W, Ht, adds=[[T.cloud(20000, 9, spread=6.0, far=30.0)]], cameras=T.drive_cameras(3, 10))
    want = sc.ref().render()
    v = product(V, sc)
    same(v.render(), want, "%dx%d (host)" % (W, Ht))
    same(render_to_device(v, hip), want, "%dx%d (device)" % (W, Ht))
    v.resize(Ht, W)      # the same object at the transposed size
    sc.W, sc.H = Ht, W
    same(v.render(), sc.ref().render(), "%dx%d after resize" % (Ht, W))


# ---- from the real chain -----------------------------------------------------------------------------------------------
def test_lists_come_from_the_map_fusion_on_the_device(V):
    """two consecutive golden urban D1 through svh_map_add, svh_view_add_map after each: counts and render equal the
    restatement on the lists downloaded with svh_map_points; a third frame of another size appends one list"""
    from svhip import mapper
    m = mapper.Mapper(721.5377, 609.5593, 172.854, 0.5371657, 12.0)
    v = V.View(160, 120)
    ref = R.View(160, 120)
    v.set_pose(T.ORBIT)
    ref.pose = T.ORBIT
    with pytest.raises(V.SvhError) as e:
        v.add_map(m)                       # before the first frame
    assert e.value.code == BAD_ARG and v.count(V.LISTS) == 0
    frames = []
    for k, name in enumerate(("urban2", "urban3")):
        z = np.load(os.path.join(H.GOLDEN, name + "_kitti.npz"))
        l, _ = H.golden_pair(str(z["crop"]))
        Ht = np.eye(4)
        Ht[2, 3] = 0.3 * k
        frames.append((z["d1"].reshape(l.shape), l, Ht))
    d, img, Ht = frames[1]
    frames.append((np.ascontiguousarray(d[60:300, 300:940]), np.ascontiguousarray(img[60:300, 300:940]), Ht))
    want_lists, lens = [1, 2, 3], []
    for k, (d, img, Ht) in enumerate(frames):
        m.add(d, img, Ht, 0.0)
        p0, p1 = m.points(0), m.points(1)
        v.add_camera(Ht, 0.1, True)
        v.add_map(m)
        ref.add_camera(Ht, 0.1, True)
        ref.add_points([p0, p1] if k == 1 else [p1])
        assert len(p1) > 1000 and (len(p0) > 0) == (k == 1)
        assert v.count(V.LISTS) == want_lists[k] == ref.count(0)
        assert v.count(V.POINTS) == ref.count(1) and v.count(V.CAMERAS) == k + 1
        same(v.render(), ref.render(), "frame %d" % k)
        lens.append([len(p0), len(p1)])
    # [C1], then [P1', C2], then the frame of another size appended C3 and dropped nothing
    assert [len(a) for a in ref.lists] == lens[1] + [lens[2][1]] and v.count(V.POINTS) == sum(lens[1]) + lens[2][1]
    m.clear()
    with pytest.raises(V.SvhError):
        v.add_map(m)                       # after svh_map_clear the map has no frame
    assert v.count(V.LISTS) == 3


def test_device_lists_through_add_points(V, hip):
    """svh_view_add_points with device pointers, an empty list among them, gives what the host path gives"""
    a, b, c = T.cloud(700, 31), T.cloud(0, 32), T.cloud(300, 33)
    ref = R.View(64, 48)
    v = V.View(64, 48)
    da, dc = Dev(hip, a), Dev(hip, c)
    for lists, ptrs in (([a], [da.addr]), ([b, c], [None, dc.addr]), ([a, b, c], [da.addr, None, dc.addr])):
        ref.add_points(lists)
        v.add_points_device(ptrs, [len(x) for x in lists])
        assert v.count(V.LISTS) == ref.count(0) and v.count(V.POINTS) == ref.count(1)
        same(v.render(), ref.render(), "device lists")
    v.clear()
    assert (v.count(V.LISTS), v.count(V.POINTS), v.count(V.CAMERAS)) == (0, 0, 0)
    ref.clear()
    same(v.render(), ref.render(), "after clear")


# ---- growth ----------------------------------------------------------------------------------------------------------
def test_store_grows_and_keeps_its_content(V):
    """3 x 4096 points: the store starts at 4096, doubles twice and moves what it holds device to device"""
    ref = R.View(64, 48)
    v = V.View(64, 48)
    caps = [v.count(V.CAPACITY)]
    for k in range(3):
        pts = T.cloud(4096, 40 + k)
        ref.add_points([pts])
        v.add_points([pts])
        caps.append(v.count(V.CAPACITY))
        same(v.render(), ref.render(), "after %d lists" % (k + 1))
    assert caps == [0, 4096, 8192, 16384], caps


# ---- playPoses -------------------------------------------------------------------------------------------------------
def test_play_poses(V):
    sc = T.Scene("fly", 32, 24, adds=[[T.cloud(500, 50)]], cameras=T.drive_cameras(2, 51))
    poses = R.human_poses(T.ORBIT)
    seq = R.play_sequence(poses)
    assert len(seq) == 102
    v = product(V, sc)
    n, frames = v.play_poses(poses)
    assert n == 102 and frames.shape == (102, 24, 32, 3)
    ref = sc.ref()
    for k in (0, 50, 51, 101):
        ref.pose = seq[k]
        same(frames[k], ref.render(), "frame %d" % k)
    assert v.pose.astuple() == seq[101]
    same(v.render(), frames[101], "the pose afterwards is the last one rendered")
    # cap = 5: five frames are written, the sixth is not, and the count is still 102
    out = np.full((6, 24, 32, 3), 0xEE, np.uint8)
    arr = V._pose_array(poses)
    assert V.lib().svh_view_play_poses(v._h, arr, 3, out.ctypes.data, 5, 0) == 102
    assert np.array_equal(out[:5], frames[:5]) and (out[5] == 0xEE).all()
    assert V.lib().svh_view_play_poses(v._h, arr, 1, out.ctypes.data, 5, 0) == 0      # n < 2: no frames
    assert V.lib().svh_view_play_poses(v._h, arr, 3, None, 0, 0) == 102               # nothing kept


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_change_nothing(V):
    L = V.lib()
    sc = T.Scene("args", 64, 48, adds=[[T.cloud(900, 60)]], cameras=T.drive_cameras(2, 61))
    v = product(V, sc)
    before = v.render()
    counts = [v.count(k) for k in range(4)]
    pts = T.cloud(10, 62)
    one_ptr = (C.c_void_p * 1)(pts.ctypes.data)
    null_ptr = (C.c_void_p * 1)(None)
    n10, nneg, nbig = (C.c_int64 * 1)(10), (C.c_int64 * 1)(-1), (C.c_int64 * 1)(2 ** 31 - 4095 - 900)
    pose, flags = V.default_pose(), V.Flags(1, 1, 0)
    Hm = np.eye(4)
    img = np.zeros((48, 64, 3), np.uint8)
    calls = [
        lambda: L.svh_view_add_points(None, one_ptr, n10, 1, 0),
        lambda: L.svh_view_add_points(v._h, one_ptr, n10, -1, 0),
        lambda: L.svh_view_add_points(v._h, one_ptr, nneg, 1, 0),
        lambda: L.svh_view_add_points(v._h, null_ptr, n10, 1, 0),
        lambda: L.svh_view_add_points(v._h, None, n10, 1, 0),
        lambda: L.svh_view_add_points(v._h, one_ptr, None, 1, 0),
        lambda: L.svh_view_resize(v._h, 0, 48),
        lambda: L.svh_view_resize(v._h, 64, 16385),
        lambda: L.svh_view_resize(None, 64, 48),
        lambda: L.svh_view_set_pose(v._h, None),
        lambda: L.svh_view_set_pose(None, C.byref(pose)),
        lambda: L.svh_view_set_flags(v._h, None),
        lambda: L.svh_view_set_flags(None, C.byref(flags)),
        lambda: L.svh_view_add_camera(v._h, None, 0.1, 1),
        lambda: L.svh_view_add_camera(None, Hm.ctypes.data, 0.1, 1),
        lambda: L.svh_view_add_map(v._h, None),
        lambda: L.svh_view_add_map(None, None),
        lambda: L.svh_view_render(v._h, None, 0),
        lambda: L.svh_view_render(None, img.ctypes.data, 0),
        lambda: L.svh_view_play_poses(v._h, None, 3, img.ctypes.data, 1, 0),
        lambda: L.svh_view_play_poses(v._h, C.byref(pose), 2, None, 1, 0),
        lambda: L.svh_view_play_poses(v._h, C.byref(pose), -1, None, 0, 0),
    ]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG, k
        assert [v.count(j) for j in range(4)] == counts, k
    assert L.svh_view_create(0, 48) is None and L.svh_view_create(64, 16385) is None
    same(v.render(), before, "after the refused calls")
    # draw indices are 32 bits: 2^31 - 4096 points are the limit, decided before a point is read
    assert L.svh_view_add_points(v._h, one_ptr, nbig, 1, 0) == UNSUPPORTED
    assert [v.count(j) for j in range(4)] == counts
    same(v.render(), before, "after the refused list")


def test_simulated_hip_errors(V, capfd):
    """svh_test_fail_at makes the n-th guarded HIP call of a kind report an error without being issued (no GPU fault is
    involved): the store's allocation in add_points, the staging allocation, the store's growth, a copy of the render"""
    import svhip as S
    L = V.lib()
    ref = R.View(64, 48)
    v = V.View(64, 48)
    a, b = T.cloud(3000, 70), T.cloud(3000, 71)
    for spec in ("malloc:1", "malloc:2"):          # the store, then the pinned staging buffer
        L.svh_test_fail_at(spec.encode())
        with pytest.raises(V.SvhError) as e:
            v.add_points([a])
        L.svh_test_fail_at(None)
        assert e.value.code == HIP_ERR and "injected failure" in S.last_error()
        assert v.count(V.LISTS) == 0 and v.count(V.POINTS) == 0
    assert "svhip: View" in capfd.readouterr().err
    v.add_points([a])
    ref.add_points([a])
    want = ref.render()
    same(v.render(), want, "after the failed allocations")
    L.svh_test_fail_at(b"malloc:1")                # the growth from 4096 to 8192 points
    with pytest.raises(V.SvhError):
        v.add_points([b])
    L.svh_test_fail_at(None)
    assert v.count(V.POINTS) == 3000 and v.count(V.CAPACITY) == 4096
    same(v.render(), want, "after the failed growth")
    img = np.full((48, 64, 3), 0xEE, np.uint8)
    for spec in ("copy:1", "copy:2", "copy:3", "copy:4", "launch:1", "wait:1"):   # segments, two clears, the copy back
        L.svh_test_fail_at(spec.encode())
        assert L.svh_view_render(v._h, img.ctypes.data, 0) == HIP_ERR, spec
        assert "injected failure" in S.last_error()
        L.svh_test_fail_at(None)
        assert (img == 0xEE).all(), spec
        same(v.render(), want, "after " + spec)
    v.add_points([b])
    ref.add_points([b])
    same(v.render(), ref.render(), "the object goes on")


# ---- the pipeline tool ---------------------------------------------------------------------------------------------------
def two_frame_drive(root):
    """the reference's two consecutive quad pairs as a KITTI-shaped drive"""
    import test_kitti_io as TK
    pairs = [(H.read_pgm(os.path.join(H.GOLDEN, "viso_I1p.pgm")), H.read_pgm(os.path.join(H.GOLDEN, "viso_I2p.pgm"))),
             (H.read_pgm(os.path.join(H.GOLDEN, "viso_I1c.pgm")), H.read_pgm(os.path.join(H.GOLDEN, "viso_I2c.pgm")))]
    for k in range(2):
        (root / ("image_0%d" % k) / "data").mkdir(parents=True)
        lines = []
        for i in range(2):
            lines.append("2011-09-26 13:02:%02d.%09d" % (25 + i, 100000000 * i))
            TK.write_png(str(root / ("image_0%d" % k) / "data" / ("%010d.png" % i)), pairs[i][k][:, :, None], filters=[i, 2])
        (root / ("image_0%d" % k) / "timestamps.txt").write_text("\n".join(lines) + "\n")
    return root


def test_pipeline_feeds_the_view(V, tmp_path):
    """tools/stereomapper_pipeline.py: after each frame the view holds the camera and the map's lists -- [C1], then
    [P1', C2] -- and draws what the restatement draws from the downloaded lists and the pipeline's poses"""
    import sys
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    from svhip import kitti
    p = SP.Pipeline(645.24, 635.96, 194.13, 0.5707, view_size=(80, 120))
    ref = R.View(80, 120)
    for i, (I1, I2, _) in enumerate(kitti.Sequence(two_frame_drive(tmp_path / "drive"))):
        ok, n0, n1 = p.push(I1, I2)
        ref.add_camera(p.poses[-1], 0.1, True)
        ref.add_points([p.map.points(1)] if i == 0 else [p.map.points(0), p.map.points(1)])
        assert n1 > 20000 and p.view.count(V.LISTS) == i + 1 and p.view.count(V.CAMERAS) == i + 1
        assert p.view.count(V.POINTS) == ref.count(1) == (n1 if i == 0 else n0 + n1)
    same(p.view.render(), ref.render(), "the pipeline's map")


def test_pipeline_render_option_writes_the_images(V, tmp_path, monkeypatch, capsys):
    """--render DIR: one PPM per frame and recordHuman's 102 images at the reference's recording size; without the
    flag no file is written and the per-frame lines are the same"""
    import sys
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    drive = two_frame_drive(tmp_path / "drive")
    calib = tmp_path / "calib_cam_to_cam.txt"
    import test_rectify as TR
    calib.write_text(TR.rig_calib_text())
    out = tmp_path / "render"
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--render", str(out), str(drive), str(calib)])
    SP.main()
    with_flag = [l for l in capsys.readouterr().out.splitlines() if l.startswith("frame ")]
    names = sorted(os.listdir(out))
    assert names == ["frame_%06d.ppm" % k for k in range(2)] + ["img_320_480_%06d.ppm" % k for k in range(102)]
    for name in (names[1], names[2], names[-1]):
        raw = open(out / name, "rb").read()
        assert raw.startswith(b"P6\n320 480\n255\n") and len(raw) == 15 + 320 * 480 * 3
        assert np.frombuffer(raw[15:], np.uint8).any()
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", str(drive), str(calib)])
    SP.main()
    assert [l for l in capsys.readouterr().out.splitlines() if l.startswith("frame ")] == with_flag
    assert sorted(os.listdir(tmp_path)) == ["calib_cam_to_cam.txt", "drive", "render"]


# ---- the drop-in class -----------------------------------------------------------------------------------------------------
def test_view3d_dropin_program(tmp_path):
    """include/view3d.h, compiled with only include/ on the path: addCamera, addPoints twice, render, recordHuman -- the
    image and the last recorded frame equal the restatement, 102 PPM files are written"""
    import subprocess
    exe, lib_dir = str(tmp_path / "view3d_dropin"), os.path.join(H.ROOT, "stereo-vision_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "view", "view3d_dropin.cpp"), "-L", lib_dir, "-lsvhip",
                           "-Wl,-rpath," + lib_dir])
    p0, p1 = T.cloud(300, 80), T.cloud(500, 81)
    (tmp_path / "points.bin").write_bytes(np.array([300, 500], np.int32).tobytes() + p0.tobytes() + p1.tobytes())
    out = tmp_path / "rec"
    out.mkdir()
    res = subprocess.run([exe, str(tmp_path / "points.bin"), str(out)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "view3d ok" in res.stdout, (res.returncode, res.stderr[-500:])
    ref = R.View(32, 24)
    H2 = np.eye(4)
    H2[2, 3], H2[0, 3] = 0.8, 0.1
    ref.add_camera(np.eye(4), 0.1, True)
    ref.add_camera(H2, 0.1, False)
    ref.add_points([p1])
    ref.add_points([p0, p1])
    assert [len(a) for a in ref.lists] == [300, 500]
    got = np.frombuffer((out / "render.rgb").read_bytes(), np.uint8).reshape(24, 32, 3)
    same(got, ref.render(), "View3D::render")
    names = sorted(n for n in os.listdir(out) if n.endswith(".ppm"))
    assert names == ["img_32_24_%06d.ppm" % k for k in range(102)]
    seq = R.play_sequence(R.human_poses(R.DEFAULT_POSE))
    for k in (0, 101):
        raw = (out / names[k]).read_bytes()
        assert raw.startswith(b"P6\n32 24\n255\n")
        ref.pose = seq[k]
        same(np.frombuffer(raw[len(b"P6\n32 24\n255\n"):], np.uint8).reshape(24, 32, 3), ref.render(), names[k])

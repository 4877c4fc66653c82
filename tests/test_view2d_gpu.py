"""GPU: the 2-D panes (include/svh_view2d.h, csrc/view2d_kernels.hip, csrc/view2d_engine.cpp) against the numpy
restatement tests/view2d_ref.py, which tests/test_view2d.py pins on the CPU.  Every image comparison is exact
(np.array_equal on the RGB bytes): the render has no tolerance, the winner of a pixel does not depend on scheduling."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import test_view2d as T
import view2d_ref as R
from test_view_gpu import Dev, same, two_frame_drive

pytestmark = pytest.mark.gpu

BAD_ARG, HIP_ERR = -1, -2


@pytest.fixture(scope="module")
def V():
    import svhip
    from svhip import view2d
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    view2d._bind()
    return view2d


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(autouse=True)
def disarm(V):
    yield
    V.lib().svh_test_fail_at(None)


class DevicePlayer:
    """a product pane whose sources all come from device memory (the indexed form of the matches is host only)"""

    def __init__(self, V, hip, W, Ht):
        self.v, self.hip, self.keep = V.View2D(W, Ht), hip, []

    def up(self, a):
        d = Dev(self.hip, a)
        self.keep.append(d)
        return d.addr

    def set_image(self, I):
        I = np.ascontiguousarray(I, np.uint8)
        self.v.set_image_device(self.up(I), I.shape[1], I.shape[0])

    def set_color_image(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.float32)
        self.v.set_color_image_device(self.up(rgb), rgb.shape[1], rgb.shape[0])

    def set_disparity(self, D):
        D = np.ascontiguousarray(D, np.float32)
        self.v.set_disparity_device(self.up(D), D.shape[1], D.shape[0])

    def set_matches(self, m, flags, left):
        m, f = np.ascontiguousarray(m, R.P_MATCH), np.ascontiguousarray(flags, np.uint8)
        self.v.set_matches_device(self.up(m), len(m), self.up(f), left)

    def set_matches_indexed(self, m, idx, left):
        self.v.set_matches_indexed(m, idx, left)

    def clear_matches(self):
        self.v.clear_matches()

    def resize(self, W, Ht):
        self.v.resize(W, Ht)


def render_to_device(v, hip, offset=0):
    """the image through a device pointer `offset` bytes into an allocation; the bytes around it stay 0xEE"""
    n = v.width * v.height * 3
    d = Dev(hip, n + offset + 5)
    v.render(device_ptr=d.addr + offset)
    raw = d.get(n + offset + 5)
    assert (raw[:offset] == 0xEE).all() and (raw[offset + n:] == 0xEE).all(), "bytes outside the image were written"
    return raw[offset:offset + n].reshape(v.height, v.width, 3)


# ---- the scenes of tests/test_view2d.py ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", T.SCENES, ids=[s.name for s in T.SCENES])
def test_scene(V, hip, sc):
    """every CPU scene: sources and output on the host, and sources and output on the device"""
    want = sc.ref().render()
    if sc.want is not None:
        assert np.array_equal(want, sc.want)
    v = sc.play(V.View2D(sc.W, sc.H))
    same(v.render(), want, sc.name + " (host)")
    d = sc.play(DevicePlayer(V, hip, sc.W, sc.H))
    same(render_to_device(d.v, hip), want, sc.name + " (device)")
    same(d.v.render(), want, sc.name + " (device sources, host image)")


# ---- block and tail edges -----------------------------------------------------------------------------------------------------
# four pixels per thread, 256 threads per block: 1, 3, 4, 5 pixels around a group; 255, 256, 257 groups' worth and 1023,
# 1024, 1025 pixels around a block; 1025 x 3 is the issue's; every width also as a height
PANES = [(1, 1), (3, 1), (4, 1), (2, 2), (5, 1), (1, 5), (255, 1), (256, 1), (257, 1), (1023, 1), (1024, 1), (1025, 1),
         (1025, 3), (64, 48)]


@pytest.mark.parametrize("W,Ht", PANES, ids=["%dx%d" % p for p in PANES])
def test_pane_sizes(V, hip, W, Ht):
    """the image and 60 matches at every pane size, at the transposed size too, to the host, to an aligned device
    pointer and to one that is 1 byte off"""
    m, f = T.random_matches(60, 21, 37, 29)
    I = T.random_image(37, 29, 22)
    ref = R.View2D(W, Ht)
    ref.set_image(I)
    ref.set_matches(m, f, True)
    v = V.View2D(W, Ht)
    v.set_image(I)
    v.set_matches(m, f, True)
    for size in ((W, Ht), (Ht, W)):
        ref.resize(*size)
        v.resize(*size)
        want = ref.render()
        same(v.render(), want, "host")
        same(render_to_device(v, hip), want, "device")
        same(render_to_device(v, hip, 1), want, "device + 1")
    v.clear_matches()
    ref.clear_matches()
    same(render_to_device(v, hip, 1), ref.render(), "no matches, device + 1")


@pytest.mark.parametrize("w", [15, 16, 17])
def test_grey_source_at_odd_pitch_and_odd_address(V, hip, w):
    """rows of w bytes, an odd pitch apart (w + 2 or w + 3), starting 1 and 3 bytes into a device allocation whose other
    bytes are 0xEE; and a strided host image"""
    h, pitch = 9, w + 3 - (w % 2)
    assert pitch % 2 == 1 and pitch > w
    I = T.random_image(w, h, 30 + w)
    ref = R.View2D(40, 23)
    ref.set_image(I)
    want = ref.render()
    for base in (1, 3):
        raw = np.full(base + pitch * (h - 1) + w, 0xEE, np.uint8)       # ends with the last row: nothing behind it
        for y in range(h):
            raw[base + y * pitch: base + y * pitch + w] = I[y]
        d = Dev(hip, raw)
        v = V.View2D(40, 23)
        v.set_image_device(d.addr + base, w, h, pitch)
        same(v.render(), want, "base %d" % base)
    wide = np.full((h, pitch), 0xEE, np.uint8)
    wide[:, 1:1 + w] = I
    v.set_image(wide[:, 1:1 + w])
    same(v.render(), want, "strided host image")


@pytest.mark.parametrize("w", [2, 3, 4, 5, 341, 342, 343])
def test_float_sources_at_any_address(V, hip, w):
    """3 w texels of a disparity map and of a float RGB image -- 6, 9, 12 and 15 around a group of four, 1023, 1026 and
    1029 around a block of groups -- 16-byte aligned, 4-byte aligned and at an odd byte"""
    D = T.random_disparity(w, 3, 40 + w)
    rgb = np.random.default_rng(41 + w).uniform(-0.2, 1.2, (3, w, 3)).astype(np.float32)
    ref = R.View2D(min(2 * w, 400), 5)
    v = V.View2D(min(2 * w, 400), 5)
    for src, setter, rset in ((D, v.set_disparity_device, ref.set_disparity), (rgb, v.set_color_image_device, ref.set_color_image)):
        rset(src)
        want = ref.render()
        for base in (0, 4, 1):
            raw = np.full(base + src.nbytes, 0xEE, np.uint8)
            raw[base:] = src.view(np.uint8).ravel()
            d = Dev(hip, raw)
            setter(d.addr + base, w, 3)
            same(v.render(), want, "%s at +%d" % (src.shape, base))


# ---- match counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_match_counts(V, hip, n):
    """64 matches per block: from the host, from the device and in the indexed form"""
    m, f = T.random_matches(n, 50 + n, 64, 48, spread=1.0)
    I = T.random_image(64, 48, 51)
    ref = R.View2D(64, 48)
    ref.set_image(I)
    ref.set_matches(m, f, True)
    want = ref.render()
    v = V.View2D(64, 48)
    v.set_image(I)
    v.set_matches(m, f, True)
    same(v.render(), want, "host matches")
    dm, df = Dev(hip, m), Dev(hip, f)
    v.clear_matches()
    v.set_matches_device(dm.addr, n, df.addr, True)
    same(v.render(), want, "device matches")
    v.clear_matches()
    v.set_matches_indexed(m, np.flatnonzero(f), True)
    same(v.render(), want, "indexed matches")
    v.set_matches(m, f, False)
    ref.set_matches(m, f, False)
    same(v.render(), ref.render(), "right pane")


def test_1024_points_on_one_pixel(V):
    """sixteen blocks of matches whose points all cover the pane's centre: the last one shows, and a second render is
    the same image"""
    n = 1024
    m = np.zeros(n, R.P_MATCH)
    rng = np.random.default_rng(60)
    m["u1p"] = m["u1c"] = 32 + rng.integers(-2, 3, n)
    m["v1p"] = m["v1c"] = 24 + rng.integers(-2, 3, n)
    m["u2p"] = m["u1p"] - rng.uniform(0, 100, n).astype(np.float32)
    f = np.ones(n, np.uint8)
    ref = R.View2D(64, 48)
    ref.set_image(np.zeros((48, 64), np.uint8))
    ref.set_matches(m, f, True)
    want = ref.render()
    assert tuple(want[24, 32]) == R.match_colour(m[n - 1], True) and len({tuple(p) for p in want.reshape(-1, 3)}) > 5
    v = V.View2D(64, 48)
    v.set_image(np.zeros((48, 64), np.uint8))
    v.set_matches(m, f, True)
    one = v.render()
    same(one, want, "ties")
    same(v.render(), one, "second render")


# ---- real data ----------------------------------------------------------------------------------------------------------------------
def test_matches_of_the_visual_odometry(V, hip):
    """the golden libviso2 frames through the product's visual odometry: both match panes, the frame taken on the device"""
    frames = [[H.read_pgm(os.path.join(H.GOLDEN, "viso_I%d%s.pgm" % (k, t))) for k in (1, 2)] for t in ("p", "c")]
    vo = H.ProductVo(H.vo_defaults(f=645.24, cu=635.96, cv=194.13, base=0.5707))
    vo.process(*frames[0])
    assert vo.process(*frames[1]) == 1
    m, idx = vo.matches(), vo.inliers()
    assert len(m) > 100 and 50 < len(idx) <= len(m)
    h, w = frames[1][0].shape
    W, Ht = w // 2, h // 2
    for k, left in ((0, True), (1, False)):
        ref = R.View2D(W, Ht)
        ref.set_image(frames[1][k])
        ref.set_matches_indexed(m, idx, left)
        v = V.View2D(W, Ht)
        d = Dev(hip, frames[1][k])
        v.set_image_device(d.addr, w, h, w)
        v.set_matches_indexed(m, idx, left)
        same(v.render(), ref.render(), "left" if left else "right")


def test_disparity_map_from_elas_on_the_device(V, hip):
    """D1 of a 640 x 240 golden crop, read where svh_elas_process_batch_device wrote it, in a 320 x 120 pane"""
    import svhip as S
    z = np.load(os.path.join(H.GOLDEN, "urban3_demo.npz"))
    prm = H.ElasParams.from_buffer_copy(z["params"].tobytes())
    l, r = H.golden_pair(str(z["crop"]))
    h, w = l.shape
    assert (w, h) == (640, 240)
    n = w * h
    dl, dr, d1, d2 = Dev(hip, l), Dev(hip, r), Dev(hip, 4 * n), Dev(hip, 4 * n)
    st = S.Elas(prm).process_batch_device(1, dl.addr, dr.addr, n, d1.addr, d2.addr, 4 * n, w, h, w)
    assert st[0] == 0
    D1 = d1.get(4 * n).view(np.float32).reshape(h, w)
    assert np.array_equal(D1.ravel(), z["d1"])
    ref = R.View2D(320, 120)
    ref.set_disparity(D1)
    want = ref.render()
    assert len({tuple(p) for p in want.reshape(-1, 3)}) > 50
    v = V.View2D(320, 120)
    v.set_disparity_device(d1.addr, w, h)
    same(v.render(), want, "device D1")
    same(render_to_device(v, hip), want, "device D1 to the device")
    v.set_disparity(D1)
    same(v.render(), want, "host D1")


# ---- contracts ------------------------------------------------------------------------------------------------------------------------
def held_pane(V):
    m, f = T.random_matches(80, 70, 37, 29)
    I = T.random_image(37, 29, 71)
    v = V.View2D(64, 48)
    v.set_image(I)
    v.set_matches(m, f, True)
    return v, m, f, I


def test_bad_arguments_change_nothing(V):
    L = V.lib()
    v, m, f, I = held_pane(V)
    before = v.render()
    dims = (C.c_int32 * 3)(37, 29, 37)
    bad_dims = [(C.c_int32 * 3)(*d) for d in ((0, 29, 37), (37, 0, 37), (37, 29, 36), (16385, 29, 16385), (37, 16385, 37))]
    rgb = np.zeros((29, 37, 3), np.float32)
    D = np.zeros((29, 37), np.float32)
    idx = np.array([0, 5, 80], np.int32)       # 80 is outside 0..79
    neg = np.array([-1], np.int32)
    img = np.zeros((48, 64, 3), np.uint8)
    calls = [
        lambda: L.svh_view2d_resize(v._h, 0, 48),
        lambda: L.svh_view2d_resize(v._h, 64, 16385),
        lambda: L.svh_view2d_resize(None, 64, 48),
        lambda: L.svh_view2d_set_image(None, I.ctypes.data, dims, 0),
        lambda: L.svh_view2d_set_image(v._h, None, dims, 0),
        lambda: L.svh_view2d_set_image(v._h, I.ctypes.data, None, 0),
    ] + [(lambda d: lambda: L.svh_view2d_set_image(v._h, I.ctypes.data, d, 0))(d) for d in bad_dims] + [
        lambda: L.svh_view2d_set_color_image(None, rgb.ctypes.data, 37, 29, 0),
        lambda: L.svh_view2d_set_color_image(v._h, None, 37, 29, 0),
        lambda: L.svh_view2d_set_color_image(v._h, rgb.ctypes.data, 0, 29, 0),
        lambda: L.svh_view2d_set_color_image(v._h, rgb.ctypes.data, 37, 16385, 0),
        lambda: L.svh_view2d_set_disparity(None, D.ctypes.data, 37, 29, 0),
        lambda: L.svh_view2d_set_disparity(v._h, None, 37, 29, 0),
        lambda: L.svh_view2d_set_disparity(v._h, D.ctypes.data, 37, -1, 0),
        lambda: L.svh_view2d_set_disparity(v._h, D.ctypes.data, 16385, 29, 0),
        lambda: L.svh_view2d_set_matches(None, m.ctypes.data, 80, f.ctypes.data, 1, 0),
        lambda: L.svh_view2d_set_matches(v._h, m.ctypes.data, -1, f.ctypes.data, 1, 0),
        lambda: L.svh_view2d_set_matches(v._h, None, 80, f.ctypes.data, 1, 0),
        lambda: L.svh_view2d_set_matches(v._h, m.ctypes.data, 80, None, 1, 0),
        lambda: L.svh_view2d_set_matches_indexed(None, m.ctypes.data, 80, idx.ctypes.data, 2, 1),
        lambda: L.svh_view2d_set_matches_indexed(v._h, m.ctypes.data, -1, idx.ctypes.data, 2, 1),
        lambda: L.svh_view2d_set_matches_indexed(v._h, None, 80, idx.ctypes.data, 2, 1),
        lambda: L.svh_view2d_set_matches_indexed(v._h, m.ctypes.data, 80, None, 2, 1),
        lambda: L.svh_view2d_set_matches_indexed(v._h, m.ctypes.data, 80, idx.ctypes.data, -1, 1),
        lambda: L.svh_view2d_set_matches_indexed(v._h, m.ctypes.data, 80, idx.ctypes.data, 3, 1),
        lambda: L.svh_view2d_set_matches_indexed(v._h, m.ctypes.data, 80, neg.ctypes.data, 1, 1),
        lambda: L.svh_view2d_render(v._h, None, 0),
        lambda: L.svh_view2d_render(None, img.ctypes.data, 0),
    ]
    for k, call in enumerate(calls):
        assert call() == BAD_ARG, k
        same(v.render(), before, "after refused call %d" % k)
    assert L.svh_view2d_create(0, 48) is None and L.svh_view2d_create(64, 16385) is None
    L.svh_view2d_clear_matches(None)
    L.svh_view2d_destroy(None)
    same(v.render(), before, "after the refused calls")


def test_simulated_hip_errors(V, hip, capfd):
    """svh_test_fail_at makes the n-th guarded HIP call of a kind report an error without being issued (no GPU fault is
    involved): allocations, copies, launches and waits of every entry.  Each call returns SVH_ERR_HIP, leaves the
    caller's buffer as it was and the pane showing what it showed"""
    import svhip as S
    L = V.lib()
    v, m, f, I = held_pane(V)
    before = v.render()

    def failing(spec, call):
        L.svh_test_fail_at(spec.encode())
        with pytest.raises(V.SvhError) as e:
            call()
        L.svh_test_fail_at(None)
        assert e.value.code == HIP_ERR and "injected failure" in S.last_error(), spec
        same(v.render(), before, "after " + spec)

    big = T.random_image(80, 60, 72)
    # the texels, the pinned staging buffer, the device staging buffer (the texels exist by then), the upload, the
    # conversion, the wait
    for spec in ("malloc:1", "malloc:2", "malloc:2", "copy:1", "launch:1", "wait:1"):
        failing(spec, lambda: v.set_image(big))
    assert "svhip: View2D" in capfd.readouterr().err
    dD = Dev(hip, T.random_disparity(80, 60, 73))
    for spec in ("launch:1", "wait:1"):
        failing(spec, lambda: v.set_disparity_device(dD.addr, 80, 60))
    failing("copy:1", lambda: v.set_color_image(np.zeros((60, 80, 3), np.float32)))
    m2, f2 = T.random_matches(3000, 74, 37, 29)
    for spec in ("malloc:1", "malloc:2", "copy:1", "copy:2", "wait:1"):
        failing(spec, lambda: v.set_matches(m2, f2, False))
    dm, df = Dev(hip, m2), Dev(hip, f2)
    for spec in ("copy:1", "copy:2"):
        failing(spec, lambda: v.set_matches_device(dm.addr, 3000, df.addr, False))
    # the render: the overlay's clear, the launches, the copy back, the wait -- the caller's image stays 0xEE
    img = np.full((48, 64, 3), 0xEE, np.uint8)
    for spec in ("copy:1", "launch:1", "copy:2", "wait:1"):
        L.svh_test_fail_at(spec.encode())
        assert L.svh_view2d_render(v._h, img.ctypes.data, 0) == HIP_ERR, spec
        assert "injected failure" in S.last_error()
        L.svh_test_fail_at(None)
        assert (img == 0xEE).all(), spec
        same(v.render(), before, "after render " + spec)
    out = Dev(hip, 64 * 48 * 3)
    for spec in ("copy:1", "launch:1"):
        L.svh_test_fail_at(spec.encode())
        assert L.svh_view2d_render(v._h, out.addr, 1) == HIP_ERR, spec
        L.svh_test_fail_at(None)
        assert (out.get() == 0xEE).all(), spec
    # a larger pane needs a larger overlay: that allocation fails, the size asked for stays and the next render works
    v.resize(128, 96)
    big_img = np.full((96, 128, 3), 0xEE, np.uint8)
    L.svh_test_fail_at(b"malloc:1")
    assert L.svh_view2d_render(v._h, big_img.ctypes.data, 0) == HIP_ERR and (big_img == 0xEE).all()
    L.svh_test_fail_at(None)
    ref = R.View2D(128, 96)
    ref.set_image(I)
    ref.set_matches(m, f, True)
    same(v.render(), ref.render(), "the larger pane")
    v.resize(64, 48)
    same(v.render(), before, "back at the first size")
    v.set_image(big)
    ref = R.View2D(64, 48)
    ref.set_image(big)
    same(v.render(), ref.render(), "the object goes on")


# ---- the drop-in class ------------------------------------------------------------------------------------------------------------------
def test_view2d_dropin_program(tmp_path):
    """include/view2d.h, compiled with only include/ on the path: setImage, setMatches for both panes, resizeGL,
    setDisparity, clearMatches, grabFrameBuffer and the PPM writer give the restatement's images"""
    exe, lib_dir = str(tmp_path / "view2d_dropin"), os.path.join(H.ROOT, "stereo-vision_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "view", "view2d_dropin.cpp"), "-L", lib_dir, "-lsvhip",
                           "-Wl,-rpath," + lib_dir])
    w, h, n = 64, 48, 150
    m, f = T.random_matches(n, 80, w, h)
    I, D = T.random_image(w, h, 81), T.random_disparity(w, h, 82)
    (tmp_path / "job.bin").write_bytes(np.array([w, h, n], np.int32).tobytes() + I.tobytes() + m.tobytes() + f.tobytes() + D.tobytes())
    out = tmp_path / "out"
    out.mkdir()
    res = subprocess.run([exe, str(tmp_path / "job.bin"), str(out)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "view2d ok" in res.stdout, (res.returncode, res.stderr[-500:])
    ref = R.View2D(w, h)
    ref.set_image(I)
    for name, left in (("left.rgb", True), ("right.rgb", False)):
        ref.set_matches(m, f, left)
        same(np.frombuffer((out / name).read_bytes(), np.uint8).reshape(h, w, 3), ref.render(), name)
    ref.resize(w // 2, h // 2)
    ref.set_disparity(D)
    raw = (out / "disp.ppm").read_bytes()
    head = b"P6\n%d %d\n255\n" % (w // 2, h // 2)
    assert raw.startswith(head)
    same(np.frombuffer(raw[len(head):], np.uint8).reshape(h // 2, w // 2, 3), ref.render(), "disp.ppm")
    ref.clear_matches()
    same(np.frombuffer((out / "clear.rgb").read_bytes(), np.uint8).reshape(h // 2, w // 2, 3), ref.render(), "clear.rgb")


# ---- the pipeline tool --------------------------------------------------------------------------------------------------------------------
def test_pipeline_panes(V, tmp_path):
    """tools/stereomapper_pipeline.py: the three panes of a resident frame are what the restatement draws from the
    frame, the visual odometry's matches and D1 downloaded"""
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    from svhip import kitti
    p = SP.Pipeline(645.24, 635.96, 194.13, 0.5707, view_size=(80, 120), resident=True)
    for I1, I2, _ in kitti.Sequence(two_frame_drive(tmp_path / "drive")):
        ok, n0, n1 = p.push(I1, I2)
    assert ok
    h, w = I1.shape
    got = p.render_panes((w // 4, h // 4))
    m, idx = p.vo.matches(), p.vo.inliers()
    ref = R.View2D(w // 4, h // 4)
    for k, I in enumerate((I1, I2)):
        ref.set_image(I)
        ref.set_matches_indexed(m, idx, k == 0)
        same(got[k], ref.render(), "pane %d" % k)
    D1 = p.buf[2].download(np.empty((h, w), np.float32))
    ref.clear_matches()
    ref.set_disparity(D1)
    same(got[2], ref.render(), "disparity pane")


def test_pipeline_panes_option_writes_the_images(V, tmp_path, monkeypatch, capsys):
    """--panes DIR [--pane-size WxH]: three PPM files per frame; the printed lines are those of a run without the flag,
    which writes nothing"""
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    import test_rectify as TR
    drive = two_frame_drive(tmp_path / "drive")
    calib = tmp_path / "calib_cam_to_cam.txt"
    calib.write_text(TR.rig_calib_text())
    out = tmp_path / "panes"
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--resident", "--panes", str(out), "--pane-size", "310x94",
                                      str(drive), str(calib)])
    SP.main()
    with_flag = [l for l in capsys.readouterr().out.splitlines() if not l.endswith("(PNG decode included)")]
    assert sorted(os.listdir(out)) == sorted("%s_%06d.ppm" % (n, k) for n in ("left", "right", "disp") for k in range(2))
    for name in os.listdir(out):
        raw = open(out / name, "rb").read()
        assert raw.startswith(b"P6\n310 94\n255\n") and len(raw) == 14 + 310 * 94 * 3, name
        assert np.frombuffer(raw[14:], np.uint8).any(), name
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--resident", str(drive), str(calib)])
    SP.main()
    assert [l for l in capsys.readouterr().out.splitlines() if not l.endswith("(PNG decode included)")] == with_flag
    assert sorted(os.listdir(tmp_path)) == ["calib_cam_to_cam.txt", "drive", "panes"]

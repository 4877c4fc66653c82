"""Frames in device memory for the Matcher, the visual odometry and the map fusion: svh_matcher_push_back_device,
svh_vo_process_device, svh_vo_mono_process_device and svh_map_add_device give, bit for bit, what the host entries give
for the same pixels.  k_pack_rows is checked alone against numpy at every alignment, k_gain against the host loop and
the numpy restatement (tests/resident_ref.py) on matches at and past the image border, and the whole stereomapper data
path with `resident=True` against the path that takes the frame back to the host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import helpers as H
import resident_ref as RR

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(H.ROOT, "tools"))


@pytest.fixture(scope="module")
def S():
    import svhip
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return svhip


@pytest.fixture(scope="module")
def RS(S):
    from svhip import resident
    return resident


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


class Dev:
    """a device allocation holding a copy of a host byte array"""

    def __init__(self, hip, a):
        self.hip, self.p = hip, C.c_void_p()
        a = np.ascontiguousarray(a)
        self.nbytes = a.nbytes
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 16))) == 0
        self.put(a)
        self.addr = self.p.value

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0   # HostToDevice

    def __del__(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = None


def embed(img, pitch, offset, total=None):
    """the bytes of a buffer of 0xAA that holds `img` at `offset`, its rows `pitch` apart"""
    h, w = img.shape
    n = offset + pitch * (h - 1) + w + 32
    buf = np.full(n if total is None else total, 0xAA, np.uint8)
    for v in range(h):
        buf[offset + v * pitch: offset + v * pitch + w] = img[v]
    return buf


def on_device(hip, img, pitch=None, offset=0):
    """(allocation, address of the frame) of `img` at a pitch and a byte offset into a larger buffer of 0xAA"""
    pitch = img.shape[1] if pitch is None else pitch
    d = Dev(hip, embed(img, pitch, offset))
    return d, d.addr + offset


def packed(img):
    """what a view holds: the rows at bpl, zero behind w"""
    return RR.padded(img)[:-1]


# ---------------------------------------------------------------------------------------------- k_pack_rows alone
PACK_SIZES = [(w, h) for w in (1, 15, 16, 17, 31, 32, 33, 255, 256, 257) for h in (1, 2, 5)] + [(4097, 2), (4096, 3)]


@pytest.mark.parametrize("w,h", PACK_SIZES)
def test_pack_rows_every_alignment(RS, hip, w, h):
    rng = np.random.default_rng(1000 * w + h)
    img = rng.integers(1, 256, (h, w)).astype(np.uint8)
    bpl = RS.bpl_of(w)
    want = packed(img)
    assert want.shape == (h, bpl)
    total = 7 + (w + 13) * (h - 1) + w + 32
    d = Dev(hip, np.zeros(total, np.uint8))
    for pitch in (w, w + 1, w + 13):
        for offset in (0, 1, 3, 7):
            d.put(embed(img, pitch, offset, total))
            got = RS.t_pack_rows(d.addr + offset, w, h, pitch, bpl)
            assert np.array_equal(got, want), (pitch, offset, np.argwhere(got != want)[:4])


# ---------------------------------------------------------------------------------------------- Matcher parity
@pytest.fixture(scope="module")
def quad():
    return [H.read_pgm(os.path.join(H.GOLDEN, "viso_%s.pgm" % n)) for n in ("I1p", "I2p", "I1c", "I2c")]


def crop(quad, w, h=230):
    return [np.ascontiguousarray(q[:h, :w]) for q in quad]


def device_push(RS, hip, m, I1, I2, pitch, offset=0, replace=False):
    d1, a1 = on_device(hip, I1, pitch, offset)
    d2, a2 = (None, None) if I2 is None else on_device(hip, I2, pitch, offset + 2)
    RS.matcher_push_back(m, a1, a2, I1.shape[1], I1.shape[0], pitch, replace)
    return d1, d2     # (held by the caller until the call has returned: it has)


def same_matches(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("half,multi", [(1, 1), (0, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("w,extra", [(607, 0), (608, 5), (609, 0), (623, 5), (624, 0), (624, 5)])
def test_matcher_device_push_equals_host_push(S, RS, hip, quad, w, extra, half, multi):
    I1p, I2p, I1c, I2c = crop(quad, w)
    prm = H.matcher_defaults(half_resolution=half, multi_stage=multi)
    a, b = H.ProductMatcher(prm), H.ProductMatcher(prm)
    a.push_back(I1p, I2p)
    a.push_back(I1c, I2c)
    device_push(RS, hip, b, I1p, I2p, w + extra, offset=1)
    device_push(RS, hip, b, I1c, I2c, w + extra, offset=3)
    for view, img in enumerate((I1p, I2p, I1c, I2c)):
        x, y = RS.t_matcher_image(a, view), RS.t_matcher_image(b, view)
        assert x is not None and np.array_equal(x, y), view
        assert np.array_equal(y.reshape(img.shape[0], -1), packed(img)), view
    for tb in range(8):
        x, y = a.features(tb), b.features(tb)
        assert (len(x) > 0 or (not multi and tb % 2 == 0)) and np.array_equal(x, y), H.M_TABLES[tb]   # (even: sparse)
    for which in (0, 1, 4, 5) + ((2, 3) if half else ()):
        (x, dx), (y, dy) = a.filter_image(which), b.filter_image(which)
        assert dx == dy and np.array_equal(x, y), which
    a.match(2)
    b.match(2)
    assert len(a.matches()) > 50 and same_matches(a.matches(), b.matches())
    inl = np.arange(len(a.matches()), dtype=np.int32)
    ga, gb = np.float32(a.gain(inl)), np.float32(b.gain(inl))
    assert ga != 1 and ga.tobytes() == gb.tobytes()


def test_alternating_host_and_device_pushes(S, RS, hip, quad):
    """host, device, device, host on one object = four host pushes: matches and gain after every frame, so getGain
    sees a pair with one, with no and again with one host copy"""
    I1p, I2p, I1c, I2c = crop(quad, 609)
    frames = [(I1p, I2p), (I1c, I2c), (I1p, I2p), (I1c, I2c)]
    prm = H.matcher_defaults()
    a, b = H.ProductMatcher(prm), H.ProductMatcher(prm)
    for k, (l, r) in enumerate(frames):
        a.push_back(l, r)
        if k in (1, 2):
            device_push(RS, hip, b, l, r, 609 + 5, offset=k)
        else:
            b.push_back(l, r)
        if k == 0:
            continue
        a.match(2)
        b.match(2)
        assert len(a.matches()) > 50 and same_matches(a.matches(), b.matches()), k
        inl = np.arange(0, len(a.matches()), 2, dtype=np.int32)
        assert np.float32(a.gain(inl)).tobytes() == np.float32(b.gain(inl)).tobytes(), k


def test_replace_and_single_image(S, RS, hip, quad):
    I1p, I2p, I1c, I2c = crop(quad, 623)
    prm = H.matcher_defaults()
    a, b = H.ProductMatcher(prm), H.ProductMatcher(prm)
    a.push_back(I1p, I2p)
    a.push_back(I1p[::-1].copy(), I2p[::-1].copy())
    a.push_back(I1c, I2c, replace=True)
    device_push(RS, hip, b, I1p, I2p, 623)
    device_push(RS, hip, b, I1p[::-1].copy(), I2p[::-1].copy(), 623)
    device_push(RS, hip, b, I1c, I2c, 623, replace=True)
    a.match(2)
    b.match(2)
    assert len(a.matches()) > 50 and same_matches(a.matches(), b.matches())
    # dI2 = NULL: the single-image variant, flow matching
    a, b = H.ProductMatcher(prm), H.ProductMatcher(prm)
    for l in (I1p, I1c):
        a.push_back(l)
        device_push(RS, hip, b, l, None, 623 + 5, offset=7)
    a.match(0)
    b.match(0)
    assert len(a.matches()) > 50 and same_matches(a.matches(), b.matches())


def test_device_push_while_a_prefetched_frame_is_pending(S, RS, hip, quad):
    I1p, I2p, I1c, I2c = crop(quad, 608)
    m = H.ProductMatcher(H.matcher_defaults())
    m.push_back(I1p, I2p)
    H.product_matcher_prefetch([m], [I1c], [I2c])
    d1, a1 = on_device(hip, I1c)
    d2, a2 = on_device(hip, I2c)
    assert RS.matcher_push_back(m, a1, a2, 608, 230, check=False) == S.ERR_BAD_ARG
    assert "prefetched frame is pending" in S.last_error()
    assert RS.matcher_push_back(m, None, None, 608, 230, check=False) == S.ERR_BAD_ARG
    H.product_matcher_take_prefetched([m], (230, 608))         # the frame is still there and is taken as usual
    ref = H.ProductMatcher(H.matcher_defaults())
    ref.push_back(I1p, I2p)
    ref.push_back(I1c, I2c)
    m.match(2)
    ref.match(2)
    assert same_matches(m.matches(), ref.matches())


# ---------------------------------------------------------------------------------------------- k_gain
@pytest.fixture(scope="module")
def gain_pair(S, RS, hip):
    """the painted pair in two objects: pushed from the host (both paths can run) and pushed from the device"""
    Ip, Ic = RR.painted_pair()
    prm = H.matcher_defaults()
    host, dev = H.ProductMatcher(prm), H.ProductMatcher(prm)
    for I in (Ip, Ic):
        host.push_back(I, I)
        device_push(RS, hip, dev, I, I, RR.GAIN_W + 3, offset=5)
    return Ip, Ic, RR.crafted_matches(), host, dev


def bits(x):
    return np.float32(x).tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 1024, 1025])
def test_gain_paths_agree_on_crafted_matches(RS, gain_pair, n):
    Ip, Ic, m, host, dev = gain_pair
    idx = RR.inlier_list(n, len(m))
    want = RR.gain(Ip, Ic, m, idx)
    g0 = RS.t_matcher_gain(host, m, idx, RS.GAIN_HOST)
    g1 = RS.t_matcher_gain(host, m, idx, RS.GAIN_DEVICE)
    g2 = RS.t_matcher_gain(dev, m, idx, RS.GAIN_DEVICE)
    assert bits(g0) == bits(want) and bits(g1) == bits(want) and bits(g2) == bits(want), (n, want, g0, g1, g2)
    if n >= 63:
        assert want != 1
    # every border case on its own, so that none hides in an average
    if n == 65:
        for k in range(11):
            one = np.array([k], np.int32)
            want = RR.gain(Ip, Ic, m, one)
            assert bits(RS.t_matcher_gain(host, m, one, RS.GAIN_HOST)) == bits(want), k
            assert bits(RS.t_matcher_gain(dev, m, one, RS.GAIN_DEVICE)) == bits(want), k


def test_gain_sum_is_in_inlier_order(RS, gain_pair):
    _, _, _, host, dev = gain_pair
    Ip, Ic, m, idx, r = RR.ordered_sum_case()
    want = np.float32(RR.sequential_sum(r) / np.float32(1025))
    assert bits(want) != bits(np.float32(np.sum(r) / np.float32(1025)))
    assert bits(RS.t_matcher_gain(host, m, idx, RS.GAIN_HOST)) == bits(want)
    assert bits(RS.t_matcher_gain(host, m, idx, RS.GAIN_DEVICE)) == bits(want)
    assert bits(RS.t_matcher_gain(dev, m, idx, RS.GAIN_DEVICE)) == bits(want)


def test_gain_host_path_needs_host_frames(S, RS, gain_pair):
    _, _, m, _, dev = gain_pair
    with pytest.raises(S.SvhError):
        RS.t_matcher_gain(dev, m, np.arange(4, dtype=np.int32), RS.GAIN_HOST)


# ---------------------------------------------------------------------------------------------- VO and mono
def drive(quad):
    """the 4-frame sequence of test_pipeline_gpu.py: the reference's two consecutive quad pairs, twice"""
    return [(quad[0], quad[1]), (quad[2], quad[3]), (quad[0], quad[1]), (quad[2], quad[3])]


def test_vo_process_device(S, RS, hip, quad):
    a, b = H.ProductVo(H.vo_defaults(), private_rand=0), H.ProductVo(H.vo_defaults(), private_rand=0)
    oks = []
    for k, (l, r) in enumerate(drive(quad)):
        h, w = l.shape
        d1, a1 = on_device(hip, l, w + (k % 2) * 3, offset=k)
        d2, a2 = on_device(hip, r, w + (k % 2) * 3, offset=2 * k + 1)
        ra = a.process(l, r)
        rb = RS.vo_process(b, a1, a2, w, h, w + (k % 2) * 3)
        assert ra == rb, k
        oks.append(ra)
        assert a.motion().tobytes() == b.motion().tobytes(), k
        assert np.array_equal(a.inliers(), b.inliers()) and same_matches(a.matches(), b.matches()), k
        if ra == 1:
            assert len(a.inliers()) > 20
            assert bits(a.gain(a.inliers())) == bits(b.gain(b.inliers())), k
    assert oks[0] == 0 and 1 in oks[1:]


def test_vo_mono_process_device(S, RS, hip):
    a, b = S.VoMono(private_rand=0), S.VoMono(private_rand=0)
    oks = []
    for k, I in enumerate(H.mono_frames()):
        h, w = I.shape
        d, addr = on_device(hip, I, w + 1, offset=3)
        ra = a.process(I)
        rb = bool(RS.vo_mono_process(b, addr, w, h, w + 1))
        assert ra == rb, k
        oks.append(ra)
        assert a.motion().tobytes() == b.motion().tobytes(), k
        assert np.array_equal(a.inliers(), b.inliers()) and same_matches(a.matches(), b.matches()), k
    assert any(oks)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- map fusion
@pytest.mark.parametrize("w,h,step", [(1, 1, 1), (5, 3, 8), (64, 4, 64), (65, 5, 80)])
def test_map_add_device(S, RS, hip, w, h, step):
    from svhip import mapper
    rng = np.random.default_rng(w * 100 + h)
    a, b = mapper.Mapper(645.24, 635.96, 194.13, 0.5707), mapper.Mapper(645.24, 635.96, 194.13, 0.5707)
    Ht = np.eye(4)
    for frame in range(2):
        D1 = rng.uniform(-5, 60, (h, w)).astype(np.float32)
        buf = rng.integers(0, 256, (h, step)).astype(np.uint8)
        I1 = buf[:, :w]
        gain = (0.0, 1.25)[frame]
        a.add(D1, I1, Ht, gain)
        dD = Dev(hip, D1)
        dI, addr = on_device(hip, np.ascontiguousarray(I1), step, offset=1 + frame)
        RS.map_add(b, dD.addr, addr, w, h, Ht, gain, pitch=step)
        for which in (0, 1):
            x, y = a.points(which), b.points(which)
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (frame, which)
        assert a.planes().tobytes() == b.planes().tobytes(), frame
        Ht = Ht.copy()
        Ht[2, 3] += 0.4
        Ht[0, 3] -= 0.05


# ---------------------------------------------------------------------------------------------- end to end
def run_pipeline(p, frames):
    """per frame: ok, pose, both point lists; the rendered view at the end"""
    p.vo.lib.svh_vo_set_private_rand.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
    p.vo.lib.svh_vo_set_private_rand(p.vo.h, 1, 0)       # the two pipelines do not share libc's rand()
    out = []
    for l, r in frames:
        ok, n0, n1 = p.push(l, r)
        out.append((ok, n0, n1, p.poses[-1].tobytes(), p.map.points(0).tobytes(), p.map.points(1).tobytes()))
    return out, p.view.render().tobytes()


def same_runs(a, b):
    (fa, va), (fb, vb) = a, b
    assert len(fa) == len(fb)
    for k, (x, y) in enumerate(zip(fa, fb)):
        assert x[:3] == y[:3], (k, x[:3], y[:3])
        assert x[3] == y[3] and x[4] == y[4] and x[5] == y[5], k
    assert va == vb


def test_pipeline_resident_equals_host_hop(S, quad):
    import stereomapper_pipeline as SP
    f, cu, cv, base = 645.24, 635.96, 194.13, 0.5707
    a = run_pipeline(SP.Pipeline(f, cu, cv, base), drive(quad))
    b = run_pipeline(SP.Pipeline(f, cu, cv, base, resident=True), drive(quad))
    same_runs(a, b)
    assert a[0][0][0] is False and any(x[0] for x in a[0][1:]) and a[0][-1][2] > 20000


def test_pipeline_resident_unrectified(S, quad):
    """raw frames of the rig's size (the reference pairs inside a 1392 x 512 frame), rectified on the device with the
    rig calibration of tests/golden/rectify.npz -- the size tests/test_rectify_gpu.py runs at full size"""
    import rectify_ref as R
    import stereomapper_pipeline as SP
    from svhip import rectify
    raw = []
    for l, r in drive(quad):
        pair = []
        for c, img in enumerate((l, r)):
            fr = R.source(*R.RIG_SRC, seed=c) // 8                  # a dim texture around the pair
            fr[60:60 + img.shape[0], 24:24 + img.shape[1]] = img
            pair.append(np.ascontiguousarray(fr, np.uint8))
        raw.append(tuple(pair))
    f, cu, cv, base = 645.24, 635.96, 194.13, 0.5707
    prm = lambda: rectify.params(R.RIG_SRC, R.RIG_DST, R.RIG)
    a = run_pipeline(SP.Pipeline(f, cu, cv, base, rectify_params=prm()), raw)
    b = run_pipeline(SP.Pipeline(f, cu, cv, base, rectify_params=prm(), resident=True), raw)
    same_runs(a, b)
    assert a[0][-1][2] > 0 and any(x[0] for x in a[0])

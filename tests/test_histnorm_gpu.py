"""GPU: k_hist_count, k_hist_table and k_hist_apply (stereo-vision_amd/csrc/histnorm_kernels.hip) behind
include/svh_histnorm.h against the numpy restatement tests/histnorm_ref.py and the reference's recorded output
tests/golden/histnorm.npz (see tests/test_histnorm.py for what pins the arithmetic itself).  Every comparison is
bit-exact: the counts are integers, the table is the restatement's IEEE operations in its order.

The shapes are the edges of the kernels' tiling: a lane takes one 16-byte-aligned window of a row, so widths around 16,
64 (a wave's 4 words), 256 and rows 3 bytes longer than the image from a base one byte off a word make heads and tails of
every length occur; what lies between the rows and around the images is painted and must stay."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import histnorm_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1242]
HEIGHTS = [1, 4, 5, 375]
PAINT = 0xEE


@pytest.fixture(scope="module")
def Z():
    return R.load_golden()


@pytest.fixture(scope="module")
def HN():
    import svhip
    from svhip import histnorm
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    return histnorm


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(autouse=True)
def disarm(HN):
    yield
    HN.lib().svh_test_fail_at(None)


class Dev:
    """device memory through the HIP runtime the library links: a copy of a host array"""

    def __init__(self, hip, a):
        self.hip, self.p = hip, C.c_void_p()
        a = np.ascontiguousarray(a)
        self.nbytes = a.nbytes
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 16))) == 0
        self.addr = self.p.value
        self.put(a)

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.nbytes
        assert self.hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0   # HostToDevice

    def get(self):
        out = np.zeros(self.nbytes, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(self.nbytes), 2) == 0
        return out

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = None


def layout(imgs, pitch, image_stride, lead):
    """the images in one painted buffer: image k at lead + k * image_stride, rows `pitch` apart; and the mask of the
    bytes that are pixels"""
    h, w = imgs[0].shape
    total = lead + (len(imgs) - 1) * image_stride + (h - 1) * pitch + w + 5
    buf = np.full(total, PAINT, np.uint8)
    mask = np.zeros(total, bool)
    for k, img in enumerate(imgs):
        for v in range(h):
            at = lead + k * image_stride + v * pitch
            buf[at:at + w] = img[v]
            mask[at:at + w] = True
    return buf, mask


def take(buf, k, shape, pitch, image_stride, lead):
    h, w = shape
    at = lead + k * image_stride
    return np.stack([buf[at + v * pitch:at + v * pitch + w] for v in range(h)])


def check_images(HN, hip, imgs, pitch, image_stride, lead, where, obj=None):
    """svh_histnorm_images_device over imgs == the restatement: images, painted bytes, counts, cdf, map"""
    h, w = imgs[0].shape
    buf, mask = layout(imgs, pitch, image_stride, lead)
    o = obj or HN.HistNorm(w, h)
    d = Dev(hip, buf)
    try:
        o.images_device(len(imgs), d.addr + lead, pitch, image_stride)
        got = d.get()
        counts, cdf, m = o.tables()
    finally:
        d.free()
        if obj is None:
            o.close()
    assert (got[~mask] == PAINT).all(), (where, "a byte outside the rows changed", np.flatnonzero((got != PAINT) & ~mask)[:5])
    assert counts.shape == (len(imgs), 256)
    for k, img in enumerate(imgs):
        want, wc, wcdf, wm = R.normalize(img)
        assert np.array_equal(counts[k], wc), (where, k, "counts", np.flatnonzero(counts[k] != wc)[:5])
        assert R.same_bits(cdf[k], wcdf), (where, k, "cdf")
        assert R.same_bits(m[k], wm), (where, k, "map")
        assert R.same_bits(take(got, k, img.shape, pitch, image_stride, lead), want), (where, k, "image")
    return m


@pytest.mark.parametrize("h", HEIGHTS)
def test_shapes_pitches_and_alignments(HN, hip, h):
    """two images with different histograms per shape; packed rows and rows 3 bytes longer, from a base 1 byte off"""
    for w in WIDTHS:
        imgs = [R.pattern(w, h, 1), (R.pattern(w, h, 5) // 2 + 3).astype(np.uint8)]
        for pitch in (w, w + 3):
            span = (h - 1) * pitch + w
            check_images(HN, hip, imgs, pitch, span + 7, 1, (w, h, pitch))


@pytest.mark.parametrize("n", [1, 2, 33])
def test_n_images_each_with_its_own_table(HN, hip, n):
    """one launch per kernel over n images whose histograms all differ: a job-index mix-up shows in counts and images"""
    w, h = 65, 5
    imgs = [((R.pattern(w, h, k + 1).astype(np.int64) * (k + 3)) // (k + 4) + k).astype(np.uint8) for k in range(n)]
    assert len({R.counts_of(i).tobytes() for i in imgs}) == n
    m = check_images(HN, hip, imgs, w + 3, h * (w + 3) + 11, 3, n)
    assert len({x.tobytes() for x in m}) == n


def test_reference_fixture_on_the_device(HN, hip, Z):
    """every case of the fixture but the largest: the reference's map and image; the flat 1392x512 frame wraps to 1, the
    flat 1242x375 one gives 254, the two-level one 84 and 255"""
    for name, img, step, keep in R.cases():
        if img.size > 1 << 22:
            continue
        h, w = img.shape
        o = HN.HistNorm(w, h)
        buf, mask = layout([img], step, 0, 0)
        d = Dev(hip, buf)
        try:
            o.apply_raw(d.addr, True, step)
            got = d.get()
            counts, cdf, m = o.tables()
        finally:
            d.free()
            o.close()
        out = take(got, 0, img.shape, step, 0, 0)
        assert (got[~mask] == PAINT).all(), name
        assert R.same_bits(m[0], Z[name + "_map"]), name
        assert R.same_bits(out, Z[name + "_img"]) if keep else R.same_bits(R.sha(out), Z[name + "_sha"]), name
        assert np.array_equal(counts[0], R.counts_of(img)), name
        if name == "flat_1392x512":
            assert (out == 1).all()
        if name == "flat_1242x375":
            assert (out == 254).all()
        if name == "two_1392x512":
            assert sorted(np.unique(out)) == [84, 255]
        if name.startswith("ramp"):
            assert (counts[0] > 0).all()


def test_counts_on_segment_boundaries(HN, hip):
    """1242x375 images whose counts sit one below, at and one above the points where the chain's step changes"""
    w, h = 1242, 375
    N = w * h
    vecs = [R.boundary_counts(w, h), R.boundary_counts(w, h, 1, 2), R.boundary_counts(w, h, 6, 1)]
    for b in R.breakpoints(w, h)[-3:]:                                 # the last ones are too large to share an image
        for d in (-1, 0, 1):
            vecs.append(R.split_counts(w, h, int(b) + d))
    n0, _, _ = HN.segments(w, h)
    assert set(int(b) for b in R.breakpoints(w, h)) <= set(int(k) for k in n0)   # the table breaks where the chain does
    imgs = [R.from_counts(c, w, h) for c in vecs]
    check_images(HN, hip, imgs, w, N + 13, 0, "boundaries")


def test_one_4097x4096_image(HN, hip, Z):
    """N > 2^24: (float)N rounds, the chain stands still, the counts pass 2^23, and the workgroups stride"""
    img = R.pattern(4097, 4096)
    o = HN.HistNorm(4097, 4096)
    d = Dev(hip, img)
    try:
        o.apply_raw(d.addr, True, 4097)
        out = d.get().reshape(img.shape)
        counts, cdf, m = o.tables()
    finally:
        d.free()
        o.close()
    wc = R.counts_of(img)
    wcdf, wm = R.table(wc, 4097, 4096)
    assert np.array_equal(counts[0], wc) and R.same_bits(cdf[0], wcdf) and R.same_bits(m[0], wm)
    assert R.same_bits(m[0], Z["pattern_4097x4096_map"])
    assert R.same_bits(R.sha(out), Z["pattern_4097x4096_sha"])


def test_host_and_device_forms_and_pairs(HN, hip):
    """apply on a host image (numpy view with longer rows) == apply on device memory; the pairs entry == two calls of
    the images entry"""
    w, h, pitch = 257, 5, 260
    n = 3
    left = [R.pattern(w, h, k + 1) for k in range(n)]
    right = [(R.pattern(w, h, k + 7) // 3 + 40).astype(np.uint8) for k in range(n)]
    o = HN.HistNorm(w, h)
    stride = h * pitch + 9
    bl, ml = layout(left, pitch, stride, 1)
    br, mr = layout(right, pitch, stride, 2)
    dl, dr = Dev(hip, bl), Dev(hip, br)
    try:
        o.pairs_device(n, dl.addr + 1, dr.addr + 2, pitch, stride)
        pl, pr = dl.get(), dr.get()
        counts, cdf, m = o.tables()
        assert counts.shape == (2 * n, 256)
        dl.put(bl), dr.put(br)
        o.images_device(n, dl.addr + 1, pitch, stride)
        tl = o.tables()
        o.images_device(n, dr.addr + 2, pitch, stride)
        tr = o.tables()
        assert R.same_bits(pl, dl.get()) and R.same_bits(pr, dr.get())
        assert (pl[~ml] == PAINT).all() and (pr[~mr] == PAINT).all()
        for k in range(n):                                             # order of the tap: left 0, right 0, left 1, ...
            for a, b in zip((counts, cdf, m), tl):
                assert R.same_bits(a[2 * k], b[k])
            for a, b in zip((counts, cdf, m), tr):
                assert R.same_bits(a[2 * k + 1], b[k])
            assert R.same_bits(take(pl, k, (h, w), pitch, stride, 1), R.normalize(left[k])[0])
            assert R.same_bits(take(pr, k, (h, w), pitch, stride, 2), R.normalize(right[k])[0])
        # host form: a view with longer rows, padding painted
        host = np.full((h, pitch), 0x5A, np.uint8)
        host[:, :w] = left[0]
        o.apply(host[:, :w])
        assert R.same_bits(host[:, :w], take(pl, 0, (h, w), pitch, stride, 1)) and (host[:, w:] == 0x5A).all()
        assert o.release() > 0 and o.tables()[0].shape == (0, 256)     # ... and the object builds its buffers again
        host[:, :w] = left[1]
        o.apply(host[:, :w])
        assert R.same_bits(host[:, :w], take(pl, 1, (h, w), pitch, stride, 1))
    finally:
        dl.free()
        dr.free()
        o.close()


# what a fresh object's first call issues, in order.  Device image: 3 allocations (segment table, its pinned copy, the
# tables), copy 1 = the segment table's upload, copy 2 = the clearing of the counters, launches 1..3 = k_hist_count,
# k_hist_table, k_hist_apply, wait 1.  Host image: allocations 4 and 5 (staging), copy 2 = the image's upload, copy 3 =
# the clearing, the three launches, copy 4 = the copy-back, wait 1.
@pytest.mark.parametrize("spec,where", [("malloc:1", "device"), ("malloc:2", "device"), ("malloc:3", "device"),
                                        ("copy:1", "device"), ("copy:2", "device"), ("launch:1", "device"),
                                        ("launch:2", "device"), ("launch:3", "device"), ("wait:1", "device"),
                                        ("malloc:4", "host"), ("malloc:5", "host"), ("copy:2", "host"),
                                        ("copy:3", "host"), ("launch:3", "host"), ("copy:4", "host"), ("wait:1", "host")])
def test_simulated_hip_error_leaves_image_and_object(HN, hip, spec, where, capfd):
    """svh_test_fail_at makes the n-th guarded HIP call of a kind report an error without being issued (no GPU fault is
    involved): the entry returns SVH_ERR_HIP and names the call; a host image is untouched after any failure, a device
    image after any failure up to the launch check of k_hist_apply; the next call on the same object is right"""
    import svhip as S
    w, h, pitch = 65, 9, 68
    img = R.pattern(w, h)
    want = R.normalize(img)[0]
    buf, mask = layout([img], pitch, 0, 0)
    host = buf.copy()
    o = HN.HistNorm(w, h)
    d = Dev(hip, buf)
    try:
        def call():
            if where == "host":
                return S.lib().svh_histnorm_apply(o._h, host.ctypes.data, 0, pitch)
            return S.lib().svh_histnorm_apply(o._h, d.addr, 1, pitch)

        assert S.lib().svh_test_fail_at(spec.encode()) == 0
        assert call() == S.ERR_HIP
        assert "injected failure" in S.last_error()
        S.lib().svh_test_fail_at(None)
        assert "svhip: HistNorm" in capfd.readouterr().err
        assert R.same_bits(host, buf), "the host image changed"
        if spec != "wait:1":
            assert R.same_bits(d.get(), buf), "the device image changed"
        assert o.tables()[0].shape == (0, 256)                         # no tables of a failed call
        d.put(buf)
        assert call() == 0
        got = host if where == "host" else d.get()
        assert R.same_bits(take(got, 0, (h, w), pitch, 0, 0), want) and (got[~mask] == PAINT).all()
        assert R.same_bits(o.tables()[2][0], R.normalize(img)[3])
    finally:
        d.free()
        o.close()


def test_failure_in_pairs_and_in_the_tap_then_timing(HN, hip, capfd):
    import svhip as S
    w, h = 65, 9
    img = R.pattern(w, h)
    want, _, _, wm = R.normalize(img)
    o = HN.HistNorm(w, h)
    o.set_timing(True)
    d = [Dev(hip, img), Dev(hip, img)]
    try:
        for spec in ("malloc:1", "launch:1", "launch:3"):
            S.lib().svh_test_fail_at(spec.encode())
            with pytest.raises(S.SvhError) as e:
                o.pairs_device(1, d[0].addr, d[1].addr, w, 0)
            assert e.value.code == S.ERR_HIP
            S.lib().svh_test_fail_at(None)
            assert R.same_bits(d[0].get().reshape(h, w), img) and R.same_bits(d[1].get().reshape(h, w), img), spec
        o.pairs_device(1, d[0].addr, d[1].addr, w, 0)
        ms = o.timing()
        assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0 and ms[0] >= ms[1]
        for k in range(2):
            assert R.same_bits(d[k].get().reshape(h, w), want)
        S.lib().svh_test_fail_at(b"copy:1")                            # the tap's download
        with pytest.raises(S.SvhError):
            o.tables()
        S.lib().svh_test_fail_at(None)
        capfd.readouterr()
        assert R.same_bits(o.tables()[2], np.stack([wm, wm]))
    finally:
        for x in d:
            x.free()
        o.close()


def test_stereoimage_dropin_on_the_device(tmp_path):
    """include/stereoimage.h: the reference's call on a flat 1392x512 host frame gives 1 everywhere"""
    exe = str(tmp_path / "stereoimage_dropin")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-I" + os.path.join(H.ROOT, "include"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "histnorm", "stereoimage_dropin.cpp"), "-L" + H.PKG, "-lsvhip",
                           "-Wl,-rpath," + H.PKG])
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout and "status 0" in r.stdout, r.stdout + r.stderr

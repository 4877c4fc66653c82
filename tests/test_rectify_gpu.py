"""GPU: k_rect_maps and k_rect_remap (stereo-vision_amd/csrc/rectify_kernels.hip) behind include/svh_rectify.h against
tests/golden/rectify.npz and the numpy restatement tests/rectify_ref.py (which produced the fixture; see
tests/test_rectify.py for what pins the arithmetic itself).  Every comparison is bit-exact: the kernels perform the
restatement's IEEE operations in its order, the remap is integer arithmetic.

The shapes are the edges of the remap kernel's tiling: a wave covers 256 destination columns less the row's
misalignment (a lane writes one 4-byte-aligned word), a workgroup four rows; rows 3 bytes longer than the image make
every alignment occur."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import rectify_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Z():
    return R.load_golden()


@pytest.fixture(scope="module")
def SR():
    import svhip
    from svhip import rectify
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    return rectify


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(autouse=True)
def disarm(SR):
    yield
    SR.lib().svh_test_fail_at(None)


class Dev:
    """device memory through the HIP runtime the library links: a copy of a host array, or `a` bytes of 0xEE"""

    def __init__(self, hip, a):
        self.hip, self.p = hip, C.c_void_p()
        if isinstance(a, int):
            a = np.full(a, 0xEE, np.uint8)
        a = np.ascontiguousarray(a)
        self.nbytes = a.nbytes
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 16))) == 0
        assert hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0   # HostToDevice
        self.addr = self.p.value

    def get(self):
        out = np.zeros(self.nbytes, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(self.nbytes), 2) == 0
        return out

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = None


def strided(a, stride, fill=0x5A):
    """[h, w] -> a [h, stride] buffer holding it, and the [h, w] view into it"""
    h, w = a.shape
    buf = np.full((h, stride), fill, np.uint8)
    buf[:, :w] = a
    return buf, buf[:, :w]


def all_cases(Z):
    out = [(n, cam, Z["hand_src"], R.HAND_W, R.HAND_H) for n, cam in R.hand_cases()]
    return out + [(n, cam, Z[n + "_src"], dw, dh) for n, (cam, sw, sh, dw, dh) in R.shape_cases()]


def test_maps_equal_fixture(SR, Z):
    """k_rect_maps through svh_rectify_get_maps: every hand-derived case, every shape, both camera slots"""
    for name, cam, S, dw, dh in all_cases(Z):
        r = SR.Rectifier(SR.params(S.shape[::-1], (dw, dh), [R.camera(), cam]))
        mx, my = r.maps(1)
        assert R.same_bits(mx, Z[name + "_mx"]) and R.same_bits(my, Z[name + "_my"]), name
        if name == "identity":
            ix, iy = r.maps(0)
            assert R.same_bits(ix, mx) and R.same_bits(iy, my)
        r.close()


@pytest.fixture(scope="module")
def rig(SR):
    r = SR.Rectifier(SR.params(R.RIG_SRC, R.RIG_DST, R.RIG))
    yield r
    r.close()


def test_rig_maps_full_size_and_window(SR, Z, rig):
    for c, cam in enumerate(R.RIG):
        mx, my = rig.maps(c)
        assert R.same_bits(R.window(mx), Z["rig%d_mx" % c]) and R.same_bits(R.window(my), Z["rig%d_my" % c])
        u, v = R.maps(cam, *R.RIG_DST)                          # the full size, once
        assert R.same_bits(mx, u) and R.same_bits(my, v), c


@pytest.mark.parametrize("border", [R.WRAP, R.ZERO])
def test_remap_shapes_strides_and_borders(SR, Z, hip, border):
    """host to host with packed rows, and device to device with rows 3 bytes longer from a base 1 byte off a word, so
    heads and tails of every length occur; what lies between the rows must stay"""
    for name, cam, S, dw, dh in all_cases(Z):
        sh, sw = S.shape
        want = Z["%s_out%d" % (name, border)]
        r = SR.Rectifier(SR.params((sw, sh), (dw, dh), [cam], border))
        assert R.same_bits(r.remap(0, S), want), (name, "host")
        sbuf, _ = strided(S, sw + 3)
        dS, dD = Dev(hip, sbuf), Dev(hip, 1 + dh * (dw + 3))
        try:
            r.remap_raw(0, dS.addr, 1, sw + 3, dD.addr + 1, 1, dw + 3)
            got = dD.get()
            rows = got[1:].reshape(dh, dw + 3)
            assert R.same_bits(rows[:, :dw], want), (name, "device")
            assert got[0] == 0xEE and (rows[:, dw:] == 0xEE).all(), (name, "bytes between the rows")
        finally:
            dS.free()
            dD.free()
            r.close()


def test_mixed_data_paths(SR, Z, hip):
    name, (cam, sw, sh, dw, dh) = [c for c in R.shape_cases() if c[0] == "shape_257x17_s"][0]
    S, want = Z[name + "_src"], Z[name + "_out0"]
    r = SR.Rectifier(SR.params((sw, sh), (dw, dh), [cam]))
    dS, dD = Dev(hip, S), Dev(hip, dw * dh)
    try:
        # device source, host destination with longer rows: the padding of the host image stays
        buf, view = strided(np.zeros((dh, dw), np.uint8), dw + 3)
        r.remap_raw(0, dS.addr, 1, sw, buf.ctypes.data, 0, dw + 3)
        assert R.same_bits(view, want) and (buf[:, dw:] == 0x5A).all()
        # host source with longer rows, device destination
        sbuf, sview = strided(S, sw + 3)
        r.remap_raw(0, sbuf.ctypes.data, 0, sw + 3, dD.addr, 1, dw)
        assert R.same_bits(dD.get().reshape(dh, dw), want)
        # the numpy-level call with a strided source view
        assert R.same_bits(r.remap(0, sview), want)
        assert r.release() > 0                                  # ... and the object builds its maps again
        assert R.same_bits(r.remap(0, S), want)
    finally:
        dS.free()
        dD.free()
        r.close()


@pytest.mark.parametrize("n", [1, 3, 5])
def test_pairs_device_equals_single_calls(SR, Z, hip, n):
    """one launch over 2 n images with different maps for the two cameras == 2 n single calls"""
    (_, (cam_a, sw, sh, dw, dh)), = [c for c in R.shape_cases() if c[0] == "shape_257x17_l"]
    cam_b = R.generic_camera(sw, sh, dw, dh, zoom=0.7, off=(1.5, -0.75))
    for border in (R.WRAP, R.ZERO):
        r = SR.Rectifier(SR.params((sw, sh), (dw, dh), [cam_a, cam_b], border))
        srs, drs = sw + 3, dw + 3
        sis, dis = sh * srs + 5, dh * drs + 7                  # image strides that are no multiple of anything
        raw = [np.stack([strided(R.source(sw, sh, seed=10 * c + k), srs)[0] for k in range(n)]) for c in range(2)]
        src = []
        for c in range(2):
            flat = np.zeros(n * sis, np.uint8)
            for k in range(n):
                flat[k * sis:k * sis + sh * srs] = raw[c][k].ravel()
            src.append(Dev(hip, flat))
        dst = [Dev(hip, n * dis), Dev(hip, n * dis)]
        try:
            r.pairs_device(n, src[0].addr, src[1].addr, srs, sis, dst[0].addr, dst[1].addr, drs, dis)
            maps = [r.maps(c) for c in range(2)]
            assert not R.same_bits(maps[0][0], maps[1][0])
            for c in range(2):
                got = dst[c].get()
                for k in range(n):
                    single = r.remap(c, raw[c][k][:, :sw])
                    assert R.same_bits(single, R.remap(raw[c][k][:, :sw], maps[c][0], maps[c][1], border))
                    img = got[k * dis:k * dis + dh * drs].reshape(dh, drs)
                    assert R.same_bits(img[:, :dw], single), (n, c, k, border)
                    assert (img[:, dw:] == 0xEE).all() and (got[k * dis + dh * drs:(k + 1) * dis] == 0xEE).all()
        finally:
            for d in src + dst:
                d.free()
            r.close()


def test_rig_remap_full_size(SR, Z, rig):
    """1392x512 -> 1242x375 (tightly packed rows of 1242 bytes: every alignment), both cameras"""
    for c in range(2):
        mx, my = rig.maps(c)
        S = R.source(*R.RIG_SRC, seed=c)
        out = rig.remap(c, S)
        assert R.same_bits(out, R.remap(S, mx, my, R.WRAP)), c
        assert R.same_bits(R.window(out), Z["rig%d_out0" % c])


def test_hand_over_to_elas_on_the_device(SR, hip):
    """the urban1 golden pair embedded at an integer offset in zeroed 1392x512 frames, a pure-translation calibration,
    svh_rectify_pairs_device straight into svh_elas_process_batch_device with no host copy: D1 and D2 of the fixture"""
    import svhip as S
    with np.load(os.path.join(H.GOLDEN, "urban1_robotics.npz")) as z:
        prm = H.ElasParams.from_buffer_copy(z["params"].tobytes())
        l, rgt = H.golden_pair(str(z["crop"]))
        want = z["d1"], z["d2"]
    h, w = l.shape
    ox, oy = 75, 68
    frames = []
    for img in (l, rgt):
        f = np.zeros((R.RIG_SRC[1], R.RIG_SRC[0]), np.uint8)
        f[oy:oy + h, ox:ox + w] = img
        frames.append(f)
    cam = R.shifted(-float(ox), -float(oy))                    # map = (j + ox, i + oy)
    r = SR.Rectifier(SR.params(R.RIG_SRC, (w, h), [cam, cam], R.ZERO))
    dS = [Dev(hip, f) for f in frames]
    dI = [Dev(hip, w * h), Dev(hip, w * h)]
    dD = [Dev(hip, np.zeros(w * h, np.float32)), Dev(hip, np.zeros(w * h, np.float32))]
    try:
        r.pairs_device(1, dS[0].addr, dS[1].addr, R.RIG_SRC[0], frames[0].size, dI[0].addr, dI[1].addr, w, w * h)
        st = S.Elas(prm).process_batch_device(1, dI[0].addr, dI[1].addr, w * h, dD[0].addr, dD[1].addr, 4 * w * h, w, h, w)
        assert st == [0]
        assert R.same_bits(dI[0].get().reshape(h, w), l) and R.same_bits(dI[1].get().reshape(h, w), rgt)
        for k in range(2):
            assert R.same_bits(dD[k].get().view(np.float32), want[k]), k
    finally:
        for d in dS + dI + dD:
            d.free()
        r.close()


# what a fresh object's first call issues, in order: 2 allocations (maps, table), one launch per camera (k_rect_maps),
# then per call: 4 allocations and the upload for host images, the remap launch, the copy-back, the wait
@pytest.mark.parametrize("spec,where", [("malloc:1", "host"), ("malloc:2", "device"), ("malloc:4", "host"),
                                        ("copy:1", "host"), ("copy:2", "host"), ("launch:1", "device"),
                                        ("launch:2", "device"), ("launch:2", "host"), ("wait:1", "host")])
def test_simulated_hip_error_leaves_destination_and_object(SR, Z, hip, spec, where, capfd):
    """svh_test_fail_at makes the n-th guarded HIP call of a kind report an error without being issued (no GPU fault is
    involved): the entry returns SVH_ERR_HIP, the destination bytes are unchanged, and the next call on the same object
    gives the right result"""
    import svhip as S
    name, (cam, sw, sh, dw, dh) = [c for c in R.shape_cases() if c[0] == "shape_65x9_l"][0]
    src, want = Z[name + "_src"], Z[name + "_out1"]
    r = SR.Rectifier(SR.params((sw, sh), (dw, dh), [cam], R.ZERO))
    dS, dD = Dev(hip, src), Dev(hip, dw * dh)
    host = np.full((dh, dw), 0xEE, np.uint8)
    try:
        def call():
            if where == "host":
                return S.lib().svh_rectify_remap(r._h, 0, src.ctypes.data, 0, sw, host.ctypes.data, 0, dw)
            return S.lib().svh_rectify_remap(r._h, 0, dS.addr, 1, sw, dD.addr, 1, dw)

        assert S.lib().svh_test_fail_at(spec.encode()) == 0
        assert call() == S.ERR_HIP
        assert "injected failure" in S.last_error()
        S.lib().svh_test_fail_at(None)
        assert "svhip: Rectify" in capfd.readouterr().err
        assert (host == 0xEE).all() and (dD.get() == 0xEE).all(), "the destination changed"
        assert call() == 0
        got = host if where == "host" else dD.get().reshape(dh, dw)
        assert R.same_bits(got, want)
        mx, my = r.maps(0)
        assert R.same_bits(mx, Z[name + "_mx"]) and R.same_bits(my, Z[name + "_my"])
    finally:
        dS.free()
        dD.free()
        r.close()


def test_simulated_hip_error_in_pairs_device_and_timing(SR, Z, hip, capfd):
    import svhip as S
    name, (cam, sw, sh, dw, dh) = [c for c in R.shape_cases() if c[0] == "shape_65x9_l"][0]
    src, want = Z[name + "_src"], Z[name + "_out0"]
    r = SR.Rectifier(SR.params((sw, sh), (dw, dh), [cam, cam]))
    r.set_timing(True)
    dS, dD = Dev(hip, src), [Dev(hip, dw * dh), Dev(hip, dw * dh)]
    try:
        for spec in ("malloc:1", "launch:2", "launch:3"):
            S.lib().svh_test_fail_at(spec.encode())
            with pytest.raises(S.SvhError) as e:
                r.pairs_device(1, dS.addr, dS.addr, sw, sw * sh, dD[0].addr, dD[1].addr, dw, dw * dh)
            assert e.value.code == S.ERR_HIP
            S.lib().svh_test_fail_at(None)
            assert (dD[0].get() == 0xEE).all() and (dD[1].get() == 0xEE).all(), spec
        capfd.readouterr()
        r.pairs_device(1, dS.addr, dS.addr, sw, sw * sh, dD[0].addr, dD[1].addr, dw, dw * dh)
        ms = r.timing()
        assert ms[0] > 0 and ms[1] > 0                          # this call built the maps
        r.pairs_device(1, dS.addr, dS.addr, sw, sw * sh, dD[0].addr, dD[1].addr, dw, dw * dh)
        ms = r.timing()
        assert ms[0] > 0 and ms[1] == 0
        for k in range(2):
            assert R.same_bits(dD[k].get().reshape(dh, dw), want)
    finally:
        dS.free()
        for d in dD:
            d.free()
        r.close()

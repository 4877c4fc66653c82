"""GPU: 16-bit KITTI disparity outputs and left-only results for host callers (svh_elas_*_out, svh_disparity_pack_u16;
include/svh.h).  The expected value everywhere is THE EXISTING FLOAT PATH'S MAPS passed through the numpy restatement of
the encoding (tests/disp_u16_ref.py: 0 when !(d >= 0), else clip(floor(d * 256), 1, 65535)); every comparison is
np.array_equal, no tolerance.  The float maps underneath are the ones the rest of the suite holds bit-exact against the
reference; the encoding itself is the development kit's as documented, unverified against the kit's own code.

Parity alone cannot show the point of the feature -- a library that copied floats down and converted on the host would
pass it -- so the bytes the engine copies down are counted (svh_test_d2h_map_bytes) and must be exactly the model's."""
import ctypes as C

import numpy as np
import pytest

import disp_u16_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

SENTINEL = 0xBEEF


@pytest.fixture(scope="module")
def svhip():
    import svhip as S
    S.lib()
    assert S.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return S


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def d2h_bytes(S, reset=False):
    out = (C.c_int64 * 2)()
    S.lib().svh_test_d2h_map_bytes(out, 1 if reset else 0)
    return out[0], out[1]


# ---------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 70977])
def test_pack_kernel_every_alignment(n, svhip, hip):
    """svh_disparity_pack_u16 with both sides on the device: source 0-3 floats and destination 0-7 elements off a
    16-byte boundary (hipMalloc aligns far beyond that), lengths around the 8-pixel vector and the 2048-pixel block and
    one odd map size (401 x 177); guard elements in front of and behind the destination keep their sentinel"""
    L = svhip.lib()
    d = R.content(n, seed=n)
    want = R.pack(d)
    G = 16                                               # guard elements on either side
    dsrc, ddst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dsrc), C.c_size_t(4 * (n + 4))) == 0
    assert hip.hipMalloc(C.byref(ddst), C.c_size_t(2 * (n + 2 * G + 8))) == 0
    assert dsrc.value % 16 == 0 and ddst.value % 16 == 0
    try:
        for so in range(4):
            assert hip.hipMemcpy(C.c_void_p(dsrc.value + 4 * so), C.c_void_p(d.ctypes.data), C.c_size_t(d.nbytes), 1) == 0
            for do in range(8):
                buf = np.full(n + 2 * G + 8, SENTINEL, np.uint16)
                assert hip.hipMemcpy(ddst, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes), 1) == 0
                rc = L.svh_disparity_pack_u16(C.c_void_p(dsrc.value + 4 * so), 1, n,
                                              C.c_void_p(ddst.value + 2 * (G + do)), 1)
                assert rc == 0, svhip.last_error()
                assert hip.hipMemcpy(C.c_void_p(buf.ctypes.data), ddst, C.c_size_t(buf.nbytes), 2) == 0
                assert np.array_equal(buf[G + do:G + do + n], want), (so, do)
                assert np.all(buf[:G + do] == SENTINEL) and np.all(buf[G + do + n:] == SENTINEL), (so, do)
        # n = 0 writes nothing
        buf = np.full(n + 2 * G + 8, SENTINEL, np.uint16)
        assert hip.hipMemcpy(ddst, C.c_void_p(buf.ctypes.data), C.c_size_t(buf.nbytes), 1) == 0
        assert L.svh_disparity_pack_u16(dsrc, 1, 0, C.c_void_p(ddst.value + 2 * G), 1) == 0
        assert hip.hipMemcpy(C.c_void_p(buf.ctypes.data), ddst, C.c_size_t(buf.nbytes), 2) == 0
        assert np.all(buf == SENTINEL)
    finally:
        hip.hipFree(dsrc)
        hip.hipFree(ddst)
    # host in, host out (the binding), and the host inverse of the result
    got = svhip.pack_u16(d)
    assert np.array_equal(got, want) and np.array_equal(svhip.unpack_u16(got), R.unpack(want))


# ---------------------------------------------------------------------------- 2. single calls
SINGLE = {
    "320x200": (320, 200, lambda: H.robotics()),
    "401x177_odd_DN": (401, 177, lambda: H.robotics()),
    "97x61_wide_gaps": (97, 61, lambda: H.robotics(ipol_gap_width=5000, add_corners=1, speckle_size=60, lr_threshold=1)),
    "401x177_subsampled": (401, 177, lambda: H.robotics(subsampling=1)),
}


@pytest.mark.parametrize("only_left", [0, 1])
@pytest.mark.parametrize("case", list(SINGLE))
def test_process_out_u16_equals_packed_float_maps(case, only_left, svhip):
    w, h, params = SINGLE[case]
    prm = params()
    prm.postprocess_only_left = only_left
    l, r = H.synth_pair(w, h, 900 + w, dmax=40, noise=4)
    e = svhip.Elas(prm)
    rc, F1, F2 = e.process(l, r)
    assert rc == 0
    # valid and invalid pixels both occur (the wide gap interpolation with corners fills its whole map)
    assert (F1 >= 0).mean() > 0.3 and ((F1 < 0).any() or case == "97x61_wide_gaps")
    if case == "401x177_odd_DN":
        assert F1.size % 2 == 1
    if case == "401x177_subsampled":
        assert F1.shape == (88, 200)
    rc, U1, U2 = e.process(l, r, out="u16")
    assert rc == 0 and U1.dtype == U2.dtype == np.uint16 and U1.shape == F1.shape
    assert np.array_equal(U1, R.pack(F1)) and np.array_equal(U2, R.pack(F2))
    # left only, into a caller's buffer; the right one is not touched (and may be absent)
    V2 = np.full(F1.shape, SENTINEL, np.uint16)
    rc, V1, _ = e.process(l, r, None, V2, out="u16", maps="left")
    assert rc == 0 and np.array_equal(V1, U1) and np.all(V2 == SENTINEL)
    rc, V1, none = e.process(l, r, out="u16", maps="left")
    assert rc == 0 and none is None and np.array_equal(V1, U1)
    rc, G1, none = e.process(l, r, out="f32", maps="left")
    assert rc == 0 and none is None and np.array_equal(G1.view(np.uint32), F1.view(np.uint32))
    # 7. the float entry on the same engine afterwards: the maps it returned before
    rc, A1, A2 = e.process(l, r)
    assert rc == 0 and np.array_equal(A1.view(np.uint32), F1.view(np.uint32))
    assert np.array_equal(A2.view(np.uint32), F2.view(np.uint32))


# ---------------------------------------------------------------------------- 3. batches
@pytest.fixture(scope="module")
def five(svhip):
    """five pairs of 401 x 177 (DN = 70977, odd) with the float path's maps, computed once: (prm, I1, I2, F1, F2).
    Windows of the committed 640 x 240 urban crop, 7 px apart, NOT helpers.synth_pair: seeded synthetic pairs of any
    size come back with status 1 from the existing float stream (svh_elas_stream_push, before and after this feature,
    while the same pairs pass the single and the batch entry), so they cannot serve a comparison with it."""
    prm = H.robotics()
    l, r = H.golden_pair("urban3_640x240")
    I1 = np.stack([l[30:207, 100 + 7 * i:501 + 7 * i] for i in range(5)])
    I2 = np.stack([r[30:207, 100 + 7 * i:501 + 7 * i] for i in range(5)])
    F = [svhip.Elas(prm).process(I1[i], I2[i]) for i in range(5)]
    assert all(f[0] == 0 for f in F)
    F1, F2 = np.stack([f[1] for f in F]), np.stack([f[2] for f in F])
    assert F1[0].size == 70977 and not np.array_equal(F1[0], F1[1])
    return prm, I1, I2, F1, F2


def batch_out(S, e, I1, I2, D1, D2, fmt, maps):
    """svh_elas_process_batch_out on per-pair arrays (D2 None: a NULL pointer array); returns the statuses"""
    n = len(I1)
    arr = C.c_void_p * n
    ptrs = [arr(*[int(X[i].ctypes.data) for i in range(n)]) if X is not None else None for X in (I1, I2, D1, D2)]
    st = (C.c_int32 * n)()
    dims = (C.c_int32 * 3)(I1[0].shape[1], I1[0].shape[0], I1[0].shape[1])
    rc = S.lib().svh_elas_process_batch_out(e._h, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], dims, st,
                                            C.byref(S.ElasOutput(fmt, maps)))
    assert rc >= 0, S.last_error()
    return list(st)


@pytest.fixture()
def groups_of_two(svhip):
    before = svhip.elas_settings()["pairs_per_launch"]
    svhip.set_group(2)
    yield
    svhip.set_group(before if before > 0 else 32)       # (32: what the automatic choice gives for images this small)


def test_batch_out_strided_and_per_pair_copies(svhip, five, groups_of_two):
    """5 pairs in groups of 2, 2, 1.  Outputs in one array: every group's maps go down in one strided copy per map;
    outputs apart from one another: one copy per pair and map.  Both from the lane's 16-bit buffer, whose slots are
    padded to a multiple of 8 elements (DN is odd here)"""
    prm, I1, I2, F1, F2 = five
    n, dn = 5, F1[0].size
    e = svhip.Elas(prm)
    d2h_bytes(svhip, reset=True)
    U1 = np.full(F1.shape, SENTINEL, np.uint16)
    U2 = np.full(F1.shape, SENTINEL, np.uint16)
    assert batch_out(svhip, e, I1, I2, U1, U2, svhip.DISP_U16, svhip.MAPS_BOTH) == [0] * n
    assert np.array_equal(U1, R.pack(F1)) and np.array_equal(U2, R.pack(F2))
    assert d2h_bytes(svhip, reset=True) == (n * dn * 4, 6)              # three groups x two maps
    # separately placed outputs: rows of a wider array, so that no two follow one another
    W1 = np.full((n, dn + 24), SENTINEL, np.uint16)
    W2 = np.full((n, dn + 24), SENTINEL, np.uint16)
    assert batch_out(svhip, e, I1, I2, [W1[i, 8:8 + dn] for i in range(n)], [W2[i, 3:3 + dn] for i in range(n)],
                     svhip.DISP_U16, svhip.MAPS_BOTH) == [0] * n
    assert np.array_equal(W1[:, 8:8 + dn], R.pack(F1).reshape(n, dn)) and np.array_equal(W2[:, 3:3 + dn], R.pack(F2).reshape(n, dn))
    assert np.all(W1[:, :8] == SENTINEL) and np.all(W1[:, 8 + dn:] == SENTINEL)
    assert np.all(W2[:, :3] == SENTINEL) and np.all(W2[:, 3 + dn:] == SENTINEL)
    assert d2h_bytes(svhip, reset=True) == (n * dn * 4, 2 * n)
    # left only, D2 = NULL
    L1 = np.full(F1.shape, SENTINEL, np.uint16)
    assert batch_out(svhip, e, I1, I2, L1, None, svhip.DISP_U16, svhip.MAPS_LEFT) == [0] * n
    assert np.array_equal(L1, R.pack(F1))
    assert d2h_bytes(svhip, reset=True) == (n * dn * 2, 3)
    # left only as floats: bit for bit the float path's
    G1 = np.full(F1.shape, -7, np.float32)
    assert batch_out(svhip, e, I1, I2, G1, None, svhip.DISP_F32, svhip.MAPS_LEFT) == [0] * n
    assert np.array_equal(G1.view(np.uint32), F1.view(np.uint32))
    # the binding's form of the same
    st, B1, B2 = e.process_batch(I1, I2, out="u16", maps="left")
    assert st == [0] * n and B2 is None and np.array_equal(B1, L1)
    # out = NULL is the existing entry
    P1 = np.zeros(F1.shape, np.float32)
    P2 = np.zeros(F1.shape, np.float32)
    arr = C.c_void_p * n
    st = (C.c_int32 * n)()
    rc = svhip.lib().svh_elas_process_batch_out(
        e._h, n, arr(*[int(I1[i].ctypes.data) for i in range(n)]), arr(*[int(I2[i].ctypes.data) for i in range(n)]),
        arr(*[int(P1[i].ctypes.data) for i in range(n)]), arr(*[int(P2[i].ctypes.data) for i in range(n)]),
        (C.c_int32 * 3)(401, 177, 401), st, None)
    assert rc == 0 and np.array_equal(P1.view(np.uint32), F1.view(np.uint32)) and np.array_equal(P2.view(np.uint32), F2.view(np.uint32))


# ---------------------------------------------------------------------------- 4. a pair that does not go through
@pytest.mark.parametrize("stage", [1, 0])
def test_flat_pair_between_good_ones_is_left_untouched(stage, svhip, capfd):
    """fewer than three support points (elas.cpp:69-75): status 1 and untouched buffers, in 16 bits as in floats, with the
    stages between the matching phases on the device (the counts decide what is copied) and on the host"""
    prm = H.robotics()
    a = H.synth_pair(96, 64, 5, dmax=16)
    b = H.synth_pair(96, 64, 6, dmax=16)
    flat = np.full((64, 96), 77, np.uint8)
    I1 = np.stack([a[0], flat, b[0]])
    I2 = np.stack([a[1], flat, b[1]])
    e = svhip.Elas(prm)
    svhip.set_stage(stage)
    try:
        st_f, F1, F2 = e.process_batch(I1, I2)
        U1 = np.full(F1.shape, SENTINEL, np.uint16)
        U2 = np.full(F1.shape, SENTINEL, np.uint16)
        st_u = batch_out(svhip, e, I1, I2, U1, U2, svhip.DISP_U16, svhip.MAPS_BOTH)
        L1 = np.full(F1.shape, SENTINEL, np.uint16)
        st_l = batch_out(svhip, e, I1, I2, L1, None, svhip.DISP_U16, svhip.MAPS_LEFT)
    finally:
        svhip.set_stage(-1)
    assert st_f == [0, 1, 0] and st_u == st_f and st_l == st_f
    assert capfd.readouterr().out.count("Need at least 3 support points") == 3
    assert np.all(U1[1] == SENTINEL) and np.all(U2[1] == SENTINEL) and np.all(L1[1] == SENTINEL)
    for i in (0, 2):
        assert np.array_equal(U1[i], R.pack(F1[i])) and np.array_equal(U2[i], R.pack(F2[i])) and np.array_equal(L1[i], U1[i])
    # the single call
    V1 = np.full((64, 96), SENTINEL, np.uint16)
    V2 = V1.copy()
    rc, V1, V2 = e.process(flat, flat, V1, V2, out="u16")
    assert rc == 1 and np.all(V1 == SENTINEL) and np.all(V2 == SENTINEL)


# ---------------------------------------------------------------------------- 5. streams
def test_streams_of_both_formats_side_by_side(svhip, five):
    """7 pairs through push_out with depth 3, popped in order, next to a float stream on the same engine with the
    pushes interleaved: each stream returns its own format"""
    prm, I1, I2, F1, F2 = five
    n, (h, w) = 7, I1[0].shape
    e = svhip.Elas(prm)
    sf = e.stream(w, h, depth=3)
    su = e.stream(w, h, depth=3, out="u16")
    assert su.dtype == np.uint16 and sf.dtype == np.float32
    Df = [(np.full((h, w), -7, np.float32), np.full((h, w), -7, np.float32)) for _ in range(n)]
    Du = [(np.full((h, w), SENTINEL, np.uint16), np.full((h, w), SENTINEL, np.uint16)) for _ in range(n)]
    popped_f, popped_u = [], []
    for i in range(n):
        if i >= 3:                                        # depth 3: make room first, a push would block
            popped_f.append(sf.pop())
            popped_u.append(su.pop())
        assert su.push(I1[i % 5], I2[i % 5], Du[i][0], Du[i][1]) == i
        assert sf.push(I1[i % 5], I2[i % 5], Df[i][0], Df[i][1]) == i
    while len(popped_u) < n:
        popped_u.append(su.pop())
        popped_f.append(sf.pop())
    assert su.pop() is None and sf.pop() is None
    assert popped_u == [(i, 0) for i in range(n)] and popped_f == popped_u
    for i in range(n):
        assert np.array_equal(Du[i][0], R.pack(F1[i % 5])) and np.array_equal(Du[i][1], R.pack(F2[i % 5])), i
        assert np.array_equal(Df[i][0].view(np.uint32), F1[i % 5].view(np.uint32)), i
        assert np.array_equal(Df[i][1].view(np.uint32), F2[i % 5].view(np.uint32)), i
    # the float push on a 16-bit stream is refused (it would be read as the wrong type), and so is a float array
    assert svhip.lib().svh_elas_stream_push(su._h, I1[0].ctypes.data, I2[0].ctypes.data, Df[0][0].ctypes.data,
                                            Df[0][1].ctypes.data, None) == svhip.ERR_BAD_ARG
    assert "push_out" in svhip.last_error() and su.pop() is None
    with pytest.raises(ValueError):
        su.push(I1[0], I2[0], Df[0][0], Df[0][1])
    sf.close()
    su.close()
    # left only, n pairs per call
    sl = e.stream(w, h, out="u16", maps="left")
    L1 = np.full((n, h, w), SENTINEL, np.uint16)
    sl.push_n([I1[i % 5] for i in range(n)], [I2[i % 5] for i in range(n)], L1)
    assert sl.pop_n(n) == [0] * n
    sl.close()
    for i in range(n):
        assert np.array_equal(L1[i], R.pack(F1[i % 5])), i


# ---------------------------------------------------------------------------- 6. what crosses PCIe
@pytest.mark.parametrize("out,maps,per_pixel", [("f32", "both", 8), ("u16", "both", 4), ("u16", "left", 2), ("f32", "left", 4)])
def test_bytes_copied_down_are_the_models(out, maps, per_pixel, svhip):
    n, w, h = 4, 320, 200
    pairs = [H.synth_pair(w, h, 70 + i, dmax=40) for i in range(n)]
    e = svhip.Elas(H.robotics())
    d2h_bytes(svhip, reset=True)
    st, D1, D2 = e.process_batch(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), out=out, maps=maps)
    assert st == [0] * n
    got, copies = d2h_bytes(svhip)
    assert got == n * w * h * per_pixel and copies >= 1
    assert (D2 is None) == (maps == "left") and D1.dtype == (np.uint16 if out == "u16" else np.float32)

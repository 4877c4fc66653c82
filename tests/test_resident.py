"""Frames in device memory for the Matcher, the visual odometry and the map fusion (svh_*_device): what can be
checked without a GPU.  The library exports the entries, their argument checks answer before any device is touched,
and the numpy restatement of getGain that tests/test_resident_gpu.py compares k_gain with gives the hand-derived
answers, including the ordered-sum case that tells a sequential float32 sum from a tree sum."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import resident_ref as RR


@pytest.fixture(scope="module")
def S():
    import svhip
    svhip.lib()
    return svhip


@pytest.fixture(scope="module")
def RS(S):
    from svhip import resident
    return resident


def test_symbols_exported(S, RS):
    lib = S.lib()
    assert [n for n in RS.SYMBOLS if not hasattr(lib, n)] == []
    assert len(RS.SYMBOLS) == 7


def test_header_declares_the_public_entries_only():
    import os
    pub = open(os.path.join(H.ROOT, "include", "svh.h")).read() + open(os.path.join(H.ROOT, "include", "svh_map.h")).read()
    for n in ("svh_matcher_push_back_device", "svh_vo_process_device", "svh_vo_mono_process_device", "svh_map_add_device"):
        assert n + "(" in pub, n
    assert "svh_test_" not in pub                       # test access is declared with svh_test_fail_at
    guard = open(os.path.join(H.ROOT, "stereo-vision_amd", "csrc", "hip_guard.h")).read()
    for n in ("svh_test_pack_rows", "svh_test_matcher_image", "svh_test_matcher_gain"):
        assert n + "(" in guard, n


def _matcher(S):
    lib = S.lib()
    lib.svh_matcher_create.restype = C.c_void_p
    lib.svh_matcher_create.argtypes = [C.POINTER(H.MatcherParams)]
    lib.svh_matcher_destroy.argtypes = [C.c_void_p]
    p = H.matcher_defaults()
    return lib, lib.svh_matcher_create(C.byref(p))


FAKE = 0x1000    # a non-null "device pointer": the checks below answer before anything is read


@pytest.mark.parametrize("dims,dI1", [((0, 4, 16), FAKE), ((-3, 4, 16), FAKE), ((8, 0, 16), FAKE), ((8, 4, 7), FAKE),
                                      ((8, 4, 8), None)])
def test_matcher_push_bad_dims(S, RS, dims, dI1, capfd):
    lib, m = _matcher(S)
    try:
        L = RS._bind()
        rc = L.svh_matcher_push_back_device(m, dI1, FAKE, (C.c_int32 * 3)(*dims), 0)
        assert rc == S.ERR_BAD_DIMS
        assert "ERROR: Image dimension mismatch!" in capfd.readouterr().err
    finally:
        lib.svh_matcher_destroy(m)


def test_null_arguments(S, RS):
    lib, m = _matcher(S)
    try:
        L = RS._bind()
        d = (C.c_int32 * 3)(8, 4, 8)
        assert L.svh_matcher_push_back_device(m, FAKE, FAKE, None, 0) == S.ERR_BAD_ARG
        assert L.svh_matcher_push_back_device(None, FAKE, FAKE, d, 0) == S.ERR_BAD_ARG
        assert L.svh_vo_process_device(None, FAKE, FAKE, d, 0) == S.ERR_BAD_ARG
        assert L.svh_vo_mono_process_device(None, FAKE, d, 0) == S.ERR_BAD_ARG
        Hm = np.eye(4)
        assert L.svh_map_add_device(None, FAKE, FAKE, d, Hm.ctypes.data, 0.0) == S.ERR_BAD_ARG
        out = np.zeros(64, np.uint8)
        assert L.svh_test_pack_rows(None, 8, 4, 8, 16, out.ctypes.data) == S.ERR_BAD_ARG
        assert L.svh_test_pack_rows(FAKE, 8, 4, 7, 16, out.ctypes.data) == S.ERR_BAD_DIMS     # pitch < w
        assert L.svh_test_pack_rows(FAKE, 8, 4, 8, 12, out.ctypes.data) == S.ERR_BAD_DIMS     # bpl not a multiple of 16
        assert L.svh_test_matcher_image(m, 4, None, 0) == S.ERR_BAD_ARG
        assert L.svh_test_matcher_image(m, RS.CUR_LEFT, None, 0) == 0                        # no frame yet
        g = L.svh_test_matcher_gain(m, None, 0, None, 0, RS.GAIN_DEVICE)
        assert g != g and "no two left frames" in S.last_error()
    finally:
        lib.svh_matcher_destroy(m)


def test_vo_objects_check_their_kind(S, RS):
    """a mono object refuses the stereo entry and the other way round, as the host entries do; null dims first"""
    L = RS._bind()
    vo = H.ProductVo(H.vo_defaults())
    mono = S.VoMono()
    d = (C.c_int32 * 3)(8, 4, 8)
    assert L.svh_vo_process_device(vo.h, FAKE, FAKE, None, 0) == S.ERR_BAD_ARG
    assert L.svh_vo_mono_process_device(mono.h, FAKE, None, 0) == S.ERR_BAD_ARG
    assert L.svh_vo_process_device(mono.h, FAKE, FAKE, d, 0) == S.ERR_BAD_ARG
    assert L.svh_vo_mono_process_device(vo.h, FAKE, d, 0) == S.ERR_BAD_ARG
    mono.close()


# ---- the numpy restatement of getGain against hand-derived answers on a 12 x 9 image
def hand_pair():
    Ip = np.full((9, 12), 10, np.uint8)
    Ip[4, 5] = 11                    # one window of 49 pixels sums to 491: mean 10 + 1/49
    Ic = np.full((9, 12), 50, np.uint8)
    return Ip, Ic


HAND = RR.make_matches([
    (0, 0, 0, 0),        # 0: window [0..3]^2 of tens: mean exactly 10 -> excluded
    (5, 4, 11, 8),       # 1: previous 491/49; current clamps to columns 8..12 and rows 5..9 (column W = 12 and row
                         #    H = 9 are zero): 16 pixels of 50 over 25 = 32
    (5, 4, 0, 0),        # 2: previous 491/49; current [0..3]^2: 50
    (9, 4, 5, 4),        # 3: previous columns 6..12, one of them padding: 420/49 < 10 -> excluded
    (8.9, 4.9, 5, 4),    # 4: truncates to (8, 4): columns 5..11 hold the 11: 491/49; current 50
])


def test_restatement_windows():
    Ip, Ic = hand_pair()
    Pp, Pc = RR.padded(Ip), RR.padded(Ic)
    assert Pp.shape == (10, 16)
    f = np.float32
    assert RR.window_mean(Pp, 12, 9, 0, 0) == f(10)
    assert RR.window_mean(Pp, 12, 9, 5, 4) == f(491) / f(49) and RR.window_mean(Pp, 12, 9, 5, 4) > 10
    assert RR.window_mean(Pc, 12, 9, 11, 8) == f(32)
    assert RR.window_mean(Pp, 12, 9, 9, 4) == f(420) / f(49)
    assert RR.window_mean(Pc, 12, 9, 17, 14) == f(0)            # only column W and row H are left
    assert RR.window_mean(Pc, 12, 9, -0.5, -0.5) == f(50)


def test_restatement_gain():
    Ip, Ic = hand_pair()
    f = np.float32
    mp = f(491) / f(49)
    r1, r2 = f(32) / mp, f(50) / mp
    assert RR.gain(Ip, Ic, HAND, [0]) == f(1)                           # mean exactly 10: no qualifying inlier
    assert RR.gain(Ip, Ic, HAND, [1]) == r1                             # 10 + 1/49 is included
    assert RR.gain(Ip, Ic, HAND, [0, 1, 2, 7, 3]) == f(f(r1 + r2) / f(2))   # 7 >= nm is skipped, 0 and 3 excluded
    assert RR.gain(Ip, Ic, HAND, [4, 2]) == f(f(r2 + r2) / f(2))
    assert RR.gain(Ip, Ic, HAND, []) == f(1)                            # n = 0
    assert RR.gain(Ip, Ic, HAND, [5, 6, 100]) == f(1)                   # only indices past the list
    assert RR.gain(Ip, Ic, HAND[:0], [0, 1]) == f(1)


def test_ordered_sum_input_tells_the_orders_apart():
    Ip, Ic, m, idx, r = RR.ordered_sum_case()
    assert len(idx) == 1025 and len(r) == 1025 and r.dtype == np.float32
    seq, tree = RR.sequential_sum(r), np.sum(r)                         # numpy adds pairwise
    assert seq != tree
    assert np.float32(seq / np.float32(1025)) != np.float32(tree / np.float32(1025))
    assert RR.gain(Ip, Ic, m, idx) == np.float32(seq / np.float32(1025))


def test_inlier_lists_reach_past_the_matches():
    nm = len(RR.crafted_matches())
    for n in (0, 1, 63, 64, 65, 256, 257, 1024, 1025):
        idx = RR.inlier_list(n, nm)
        assert len(idx) == n and (idx >= 0).all()
        assert (idx >= nm).any() == (n >= 17)

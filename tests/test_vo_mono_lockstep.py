"""CPU: the lockstep entries of VisualOdometryMono (svh_vo_mono_process_batch, _prefetch_batch, _process_next_batch,
_process_matches_batch; include/svh.h) at the boundary.  They are exported; their argument checks answer
SVH_ERR_BAD_ARG; without a device they report what the single call svh_vo_mono_process reports instead of crashing;
the C++ program that drives them (tests/mono/mono_lockstep.cpp) compiles against include/ alone.  What they compute is
checked on the GPU (tests/test_vo_mono_lockstep_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H

NAMES = ["svh_vo_mono_process_batch", "svh_vo_mono_prefetch_batch", "svh_vo_mono_process_next_batch",
         "svh_vo_mono_process_matches_batch"]


@pytest.fixture(scope="module")
def S():
    import svhip
    return svhip


@pytest.fixture(scope="module")
def L(S):
    L = S.lib()
    v = C.c_void_p
    L.svh_vo_mono_process_batch.argtypes = [v, C.c_int32, v, v, v, v]
    L.svh_vo_mono_prefetch_batch.argtypes = [v, C.c_int32, v, v]
    L.svh_vo_mono_process_next_batch.argtypes = [v, C.c_int32, v, v, v, v]
    L.svh_vo_mono_process_matches_batch.argtypes = [v, C.c_int32, v, v, v]
    L.svh_vo_mono_process.argtypes = [v, v, v, C.c_int32]
    return L


def calls(L, hs, K, ims, dims, mp, n, ok):
    """the four entries on the same objects: name -> return value"""
    return {
        "process_batch": L.svh_vo_mono_process_batch(hs, K, ims, dims, None, ok),
        "prefetch_batch": L.svh_vo_mono_prefetch_batch(hs, K, ims, dims),
        "process_next_batch": L.svh_vo_mono_process_next_batch(hs, K, ims, dims, None, ok),
        "process_matches_batch": L.svh_vo_mono_process_matches_batch(hs, K, mp, n, ok),
    }


def test_symbols_are_exported_and_declared(S):
    hdr = open(os.path.join(H.ROOT, "include", "svh.h")).read()
    for name in NAMES:
        assert hasattr(S.lib(), name), name
        assert ("int32_t %s(" % name) in hdr, name


def test_argument_checks_and_no_device(S, L):
    img = np.zeros((48, 64), np.uint8)
    dims = (C.c_int32 * 3)(64, 48, 64)
    m = np.zeros(16, S.P_MATCH)
    a, b = S.VoMono(S.vo_mono_params()), S.VoMono(S.vo_mono_params())
    st = H.ProductVo(H.vo_defaults())
    ims = (C.c_void_p * 2)(img.ctypes.data, img.ctypes.data)
    mp = (C.c_void_p * 2)(m.ctypes.data, m.ctypes.data)
    n = (C.c_int32 * 2)(16, 16)
    ok = (C.c_int32 * 2)()
    bad = {
        "null object": (C.c_void_p * 2)(a.h, None),
        "stereo handle": (C.c_void_p * 2)(a.h, st.h),
        "duplicate": (C.c_void_p * 2)(a.h, a.h),
    }
    for why, hs in bad.items():
        for name, rc in calls(L, hs, 2, ims, dims, mp, n, ok).items():
            assert rc == S.ERR_BAD_ARG, (why, name, rc)
    good = (C.c_void_p * 2)(a.h, b.h)
    for name, rc in calls(L, good, -1, ims, dims, mp, n, ok).items():
        assert rc == S.ERR_BAD_ARG, ("K < 0", name, rc)
    for name, rc in calls(L, None, 2, ims, dims, mp, n, ok).items():
        assert rc == S.ERR_BAD_ARG, ("null object array", name, rc)
    r = calls(L, good, 2, ims, None, mp, n, ok)
    for name in ("process_batch", "prefetch_batch", "process_next_batch"):
        assert r[name] == S.ERR_BAD_ARG, ("null dims", name, r[name])
    # the stereo lockstep entries still refuse a mono handle
    L.svh_vo_process_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert L.svh_vo_process_batch(good, 2, ims, ims, dims, 0, ok) == S.ERR_BAD_ARG
    if S.device_count() > 0:
        return   # (what the entries compute with a device: tests/test_vo_mono_lockstep_gpu.py)
    # no device: the value of the single call, for K = 2 and for K = 1, and nothing crashes
    single = L.svh_vo_mono_process(a.h, img.ctypes.data, dims, 0)
    assert single == S.ERR_NO_DEVICE, single
    for K in (2, 1):
        for name, rc in calls(L, good, K, ims, dims, mp, n, ok).items():
            assert rc == single, (K, name, rc)
    assert "no HIP device" in S.last_error()


def test_program_compiles_against_include_alone(tmp_path):
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(H.ROOT, "include"), "-c",
                           os.path.join(H.ROOT, "tests", "mono", "mono_lockstep.cpp"), "-o", str(tmp_path / "l.o")])

"""K objects in lockstep on device frames (svh_matcher_push_back_batch_device, svh_vo_process_batch_device,
svh_vo_mono_process_batch_device, svh_vo_get_gain_batch, svh_map_add_batch_device): what can be checked without a GPU.
The library exports the entries with the documented signatures, their argument checks answer before any device is
touched, and the lockstep counters (svh_test_lockstep_counts) count what they say over a stub device layer --
tests/cxx/lockstep_counts_check.cpp, built here by this test's own compiler command, plain and under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H

FAKE = 0x1000    # a non-null "device pointer": the checks below answer before anything is read

DECLARATIONS = {
    "svh.h": [
        "int32_t svh_matcher_push_back_batch_device(svh_matcher* const* ms, int32_t K, const uint8_t* const* dI1, "
        "const uint8_t* const* dI2, const int32_t* dims, int32_t replace);",
        "int32_t svh_vo_process_batch_device(svh_vo* const* vs, int32_t K, const uint8_t* const* dI1, "
        "const uint8_t* const* dI2, const int32_t* dims, int32_t replace, int32_t* ok);",
        "int32_t svh_vo_mono_process_batch_device(svh_vo* const* vs, int32_t K, const uint8_t* const* dI, "
        "const int32_t* dims, const int32_t* replace, int32_t* ok);",
        "int32_t svh_vo_get_gain_batch(svh_vo* const* vs, int32_t K, const int32_t* const* inliers, const int32_t* n, "
        "float* gain);",
    ],
    "svh_map.h": [
        "int32_t svh_map_add_batch_device(svh_map* const* ms, int32_t K, const float* const* dD1, "
        "const uint8_t* const* dI1, const int32_t* dims, const double* const* H_total, const float* gain);",
    ],
}


@pytest.fixture(scope="module")
def S():
    import svhip
    svhip.lib()
    return svhip


@pytest.fixture(scope="module")
def RS(S):
    from svhip import resident
    return resident


def squeeze(text):
    return re.sub(r"\s+", " ", text)


def test_symbols_exported_and_declared(S, RS):
    lib = S.lib()
    assert [n for n in RS.LOCKSTEP_SYMBOLS if not hasattr(lib, n)] == []
    assert len(RS.LOCKSTEP_SYMBOLS) == 6
    pub = ""
    for name, decls in DECLARATIONS.items():
        text = squeeze(open(os.path.join(H.ROOT, "include", name)).read())
        pub += text
        for d in decls:
            assert d in text, d
    assert "svh_test_" not in pub                       # the tap is declared with svh_test_fail_at
    guard = squeeze(open(os.path.join(H.ROOT, "stereo-vision_amd", "csrc", "hip_guard.h")).read())
    assert 'extern "C" void svh_test_lockstep_counts(int64_t out[3]);' in guard


def table(*xs):
    return (C.c_void_p * len(xs))(*xs)


def matchers(S, n):
    lib = S.lib()
    lib.svh_matcher_create.restype = C.c_void_p
    lib.svh_matcher_create.argtypes = [C.POINTER(H.MatcherParams)]
    lib.svh_matcher_destroy.argtypes = [C.c_void_p]
    p = H.matcher_defaults()
    return lib, [lib.svh_matcher_create(C.byref(p)) for _ in range(n)]


def test_matcher_batch_arguments(S, RS, capfd):
    lib, ms = matchers(S, 2)
    try:
        L = RS._bind()
        before = RS.lockstep_counts()
        d = (C.c_int32 * 3)(8, 4, 8)
        f2 = table(FAKE, FAKE)
        assert L.svh_matcher_push_back_batch_device(None, 2, f2, f2, d, 0) == S.ERR_BAD_ARG
        assert L.svh_matcher_push_back_batch_device(table(*ms), -1, f2, f2, d, 0) == S.ERR_BAD_ARG
        assert L.svh_matcher_push_back_batch_device(table(*ms), 2, f2, f2, None, 0) == S.ERR_BAD_ARG
        assert L.svh_matcher_push_back_batch_device(table(*ms), 2, None, None, d, 0) == S.ERR_BAD_ARG   # takes no hand-over
        assert L.svh_matcher_push_back_batch_device(table(*ms), 0, f2, f2, d, 0) == 0
        assert L.svh_matcher_push_back_batch_device(table(ms[0], ms[0]), 2, f2, f2, d, 0) == S.ERR_BAD_ARG
        assert "twice" in S.last_error()
        assert L.svh_matcher_push_back_batch_device(table(ms[0], None), 2, f2, f2, d, 0) == S.ERR_BAD_ARG
        for dims in ((0, 4, 16), (8, 0, 16), (8, 4, 7)):
            capfd.readouterr()
            assert L.svh_matcher_push_back_batch_device(table(*ms), 2, f2, f2, (C.c_int32 * 3)(*dims), 0) == S.ERR_BAD_DIMS
            assert "ERROR: Image dimension mismatch!" in capfd.readouterr().err
        assert RS.lockstep_counts() == before           # nothing of this recorded a phase
    finally:
        for m in ms:
            lib.svh_matcher_destroy(m)


def test_vo_batch_arguments(S, RS):
    L = RS._bind()
    vos = [H.ProductVo(H.vo_defaults()) for _ in range(2)]
    mono = [S.VoMono() for _ in range(2)]
    d = (C.c_int32 * 3)(8, 4, 8)
    f2 = table(FAKE, FAKE)
    ok = (C.c_int32 * 2)()
    hs, hm = table(*[v.h for v in vos]), table(*[v.h for v in mono])
    assert L.svh_vo_process_batch_device(None, 2, f2, f2, d, 0, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_process_batch_device(hs, 2, None, f2, d, 0, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_process_batch_device(hs, 2, f2, None, d, 0, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_process_batch_device(hs, 2, None, None, d, 0, ok) == S.ERR_BAD_ARG       # takes no hand-over
    assert L.svh_vo_process_batch_device(hs, 2, f2, f2, None, 0, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_process_batch_device(hs, -1, f2, f2, d, 0, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_process_batch_device(table(vos[0].h, vos[0].h), 2, f2, f2, d, 0, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_process_batch_device(table(vos[0].h, None), 2, f2, f2, d, 0, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_process_batch_device(hm, 2, f2, f2, d, 0, ok) == S.ERR_BAD_ARG           # mono objects
    assert L.svh_vo_process_batch_device(hs, 0, f2, f2, d, 0, ok) == 0
    assert L.svh_vo_mono_process_batch_device(None, 2, f2, d, None, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_mono_process_batch_device(hm, 2, None, d, None, ok) == S.ERR_BAD_ARG     # takes no hand-over
    assert L.svh_vo_mono_process_batch_device(hm, 2, f2, None, None, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_mono_process_batch_device(hm, -1, f2, d, None, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_mono_process_batch_device(hs, 2, f2, d, None, ok) == S.ERR_BAD_ARG       # stereo objects
    assert L.svh_vo_mono_process_batch_device(table(mono[0].h, mono[0].h), 2, f2, d, None, ok) == S.ERR_BAD_ARG
    assert L.svh_vo_mono_process_batch_device(hm, 0, f2, d, None, ok) == 0
    for v in mono:
        v.close()


def test_gain_batch_arguments_and_objects_without_frames(S, RS):
    L = RS._bind()
    vos = [H.ProductVo(H.vo_defaults()), S.VoMono()]
    hs = table(*[v.h for v in vos])
    idx = np.arange(3, dtype=np.int32)
    lists = table(idx.ctypes.data, idx.ctypes.data)
    n = (C.c_int32 * 2)(3, 0)
    gain = np.full(2, 7, np.float32)
    assert L.svh_vo_get_gain_batch(None, 2, lists, n, gain.ctypes.data) == S.ERR_BAD_ARG
    assert L.svh_vo_get_gain_batch(hs, 2, None, n, gain.ctypes.data) == S.ERR_BAD_ARG
    assert L.svh_vo_get_gain_batch(hs, 2, lists, None, gain.ctypes.data) == S.ERR_BAD_ARG
    assert L.svh_vo_get_gain_batch(hs, 2, lists, n, None) == S.ERR_BAD_ARG
    assert L.svh_vo_get_gain_batch(hs, -1, lists, n, gain.ctypes.data) == S.ERR_BAD_ARG
    assert L.svh_vo_get_gain_batch(table(vos[0].h, vos[0].h), 2, lists, n, gain.ctypes.data) == S.ERR_BAD_ARG
    assert L.svh_vo_get_gain_batch(table(vos[0].h, None), 2, lists, n, gain.ctypes.data) == S.ERR_BAD_ARG
    assert L.svh_vo_get_gain_batch(hs, 2, lists, (C.c_int32 * 2)(3, -1), gain.ctypes.data) == S.ERR_BAD_ARG
    assert L.svh_vo_get_gain_batch(hs, 2, table(None, None), (C.c_int32 * 2)(3, 0), gain.ctypes.data) == S.ERR_BAD_ARG
    assert np.all(gain == 7)                            # (refused calls write nothing)
    assert L.svh_vo_get_gain_batch(None, 0, None, None, None) == 0
    # objects without two frames: gain 1, as svh_vo_get_gain says, and no device is needed for that
    before = RS.lockstep_counts()
    assert L.svh_vo_get_gain_batch(hs, 2, lists, n, gain.ctypes.data) == 0
    assert np.all(gain == 1)
    assert list(RS.vo_gain_batch(vos, [idx, []])) == [1, 1]
    assert RS.lockstep_counts() == before
    vos[1].close()


def test_map_batch_arguments(S, RS):
    L = RS._bind()
    Hm = np.eye(4)
    d = (C.c_int32 * 3)(8, 4, 8)
    m2, f2, h2 = table(FAKE, FAKE + 64), table(FAKE, FAKE), table(Hm.ctypes.data, Hm.ctypes.data)
    g = np.zeros(2, np.float32)
    call = L.svh_map_add_batch_device
    assert call(None, 2, f2, f2, d, h2, g.ctypes.data) == S.ERR_BAD_ARG
    assert call(m2, 2, None, f2, d, h2, g.ctypes.data) == S.ERR_BAD_ARG
    assert call(m2, 2, f2, None, d, h2, g.ctypes.data) == S.ERR_BAD_ARG
    assert call(m2, 2, f2, f2, None, h2, g.ctypes.data) == S.ERR_BAD_ARG
    assert call(m2, 2, f2, f2, d, None, g.ctypes.data) == S.ERR_BAD_ARG
    assert call(m2, 2, f2, f2, d, h2, None) == S.ERR_BAD_ARG
    assert call(m2, -1, f2, f2, d, h2, g.ctypes.data) == S.ERR_BAD_ARG
    for dims in ((0, 4, 8), (8, 0, 8), (8, 4, 7), (1 << 15, 1 << 14, 1 << 15)):
        assert call(m2, 2, f2, f2, (C.c_int32 * 3)(*dims), h2, g.ctypes.data) == S.ERR_BAD_ARG     # (before a map is read)
    assert call(m2, 2, table(FAKE, None), f2, d, h2, g.ctypes.data) == S.ERR_BAD_ARG
    assert call(m2, 2, f2, table(None, FAKE), d, h2, g.ctypes.data) == S.ERR_BAD_ARG
    assert call(m2, 2, f2, f2, d, table(Hm.ctypes.data, None), g.ctypes.data) == S.ERR_BAD_ARG
    assert call(table(None, None), 2, f2, f2, d, h2, g.ctypes.data) == S.ERR_BAD_ARG
    assert call(m2, 0, f2, f2, d, h2, g.ctypes.data) == 0


def test_counters_start_readable(S, RS):
    c = RS.lockstep_counts()
    assert len(c) == 3 and all(isinstance(v, int) and v >= 0 for v in c)
    RS._bind().svh_test_lockstep_counts(None)           # (ignored)


# ---- the counters over the stub device layer -------------------------------------------------------------------------
CSRC = os.path.join(H.ROOT, "stereo-vision_amd", "csrc")
SOURCES = [os.path.join(H.ROOT, "tests", "cxx", "lockstep_counts_check.cpp"), os.path.join(CSRC, "batch_rec.cpp"),
           os.path.join(CSRC, "svh_error.cpp")]


def build_and_run(tmp_path, san):
    exe = str(tmp_path / "lockstep_counts_check")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall"] + san + [
        "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe] + SOURCES + ["-lpthread"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lockstep_counts_check: 0 failed checks" in r.stdout, r.stdout


def test_counters_over_the_stub_device_layer(tmp_path):
    """a recorded phase with K = 1, 2, 5 flushes once with a launch count independent of K; a sequence mismatch counts
    as a fallback; a phase that fails counts as neither"""
    build_and_run(tmp_path, [])


def test_counters_over_the_stub_device_layer_under_sanitizers(tmp_path):
    build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])

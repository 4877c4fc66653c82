"""GPU parity on the reference's own images at full size (tests/golden/full, make_goldens_full.py):
the seven stereo pairs of libelas/src/main.cpp's demo and the mono sequence I1_000000..6.

These are the first real inputs to reach the size-picked kernel forms (see FORMS below): rows past
1280 px (k_match_list with 384 threads per side), lattices too large for k_lattice's LDS, point sets
beyond the LDS records of the small k_delaunay (cones) and the split 1024-thread k_delaunay (aloe,
raindeer).  Taps on: every stage by its sha256 against the reference's, in both forms of the middle
stages.  Taps off (what an application runs: tile post-filters, descriptors on the fly, fused L/R
check): the final maps of every entry point.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from test_elas_gpu import product_run
from test_oracle_full import ELAS_CASES, MONO_SETS, assert_lists, check_mono_step, first_bad_stage, mono_params

pytestmark = pytest.mark.gpu

URBAN = ["urban1", "urban2", "urban3", "urban4"]

# per pair: (k_lattice holds the lattice in LDS, k_delaunay in its large split form, threads per side of
# k_match_list); whether the small k_delaunay keeps its point records in LDS is asserted per case.
# What the kernel profile observes is only the stage's side: k_lattice / k_delaunay run on the device or not.
# The profile times every matcher form as "k_match" and every triangulation form as "k_delaunay", so the forms
# in this table are INFERRED from the engine's thresholds (engine_forms), not observed.
FORMS = {
    "urban": (False, False, 384),        # 269 x 79 lattice = 63 756 B > 62 KB; 1344-px rows
    "cones": (False, False, 256),        # 180 x 150 lattice; 900-px rows
    "aloe": (False, True, 384),          # 257 x 222 lattice; 1282-px rows, just past 1280
    "raindeer": (False, True, 384),
    "urban_sub": (True, False, 256),     # subsampled: step 6, 224 x 66 lattice; 672-px output rows
}
SMALL_DT_LDS_CAP = (96 * 1024 - 32) // 48 - 1     # 2046 points: k_delaunay<512, 0> records in 96 KB of LDS
ML_CAP = 32                                        # uint16 per cell record of k_match_list (elas_kernels.hip)


def prior_absmax(prm, plane_radius):
    """max |P[dd]| for dd <= plane_radius of the prior table (elas_host.cpp prior_table), in float32"""
    f = np.float32
    two_sigma_squared = f(2) * f(prm.sigma) * f(prm.sigma)
    out = 0
    for dd in range(min(plane_radius, prm.disp_max) + 1):
        tmp = -np.log(f(prm.gamma) + np.exp(f(-dd * dd) / two_sigma_squared)) + np.log(f(prm.gamma))
        out = max(out, abs(int(f(tmp) / f(prm.beta))))
    return out


def engine_forms(prm, w, h, nsup):
    """the engine's form thresholds (elas_host.cpp make_dims, elas_stage_kernels.hip launch_stage_device,
    elas_kernels.hip match_list_usable) recomputed for one pair at the default settings (no SVH_* overrides).
    Not mirrored: the driver's answers to the LDS opt-ins (hipFuncSetAttribute above 64 KB, which the MI355X's
    160 KB of LDS per CU grants) and whether the lane has its candidate lists allocated"""
    step = prm.candidate_stepsize + (prm.candidate_stepsize % 2 if prm.subsampling else 0)
    wc, hc = (w + step - 1) // step, (h + step - 1) // step
    nc = wc * hc
    lat_bytes = 2 * ((nc + 1) & ~1) + 4 * ((nc + 3) // 4)
    big = nc // 8 * 16 > 63 * 1024
    dw = w // 2 if prm.subsampling else w
    iters = (dw + 255) // 256
    half = min(256, ((dw + iters - 1) // iters + 63) // 64 * 64)
    if iters > 5 and dw <= 5 * 384:
        iters = (dw + 383) // 384
        half = min(384, ((dw + iters - 1) // iters + 63) // 64 * 64)
    plane_radius = max(math.ceil(prm.sigma * prm.sradius), 2)
    absmax = prior_absmax(prm, plane_radius)
    gw = math.ceil(w / prm.grid_size)
    ws, wr = ((w + 3) & ~3) + 2, (w + 7) // 8 * 8
    list_lds = 2 * ws * 16 + 2 * gw * ML_CAP * 2 + 2 * wr * 2 + 256
    list_ok = (absmax < (1 << 19) and prm.disp_max < 512 and plane_radius <= 15 and w < 65536 and prm.grid_size > 1
               and (prm.disp_max + 1 + 31) // 32 <= 8 and absmax < 28000 and dw <= 8 * 256
               and list_lds <= 160 * 1024)
    return {"lattice_lds": lat_bytes <= 62 * 1024, "dt_large": big, "match_half": half if list_ok else None,
            "records_lds": not big and nsup <= SMALL_DT_LDS_CAP, "cells": nc, "lat_bytes": lat_bytes}


def expected_forms(case, pair):
    key = "urban_sub" if case.endswith("_sub") else ("urban" if pair.startswith("urban") else pair)
    lds, big, half = FORMS[key]
    return {"lattice_lds": lds, "dt_large": big, "match_half": half}


def read_profile(S):
    lib = S.lib()
    lib.svh_profile_get.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    out = {}
    for i in range(lib.svh_profile_get(-1, None, None, None)):
        name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
        lib.svh_profile_get(i, C.byref(name), C.byref(ms), C.byref(cnt))
        out[name.value.decode()] = cnt.value
    return out


@pytest.fixture(scope="module")
def S():
    import svhip
    svhip.lib()
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_profile_only.argtypes = [C.c_char_p]
    return svhip


def locate(prm, w, h, s, i):
    """where element i of stage s lies: a pixel, a lattice cell, a grid cell or a list entry"""
    dw, dh = (w // 2, h // 2) if prm.subsampling else (w, h)
    if s in (H.DESC1, H.DESC2):                       # 16 bytes per pixel of the full image
        return "pixel (u=%d, v=%d) byte %d" % (i // 16 % w, i // 16 // w, i % 16)
    if s == H.DCAN_RAW:                               # the candidate lattice, Wc x Hc
        step = prm.candidate_stepsize + (prm.candidate_stepsize % 2 if prm.subsampling else 0)
        wc = (w + step - 1) // step
        return "lattice cell (%d, %d)" % (i % wc, i // wc)
    if s in (H.GRID1, H.GRID2):                       # disp_max + 2 ints per grid cell
        gw, k = math.ceil(w / prm.grid_size), i // (prm.disp_max + 2)
        return "grid cell (%d, %d) slot %d" % (k % gw, k // gw, i % (prm.disp_max + 2))
    if s in (H.PLANES1, H.PLANES2):
        return "triangle %d coefficient %d" % (i // 6, i % 6)
    if s >= H.D1_RAW:
        return "pixel (u=%d, v=%d)" % (i % dw, i // dw)
    return "entry %d value %d" % (i // 3, i % 3)


def explain_mismatch(request, z, prm, l, r, got, bad):
    """one live oracle run: the first element of the first differing stage, and where it lies"""
    request.getfixturevalue("oracle_lib")            # builds oracle/liboracle.so if it is missing
    s = next(k for k, v in H.STAGE_NAMES.items() if v == bad)
    tri = None if H.have_ref_elas() else H.fixture_triangulator([z["tri1"], z["tri2"]])
    want = H.oracle_elas_run(prm, l, r, tri)
    if s not in got or s not in want:
        return "stage %s: missing (product %s, oracle %s)" % (bad, s in got, s in want)
    a, b = got[s].ravel(), want[s].ravel()
    if a.shape != b.shape:
        return "stage %s: %d values, the oracle's %d" % (bad, a.size, b.size)
    diff = np.flatnonzero(a != b)                     # element compare: -0.0 == +0.0 like the golden hash
    if not len(diff):
        return "stage %s: equal to the live oracle, but not to the golden hash" % bad
    i = int(diff[0])
    return "stage %s first differs at %s (element %d of %d, %d differ): %r, oracle %r" % (
        bad, locate(prm, l.shape[1], l.shape[0], s, i), i, a.size, len(diff), a[i], b[i])


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("case", ELAS_CASES)
def test_every_stage_with_taps(case, stage, S, request):
    """single call, taps on, middle stages forced to the host (0) or the device (1): lists exact, every stage's
    hash the reference's; the device takes the group without handing it back"""
    z, prm, l, r = H.full_case(case)
    pair = str(z["pair"])
    nsup = len(z["support"]) // 3
    forms = engine_forms(prm, l.shape[1], l.shape[0], nsup)
    want_forms = expected_forms(case, pair)
    assert {k: forms[k] for k in want_forms} == want_forms, forms
    if pair == "cones":
        assert nsup > SMALL_DT_LDS_CAP and not forms["records_lds"]     # the small form's L2-record branch
    if pair.startswith("urban") and not prm.subsampling:
        assert forms["lat_bytes"] == 63756 and nsup <= SMALL_DT_LDS_CAP
    if forms["dt_large"]:
        assert nsup <= 8000                                             # 16-bit handles of the large form
    S.set_stage(stage)
    S.lib().svh_profile_only(None)
    S.lib().svh_profile_reset()
    S.lib().svh_profile_enable(1)
    before = S.stage_stats()
    try:
        got = product_run(S, prm, l, r)
    finally:
        S.lib().svh_profile_enable(0)
        S.set_stage(-1)
    after = S.stage_stats()
    prof = read_profile(S)
    assert got.status == 0
    if stage == 1:
        assert after == (before[0] + 1, before[1]), (before, after)    # device stage, nothing handed back
        assert prof.get("k_lattice", 0) == 1 and prof.get("k_delaunay", 0) >= 1, prof
    else:
        assert after == before, (before, after)
        assert "k_lattice" not in prof and "k_delaunay" not in prof, prof
    assert prof.get("k_match", 0) >= 1, prof        # (one name for every matcher form: see FORMS)
    assert_lists(z, got)
    bad = first_bad_stage(z, got)
    if bad is not None:
        pytest.fail("%s, stage %d: %s" % (case, stage, explain_mismatch(request, z, prm, l, r, got, bad)))
    assert int((got[H.D1_FINAL] >= 0).sum()) == int(z["d1_valid"])
    assert int((got[H.D2_FINAL] >= 0).sum()) == int(z["d2_valid"])


def assert_final(z, D1, D2, what):
    assert H.stage_sha256(D1.ravel()) == str(z["d1_sha256"]), (what, "d1")
    assert H.stage_sha256(D2.ravel()) == str(z["d2_sha256"]), (what, "d2")


@pytest.mark.parametrize("case", ELAS_CASES)
def test_single_call_without_taps(case, S):
    """automatic stage, taps off: a single call takes the host stage"""
    z, prm, l, r = H.full_case(case)
    before = S.stage_stats()
    rc, D1, D2 = S.Elas(prm).process(l, r)
    assert rc == 0
    assert S.stage_stats() == before
    assert_final(z, D1, D2, case)


def urban_batch(setting):
    zs, ls, rs = [], [], []
    for p in URBAN:
        z, prm, l, r = H.full_case(p + "_" + setting)
        zs.append(z)
        ls.append(l)
        rs.append(r)
    return zs, prm, np.stack(ls), np.stack(rs)


@pytest.mark.parametrize("setting", ["robotics", "demo"])
def test_urban_batch_without_taps(setting, S):
    zs, prm, I1, I2 = urban_batch(setting)
    st, D1, D2 = S.Elas(prm).process_batch(I1, I2)
    assert st == [0] * 4
    for i, z in enumerate(zs):
        assert_final(z, D1[i], D2[i], URBAN[i])


def test_urban_batch_device_without_taps(S):
    """svh_elas_process_batch_device (what bench.py calls), device memory from the HIP runtime the library links"""
    hip = C.CDLL("libamdhip64.so")
    zs, prm, I1, I2 = urban_batch("robotics")
    n, h, w = I1.shape
    D0 = np.full((n, h, w), -7.0, np.float32)

    def to_device(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0   # H2D
        return p
    ptrs = [to_device(a) for a in (np.ascontiguousarray(I1), np.ascontiguousarray(I2), D0, D0)]
    try:
        st = S.Elas(prm).process_batch_device(n, ptrs[0], ptrs[1], w * h, ptrs[2], ptrs[3], w * h * 4, w, h, w)
        assert st == [0] * n
        D1, D2 = np.empty_like(D0), np.empty_like(D0)
        assert hip.hipMemcpy(C.c_void_p(D1.ctypes.data), ptrs[2], C.c_size_t(D1.nbytes), 2) == 0   # D2H
        assert hip.hipMemcpy(C.c_void_p(D2.ctypes.data), ptrs[3], C.c_size_t(D2.nbytes), 2) == 0
    finally:
        for p in ptrs:
            hip.hipFree(p)
    for i, z in enumerate(zs):
        assert_final(z, D1[i], D2[i], URBAN[i])


def test_urban_stream_without_taps(S):
    """svh_elas_stream_*: the four urban pairs (demo setting) one at a time, results in order"""
    zs, prm, I1, I2 = urban_batch("demo")
    n, h, w = I1.shape
    e = S.Elas(prm)
    D1 = np.zeros((n, h, w), np.float32)
    D2 = np.zeros((n, h, w), np.float32)
    st = e.stream(w, h)
    try:
        tickets = [st.push(I1[i], I2[i], D1[i], D2[i]) for i in range(n)]
        got = [st.pop() for _ in range(n)]
    finally:
        st.close()
    assert [t for t, _ in got] == tickets and [s for _, s in got] == [0] * n
    for i, z in enumerate(zs):
        assert_final(z, D1[i], D2[i], URBAN[i])


@pytest.mark.parametrize("pair", ["urban1", "aloe"])
def test_cxx_dropin_demo_full_size(pair, tmp_path, S):
    """libelas/src/main.cpp's demo call sequence through include/elas.h on the full-size pair"""
    z, prm, l, r = H.full_case(pair + "_demo")
    subprocess.check_call(["make", "-C", os.path.join(H.ROOT, "tests", "cxx"), "all"], stdout=subprocess.DEVNULL)
    lp, rp = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm")
    H.write_pgm(lp, l)
    H.write_pgm(rp, r)
    o1, o2 = str(tmp_path / "d1.f32"), str(tmp_path / "d2.f32")
    subprocess.check_call([os.path.join(H.ROOT, "tests", "cxx", "elas_dropin"), lp, rp, "demo", o1, o2])
    assert_final(z, np.fromfile(o1, np.float32), np.fromfile(o2, np.float32), pair)


@pytest.mark.parametrize("name", MONO_SETS)
def test_mono_sequence_with_taps(name, S):
    """pushBack(I1_k) + matchFeatures(0) over the seven frames, stage taps on"""
    z, prm = mono_params(name)
    m = H.ProductMatcher(prm)
    for k, img in enumerate(H.mono_frames()):
        m.push_back(img)
        if k:
            assert m.match(0) == 0
            check_mono_step(z, m, k, m.matches())


def test_mono_sequence_without_taps(S):
    """the latency path (no taps) on the default parameters"""
    z, prm = mono_params("default")
    m = plain_matcher(prm)
    for k, img in enumerate(H.mono_frames()):
        m.push_back(img)
        if k:
            assert m.match(0) == 0
            check_mono_step(z, m, k, m.matches())


def plain_matcher(prm):
    """a Matcher as an application makes it: no stage taps (taps also send the batch entries one by one)"""
    m = H.ProductMatcher(prm)
    m.lib.svh_matcher_set_taps(C.c_void_p(m.h), 0)
    return m


def test_mono_lockstep_batch(S):
    """three mono objects started at frames 0 / 1 / 2 advanced together (svh_matcher_*_batch, no right images):
    each one equals its own golden steps.  Same parameters, same image size, taps off and no right image for any of
    them: the conditions under which both batch entries run the K objects in lockstep (matcher_engine.cpp) rather
    than one after the other"""
    z, prm = mono_params("default")
    frames = H.mono_frames()
    ms = [plain_matcher(prm) for _ in range(3)]
    for t in range(5):
        H.product_matcher_batch(ms, [frames[j + t] for j in range(3)], None, 0 if t else None)
        if t:
            for j, m in enumerate(ms):
                check_mono_step(z, m, j + t, m.matches())

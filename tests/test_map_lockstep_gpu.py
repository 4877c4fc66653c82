"""Map fusion for K maps in lockstep (svh_map_add_batch_device, csrc/map_kernels.hip): after every batch frame both
point lists and the five planes of EVERY map equal oracle/map_oracle.cpp's, in order and bit for bit -- at the tile, block
and scan-chunk sizes of tests/test_map_edges.py, with its hand-built cases as members of a batch, with maps in different
states and with different parameters in one call.  The lockstep counters show that a batch is at most two recorded
phases whatever K is; the argument and error contracts of include/svh_map.h are checked on the objects' state.  The
inputs of every case are proven on the oracle in tests/test_map_edges.py.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import lockstep_helpers as LH
import test_map as M
import test_map_edges as E

pytestmark = pytest.mark.gpu

BAD_ARG, ERR_HIP = -1, -2


@pytest.fixture(scope="module")
def S():
    import svhip
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    assert (svhip.ERR_BAD_ARG, svhip.ERR_HIP) == (BAD_ARG, ERR_HIP)
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    return svhip


@pytest.fixture(scope="module")
def RS(S):
    from svhip import resident
    return resident


@pytest.fixture(scope="module")
def hip():
    return LH.hip_runtime()


@pytest.fixture(autouse=True)
def disarm(S):
    yield
    S.lib().svh_test_fail_at(None)


def device_mapper(prm):
    from svhip import mapper
    return mapper.Mapper(*(float(v) for v in prm))


def named(case, name):
    case.name = name          # (run_oracle's cache is keyed by the name)
    return case


def synth_case(name, w, h, n, seed, prm=None, valid=0.8):
    (f, cu, cv, base), frames = M.synth_frames(w, h, n, seed, valid=valid)
    return E.Case(name, prm if prm is not None else (f, cu, cv, base, 20), frames)


def same_frame(want, g, tag):
    p0, p1, planes = want
    for which, a in ((0, p0), (1, p1)):
        b = g.points(which)
        assert a.shape == b.shape, (tag, which, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, which)
    got = g.planes()
    for k, name in enumerate("IDXYZ"):
        assert np.array_equal(planes[k].view(np.uint32), got[k].view(np.uint32)), (tag, name)


def batch_add(RS, hip, maps, frames, extra=0, odd=False, check=True):
    """one svh_map_add_batch_device call: frames[i] = (D1, I1, H_total, gain) of maps[i]; the images at pitch w + extra
    and, with `odd`, at byte offset 2 i + 1 of their allocation"""
    h, w = frames[0][1].shape
    held, dD, dI = [], [], []
    for i, (d, img, _, _) in enumerate(frames):
        a = LH.Dev(hip, np.ascontiguousarray(d, np.float32))
        b, addr = LH.on_device(hip, img, w + extra, 2 * i + 1 if odd else 0)
        held += [a, b]
        dD.append(a.addr)
        dI.append(addr)
    return RS.map_add_batch(maps, dD, dI, w, h, [f[2] for f in frames], [f[3] for f in frames], pitch=w + extra,
                            check=check)


def run_batch(RS, hip, oracle_lib, cases, extra=0, odd=False, maps=None):
    """the cases frame by frame, one batch call per frame index (a case with fewer frames leaves the batch when it is
    through); every map against the oracle after every call"""
    want = [E.run_oracle(oracle_lib, c) for c in cases]
    maps = maps or [device_mapper(c.prm) for c in cases]
    for k in range(max(len(c.frames) for c in cases)):
        live = [i for i, c in enumerate(cases) if k < len(c.frames)]
        batch_add(RS, hip, [maps[i] for i in live], [cases[i].frames[k] for i in live], extra, odd)
        for i in live:
            same_frame(want[i][k], maps[i], (cases[i].name, k))
    return maps


# ---- sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (65, 5), (32, 32), (41, 25), (1023, 1), (33, 65)])
def test_batch_at_tile_and_block_edges(RS, hip, oracle_lib, w, h):
    cases = [named(E.size_case(w, h, seed=11 + i), "lockstep_size_%dx%d_%d" % (w, h, i)) for i in range(3)]
    c = LH.Counts(RS)
    run_batch(RS, hip, oracle_lib, cases)
    flushed, fallback, launches = c.delta()
    assert (flushed, fallback) == (2, 0)          # frame 0: three maps start; frame 1: three maps fuse
    assert launches == 4 + 9                      # create, count, scan, scatter; + project, fuse, count, scan, scatter


def test_batch_scan_carry(RS, hip, oracle_lib):
    """1025 x 1024: 1025 scan-order blocks, one carry of k_map_scan_b into its one-element second chunk, per job"""
    cases = [E.chunk_case(1025, 1024),            # (name and content of test_map_edges_gpu's case: one oracle run)
             named(E.size_case(1025, 1024, seed=17, valid=0.5), "lockstep_chunk_1025x1024_1")]
    run_batch(RS, hip, oracle_lib, cases)


# ---- hand-built cases as members of a batch ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", "nonfinite", "gain"])
def test_hand_case_beside_two_ordinary_maps(RS, hip, oracle_lib, name):
    hand = E.HAND_CASES[name]()
    n = len(hand.frames)
    cases = [synth_case("lockstep_beside_%s_0" % name, E.W, E.HH, n, seed=31),
             hand,
             synth_case("lockstep_beside_%s_2" % name, E.W, E.HH, n, seed=32)]
    run_batch(RS, hip, oracle_lib, cases, extra=13, odd=True)


# ---- maps in different states, with different parameters ---------------------------------------------------------------
def test_first_frame_cleared_and_continuing_in_one_call(RS, hip, oracle_lib):
    w, h = 65, 33
    L = M.oracle_map(oracle_lib)
    sets = [M.synth_frames(w, h, 3, seed=41 + i) for i in range(3)]
    prm = sets[0][0] + (np.float32(20),)
    fr = [s[1] for s in sets]
    orc = [M.OracleMapper(L, M.MapParams(*prm)) for _ in range(3)]
    maps = [device_mapper(prm) for _ in range(3)]
    # map 1 has two frames behind it, map 2 one; map 0 none
    batch_add(RS, hip, maps[1:], [fr[1][0], fr[2][0]])
    batch_add(RS, hip, maps[1:2], [fr[1][1]])             # (K = 1: the single entry)
    for k, i in ((0, 1), (1, 1), (0, 2)):
        orc[i].add(*fr[i][k])
    maps[1].clear()
    orc[1].clear()
    c = LH.Counts(RS)
    batch_add(RS, hip, maps, [fr[0][0], fr[1][2], fr[2][1]], extra=13, odd=True)
    flushed, fallback, launches = c.delta()
    assert (flushed, fallback, launches) == (2, 0, 9 + 4)
    for i, k in ((0, 0), (1, 2), (2, 1)):
        orc[i].add(*fr[i][k])
        same_frame((orc[i].points(0), orc[i].points(1), orc[i].planes()), maps[i], ("mixed", i))
    assert len(orc[0].points(0)) == 0 and len(orc[1].points(0)) == 0 and len(orc[2].points(0)) > 0
    # ... and all three continue
    batch_add(RS, hip, maps, [fr[0][1], fr[1][0], fr[2][2]])
    for i, k in ((0, 1), (1, 0), (2, 2)):
        orc[i].add(*fr[i][k])
        same_frame((orc[i].points(0), orc[i].points(1), orc[i].planes()), maps[i], ("mixed, next", i))
        assert len(orc[i].points(0)) > 0


def test_launches_do_not_grow_with_K(RS, hip, oracle_lib):
    seen = {}
    for K in (2, 5):
        cases = [synth_case("lockstep_K_%d" % i, 41, 25, 2, seed=51 + i) for i in range(K)]
        maps = [device_mapper(c.prm) for c in cases]
        batch_add(RS, hip, maps, [c.frames[0] for c in cases])
        c = LH.Counts(RS)
        batch_add(RS, hip, maps, [c_.frames[1] for c_ in cases])
        seen[K] = c.delta()
        for i, case in enumerate(cases):
            same_frame(E.run_oracle(oracle_lib, case)[1], maps[i], (K, i))
    assert seen[2] == seen[5] == (1, 0, 9)


def test_maps_with_different_parameters_in_one_batch(RS, hip, oracle_lib):
    (f, cu, cv, base), _ = M.synth_frames(41, 25, 1, seed=0)
    prms = [(f, cu, cv, base, 20), (f * np.float32(1.25), cu + 2, cv - 1, base, 6), (f, cu, cv, base * np.float32(0.5), 9)]
    cases = [synth_case("lockstep_params_%d" % i, 41, 25, 3, seed=61 + i, prm=p) for i, p in enumerate(prms)]
    want = [E.run_oracle(oracle_lib, c) for c in cases]
    assert len({len(w[2][1]) for w in want}) == 3          # (the parameters matter: three different maps)
    run_batch(RS, hip, oracle_lib, cases, extra=13, odd=True)


# ---- contracts ---------------------------------------------------------------------------------------------------------
def raw_call(RS, maps, dD, dI, dims, Hs, gain, K=None):
    L = RS._bind()
    tab = lambda xs: None if xs is None else (C.c_void_p * len(xs))(*xs)
    return L.svh_map_add_batch_device(tab(None if maps is None else [m if m is None else m._h for m in maps]),
                                      len(maps) if K is None else K, tab(dD), tab(dI),
                                      None if dims is None else (C.c_int32 * 3)(*dims), tab(Hs),
                                      None if gain is None else gain.ctypes.data)


def test_argument_errors_leave_the_objects_unchanged(S, RS, hip, oracle_lib):
    cases = [synth_case("lockstep_args_%d" % i, 33, 17, 3, seed=71 + i) for i in range(2)]
    want = [E.run_oracle(oracle_lib, c) for c in cases]
    maps = [device_mapper(c.prm) for c in cases]
    batch_add(RS, hip, maps, [c.frames[0] for c in cases])
    batch_add(RS, hip, maps, [c.frames[1] for c in cases])
    w, h = 33, 17
    d = [LH.Dev(hip, c.frames[2][0]) for c in cases]
    im = [LH.Dev(hip, c.frames[2][1]) for c in cases]
    Hk = [np.ascontiguousarray(c.frames[2][2], np.float64) for c in cases]
    dD, dI, Hs = [x.addr for x in d], [x.addr for x in im], [x.ctypes.data for x in Hk]
    g = np.zeros(2, np.float32)
    ok_dims = (w, h, w)
    bad = [
        (None, dD, dI, ok_dims, Hs, g, 2), (maps, None, dI, ok_dims, Hs, g, None), (maps, dD, None, ok_dims, Hs, g, None),
        (maps, dD, dI, None, Hs, g, None), (maps, dD, dI, ok_dims, None, g, None), (maps, dD, dI, ok_dims, Hs, None, None),
        ([maps[0], None], dD, dI, ok_dims, Hs, g, None), (maps, [dD[0], None], dI, ok_dims, Hs, g, None),
        (maps, dD, [None, dI[1]], ok_dims, Hs, g, None), (maps, dD, dI, ok_dims, [Hs[0], None], g, None),
        ([maps[0], maps[0]], dD, dI, ok_dims, Hs, g, None), (maps, dD, dI, ok_dims, Hs, g, -1),
        (maps, dD, dI, (0, h, w), Hs, g, None), (maps, dD, dI, (w, 0, w), Hs, g, None),
        (maps, dD, dI, (w, h, w - 1), Hs, g, None), (maps, dD, dI, (1 << 15, 1 << 14, 1 << 15), Hs, g, None),
    ]
    for k, args in enumerate(bad):
        assert raw_call(RS, *args) == BAD_ARG, k
        assert S.last_error() != "", k
    assert raw_call(RS, maps, dD, dI, ok_dims, Hs, g, 0) == 0          # K = 0
    for i in range(2):
        same_frame(want[i][1], maps[i], ("after the refused calls", i))
    batch_add(RS, hip, maps, [c.frames[2] for c in cases])              # ... and the maps fuse on
    for i in range(2):
        same_frame(want[i][2], maps[i], ("frame 2", i))
        assert len(want[i][2][0]) > 0


def test_batch_and_single_calls_interleaved(RS, hip, oracle_lib):
    cases = [synth_case("lockstep_interleaved_%d" % i, 65, 33, 4, seed=81 + i) for i in range(3)]
    want = [E.run_oracle(oracle_lib, c) for c in cases]
    maps = [device_mapper(c.prm) for c in cases]
    for k in range(4):
        if k % 2 == 0:
            batch_add(RS, hip, maps, [c.frames[k] for c in cases])
        else:
            for m, c in zip(maps, cases):
                m.add(*c.frames[k])
        for i in range(3):
            same_frame(want[i][k], maps[i], ("interleaved", k, i))


def test_view_add_map_after_a_batch_frame(RS, hip):
    from svhip import view
    cases = [synth_case("lockstep_view_%d" % i, 65, 33, 2, seed=91 + i) for i in range(2)]
    bat = [device_mapper(c.prm) for c in cases]
    one = [device_mapper(c.prm) for c in cases]
    vb, vo = [view.View(64, 48) for _ in cases], [view.View(64, 48) for _ in cases]
    for k in range(2):
        batch_add(RS, hip, bat, [c.frames[k] for c in cases])
        for i, c in enumerate(cases):
            one[i].add(*c.frames[k])
            vb[i].add_map(bat[i])
            vo[i].add_map(one[i])
            for what in (view.POINTS, view.LISTS):
                assert vb[i].count(what) == vo[i].count(what) and vo[i].count(what) > 0, (k, i, what)
    for i in range(2):
        assert vb[i].render().tobytes() == vo[i].render().tobytes(), i


# ---- injected HIP errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["copy:1", "copy:2", "wait:1", "wait:2"])
def test_injected_failure_then_the_same_call_again(S, RS, hip, oracle_lib, spec, capfd):
    """svh_test_fail_at makes the guard report a failed call (the job-table copy or the wait of the first or the second
    recorded phase); nothing faults on the device.  SVH_ERR_HIP, no object has taken the frame, and the same call repeated
    gives the oracle's result"""
    cases = [synth_case("lockstep_fault_%d" % i, 41, 25, 2, seed=101 + i) for i in range(3)]
    want = [E.run_oracle(oracle_lib, c) for c in cases]
    maps = [device_mapper(c.prm) for c in cases]
    batch_add(RS, hip, maps[:2], [c.frames[0] for c in cases[:2]])
    frames = [cases[0].frames[1], cases[1].frames[1], cases[2].frames[0]]      # two maps fuse, one starts
    before = [(len(m.points(0)), len(m.points(1))) for m in maps]
    assert S.lib().svh_test_fail_at(spec.encode()) == 0
    capfd.readouterr()
    assert batch_add(RS, hip, maps, frames, check=False) == ERR_HIP
    S.lib().svh_test_fail_at(None)
    assert "injected failure" in S.last_error()
    assert capfd.readouterr().err.count("svhip:") == 1
    assert [(len(m.points(0)), len(m.points(1))) for m in maps] == before
    c = LH.Counts(RS)
    batch_add(RS, hip, maps, frames)
    assert c.delta() == (2, 0, 13)
    for i, k in ((0, 1), (1, 1), (2, 0)):
        same_frame(want[i][k], maps[i], (spec, i))

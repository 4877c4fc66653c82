"""GPU: the map fusion (include/svh_map.h, csrc/map_kernels.hip) at the sizes, thresholds and orders that
tests/test_map_edges.py builds and proves on the oracle, plus the accessor and argument contracts of the C-ABI.

The comparison is test_fusion_matches_oracle's: after every frame both point lists equal oracle/map_oracle.cpp's in
order and bit for bit, and so do the five planes.  No tolerance anywhere."""
import ctypes as C
import threading

import numpy as np
import pytest

import test_map as M
import test_map_edges as E

pytestmark = pytest.mark.gpu

BAD_ARG = -1
GUARD = np.float32(-12345.5)


def device_mapper(prm):
    from svhip import mapper
    return mapper.Mapper(*prm)


def same_frame(want, g, tag):
    p0, p1, planes = want
    for which, a in ((0, p0), (1, p1)):
        b = g.points(which)
        assert a.shape == b.shape, (tag, which, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, which)
    got = g.planes()
    for k, name in enumerate("IDXYZ"):
        assert np.array_equal(planes[k].view(np.uint32), got[k].view(np.uint32)), (tag, name)


def run_case(case, oracle_lib, g=None):
    want = E.run_oracle(oracle_lib, case)
    g = g or device_mapper(case.prm)
    for k, (d, img, Ht, gain) in enumerate(case.frames):
        g.add(d, img, Ht, gain)
        same_frame(want[k], g, (case.name, k))
    return g


# ---- A: block, tile and scan boundaries --------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", E.TILE_SIZES + E.BLOCK_SIZES)
def test_tile_and_block_edges(w, h, oracle_lib):
    """the 64 x 4 tiles of k_map_create with margins 0, 1, 2 and a portrait frame; 1023, 1024, 1025, 2047 and 2049
    pixels for the 1024-element blocks of k_map_count / k_map_scatter"""
    run_case(E.size_case(w, h), oracle_lib)


def test_empty_frame_then_last_block_only(oracle_lib):
    """no valid pixel: both lists empty, svh_map_points returns 0 and touches nothing; then valid pixels in the last
    scan-order block only; then an ordinary frame"""
    from svhip import mapper
    case = E.last_block_case()
    want = E.run_oracle(oracle_lib, case)
    g = device_mapper(case.prm)
    L = mapper._bind()
    d, img, Ht, gain = case.frames[0]
    g.add(d, img, Ht, gain)
    buf = np.full((8, 4), GUARD, np.float32)
    for which in (0, 1):
        assert L.svh_map_points(g._h, which, buf.ctypes.data, 8) == 0
        assert np.all(buf == GUARD)
    same_frame(want[0], g, (case.name, 0))
    for k in (1, 2):
        d, img, Ht, gain = case.frames[k]
        g.add(d, img, Ht, gain)
        same_frame(want[k], g, (case.name, k))


@pytest.mark.parametrize("w,h", E.CHUNK_SIZES)
def test_scan_chunks(w, h, oracle_lib):
    """k_map_scan: 1024 blocks = one chunk, 1025 = one carry into a one-element chunk, 2049 = two carries; these
    frames also have the 200-pixel cap of the gain margin"""
    run_case(E.chunk_case(w, h), oracle_lib)


def test_scan_total_from_the_second_chunk_alone(oracle_lib):
    run_case(E.second_chunk_only_case(), oracle_lib)


# ---- B: thresholds, borders, order, odd values ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.HAND_CASES))
def test_hand_built_case(name, oracle_lib):
    """what each case reaches is asserted on the oracle in tests/test_map_edges.py"""
    run_case(E.HAND_CASES[name](), oracle_lib)


# ---- D: contract ---------------------------------------------------------------------------------------------------------
def test_another_size_starts_a_new_reconstruction(oracle_lib):
    """96x64 -> 64x96 -> 64x96: the change of size is a svh_map_clear (the oracle is cleared there by hand: it would
    fuse across sizes), the third frame fuses again"""
    (f, cu, cv, base), a = M.synth_frames(96, 64, 1, seed=21)
    _, b = M.synth_frames(64, 96, 3, seed=22)
    prm = M.MapParams(f, cu, cv, base, 20)
    o = M.OracleMapper(M.oracle_map(oracle_lib), prm)
    g = device_mapper((f, cu, cv, base, 20))
    for k, (d, img, Ht, gain) in enumerate([a[0], b[1], b[2]]):
        if k == 1:
            o.clear()
        o.add(d, img, Ht, gain)
        g.add(d, img, Ht, gain)
        same_frame((o.points(0), o.points(1), o.planes()), g, ("resize", k))
        assert (len(o.points(0)) > 0) == (k == 2)


def test_clear_on_the_device(oracle_lib):
    """add, clear, add == a fresh object's first frame; list 0 is empty; the frame after fuses with that one only"""
    (f, cu, cv, base), fr = M.synth_frames(96, 64, 3, seed=23)
    o = M.OracleMapper(M.oracle_map(oracle_lib), M.MapParams(f, cu, cv, base, 20))
    g = device_mapper((f, cu, cv, base, 20))
    g.add(*fr[0])
    g.add(*fr[1])
    assert len(g.points(0)) > 0
    g.clear()
    assert len(g.points(0)) == 0 and len(g.points(1)) == 0
    for k in (2, 1):
        o.add(*fr[k])
        g.add(*fr[k])
        same_frame((o.points(0), o.points(1), o.planes()), g, ("clear", k))
        assert (len(o.points(0)) == 0) == (k == 2)


def test_points_accessor_caps(oracle_lib):
    from svhip import mapper
    L = mapper._bind()
    case = E.size_case(65, 5)
    want = E.run_oracle(oracle_lib, case)
    g = run_case(case, oracle_lib)
    for which in (0, 1, 7):
        full = want[-1][1 if which else 0]
        n = len(full)
        assert n > 3
        assert L.svh_map_points(g._h, which, None, 0) == n and L.svh_map_points(g._h, which, None, n) == n
        for cap in (n - 1, 1, 0, n, n + 5):
            buf = np.full((n + 8, 4), GUARD, np.float32)
            assert L.svh_map_points(g._h, which, buf.ctypes.data, cap) == n
            k = min(n, cap)
            assert np.array_equal(buf[:k].view(np.uint32), full[:k].view(np.uint32)), (which, cap)
            assert np.all(buf[k:] == GUARD), (which, cap)


def test_planes_accessor_contract(oracle_lib):
    import svhip as S
    from svhip import mapper
    L = mapper._bind()
    case = E.size_case(65, 5)
    g = device_mapper(case.prm)
    n = 65 * 5
    buf = np.full(5 * n + 8, GUARD, np.float32)
    assert L.svh_map_planes(g._h, buf.ctypes.data, 5 * n) == BAD_ARG == S.ERR_BAD_ARG       # no frame yet
    d, img, Ht, gain = case.frames[0]
    g.add(d, img, Ht, gain)
    assert L.svh_map_planes(g._h, buf.ctypes.data, 5 * n - 1) == BAD_ARG
    assert L.svh_map_planes(g._h, None, 5 * n) == BAD_ARG
    assert np.all(buf == GUARD)
    assert L.svh_map_planes(g._h, buf.ctypes.data, 5 * n) == 0
    want = E.run_oracle(oracle_lib, case)[0][2]
    assert np.array_equal(buf[:5 * n].view(np.uint32), want.ravel().view(np.uint32)) and np.all(buf[5 * n:] == GUARD)
    g.clear()
    assert L.svh_map_planes(g._h, buf.ctypes.data, 5 * n) == BAD_ARG                         # forgotten


def test_add_refuses_bad_arguments_and_goes_on(oracle_lib):
    from svhip import mapper
    L = mapper._bind()
    case = E.size_case(65, 5)
    want = E.run_oracle(oracle_lib, case)
    g = device_mapper(case.prm)
    d, img, Ht, gain = case.frames[0]
    g.add(d, img, Ht, gain)
    same_frame(want[0], g, "before")
    d = np.ascontiguousarray(d, np.float32)
    img = np.ascontiguousarray(img, np.uint8)
    Hc = np.ascontiguousarray(Ht, np.float64)

    def add(dims, Dp=d.ctypes.data, Ip=img.ctypes.data, Hp=Hc.ctypes.data):
        return L.svh_map_add(g._h, Dp, 0, Ip, (C.c_int32 * 3)(*dims) if dims else None, Hp, gain)

    assert add((0, 5, 65)) == BAD_ARG
    assert add((65, 0, 65)) == BAD_ARG
    assert add((65, 5, 64)) == BAD_ARG                    # step = w - 1
    assert add((1, 2 ** 28 + 1, 1)) == BAD_ARG            # refused before anything is read: the buffers are tiny
    assert add((65, 5, 65), Hp=None) == BAD_ARG
    assert add((65, 5, 65), Dp=None) == BAD_ARG
    assert add((65, 5, 65), Ip=None) == BAD_ARG
    assert add(None) == BAD_ARG
    same_frame(want[0], g, "after the refusals")
    d, img, Ht, gain = case.frames[1]
    g.add(d, img, Ht, gain)
    same_frame(want[1], g, "next good frame")


def test_two_objects_in_two_threads(oracle_lib):
    """each object has its own stream and buffers: two 4-frame 322 x 117 sequences run side by side, every frame of
    each equal to the oracle's for its sequence"""
    seqs = [M.synth_frames(322, 117, 4, seed=s) for s in (31, 32)]
    wants = [E.run_oracle(oracle_lib, E.Case("thread_seq_%d" % i, prm + (20,), fr)) for i, (prm, fr) in enumerate(seqs)]
    objs = [device_mapper(prm + (20,)) for prm, _ in seqs]
    gots, errs = [[], []], []
    barrier = threading.Barrier(2)

    def work(i):
        try:
            barrier.wait(timeout=30)
            for d, img, Ht, gain in seqs[i][1]:
                objs[i].add(d, img, Ht, gain)
                gots[i].append((objs[i].points(0), objs[i].points(1), objs[i].planes()))
        except Exception as e:      # noqa: BLE001 -- reported by the assert below
            errs.append((i, repr(e)))

    ts = [threading.Thread(target=work, args=(i,)) for i in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in (0, 1):
        assert len(gots[i]) == 4
        for k in range(4):
            for a, b in zip(wants[i][k], gots[i][k]):
                assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, k)
        assert len(wants[i][3][0]) > 0
    assert not np.array_equal(wants[0][3][2], wants[1][3][2])

"""GPU: the group feed of the ELAS engine's batch entries (stereo-vision_amd/csrc/group_feed.h, batch_impl and the lane
pool in elas_engine.cpp).  Lanes keep the parity they were created with, a worker draws its groups on demand and
refills whichever of its two lanes is free first; SVH_FEED (a bit set, read per call) brings back each of the three
earlier behaviours.  None of it may show in a result: statuses and maps are addressed by the group index.

The setup is that of test_queue_plan_gpu.py: 640 x 240, the committed urban3 crop and seeded synthetic pairs, every one
different (a lane refilled too early, or a group written to another group's place, shows as a wrong map), 2 pairs per
launch on 3 workers, device stage, outputs preset to a sentinel.
  * SVH_FEED=0 against SVH_FEED=7, bit for bit in maps and statuses, with svh_elas_trim between the two: the
    device-resident batch entry, the host-buffer batch entry with and without postprocess_only_left, for n = 36, 35
    (a last group of one pair), 2 (a lone group), 4 (fewer groups than workers) and 8 (one group more than lanes);
    and a stream of 12 pairs;
  * two pairs without texture among the 36 (17 and 34: fewer than three support points on the CPU oracle) get
    SVH_ERR_FEW_SUPPORT at exactly their indices and keep the sentinel; every other map is that of the clean run;
  * after four batch calls with a single call in between the pool holds 2 x workers lanes and, under plan 4, workers
    streams in each of two classes (plan 0: 2 x workers in one), the same after call 2 and after call 4;
  * the groups the workers took sum to the groups of the call."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

W, HGT, N, GROUP, WORKERS = 640, 240, 36, 2, 3
SENTINEL = -7.0
SIZES = [36, 35, 2, 4, 8]
FEW_SUPPORT = 1


@contextlib.contextmanager
def feed(bits):
    old = os.environ.get("SVH_FEED")
    os.environ["SVH_FEED"] = str(bits)
    try:
        yield
    finally:
        if old is None:
            del os.environ["SVH_FEED"]
        else:
            os.environ["SVH_FEED"] = old


@pytest.fixture(scope="module")
def S():
    import svhip as S
    S.lib()
    assert S.device_count() > 0, "no HIP device: the product has no CPU fallback"
    before = S.elas_settings()
    S.trim()
    S.set_group(GROUP)
    S.set_lanes(WORKERS)
    S.set_stage(1)
    yield S
    S.set_queue_plan(-1)
    S.set_stage(before["stage"])
    S.set_lanes(before["workers"])
    S.set_group(before["pairs_per_launch"] if before["pairs_per_launch"] > 0 else 32)
    S.trim()


@pytest.fixture(scope="module")
def pairs():
    l, r = H.golden_pair("urban3_640x240")
    assert l.shape == (HGT, W)
    ls, rs = [l], [r]
    for i in range(1, N):
        a, b = H.synth_pair(W, HGT, 400 + i)
        ls.append(a)
        rs.append(b)
    I1, I2 = np.ascontiguousarray(np.stack(ls)), np.ascontiguousarray(np.stack(rs))
    assert len({a.tobytes() for a in I1}) == N
    return I1, I2


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(scope="module")
def dev(hip, S):
    """room for 36 pairs and their maps in device memory"""
    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p
    d = dict(I1=alloc(N * W * HGT), I2=alloc(N * W * HGT), D1=alloc(N * W * HGT * 4), D2=alloc(N * W * HGT * 4))
    yield d
    for p in d.values():
        hip.hipFree(p)


def run_device(S, hip, dev, pairs, prm, n):
    fill = np.full((n, HGT, W), SENTINEL, np.float32)
    for k, a in (("I1", pairs[0][:n]), ("I2", pairs[1][:n]), ("D1", fill), ("D2", fill)):
        a = np.ascontiguousarray(a)
        assert hip.hipMemcpy(dev[k], C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    st = (C.c_int32 * n)(*([99] * n))
    e = S.Elas(prm)
    rc = S.lib().svh_elas_process_batch_device(e._h, n, dev["I1"], dev["I2"], W * HGT, dev["D1"], dev["D2"],
                                               W * HGT * 4, (C.c_int32 * 3)(W, HGT, W), st)
    assert rc >= 0, S.last_error()
    D1, D2 = np.empty_like(fill), np.empty_like(fill)
    assert hip.hipMemcpy(C.c_void_p(D1.ctypes.data), dev["D1"], C.c_size_t(D1.nbytes), 2) == 0
    assert hip.hipMemcpy(C.c_void_p(D2.ctypes.data), dev["D2"], C.c_size_t(D2.nbytes), 2) == 0
    return list(st), D1, D2


def run_host(S, pairs, prm, n):
    I1, I2 = pairs
    D1 = np.full((n, HGT, W), SENTINEL, np.float32)
    D2 = np.full((n, HGT, W), SENTINEL, np.float32)
    arr = C.c_void_p * n
    ptrs = [arr(*[a[i].ctypes.data for i in range(n)]) for a in (I1, I2, D1, D2)]
    st = (C.c_int32 * n)(*([99] * n))
    e = S.Elas(prm)
    rc = S.lib().svh_elas_process_batch(e._h, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], (C.c_int32 * 3)(W, HGT, W), st)
    assert rc >= 0, S.last_error()
    return list(st), D1, D2


def run_stream(S, pairs, prm, n=12):
    I1, I2 = pairs
    D1 = np.full((n, HGT, W), SENTINEL, np.float32)
    D2 = np.full((n, HGT, W), SENTINEL, np.float32)
    s = S.Elas(prm).stream(W, HGT)
    for i in range(n):
        assert s.push(I1[i], I2[i], D1[i], D2[i]) == i
    got = [s.pop() for _ in range(n)]
    s.close()
    assert [t for t, _ in got] == list(range(n))
    return [st for _, st in got], D1, D2


def same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for k in (1, 2):
        diff = [i for i in range(len(a[k])) if not np.array_equal(a[k][i].view(np.uint32), b[k][i].view(np.uint32))]
        assert not diff, (what, "D%d of pairs" % k, diff)


def ab(S, fn, what):
    """the entry under SVH_FEED=7 (everything as before the feed) and under the default, lanes rebuilt in between"""
    S.trim()
    with feed(7):
        old = fn()
        stats_old = S.feed_stats()
    assert S.trim() > 0
    with feed(0):
        new = fn()
        stats_new = S.feed_stats()
    assert set(old[0]) == {0}, (what, old[0])
    for D in old[1:]:
        assert (D != SENTINEL).all() and (D >= 0).mean() > 0.1, what
    same(new, old, what)
    return stats_old, stats_new


def groups_counted_once(stats, n, what):
    ngroups = (n + GROUP - 1) // GROUP
    for st in stats:
        assert st["groups"] == ngroups and st["workers"] == min(WORKERS, ngroups), (what, st)
        assert sum(st["taken"]) == ngroups and all(t >= 1 for t in st["taken"]), (what, st)
        assert all(0 < us <= st["call_us"] for us in st["finish_us"]), (what, st)


@pytest.mark.parametrize("n", SIZES)
def test_device_resident_batch_equals_the_earlier_feed(S, hip, dev, pairs, n):
    prm = H.robotics()
    S.set_queue_plan(-1)
    stats = ab(S, lambda: run_device(S, hip, dev, pairs, prm, n), ("device batch", n))
    groups_counted_once(stats, n, ("device batch", n))


@pytest.mark.parametrize("only_left", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_host_buffer_batch_equals_the_earlier_feed(S, pairs, n, only_left):
    prm = H.robotics(postprocess_only_left=only_left)        # 1: the right map is final after the L/R check
    S.set_queue_plan(-1)
    stats = ab(S, lambda: run_host(S, pairs, prm, n), ("host batch", n, only_left))
    groups_counted_once(stats, n, ("host batch", n, only_left))


def test_stream_of_12_pairs_equals_the_earlier_feed(S, pairs):
    prm = H.robotics()
    S.set_queue_plan(-1)
    ab(S, lambda: run_stream(S, pairs, prm), "stream")


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_each_switch_on_its_own(S, hip, dev, pairs, bits):
    """(every one of the three earlier behaviours alone, against all three: the device-resident entry, 35 pairs)"""
    prm = H.robotics()
    S.set_queue_plan(-1)
    S.trim()
    with feed(7):
        want = run_device(S, hip, dev, pairs, prm, 35)
    S.trim()
    with feed(bits):
        got = run_device(S, hip, dev, pairs, prm, 35)
        stats = S.feed_stats()
    same(got, want, ("SVH_FEED", bits))
    groups_counted_once([stats], 35, ("SVH_FEED", bits))
    if bits & 2:
        assert stats["taken"] == [len(range(w, 18, WORKERS)) for w in range(WORKERS)], stats


def test_status_lands_at_the_index_of_its_pair(S, hip, dev, pairs):
    prm = H.robotics()
    flat = np.full((HGT, W), 90, np.uint8)
    tri = None if H.have_ref_elas() else H.fixture_triangulator([])
    want = H.oracle_elas_run(prm, flat, flat, tri)
    nsup = len(want.stages[H.SUPPORT]) // 3 if H.SUPPORT in want else 0
    assert nsup < 3 and want.status == FEW_SUPPORT, (nsup, want.status)
    S.set_queue_plan(-1)
    S.trim()
    clean = run_device(S, hip, dev, pairs, prm, N)
    assert set(clean[0]) == {0}
    I1, I2 = pairs[0].copy(), pairs[1].copy()
    bad = (17, 34)
    for i in bad:
        I1[i] = flat
        I2[i] = flat
    for bits in (0, 7):
        S.trim()
        with feed(bits):
            for st, D1, D2 in (run_device(S, hip, dev, (I1, I2), prm, N), run_host(S, (I1, I2), prm, N)):
                assert [i for i in range(N) if st[i] != 0] == list(bad), (bits, st)
                assert all(st[i] == FEW_SUPPORT for i in bad), (bits, st)
                for i in range(N):
                    for D, C0 in ((D1, clean[1]), (D2, clean[2])):
                        if i in bad:
                            assert (D[i] == SENTINEL).all(), (bits, i, "outputs of a pair without support are untouched")
                        else:
                            assert np.array_equal(D[i].view(np.uint32), C0[i].view(np.uint32)), (bits, i)


@pytest.mark.parametrize("plan", [4, 0])
def test_lanes_and_streams_stay_fixed(S, hip, dev, pairs, plan):
    prm = H.robotics()
    least, greatest = C.c_int(0), C.c_int(0)
    assert hip.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest)) == 0
    S.trim()
    assert S.set_queue_plan(plan) == plan
    assert S.trim() == 0
    two_classes = plan == 4 and least.value > 0          # (a device without a low class folds it into normal)
    assert S.queue_plan()["classes"] == (2 if two_classes else 1)
    seen = []
    with feed(0):
        for call in range(4):
            st, _, _ = run_device(S, hip, dev, pairs, prm, N)
            assert set(st) == {0}
            if call == 1:
                rc, _, _ = S.Elas(prm).process(pairs[0][0], pairs[1][0])
                assert rc == 0
            if call in (1, 3):
                seen.append(S.feed_stats())
    for st in seen:
        assert st["lanes"] == 2 * WORKERS, st
        if two_classes:
            assert st["streams"] == dict(normal=WORKERS, high=0, low=WORKERS), st
        else:
            assert st["streams"] == dict(normal=2 * WORKERS, high=0, low=0), st
        assert sum(st["taken"]) == N // GROUP == st["groups"], st
    assert (seen[0]["lanes"], seen[0]["streams"]) == (seen[1]["lanes"], seen[1]["streams"])
    S.set_queue_plan(-1)

"""GPU: the queue plans of the ELAS engine (svh_elas_set_queue_plan, stereo-vision_amd/csrc/queue_plan.h) move the
phases of a pipelined group onto streams of other priority classes; they must never show in a result.

36 pairs of 640 x 240 -- the committed urban3 crop and 35 seeded synthetic pairs, every one different, so that a
buffer read too early or too late (the lane's next group starting on what the last one still reads, phase B starting
before the stage chain has written its lists) shows as a wrong map -- run at 2 pairs per launch on 3 workers: 18
groups, three for each of the six lanes.  Outputs start from a sentinel.  For plans 1 to 4, three repetitions
each, with svh_elas_trim between plans (lanes are built with the plan in force when they are created):
  * the device-resident batch entry, the host-buffer batch entry with and without postprocess_only_left, and a stream
    of 12 pairs give the maps and statuses of plan 0, bit for bit;
  * a single call of the urban3 pair equals the CPU oracle (the reference's triangulation where oracle/_ref is built);
  * svh_elas_get_queue_plan reports what was set;
  * the per-kernel timer lists the same kernels, as often, as under plan 0: every kernel of a group once per group."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

W, HGT, N, GROUP, WORKERS, REPS = 640, 240, 36, 2, 3, 3
SENTINEL = -7.0


@pytest.fixture(scope="module")
def S():
    import svhip as S
    S.lib()
    assert S.device_count() > 0, "no HIP device: the product has no CPU fallback"
    before = S.elas_settings()
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
def dev(hip, pairs, S):
    """the 36 pairs and their maps in device memory"""
    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p
    I1, I2 = pairs
    d = dict(I1=alloc(I1.nbytes), I2=alloc(I2.nbytes), D1=alloc(N * W * HGT * 4), D2=alloc(N * W * HGT * 4))
    for k, a in (("I1", I1), ("I2", I2)):
        assert hip.hipMemcpy(d[k], C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    yield d
    for p in d.values():
        hip.hipFree(p)


def use_plan(S, plan):
    S.trim()
    assert S.set_queue_plan(plan) == plan
    assert S.trim() == 0


def run_device(S, hip, dev, prm):
    fill = np.full((N, HGT, W), SENTINEL, np.float32)
    for k in ("D1", "D2"):
        assert hip.hipMemcpy(dev[k], C.c_void_p(fill.ctypes.data), C.c_size_t(fill.nbytes), 1) == 0
    st = S.Elas(prm).process_batch_device(N, dev["I1"].value, dev["I2"].value, W * HGT, dev["D1"].value,
                                          dev["D2"].value, W * HGT * 4, W, HGT, W)
    D1, D2 = np.empty_like(fill), np.empty_like(fill)
    assert hip.hipMemcpy(C.c_void_p(D1.ctypes.data), dev["D1"], C.c_size_t(D1.nbytes), 2) == 0
    assert hip.hipMemcpy(C.c_void_p(D2.ctypes.data), dev["D2"], C.c_size_t(D2.nbytes), 2) == 0
    return st, D1, D2


def run_host(S, pairs, prm):
    I1, I2 = pairs
    D1 = np.full((N, HGT, W), SENTINEL, np.float32)
    D2 = np.full((N, HGT, W), SENTINEL, np.float32)
    arr = C.c_void_p * N
    ptrs = [arr(*[a[i].ctypes.data for i in range(N)]) for a in (I1, I2, D1, D2)]
    st = (C.c_int32 * N)(*([99] * N))
    e = S.Elas(prm)
    rc = S.lib().svh_elas_process_batch(e._h, N, ptrs[0], ptrs[1], ptrs[2], ptrs[3], (C.c_int32 * 3)(W, HGT, W), st)
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
    assert a[0] == b[0] and set(a[0]) == {0}, (what, a[0], b[0])
    for k in (1, 2):
        diff = [i for i in range(len(a[k])) if not np.array_equal(a[k][i].view(np.uint32), b[k][i].view(np.uint32))]
        assert not diff, (what, "D%d of pairs" % k, diff)


_base = {}


def base(S, key, fn):
    """the entry's result under plan 0, once per module"""
    if key not in _base:
        use_plan(S, 0)
        _base[key] = fn()
        again = fn()                                 # (plan 0 agrees with itself: the inputs decide, not the run)
        same(again, _base[key], (key, "plan 0 twice"))
        for D in _base[key][1:]:
            assert (D != SENTINEL).all() and (D >= 0).mean() > 0.1
    return _base[key]


PLANS = [1, 2, 3, 4]


@pytest.mark.parametrize("plan", PLANS)
def test_device_resident_batch_equals_plan_0(S, hip, dev, plan):
    prm = H.robotics()
    want = base(S, "device", lambda: run_device(S, hip, dev, prm))
    before = S.stage_stats()
    use_plan(S, plan)
    for rep in range(REPS):
        same(run_device(S, hip, dev, prm), want, ("device batch", plan, rep))
    after = S.stage_stats()
    assert after[0] - before[0] == REPS * N // GROUP and after[1] == before[1]      # every group on the device stage


@pytest.mark.parametrize("only_left", [1, 0])
@pytest.mark.parametrize("plan", PLANS)
def test_host_buffer_batch_equals_plan_0(S, pairs, plan, only_left):
    prm = H.robotics(postprocess_only_left=only_left)        # 1: the right map is final after the L/R check
    want = base(S, ("host", only_left), lambda: run_host(S, pairs, prm))
    use_plan(S, plan)
    for rep in range(REPS):
        same(run_host(S, pairs, prm), want, ("host batch", plan, only_left, rep))


@pytest.mark.parametrize("plan", PLANS)
def test_stream_of_12_pairs_equals_plan_0(S, pairs, plan):
    prm = H.robotics()
    want = base(S, "stream", lambda: run_stream(S, pairs, prm))
    use_plan(S, plan)
    for rep in range(REPS):
        same(run_stream(S, pairs, prm), want, ("stream", plan, rep))


def test_stream_and_batches_agree_under_plan_0(S, hip, dev, pairs):
    """(the three entries are one pipeline: what the comparisons above rest on is one set of maps)"""
    prm = H.robotics()
    d = base(S, "device", lambda: run_device(S, hip, dev, prm))
    h = base(S, ("host", 1), lambda: run_host(S, pairs, prm))
    s = base(S, "stream", lambda: run_stream(S, pairs, prm))
    same(d, h, "device / host")
    same((s[0], s[1], s[2]), (h[0][:12], h[1][:12], h[2][:12]), "stream / host")


@pytest.fixture(scope="module")
def urban_want():
    z = np.load(os.path.join(H.GOLDEN, "urban3_demo.npz"))
    prm = H.ElasParams.from_buffer_copy(z["params"].tobytes())
    l, r = H.golden_pair(str(z["crop"]))
    tri = None if H.have_ref_elas() else H.fixture_triangulator([z["tri1"], z["tri2"]])
    return prm, l, r, H.oracle_elas_run(prm, l, r, tri)


@pytest.mark.parametrize("plan", [0, 1, 2, 3, 4])
def test_single_call_equals_the_reference(S, urban_want, plan):
    prm, l, r, want = urban_want
    use_plan(S, plan)
    D1 = np.full(l.shape, SENTINEL, np.float32)
    D2 = np.full(l.shape, SENTINEL, np.float32)
    rc, D1, D2 = S.Elas(prm).process(l, r, D1, D2)
    assert rc == 0 and want.status == 0
    assert np.array_equal(D1.ravel(), want[H.D1_FINAL]) and np.array_equal(D2.ravel(), want[H.D2_FINAL])


def test_get_queue_plan_reports_what_was_set(S, hip):
    least, greatest = C.c_int(0), C.c_int(0)
    assert hip.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest)) == 0
    levels = least.value - greatest.value + 1
    text = os.environ.get("GPU_MAX_HW_QUEUES", "")
    cap = int(text) if text.isdigit() and int(text) > 0 else 4
    use_plan(S, 0)
    assert S.queue_plan() == dict(plan=0, streams_per_lane=1, classes=1)
    exact = {1: dict(plan=1, streams_per_lane=2, classes=2), 2: dict(plan=2, streams_per_lane=2, classes=3),
             3: dict(plan=3, streams_per_lane=3, classes=3), 4: dict(plan=4, streams_per_lane=1, classes=2)}
    for plan in PLANS:
        use_plan(S, plan)
        got = S.queue_plan()
        if levels >= 3 and cap <= 4:             # three classes of at most 4 queues: always within the budget of 12
            assert got == exact[plan], (plan, got)
        else:                                    # fewer levels fold classes, a larger cap may exceed the budget
            assert got["plan"] in (plan, 0) and 1 <= got["streams_per_lane"] <= 3 and 1 <= got["classes"] <= levels
    assert S.set_queue_plan(-1) == -1 and S.set_queue_plan(7) == -1 and S.set_queue_plan(-5) == -1
    assert 0 <= S.queue_plan()["plan"] <= 4
    assert S.lib().svh_elas_get_queue_plan(None, None, None) == 0


def kernel_profile(S):
    L = S.lib()
    L.svh_profile_get.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    out = {}
    for i in range(L.svh_profile_get(-1, None, None, None)):
        name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
        assert L.svh_profile_get(i, C.byref(name), C.byref(ms), C.byref(cnt)) == 0
        out[name.value.decode()] = (cnt.value, ms.value)
    return out


def test_kernel_profile_lists_every_kernel_once_per_group_under_plan_2(S, hip, dev):
    prm = H.robotics()
    L = S.lib()
    L.svh_profile_only.argtypes = [C.c_char_p]
    prof = {}
    try:
        for plan in (0, 2):
            use_plan(S, plan)
            L.svh_profile_only(None)
            L.svh_profile_reset()
            L.svh_profile_enable(1)
            st, _, _ = run_device(S, hip, dev, prm)
            L.svh_profile_enable(0)
            assert set(st) == {0}
            prof[plan] = kernel_profile(S)
    finally:
        L.svh_profile_enable(0)
        L.svh_profile_reset()
    groups = N // GROUP
    counts = {p: {k: v[0] for k, v in prof[p].items()} for p in prof}
    print("launches per kernel, plan 0:", counts[0], "plan 2:", counts[2])
    assert counts[2] == counts[0], (counts[0], counts[2])
    for k in ("k_lattice_count", "k_lattice", "k_delaunay", "k_stage_pack"):
        assert counts[2][k] == groups, (k, counts[2])
    assert len(counts[2]) >= 10 and all(c > 0 and c % groups == 0 for c in counts[2].values()), counts[2]
    assert all(0 < ms < 1e4 for _, ms in prof[2].values()), prof[2]       # every pair of events was on one stream

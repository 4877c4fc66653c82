"""K objects in lockstep on frames that are already in device memory: svh_matcher_push_back_batch_device,
svh_vo_process_batch_device, svh_vo_mono_process_batch_device and svh_vo_get_gain_batch give, bit for bit, what the
single host entries give for the same pixels -- and the lockstep counters (svh_test_lockstep_counts) show that they
did so as batched launches, not as a loop over the single entries.  Every object carries its own variant of the
images at its own byte offset, so a job that read another object's frame would show.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

import helpers as H
import lockstep_helpers as LH

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(H.ROOT, "tools"))


@pytest.fixture(scope="module")
def S():
    import svhip
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [LH.C.c_char_p]
    return svhip


@pytest.fixture(scope="module")
def RS(S):
    from svhip import resident
    return resident


@pytest.fixture(scope="module")
def hip():
    return LH.hip_runtime()


@pytest.fixture(scope="module")
def quad():
    return LH.quad()


@pytest.fixture(autouse=True)
def disarm(S):
    yield
    S.lib().svh_test_fail_at(None)


# ---------------------------------------------------------------------------------------------- Matcher
KMAX = 5
_host_runs = {}


def object_frames(quad, w, K):
    """object i's two pairs: variant i of the quad, cropped to w x 230"""
    return [LH.crop(LH.variant(quad, i), w) for i in range(K)]


def host_reference(RS, quad, w, half, multi):
    """KMAX objects fed by single host pushes and matched (method 2): their states, computed once per geometry and
    parameter set and never modified"""
    key = (w, half, multi)
    if key not in _host_runs:
        prm = H.matcher_defaults(half_resolution=half, multi_stage=multi)
        out = []
        for fr in object_frames(quad, w, KMAX):
            m = LH.plain_matcher(prm)
            m.push_back(fr[0], fr[1])
            m.push_back(fr[2], fr[3])
            m.match(2)
            out.append(LH.matcher_state(RS, m))
        _host_runs[key] = out
    return _host_runs[key]


def device_batch_push(RS, hip, ms, lefts, rights, pitch=None, replace=False):
    h, w = lefts[0].shape
    k1, a1 = LH.frames_on_device(hip, lefts, pitch)
    k2, a2 = (None, None) if rights is None else LH.frames_on_device(hip, rights, pitch)
    RS.matcher_push_back_batch(ms, a1, a2, w, h, pitch, replace)


@pytest.mark.parametrize("half,multi", [(1, 1), (0, 0)])
@pytest.mark.parametrize("extra", [0, 13])
@pytest.mark.parametrize("w", [607, 608, 609, 624])
@pytest.mark.parametrize("K", [2, 5])
def test_matcher_device_batch_equals_host_pushes(RS, hip, quad, K, w, extra, half, multi):
    want = host_reference(RS, quad, w, half, multi)
    prm = H.matcher_defaults(half_resolution=half, multi_stage=multi)
    ms = [LH.plain_matcher(prm) for _ in range(K)]
    frames = object_frames(quad, w, K)
    c = LH.Counts(RS)
    device_batch_push(RS, hip, ms, [f[0] for f in frames], [f[1] for f in frames], w + extra)
    device_batch_push(RS, hip, ms, [f[2] for f in frames], [f[3] for f in frames], w + extra)
    flushed, fallback, _ = c.delta()
    assert (flushed, fallback) == (2, 0)
    H.product_matcher_batch(ms, None, None, 2, push=False)
    for i, m in enumerate(ms):
        assert len(want[i][2]) > 50
        LH.assert_same_matcher_state(LH.matcher_state(RS, m), want[i], (K, w, extra, half, multi, i))


def test_matcher_device_batch_single_image_flow(RS, hip, quad):
    """dI2 = NULL: one camera, method 0"""
    K, w = 3, 609
    prm = H.matcher_defaults()
    frames = object_frames(quad, w, K)
    ms = [LH.plain_matcher(prm) for _ in range(K)]
    device_batch_push(RS, hip, ms, [f[0] for f in frames], None, w + 13)
    device_batch_push(RS, hip, ms, [f[2] for f in frames], None, w + 13)
    H.product_matcher_batch(ms, None, None, 0, push=False)
    for i, m in enumerate(ms):
        one = LH.plain_matcher(prm)
        one.push_back(frames[i][0])
        one.push_back(frames[i][2])
        one.match(0)
        assert len(one.matches()) > 50
        LH.assert_same_matcher_state(LH.matcher_state(RS, m), LH.matcher_state(RS, one), ("flow", i))


def test_matcher_device_batch_replace(RS, hip, quad):
    K, w = 3, 624
    prm = H.matcher_defaults()
    frames = object_frames(quad, w, K)
    ms = [LH.plain_matcher(prm) for _ in range(K)]
    ones = [LH.plain_matcher(prm) for _ in range(K)]
    flip = lambda a: np.ascontiguousarray(a[::-1])
    seq = [(0, 1, False, False), (0, 1, True, False), (2, 3, False, True)]     # left, right, flipped, replace
    for a, b, flipped, rep in seq:
        l = [flip(f[a]) if flipped else f[a] for f in frames]
        r = [flip(f[b]) if flipped else f[b] for f in frames]
        device_batch_push(RS, hip, ms, l, r, w, replace=rep)
        for i, one in enumerate(ones):
            one.push_back(l[i], r[i], replace=rep)
    H.product_matcher_batch(ms, None, None, 2, push=False)
    for i, (m, one) in enumerate(zip(ms, ones)):
        one.match(2)
        assert len(one.matches()) > 50
        LH.assert_same_matcher_state(LH.matcher_state(RS, m), LH.matcher_state(RS, one), ("replace", i))


def test_matcher_host_and_device_batches_alternate(RS, hip, quad):
    """host batch, device batch, device batch, host batch, then a single device push on the same objects: matches and
    gain after every frame equal those of single host pushes (getGain sees pairs with one, no and one host copy)"""
    K, w = 3, 609
    prm = H.matcher_defaults()
    frames = object_frames(quad, w, K)
    ms = [LH.plain_matcher(prm) for _ in range(K)]
    ones = [LH.plain_matcher(prm) for _ in range(K)]
    for step in range(5):
        a, b = ((0, 1), (2, 3))[step % 2]
        l, r = [f[a] for f in frames], [f[b] for f in frames]
        if step in (0, 3):
            H.product_matcher_batch(ms, l, r, None)
        elif step in (1, 2):
            device_batch_push(RS, hip, ms, l, r, w + 13)
        else:
            for i, m in enumerate(ms):
                d1, a1 = LH.on_device(hip, l[i], w + 5, 1)
                d2, a2 = LH.on_device(hip, r[i], w + 5, 3)
                RS.matcher_push_back(m, a1, a2, w, 230, w + 5)
        for i, one in enumerate(ones):
            one.push_back(l[i], r[i])
        if step == 0:
            continue
        H.product_matcher_batch(ms, None, None, 2, push=False)
        for i, (m, one) in enumerate(zip(ms, ones)):
            one.match(2)
            LH.assert_same_matcher_state(LH.matcher_state(RS, m), LH.matcher_state(RS, one), ("alternate", step, i))
            inl = np.arange(0, len(one.matches()), 2, dtype=np.int32)
            assert LH.bits(RS.matcher_gain(m, inl)) == LH.bits(one.gain(inl)), (step, i)


def test_matcher_device_batch_with_an_object_that_differs(RS, hip, quad):
    """nms_n differs on object 1: the call runs one by one through the single device entry and still gives equal
    results; no phase is recorded"""
    K, w = 3, 608
    prms = [H.matcher_defaults(), H.matcher_defaults(nms_n=4), H.matcher_defaults()]
    frames = object_frames(quad, w, K)
    ms = [LH.plain_matcher(p) for p in prms]
    c = LH.Counts(RS)
    device_batch_push(RS, hip, ms, [f[0] for f in frames], [f[1] for f in frames], w + 13)
    device_batch_push(RS, hip, ms, [f[2] for f in frames], [f[3] for f in frames], w + 13)
    assert c.delta() == (0, 0, 0)
    H.product_matcher_batch(ms, None, None, 2, push=False)
    for i, m in enumerate(ms):
        one = LH.plain_matcher(prms[i])
        one.push_back(frames[i][0], frames[i][1])
        one.push_back(frames[i][2], frames[i][3])
        one.match(2)
        assert len(one.matches()) > 50
        LH.assert_same_matcher_state(LH.matcher_state(RS, m), LH.matcher_state(RS, one), ("mixed", i))


def test_matcher_device_batch_argument_contracts(S, RS, hip, quad):
    K, w = 2, 608
    frames = object_frames(quad, w, K)
    ms = [LH.plain_matcher(H.matcher_defaults()) for _ in range(K)]
    held, a1 = LH.frames_on_device(hip, [f[0] for f in frames])
    held2, a2 = LH.frames_on_device(hip, [f[1] for f in frames])
    assert RS.matcher_push_back_batch([ms[0], ms[0]], a1, a2, w, 230, check=False) == S.ERR_BAD_ARG
    assert "twice" in S.last_error()
    assert RS.matcher_push_back_batch([ms[0], None], a1, a2, w, 230, check=False) == S.ERR_BAD_ARG
    assert RS.matcher_push_back_batch([], [], [], w, 230) == 0
    RS.matcher_push_back_batch(ms, a1, a2, w, 230)
    # a pending prefetched frame: refused, and it is still there afterwards
    l, r = [f[2] for f in frames], [f[3] for f in frames]
    H.product_matcher_prefetch(ms, l, r)
    held3, b1 = LH.frames_on_device(hip, l)
    held4, b2 = LH.frames_on_device(hip, r)
    assert RS.matcher_push_back_batch(ms, b1, b2, w, 230, check=False) == S.ERR_BAD_ARG
    assert "prefetched frame is pending" in S.last_error()
    L = RS._bind()
    hs = (LH.C.c_void_p * K)(*[m.h for m in ms])
    dims = (LH.C.c_int32 * 3)(w, 230, w)
    assert L.svh_matcher_push_back_batch_device(hs, K, None, None, dims, 0) == S.ERR_BAD_ARG
    H.product_matcher_take_prefetched(ms, (230, w))
    H.product_matcher_batch(ms, None, None, 2, push=False)
    for i, m in enumerate(ms):
        one = LH.plain_matcher(H.matcher_defaults())
        one.push_back(frames[i][0], frames[i][1])
        one.push_back(frames[i][2], frames[i][3])
        one.match(2)
        assert one.matches().tobytes() == m.matches().tobytes(), i


def test_matcher_counters_do_not_grow_with_K(RS, hip, quad):
    """a K = 5 device push issues exactly as many batched launches as a K = 2 one and as the host batch push of the same
    objects, in one flushed phase and no fallback: the work of the K objects shares its launches"""
    w = 608
    prm = H.matcher_defaults()
    frames = object_frames(quad, w, 5)
    seen = {}
    for K in (2, 5):
        ms = [LH.plain_matcher(prm) for _ in range(K)]
        device_batch_push(RS, hip, ms, [f[0] for f in frames[:K]], [f[1] for f in frames[:K]])   # (buffers, arena)
        c = LH.Counts(RS)
        device_batch_push(RS, hip, ms, [f[2] for f in frames[:K]], [f[3] for f in frames[:K]], w + 13)
        seen[K] = c.delta()
        H.product_matcher_batch(ms, [f[0] for f in frames[:K]], [f[1] for f in frames[:K]], None)
        seen[K, "host"] = c.delta()
    assert seen[5][0] == 1 and seen[5][1] == 0 and seen[5][2] > 0
    assert seen[2] == seen[5] == seen[2, "host"] == seen[5, "host"]


def test_matcher_device_batch_failing_wait(S, RS, hip, quad, capfd):
    """a wait inside the entry fails (the second one: object 0's right view is being sized; the recorded phase's own wait
    is of the kind the Matcher never injects): SVH_ERR_HIP, one line, and the same call repeated gives the host entry's
    result.  The return code is injected on the host: nothing faults on the device."""
    K, w = 3, 607
    want = host_reference(RS, quad, w, 1, 1)
    frames = object_frames(quad, w, K)
    ms = [LH.plain_matcher(H.matcher_defaults(half_resolution=1, multi_stage=1)) for _ in range(K)]
    held, a1 = LH.frames_on_device(hip, [f[0] for f in frames])
    held2, a2 = LH.frames_on_device(hip, [f[1] for f in frames])
    assert S.lib().svh_test_fail_at(b"wait:2") == 0
    capfd.readouterr()
    assert RS.matcher_push_back_batch(ms, a1, a2, w, 230, check=False) == S.ERR_HIP
    S.lib().svh_test_fail_at(None)
    assert "injected failure" in S.last_error()
    assert capfd.readouterr().err.count("svhip:") == 1
    RS.matcher_push_back_batch(ms, a1, a2, w, 230)
    device_batch_push(RS, hip, ms, [f[2] for f in frames], [f[3] for f in frames])
    H.product_matcher_batch(ms, None, None, 2, push=False)
    for i, m in enumerate(ms):
        LH.assert_same_matcher_state(LH.matcher_state(RS, m), want[i], ("after a failed wait", i))


# ---------------------------------------------------------------------------------------------- stereo visual odometry
def six_frames(quad, i):
    return (LH.drive(LH.variant(quad, i)) * 2)[:6]


@pytest.fixture(scope="module")
def stereo_run(RS, hip, quad):
    """K = 3 objects through six frames of svh_vo_process_batch_device next to twins in a loop of svh_vo_process on host
    frames; what is compared, and the counters per frame"""
    K = 3
    seqs = [six_frames(quad, i) for i in range(K)]
    bat = [H.ProductVo(H.vo_defaults(), private_rand=0) for _ in range(K)]
    one = [H.ProductVo(H.vo_defaults(), private_rand=0) for _ in range(K)]
    got, want, counts = [], [], []
    c = LH.Counts(RS)
    for k in range(6):
        h, w = seqs[0][k][0].shape
        pitch = w + (k % 2) * 13
        k1, a1 = LH.frames_on_device(hip, [s[k][0] for s in seqs], pitch)
        k2, a2 = LH.frames_on_device(hip, [s[k][1] for s in seqs], pitch)
        c.mark()
        ok = RS.vo_process_batch(bat, a1, a2, w, h, pitch)
        counts.append(c.delta())
        got.append([LH.vo_state(v, o) for v, o in zip(bat, ok)])
        want.append([LH.vo_state(v, v.process(s[k][0], s[k][1])) for v, s in zip(one, seqs)])
    return bat, one, got, want, counts


def test_vo_device_batch_equals_loop_of_host_calls(stereo_run):
    bat, one, got, want, counts = stereo_run
    for k in range(6):
        for i in range(3):
            LH.assert_same_vo_state(got[k][i], want[k][i], ("stereo", k, i))
    assert [w[0] for w in want[0]] == [0, 0, 0] and sum(w[0] for f in want[2:] for w in f) >= 9
    # frames 0 and 1 bootstrap one by one (no phase recorded); once every object has a motion, the frames run in lockstep
    assert counts[0] == (0, 0, 0) and counts[1] == (0, 0, 0)
    for k in (3, 4, 5):
        assert counts[k][0] >= 4 and counts[k][1] == 0 and counts[k][2] > 0, (k, counts[k])


def test_vo_gain_batch_equals_single_calls(RS, stereo_run):
    bat, one, _, _, _ = stereo_run
    inl = [v.inliers() for v in bat]
    assert all(len(a) > 20 for a in inl)
    want = [one[i].gain(inl[i]) for i in range(3)]
    c = LH.Counts(RS)
    got = RS.vo_gain_batch(bat, inl)
    assert c.delta() == (1, 0, 1)          # one phase, one k_gain_b launch for the three objects
    for i in range(3):
        assert want[i] != 1 and LH.bits(got[i]) == LH.bits(want[i]) == LH.bits(bat[i].gain(inl[i])), i


def test_vo_gain_batch_with_unequal_jobs(S, RS, hip, quad, stereo_run):
    """inlier lists of 0, 1, 63, 64, 65 and 1025 entries in ONE call (the grid is the largest job's: k_gain_b's guard
    blockIdx.x * 64 < a.n), an index past the match list among them, an object whose frames were pushed from the host
    (it keeps the host loop) next to the device ones, and an object without two frames"""
    bat = stereo_run[0]
    vos = list(bat)
    for i in range(3, 6):                                  # three more device-fed objects, two frames each
        v = H.ProductVo(H.vo_defaults(), private_rand=0)
        for l, r in six_frames(quad, i)[:2]:
            d1, a1 = LH.on_device(hip, l, None, 1)
            d2, a2 = LH.on_device(hip, r, None, 2)
            RS.vo_process(v, a1, a2, l.shape[1], l.shape[0])
        vos.append(v)
    host = H.ProductVo(H.vo_defaults(), private_rand=0)
    for l, r in six_frames(quad, 6)[:2]:
        host.process(l, r)
    fresh = H.ProductVo(H.vo_defaults(), private_rand=0)
    vos += [host, fresh]
    sizes = [0, 1, 63, 64, 65, 1025, 65, 5]
    lists = []
    for v, n in zip(vos, sizes):
        nm = max(len(v.matches()), 1)
        idx = (np.arange(n, dtype=np.int64) * 7) % (nm + 3)           # (some past the match list: they are skipped)
        lists.append(idx.astype(np.int32))
    assert all(len(v.matches()) > 50 for v in vos[:7]) and any((l >= len(v.matches())).any() for l, v in zip(lists, vos))
    want = [np.float32(v.gain(l)) for v, l in zip(vos, lists)]
    c = LH.Counts(RS)
    got = RS.vo_gain_batch(vos, lists)
    assert c.delta() == (1, 0, 1)
    for i in range(len(vos)):
        assert LH.bits(got[i]) == LH.bits(want[i]), (i, sizes[i], got[i], want[i])
    assert want[0] == 1 and want[7] == 1 and all(want[i] != 1 for i in range(2, 7))
    # argument errors
    assert RS._bind().svh_vo_get_gain_batch(None, 2, None, None, None) == S.ERR_BAD_ARG
    with pytest.raises(S.SvhError):
        RS.vo_gain_batch([vos[0], vos[0]], lists[:2])
    assert len(RS.vo_gain_batch([], [])) == 0


# ---------------------------------------------------------------------------------------------- mono visual odometry
def test_vo_mono_device_batch_equals_loop_of_host_calls(S, RS, hip):
    """K = 3 staggered sequences (object i starts at frame i); from the second frame on a different object replaces
    its current frame every step, so the batch splits into the two groups of its push every time"""
    K = 3
    frames = H.mono_frames()
    feeds = [[frames[(i + k) % 7] for k in range(7)] for i in range(K)]
    bat = [S.VoMono(private_rand=0) for _ in range(K)]
    one = [S.VoMono(private_rand=0) for _ in range(K)]
    rep = [False] * K
    h, w = frames[0].shape
    c = LH.Counts(RS)
    oks, lockstep_frames = [], 0
    for k in range(7):
        keep, addrs = LH.frames_on_device(hip, [f[k] for f in feeds], w + 1)
        c.mark()
        ok = RS.vo_mono_process_batch(bat, addrs, w, h, w + 1, rep)
        flushed, fallback, launches = c.delta()
        assert fallback == 0
        lockstep_frames += flushed > 0 and launches > 0
        for i in range(K):
            o = one[i].process(feeds[i][k], rep[i])
            LH.assert_same_vo_state(LH.vo_state(bat[i], ok[i]), LH.vo_state(one[i], o), ("mono", k, i))
        rep = [(k + i) % 3 == 0 for i in range(K)]
        oks.append(ok)
    assert any(any(o) for o in oks) and lockstep_frames == 7
    # the gain of mono objects, device frames: one launch
    L = S.lib()
    L.svh_vo_get_gain.restype = LH.C.c_float
    L.svh_vo_get_gain.argtypes = [LH.C.c_void_p, LH.C.c_void_p, LH.C.c_int32]
    inl = [np.arange(0, len(v.matches()), 3, dtype=np.int32) for v in bat]
    want = [L.svh_vo_get_gain(v.h, a.ctypes.data, len(a)) for v, a in zip(one, inl)]
    c.mark()
    got = RS.vo_gain_batch(bat, inl)
    assert c.delta() == (1, 0, 1)
    for i in range(K):
        assert len(inl[i]) > 5 and LH.bits(got[i]) == LH.bits(want[i]), i
    for v in bat + one:
        v.close()


# ---------------------------------------------------------------------------------------------- end to end
def test_lockstep_pipeline_equals_two_resident_pipelines(S, quad):
    """LockstepPipeline with K = 2 over drive(quad) and its variant = two Pipeline(resident=True) runs: ok, pose bytes,
    both point lists per frame and the rendered view"""
    import stereomapper_pipeline as SP
    f, cu, cv, base = 645.24, 635.96, 194.13, 0.5707
    drives = [LH.drive(quad), LH.drive(LH.variant(quad, 2))]
    want = []
    for d in drives:
        p = SP.Pipeline(f, cu, cv, base, resident=True)
        p.vo.lib.svh_vo_set_private_rand.argtypes = [LH.C.c_void_p, LH.C.c_int32, LH.C.c_uint32]
        p.vo.lib.svh_vo_set_private_rand(p.vo.h, 1, 0)
        out = []
        for l, r in d:
            ok, n0, n1 = p.push(l, r)
            out.append((ok, n0, n1, p.poses[-1].tobytes(), p.map.points(0).tobytes(), p.map.points(1).tobytes()))
        want.append((out, p.view.render().tobytes()))
    lp = SP.LockstepPipeline(2, f, cu, cv, base, private_rand=0)
    for k in range(4):
        res = lp.push([d[k] for d in drives])
        for i in range(2):
            got = res[i] + (lp.poses[i][-1].tobytes(), lp.maps[i].points(0).tobytes(), lp.maps[i].points(1).tobytes())
            assert got[:3] == want[i][0][k][:3], (k, i, got[:3], want[i][0][k][:3])
            assert got[3:] == want[i][0][k][3:], (k, i)
    for i in range(2):
        assert lp.views[i].render().tobytes() == want[i][1], i
    assert want[0][0][0][0] is False and any(x[0] for x in want[0][0][1:]) and want[0][0][-1][2] > 20000

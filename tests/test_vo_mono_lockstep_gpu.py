"""GPU: K VisualOdometryMono objects in lockstep (svh_vo_mono_process_batch, _prefetch_batch, _process_next_batch,
_process_matches_batch; the batched kernels of vo_mono_kernels.hip) against the reference's own results in
tests/golden/vo_mono.npz, with the comparison of test_vo_mono_gpu.py::check_frame: return value, bucketed matches,
inlier indices and the votes of every hypothesis identical, the 4x4 motion within that file's TOL = 1e-9 (the device
exp of the plane vote).  Where two runs on the device are compared with each other -- a batch against a loop of single
calls -- everything must be equal bit for bit: the batched kernels run the single kernels' bodies and the host steps
are the same functions, so any difference is a bug."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import mono_ref as R
from test_vo_mono_gpu import TOL, check_frame, golden_seq, params

pytestmark = pytest.mark.gpu
EST_DEMO = ["syn9", "syn10", "syn200", "syn2000", "syn5000", "identical"]


@pytest.fixture(scope="module")
def Z():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def S():
    import svhip
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    return svhip


@pytest.fixture(autouse=True)
def disarm(S):
    yield
    S.lib().svh_test_fail_at(None)


def state(vo, ok):
    return int(ok), vo.matches().copy(), vo.inliers().copy(), vo.motion().copy(), vo.votes().copy()


def assert_same(got, want, where):
    """two device runs: bit for bit"""
    assert got[0] == want[0], where
    assert got[1].tobytes() == want[1].tobytes(), where
    assert np.array_equal(got[2], want[2]), where
    assert got[3].tobytes() == want[3].tobytes(), (where, np.abs(got[3] - want[3]).max())
    assert np.array_equal(got[4], want[4]), where


class Group:
    """demo_viso_mono.m's loop for K sequences through the lockstep entries: object i is fed feed[i][k] on step k;
    replace is kept per object (demo: replace = !ok from the second frame on)"""

    def __init__(self, S, prms, demo, feeds, private_rand=0, pipelined=False):
        self.S, self.K = S, len(prms)
        self.vos = [S.VoMono(p, private_rand=private_rand) for p in prms]
        self.demo, self.feeds, self.pipelined = demo, feeds, pipelined
        self.replace, self.k = [False] * self.K, 0
        self.shape = feeds[0][0].shape
        if pipelined:
            S.VoMono.prefetch_batch(self.vos, [f[0] for f in feeds])

    def step(self):
        k = self.k
        if self.pipelined:
            nxt = [f[k + 1] for f in self.feeds] if k + 1 < len(self.feeds[0]) else None
            ok = self.S.VoMono.process_next_batch(self.vos, nxt, self.shape, self.replace)
        else:
            ok = self.S.VoMono.process_batch(self.vos, [f[k] for f in self.feeds], self.replace)
        for i in range(self.K):
            if self.demo[i] and k > 0:
                self.replace[i] = not ok[i]
        self.k += 1
        return [state(v, o) for v, o in zip(self.vos, ok)]


def golden_group(S, Z, names, K=None, **kw):
    names = names if K is None else [names] * K
    frames = H.mono_frames()
    return Group(S, [params(S, Z["seq_%s_params" % n]) for n in names],
                 [bool(Z["seq_%s_demo_replace" % n]) for n in names], [frames] * len(names), **kw)


@pytest.mark.parametrize("name", ["still", "demo", "alt"])
def test_four_sequences_equal_the_reference(S, Z, name):
    g = golden_group(S, Z, name, K=4)
    want = golden_seq(Z, name)
    for k in range(7):
        for i, got in enumerate(g.step()):
            check_frame(got[:4], want[k], (name, k, i))


def test_staggered_sequences_equal_single_calls(S, Z):
    """object i starts at frame i: the objects of a batch differ in images, N, replace and in the exit they take"""
    frames = H.mono_frames()
    K = 4
    feeds = [[frames[(i + k) % 7] for k in range(7)] for i in range(K)]
    prm = [params(S, Z["seq_demo_params"]) for _ in range(K)]
    g = Group(S, prm, [True] * K, feeds)
    twins = [S.VoMono(params(S, Z["seq_demo_params"]), private_rand=0) for _ in range(K)]
    rep = [False] * K
    want0 = golden_seq(Z, "demo")
    for k in range(7):
        got = g.step()
        for i in range(K):
            ok = twins[i].process(feeds[i][k], rep[i])
            if k > 0:
                rep[i] = not ok
            assert_same(got[i], state(twins[i], ok), ("staggered", k, i))
        check_frame(got[0][:4], want0[k], ("staggered golden", k))
        assert g.replace == rep


def test_estimate_cases_in_one_call(S, Z):
    """N from 9 to 5000, an object that leaves before its inliers are cleared, one whose normalisation fails and
    full runs, side by side in ONE svh_vo_mono_process_matches_batch"""
    for n in EST_DEMO:
        assert np.array_equal(Z["est_%s_params" % n], Z["est_%s_params" % EST_DEMO[0]]), n
    vos = [S.VoMono(params(S, Z["est_%s_params" % n]), private_rand=0) for n in EST_DEMO]
    ok = S.VoMono.process_matches_batch(vos, [Z["est_%s_matches" % n] for n in EST_DEMO])
    for vo, o, name in zip(vos, ok, EST_DEMO):
        assert int(o) == int(Z["est_%s_ok" % name]), name
        assert np.array_equal(vo.votes(), Z["est_%s_votes" % name]), name
        assert np.array_equal(vo.inliers(), Z["est_%s_inliers" % name]), name
        assert np.abs(vo.motion() - Z["est_%s_motion" % name]).max() < TOL, name
    assert [int(o) for o in ok] == [0, 0, 1, 1, 1, 0]
    # ... and bit for bit what single calls on fresh objects give
    for vo, o, name in zip(vos, ok, EST_DEMO):
        one = S.VoMono(params(S, Z["est_%s_params" % name]), private_rand=0)
        o1 = one.process_matches(Z["est_%s_matches" % name])
        assert_same(state(vo, o), state(one, o1), name)
        assert int(o) == int(o1), name


def test_libc_rand_equals_the_loop_of_single_calls(S, Z):
    """srand(0), one batch call per frame for K = 3 objects that draw from libc rand(): the draws happen object by
    object, so the results are those of srand(0) and the loop of single calls"""
    libc = C.CDLL(None)
    K = 3
    frames = H.mono_frames()
    prm = Z["seq_still_params"]
    warm = Group(S, [params(S, prm) for _ in range(K)], [False] * K, [frames] * K)   # (arena, helper threads)
    warm.step(), warm.step()
    g = Group(S, [params(S, prm) for _ in range(K)], [False] * K, [frames] * K, private_rand=None)
    libc.srand(0)
    got = [g.step() for _ in range(7)]
    twins = [S.VoMono(params(S, prm)) for _ in range(K)]
    libc.srand(0)
    for k in range(7):
        for i in range(K):
            ok = twins[i].process(frames[k], False)
            assert_same(got[k][i], state(twins[i], ok), ("libc", k, i))
    # object 0 drew first after srand(0): on frame 1 it is the reference's run
    check_frame(got[1][0][:4], golden_seq(Z, "still")[1], "libc frame 1")


def test_mixed_parameters_and_single_object(S, Z):
    """objects that cannot run in lockstep are run one after the other; K = 1 is the single call"""
    names = ["still", "alt", "still", "alt"]
    g = golden_group(S, Z, names)
    one = golden_group(S, Z, ["alt"])
    want = {n: golden_seq(Z, n) for n in ("still", "alt")}
    for k in range(7):
        for i, got in enumerate(g.step()):
            check_frame(got[:4], want[names[i]][k], ("mixed", k, i))
        check_frame(one.step()[0][:4], want["alt"][k], ("K=1", k))


@pytest.mark.parametrize("name", ["still", "demo"])
def test_pipelined_loop_equals_the_reference(S, Z, name):
    g = golden_group(S, Z, name, K=4, pipelined=True)
    plain = golden_group(S, Z, name, K=4)
    want = golden_seq(Z, name)
    for k in range(7):
        got, ref = g.step(), plain.step()
        for i in range(4):
            check_frame(got[i][:4], want[k], (name, k, i))
            assert_same(got[i], ref[i], ("pipelined", name, k, i))


def test_mono_and_stereo_batches_alternate(S, Z):
    """the recorders and helper threads are shared: a mono batch and a stereo svh_vo_process_batch alternating in one
    process each give what they give alone"""
    quad = [H.read_pgm(os.path.join(H.GOLDEN, "viso_%s.pgm" % k)) for k in ("I1p", "I2p", "I1c", "I2c")]
    K = 3

    def stereo_step(vos, f):
        rc, ok = H.product_vo_process_batch(vos, [quad[2 * (f % 2)]] * K, [quad[2 * (f % 2) + 1]] * K)
        return [(int(o), v.matches().tobytes(), v.inliers().tobytes(), v.motion().tobytes()) for v, o in zip(vos, ok)]

    alone = [H.ProductVo(H.vo_defaults(), private_rand=0) for _ in range(K)]
    want_st = [stereo_step(alone, f) for f in range(5)]
    st = [H.ProductVo(H.vo_defaults(), private_rand=0) for _ in range(K)]
    g = golden_group(S, Z, "still", K=4)
    want = golden_seq(Z, "still")
    for k in range(7):
        if k < 5:
            assert stereo_step(st, k) == want_st[k], ("stereo", k)
        for i, got in enumerate(g.step()):
            check_frame(got[:4], want[k], ("mono", k, i))
    assert any(r[0] for f in want_st for r in f)   # (the stereo objects did estimate motion)


@pytest.mark.parametrize("kind", ["copy", "launch", "wait"])
def test_injected_failures_in_every_phase(S, Z, kind, capfd):
    """svh_test_fail_at: the n-th copy (the job tables of a phase), launch check or wait of an estimate-only batch is
    the one of phase n.  SVH_ERR_HIP with the call named; then the same objects go on with the frames of their
    sequence and give, bit for bit, what twins give that made the same calls without the failure.  Return codes are
    injected on the host: nothing faults on the device."""
    K = 3
    frames = H.mono_frames()
    gold = golden_seq(Z, "still")
    for phase in (1, 2, 3):
        g = golden_group(S, Z, "still", K=K)
        twins = [S.VoMono(params(S, Z["seq_still_params"]), private_rand=0) for _ in range(K)]
        for k in range(3):
            got = g.step()
            for i in range(K):
                check_frame(got[i][:4], gold[k], (kind, phase, k, i))
                twins[i].process(frames[k], False)
        m = gold[2][1]   # (a full run: all three phases are reached)
        assert S.lib().svh_test_fail_at(("%s:%d" % (kind, phase)).encode()) == 0
        capfd.readouterr()
        with pytest.raises(S.SvhError) as e:
            S.VoMono.process_matches_batch(g.vos, [m] * K)
        S.lib().svh_test_fail_at(None)
        assert e.value.code == S.ERR_HIP, (kind, phase, e.value)
        assert "injected failure" in str(e.value), e.value
        assert capfd.readouterr().err.count("svhip:") == 1
        for t in twins:
            assert t.process_matches(m)
        for k in range(3, 7):
            got = g.step()
            for i in range(K):
                ok = twins[i].process(frames[k], False)
                assert_same(got[i], state(twins[i], ok), (kind, phase, k, i))
                assert got[i][0] == 1, (kind, phase, k, i)

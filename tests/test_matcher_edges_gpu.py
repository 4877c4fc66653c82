"""GPU parity of the Matcher (svh_matcher_*, csrc/matcher_kernels.hip) with the oracle on the generated scenes of
tests/matcher_scenes.py: the size-switched paths (global k_bin_index, broken recording, the three write paths of
d_compact_matches, both branches of d_compact_slots, both download routes, `ranked` on and off), the tie rules
(find_match's traversal position, d_nms's scan-order key and strict vote, relocate_group's and parabolic's first
minimum), saturated filters and starved frames.  tests/test_matcher_edges.py proves on the oracle alone that each
scene reaches its edge.  Eight tables, six stages and the match list bit for bit (helpers.compare_matchers); the six
filter planes inside the 2-pixel margin tests/test_matcher_gpu.py uses."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import matcher_scenes as MS

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not H.have_ref_viso(), reason="the oracle needs the real Triangle (oracle/_ref)")]

INTR = (645.24, 635.96, 194.13, 0.5707)
BIG = ("big", "middle", "natural", "small", "under")


def motion():
    T = np.eye(4)
    T[2, 3] = -0.75
    T[0, 3] = 0.02
    return T


_oracles = {}


def oracle_of(case, method=2, tr=False, **more):
    """the oracle after the case's quad: computed once per (case, method, parameters), only read afterwards"""
    key = (case.name, case.w, case.h, str(case.kw), str(case.prm), method, tr, tuple(sorted(more.items())))
    if key not in _oracles:
        _oracles[key] = MS.run(H.OracleMatcher(case.params(**more)), case.quad(), method,
                               motion() if tr else None, INTR if tr else None)
    return _oracles[key]


def product_of(case, method=2, tr=False, **more):
    return MS.run(H.ProductMatcher(case.params(**more)), case.quad(), method,
                  motion() if tr else None, INTR if tr else None)


def no_difference(a, b, method=2):
    bad = [x for x in H.compare_matchers(a, b, method) if x[1] != 0]
    assert not bad, bad
    x, y = a.matches(), b.matches()
    assert x.shape == y.shape and x.tobytes() == y.tobytes()


def same_planes(a, b, half):
    for w in range(6):
        if w in (2, 3) and not half:
            continue
        x, dx = a.filter_image(w)
        y, dy = b.filter_image(w)
        assert dx == dy and np.array_equal(x[2:-2, 2:-2], y[2:-2, 2:-2]), w


def same_list(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def untapped(prm):
    m = H.ProductMatcher(prm)
    m.lib.svh_matcher_set_taps(C.c_void_p(m.h), 0)
    return m


# ---- every scene, method 2; the big, periodic and 0 / 255 scenes with the other methods and refinements -------------
RUNS = [(n, 2, {}) for n in MS.CASES]
RUNS += [(n, meth, {}) for n in ("big", "periodic", "periodic16", "binary3", "binary8") for meth in (0, 1)]
RUNS += [(n, 2, {"refinement": r}) for n in ("big", "periodic", "periodic16", "binary3", "binary8") for r in (0, 2)]
RUNS += [("middle", 2, {"refinement": 2}), ("small", 2, {"refinement": 2}),       # k_compact_matches' second use
         ("big", 1, {"refinement": 2}), ("binary8", 0, {"refinement": 2}),
         ("periodic", 2, {"multi_stage": 0}), ("periodic16", 2, {"multi_stage": 0}), ("small", 2, {"multi_stage": 0}),
         ("levels3", 2, {"nms_n": 2}), ("levels3", 2, {"nms_n": 5}), ("levels4c2", 0, {}), ("levels3", 1, {})]


@pytest.mark.parametrize("name,method,more", RUNS,
                         ids=["-".join([n, "m%d" % meth] + ["%s%d" % kv for kv in more.items()]) for n, meth, more in RUNS])
def test_scene_matches_oracle(name, method, more):
    case = MS.CASES[name]
    a, b = oracle_of(case, method, **more), product_of(case, method, **more)
    no_difference(a, b, method)
    same_planes(a, b, case.params(**more).half_resolution)


@pytest.mark.parametrize("name", ["periodic", "periodic16", "binary8"])
def test_predicted_motion_breaks_ties_as_the_oracle_does(name):
    """set_intrinsics + Tr: the `predicted` term of find_match's cost separates candidates whose descriptors are equal"""
    case = MS.CASES[name]
    no_difference(oracle_of(case, 2, tr=True), product_of(case, 2, tr=True))


@pytest.mark.parametrize("w,h,half", MS.FILTER_SIZES)
def test_filter_block_geometry(w, h, half):
    case = MS.Case("filter", MS.noise, w, h, {"seed": w + h}, {"half_resolution": half}, disp=3, flow=(1, 1))
    a, b = oracle_of(case), product_of(case)
    assert len(a.features(5)) > 0
    no_difference(a, b)
    same_planes(a, b, half)


@pytest.mark.parametrize("size", MS.SLOT_SIZES, ids=lambda s: s[3])
def test_slot_compaction_sizes(size):
    case = MS.slot_case(size)
    a, b = oracle_of(case), product_of(case)
    no_difference(a, b)
    same_planes(a, b, 0)


# ---- the form an application runs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BIG)
def test_without_taps_twice_in_a_row(name):
    """taps off: the dense vote starts on the unrefined list while the device refines; alternating pushes, so every
    call is a fresh quad; the list is the oracle's, which test_scene_matches_oracle shows the tapped run's to be"""
    case = MS.CASES[name]
    want = oracle_of(case).matches()
    tapped = product_of(case).matches()
    m = untapped(case.params())
    q = case.quad()
    for rep in range(2):
        m.push_back(q[0], q[1])
        m.push_back(q[2], q[3])
        assert m.match(2) == 0
        got = m.matches()
        assert same_list(got, want) and same_list(got, tapped), rep


@pytest.mark.parametrize("other", ["same", "quad"])
def test_recorded_batch_falls_back_object_by_object(other):
    """K = 2 in lockstep on the big scene: the bin index of a 45 000-feature table needs more LDS than a recorded
    batch gets (156 KiB), the recording is marked broken and run_recorded runs the objects one by one; the second
    phase is recorded again.  `quad`: the second object has a natural image of the same size with a fraction of the
    features, so the two objects' counts differ and only one of them breaks the recording"""
    case = MS.CASES["big"]
    prm = case.params()
    seqs = [case.quad(), case.quad() if other == "same" else MS.CASES["natural"].quad()]
    one = [untapped(prm) for _ in seqs]
    for m, s in zip(one, seqs):
        MS.run(m, s)
    assert same_list(one[0].matches(), oracle_of(case).matches())
    bat = [untapped(prm) for _ in seqs]
    H.product_matcher_batch(bat, [s[0] for s in seqs], [s[1] for s in seqs], None)
    H.product_matcher_batch(bat, [s[2] for s in seqs], [s[3] for s in seqs], 2)
    for k in range(2):
        for tb in range(8):
            assert np.array_equal(one[k].features(tb), bat[k].features(tb)), (k, tb)
        assert len(one[k].matches()) > 500 and same_list(one[k].matches(), bat[k].matches()), k
    # once more through the ring buffer: the indices the one-by-one pass built are those of the new previous frame
    H.product_matcher_batch(bat, [s[0] for s in seqs], [s[1] for s in seqs], 2)
    for m, s in zip(one, seqs):
        m.push_back(s[0], s[1])
        assert m.match(2) == 0
    for k in range(2):
        assert len(one[k].matches()) > 500 and same_list(one[k].matches(), bat[k].matches()), k


# ---- frames in device memory ---------------------------------------------------------------------------------------
class Dev:
    """a device allocation holding a copy of a host byte array"""

    def __init__(self, hip, a):
        self.hip, self.p = hip, C.c_void_p()
        a = np.ascontiguousarray(a)
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 16))) == 0
        assert hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0   # HostToDevice
        self.addr = self.p.value

    def __del__(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = None


def device_frame(hip, img, pitch, offset):
    """`img` inside a larger device buffer of 0xAA, its rows `pitch` apart, starting `offset` bytes in"""
    h, w = img.shape
    buf = np.full(offset + pitch * (h - 1) + w + 32, 0xAA, np.uint8)
    for v in range(h):
        buf[offset + v * pitch: offset + v * pitch + w] = img[v]
    d = Dev(hip, buf)
    return d, d.addr + offset


@pytest.mark.parametrize("name", ["big", "ragged"])
def test_device_frames_equal_host_frames(name):
    """svh_matcher_push_back_device with a pitch above w and a pointer one byte off alignment"""
    from svhip import resident as RS
    hip = C.CDLL("libamdhip64.so")
    case = MS.CASES[name] if name in MS.CASES else \
        MS.Case("ragged", MS.noise, 333, 77, {"seed": 21}, {"half_resolution": 0}, disp=3, flow=(1, 1))
    a = product_of(case)
    b = H.ProductMatcher(case.params())
    q = case.quad()
    for I1, I2 in ((q[0], q[1]), (q[2], q[3])):
        (d1, a1), (d2, a2) = device_frame(hip, I1, case.w + 5, 1), device_frame(hip, I2, case.w + 5, 3)
        RS.matcher_push_back(b, a1, a2, case.w, case.h, case.w + 5, False)
        del d1, d2            # (the call has returned: the frame was packed into the view)
    assert b.match(2) == 0
    no_difference(a, b)
    assert len(a.matches()) > 100
    no_difference(oracle_of(case), b)


# ---- starved frames in a sequence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("method,blank", [(2, "right"), (2, "left"), (0, "left")])
def test_blank_camera_keeps_the_matches_and_the_object_recovers(method, blank):
    """a frame with a constant image has an empty table: matchFeatures returns silently (matcher.cpp:216-259) and the
    previous matches stay; two good frames later the object matches as if nothing had happened -- on both drivers"""
    case = MS.CASES["ranked_on"]
    q = case.quad()
    flat = MS.constant(case.w, case.h)
    kept = []
    drivers = [H.OracleMatcher(case.params()), H.ProductMatcher(case.params())]
    for m in drivers:
        MS.run(m, q, method)
        keep = m.matches()
        assert len(keep) > 1000
        if blank == "right":
            m.push_back(q[0], flat)
        else:
            m.push_back(flat, q[1] if method else None)
        assert m.match(method) in (0, None)
        assert same_list(m.matches(), keep)                   # the blank frame is `current`
        m.push_back(q[2], q[3] if method else None)
        assert m.match(method) in (0, None)
        assert same_list(m.matches(), keep)                   # ... and now `previous`
        m.push_back(q[0], q[1] if method else None)
        assert m.match(method) in (0, None)
        assert not same_list(m.matches(), keep) and len(m.matches()) > 1000
        kept.append(keep)
    assert same_list(kept[0], kept[1])
    no_difference(drivers[0], drivers[1], method)


def test_shrink_and_grow():
    """one object: the big scene, 33 x 31, the big scene again -- a size change reallocates the views and must leave
    no stale count or bin index behind"""
    big, tiny = MS.CASES["big"], MS.CASES["dense_only"]
    a, b = H.OracleMatcher(big.params()), H.ProductMatcher(big.params())
    for step, case in enumerate((big, tiny, big)):
        for m in (a, b):
            MS.run(m, case.quad())
        no_difference(a, b)
        assert len(b.features(5)) > 0, step
    assert len(b.matches()) > 10000

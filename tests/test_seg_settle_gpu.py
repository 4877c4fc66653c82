"""The speckle filter settles component verdicts inside the tile (k_seg_tile, k_seg_border, k_seg_sum, k_seg_mask and
k_gap_tile's load in stereo-vision_amd/csrc/elas_kernels.hip).  removeSmallSegments only asks whether a component has
speckle_size pixels or more.  A component of a 64 x 16 tile that large is kept whatever it joins across a seam; a
smaller one that touches no side with another tile behind it is complete and removed; only small components on a seam
go through the global union-find.  SVH_SEG_SETTLE=0 (read once per process) leaves every component undecided, which is
the two-level labelling as it was.

  * a CPU model in numpy (no GPU): the three classes of a map, the seam pass and the sums as the kernels do them, on
    random maps and planted components -- kept in tile U (undecided and global size >= min) == global size >= min,
    nothing removed in a tile lies on a seam, and the kernels' verdict is the flood fill's;
  * GPU, switch on against switch off, bit for bit, one child process per setting: seams everywhere (widths 64 .. 320,
    heights 16 .. 117), speckle_size 1 .. 5000, two similarity thresholds, half resolution, both maps post-processed,
    each on the tile path and on the k_seg_mask path;
  * GPU: the speckle stage of the mask path equals the CPU model applied to the stage before it;
  * GPU against the oracle and against a committed 1242 x 375 golden;
  * GPU: batches of 4 pairs in groups of 4 and of 2, twice in another order, equal the single calls (labels, counts
    and root lists of the group before must not leak)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

gpu = pytest.mark.gpu
TW, TH = 64, 16                      # k_seg_tile's tile


# ----------------------------------------------------------------------------- the CPU model
def _components(D, thr, tw=None, th=None):
    """labels (root index per valid pixel, -1 invalid) of the 4-neighbourhood graph "both valid, |a - b| <= thr";
    with a tile size, edges across tile seams are left out"""
    h, w = D.shape
    par = np.arange(h * w)

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    v = D >= 0
    jh = v[:, 1:] & v[:, :-1] & (np.abs(D[:, 1:] - D[:, :-1]) <= thr)
    jv = v[1:, :] & v[:-1, :] & (np.abs(D[1:, :] - D[:-1, :]) <= thr)
    if tw:
        jh[:, np.arange(1, w) % tw == 0] = False
        jv[np.arange(1, h) % th == 0, :] = False
    for y, x in zip(*np.nonzero(jh)):
        a, b = find(y * w + x), find(y * w + x + 1)
        if a != b:
            par[max(a, b)] = min(a, b)
    for y, x in zip(*np.nonzero(jv)):
        a, b = find(y * w + x), find((y + 1) * w + x)
        if a != b:
            par[max(a, b)] = min(a, b)
    lab = np.array([find(i) for i in range(h * w)]).reshape(h, w)
    lab[~v] = -1
    return lab


def _sizes(lab):
    n = np.bincount(lab[lab >= 0], minlength=lab.size)
    return np.where(lab >= 0, n[np.maximum(lab, 0)], 0)


KEEP, REMOVE, UNDECIDED, INVALID = 2, 3, 1, 0


def classes(D, thr, min_size, tw, th):
    """per pixel: KEEP (tile-local size >= min_size), REMOVE (smaller, on no seam), UNDECIDED, INVALID; and the
    tile-local labels"""
    h, w = D.shape
    lab = _components(D, thr, tw, th)
    size = _sizes(lab)
    yy, xx = np.mgrid[0:h, 0:w]
    # a pixel lies on a seam when it is on a side of its tile with another tile beyond (an image edge is none)
    seam = ((yy % th == 0) & (yy > 0)) | ((yy % th == th - 1) & (yy + 1 < h)) | \
           ((xx % tw == 0) & (xx > 0)) | ((xx % tw == tw - 1) & (xx + 1 < w))
    touch = np.zeros(h * w, bool)
    touch[lab[seam & (lab >= 0)]] = True
    cls = np.full((h, w), INVALID)
    v = lab >= 0
    big = v & (size >= max(min_size, 1))
    cls[big] = KEEP
    cls[v & ~big & ~touch[np.maximum(lab, 0)]] = REMOVE
    cls[v & ~big & touch[np.maximum(lab, 0)]] = UNDECIDED
    return cls, lab, seam


def kernel_verdict(D, thr, min_size, tw, th):
    """kept pixels as the kernels decide them: unions between undecided components only, a mark on the undecided side
    of a joined pair whose other side is kept, sums over the merged undecided components"""
    h, w = D.shape
    cls, lab, seam = classes(D, thr, min_size, tw, th)
    assert not (seam & (cls == REMOVE)).any(), "a component removed in its tile lies on a seam"
    par = np.arange(h * w)
    count = np.zeros(h * w, np.int64)
    und = cls == UNDECIDED
    np.add.at(count, lab[und], 1)

    def find(x):
        while par[x] != x:
            x = par[x]
        return x

    def pairs():
        for y in range(th, h, th):
            for x in range(w):
                yield (y, x), (y - 1, x)
        for x in range(tw, w, tw):
            for y in range(h):
                yield (y, x), (y, x - 1)

    for p, q in pairs():
        if cls[p] == INVALID or cls[q] == INVALID or (cls[p] == KEEP and cls[q] == KEEP):
            continue
        assert REMOVE not in (cls[p], cls[q])
        if abs(D[p] - D[q]) > thr:
            continue
        if KEEP in (cls[p], cls[q]):
            u = lab[p] if cls[p] == UNDECIDED else lab[q]
            count[u] = max(count[u], min_size)
        else:
            a, b = find(lab[p]), find(lab[q])
            if a != b:
                par[max(a, b)] = min(a, b)
    total = np.zeros(h * w, np.int64)
    for i in np.unique(lab[und]):
        total[find(i)] += count[i]
    keep = cls == KEEP
    for y, x in zip(*np.nonzero(und)):
        keep[y, x] = total[find(lab[y, x])] >= min_size
    return keep, cls


def check_model(D, thr, min_size, tw, th):
    glob = _sizes(_components(D, thr)) >= max(min_size, 1)
    glob &= D >= 0
    keep, cls = kernel_verdict(D, thr, min_size, tw, th)
    # the argument: what a tile settles is right, and the rest is settled by the global size
    assert np.array_equal((cls == KEEP) | ((cls == UNDECIDED) & glob), glob)
    assert not (glob & (cls == REMOVE)).any()
    assert np.array_equal(keep, glob)
    return cls


def speckle_reference(D, thr, min_size):
    """removeSmallSegments on a map: components below min_size become -10, and so does every invalid pixel (a
    segment of one) when min_size > 1"""
    out = D.copy()
    small = _sizes(_components(D, thr)) < min_size
    out[(D >= 0) & small] = -10
    if min_size > 1:
        out[~(D >= 0)] = -10
    return out


def _blank(h, w):
    return np.full((h, w), -10.0, np.float32)


@pytest.mark.parametrize("tw,th", [(8, 4), (64, 16)])
def test_model_planted_components(tw, th):
    m = 12 if tw == 8 else 40                      # min_size; below a tile's pixels and its width + 1
    # a component of exactly min_size pixels split 1 / min_size - 1 across a vertical seam is kept ...
    D = _blank(3 * th, 3 * tw)
    rows = -(-(m - 1) // tw)
    cells = [(th + 1 + k // tw, tw + k % tw) for k in range(m - 1)]
    assert rows <= th - 2
    for y, x in cells:
        D[y, x] = 5
    D[th + 1, tw - 1] = 5
    cls = check_model(D, 1.0, m, tw, th)
    assert cls[th + 1, tw - 1] == UNDECIDED and cls[th + 1, tw] == UNDECIDED and (D >= 0).sum() == m
    assert (kernel_verdict(D, 1.0, m, tw, th)[0] == (D >= 0)).all()
    # ... and one pixel fewer is removed
    D[cells[-1]] = -10
    check_model(D, 1.0, m, tw, th)
    assert not kernel_verdict(D, 1.0, m, tw, th)[0].any()
    # a U whose arms join in the tile below: two undecided components of the upper tile, one below
    for bar in (tw - 2, 2):
        D = _blank(2 * th, 2 * tw)
        D[th - 3:th + 2, 1] = 7
        D[th - 3:th + 2, 1 + bar] = 7
        D[th + 1, 1:2 + bar] = 7
        n = int((D >= 0).sum())
        for ms in (n, n + 1):
            cls = check_model(D, 1.0, ms, tw, th)
            assert (cls[D >= 0] == UNDECIDED).all()
            assert kernel_verdict(D, 1.0, ms, tw, th)[0].any() == (ms == n)
    # a chain of small pieces over four tiles that ends in a large one: kept through the mark alone
    D = _blank(3 * th, 5 * tw)
    D[th + 1, 1:4 * tw] = 9                                     # tiles 0 .. 3 of the middle band
    D[th:2 * th, 4 * tw:5 * tw] = 9                             # the whole last tile
    big = 3 * tw + tw - 1 + tw * th
    cls = check_model(D, 1.0, tw * th, tw, th)
    assert (cls[th + 1, 1:4 * tw] == UNDECIDED).all() and (cls[th:2 * th, 4 * tw:] == KEEP).all()
    assert kernel_verdict(D, 1.0, tw * th, tw, th)[0].sum() == big
    D[th + 1, 2 * tw] = -10                                     # the chain broken: the far part is small
    keep, _ = kernel_verdict(D, 1.0, tw * th, tw, th)
    check_model(D, 1.0, tw * th, tw, th)
    assert not keep[th + 1, :2 * tw].any() and keep[th + 1, 2 * tw + 1:4 * tw].all()
    # the same chain without a large end, kept or not by the sum of its pieces
    D = _blank(3 * th, 5 * tw)
    D[th + 1, 1:4 * tw] = 9
    n = 4 * tw - 1
    assert kernel_verdict(D, 1.0, n, tw, th)[0].sum() == n and not kernel_verdict(D, 1.0, n + 1, tw, th)[0].any()
    # a small component in a tile corner that touches two seams
    D = _blank(3 * th, 3 * tw)
    D[th, tw] = 3
    cls = check_model(D, 1.0, 2, tw, th)
    assert cls[th, tw] == UNDECIDED
    D[th, tw - 1] = D[th - 1, tw] = 3                           # three tiles, three pixels
    for ms in (3, 4):
        check_model(D, 1.0, ms, tw, th)
        assert kernel_verdict(D, 1.0, ms, tw, th)[0].any() == (ms == 3)
    # an image edge is no seam: a small component in the corner of the image is removed in its tile
    D = _blank(2 * th, 2 * tw)
    D[0, 0] = D[2 * th - 1, 2 * tw - 1] = 3
    cls = check_model(D, 1.0, 2, tw, th)
    assert cls[0, 0] == REMOVE and cls[-1, -1] == REMOVE
    # min_size <= 1: everything valid is kept in the tile
    assert (check_model(D, 1.0, 1, tw, th)[D >= 0] == KEEP).all()


@pytest.mark.parametrize("seed", range(6))
def test_model_random_maps(seed):
    rng = np.random.default_rng(seed)
    tw, th = [(8, 4), (5, 3), (16, 4)][seed % 3]
    h, w = int(rng.integers(2 * th + 1, 5 * th)), int(rng.integers(2 * tw + 1, 5 * tw))
    # coarse plateaus (components of every size), speckles and holes
    D = np.kron(rng.integers(0, 4, (h // 3 + 1, w // 3 + 1)), np.ones((3, 3)))[:h, :w].astype(np.float32) * 2
    D[rng.random((h, w)) < 0.25] = -10
    D += (rng.random((h, w)) < 0.1) * 1.5
    seen = set()
    for ms in (1, 2, 5, 20, tw * th + 7):
        for thr in (0.5, 2.5):
            seen |= set(np.unique(check_model(D, thr, ms, tw, th)).tolist())
    assert {KEEP, REMOVE, UNDECIDED, INVALID} <= seen


# ----------------------------------------------------------------------------- GPU: on against off
MASK = [{"filter_median": 1}, {"ipol_gap_width": 6}]        # either one takes the k_seg_mask path


def ab_cases():
    """(seed, w, h, parameters): every case on the tile path and on the mask path"""
    base = []
    seed = 900
    for w in (64, 65, 127, 129, 320):
        for h in (16, 17, 33, 117):
            seed += 1
            base.append((seed, w, h, {}))
    for w, h in ((129, 33), (320, 117)):
        for size in (1, 2, 20, 200, 1100, 5000):
            for thr in (0.5, 2.5):
                seed += 1
                base.append((seed, w, h, {"speckle_size": size, "speckle_sim_threshold": thr}))
    for w, h in ((127, 33), (320, 117), (129, 117)):
        for kw in ({"subsampling": 1}, {"postprocess_only_left": 0},
                   {"subsampling": 1, "postprocess_only_left": 0, "speckle_size": 20}):
            seed += 1
            base.append((seed, w, h, kw))
    out = []
    for k, (s, w, h, kw) in enumerate(base):
        out.append((s, w, h, kw))
        out.append((s, w, h, dict(kw, **MASK[k % 2])))
    return out


def _pair(seed, w, h):
    return H.synth_pair(w, h, seed, dmax=min(40, max(8, w // 4)))


def child_main(path):
    import svhip as S
    S.lib()
    assert S.device_count() > 0, "no HIP device: the product has no CPU fallback"
    out = {}
    for k, (seed, w, h, kw) in enumerate(ab_cases()):
        l, r = _pair(seed, w, h)
        rc, D1, D2 = S.Elas(H.robotics(**kw)).process(l, r)
        out["rc%d" % k] = np.int32(rc)
        out["a%d" % k] = D1
        out["b%d" % k] = D2
    np.savez(path, **out)


@pytest.fixture(scope="module")
def on_off(tmp_path_factory):
    d = tmp_path_factory.mktemp("seg_settle")
    res = []
    for name, val in (("on", None), ("off", "0")):
        env = dict(os.environ)
        env.pop("SVH_SEG_SETTLE", None)
        if val is not None:
            env["SVH_SEG_SETTLE"] = val
        path = str(d / (name + ".npz"))
        subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, timeout=300)
        res.append(np.load(path))
    return res


@gpu
def test_settled_equals_unsettled_bit_for_bit(on_off):
    on, off = on_off
    cases = ab_cases()
    ok = valid = 0
    for k, case in enumerate(cases):
        assert int(on["rc%d" % k]) == int(off["rc%d" % k]), case
        for m in "ab":
            assert np.array_equal(on[m + str(k)].view(np.uint32), off[m + str(k)].view(np.uint32)), (case, m)
        if int(on["rc%d" % k]) == 0:
            ok += 1
            valid += (on["a%d" % k] >= 0).mean() > 0.2
        print(case, "status", int(on["rc%d" % k]), "valid %.3f" % (on["a%d" % k] >= 0).mean())
    print("cases %d, status 0 in %d, more than 20 %% valid in %d" % (len(cases), ok, valid))
    # the comparison must not be one of empty maps (a large speckle_size removes everything from a small map, and
    # the smallest shapes may find too few support points): where components of 20 pixels are kept, much is left
    some = [k for k, c in enumerate(cases) if c[1] >= 127 and c[2] >= 33 and c[3].get("speckle_size", 200) <= 20
            and not c[3].get("subsampling")]
    assert len(some) >= 10
    assert all(int(on["rc%d" % k]) == 0 and (on["a%d" % k] >= 0).mean() > 0.2 for k in some)


# ----------------------------------------------------------------------------- GPU: in this process (switch at its default)
@pytest.fixture(scope="module")
def S():
    import svhip as S
    S.lib()
    assert S.device_count() > 0, "no HIP device: the product has no CPU fallback"
    before = S.elas_settings()
    yield S
    S.set_stage(before["stage"])
    S.set_lanes(before["workers"])
    S.set_group(before["pairs_per_launch"] if before["pairs_per_launch"] > 0 else 32)
    S.trim()


def _taps(S, prm, l, r):
    e = S.Elas(prm)
    e.set_taps(True)
    rc, D1, D2 = e.process(l, r)
    assert rc == 0
    return e, D1, D2


@gpu
@pytest.mark.parametrize("seed,w,h,kw", [
    (941, 320, 117, {}), (942, 129, 33, {"speckle_size": 20, "speckle_sim_threshold": 2.5}),
    (943, 257, 49, {"speckle_size": 1100}), (944, 320, 117, {"subsampling": 1, "speckle_size": 400}),
    (945, 193, 65, {"speckle_size": 2, "speckle_sim_threshold": 0.5, "postprocess_only_left": 0}),
])
def test_speckle_stage_equals_the_model(S, seed, w, h, kw):
    """with taps the stages are kept (the mask path): the map after the speckle filter is removeSmallSegments of the
    map before it, and the three classes all occur in it"""
    prm = H.robotics(**kw)
    l, r = _pair(seed, w, h)
    e, _, _ = _taps(S, prm, l, r)
    min_size = int(np.float32(np.sqrt(np.float32(prm.speckle_size))) * 2) if prm.subsampling else prm.speckle_size
    for before, after in ((H.D1_LR, H.D1_SEG), (H.D2_LR, H.D2_SEG)):
        if after == H.D2_SEG and prm.postprocess_only_left:
            continue
        lr = np.asarray(e.stage(before, H.stage_dtype(before)))
        got = np.asarray(e.stage(after, H.stage_dtype(after)))
        dh = h // 2 if prm.subsampling else h
        lr, got = lr.reshape(dh, -1), got.reshape(dh, -1)
        want = speckle_reference(lr, prm.speckle_sim_threshold, min_size)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        cls, _, _ = classes(lr, prm.speckle_sim_threshold, min_size, TW, TH)
        print("valid %.3f  kept in tile %d  removed in tile %d  undecided %d" % (
            (lr >= 0).mean(), (cls == KEEP).sum(), (cls == REMOVE).sum(), (cls == UNDECIDED).sum()))


ORACLE_SHAPES = [(951, 65, 33, {}), (952, 129, 117, {}), (953, 320, 117, {"speckle_size": 20}),
                 (954, 127, 33, {"speckle_size": 1100, "postprocess_only_left": 0}),
                 (955, 320, 33, {"subsampling": 1, "speckle_sim_threshold": 2.5})]


@gpu
@pytest.mark.skipif(not H.have_ref_elas(), reason="needs oracle/_ref triangulator")
@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("seed,w,h,kw", ORACLE_SHAPES)
def test_final_maps_match_oracle(S, oracle_lib, seed, w, h, kw, mask):
    prm = H.robotics(**dict(kw, **(MASK[0] if mask else {})))
    l, r = _pair(seed, w, h)
    rc, D1, D2 = S.Elas(prm).process(l, r)
    want = H.oracle_elas_run(prm, l, r)
    assert rc == want.status
    if rc == 0:
        assert np.array_equal(D1.ravel(), np.asarray(want[H.D1_FINAL]).ravel())
        assert np.array_equal(D2.ravel(), np.asarray(want[H.D2_FINAL]).ravel())


@gpu
def test_urban_crop_matches_its_golden(S):
    z = np.load(os.path.join(H.GOLDEN, "urban3_kitti.npz"))
    prm = H.ElasParams.from_buffer_copy(z["params"].tobytes())
    l, r = H.golden_pair(str(z["crop"]))
    rc, D1, D2 = S.Elas(prm).process(l, r)
    assert rc == 0
    assert np.array_equal(D1.ravel(), z["d1"]) and np.array_equal(D2.ravel()[:z["d2"].size], z["d2"])


@gpu
@pytest.mark.parametrize("mask", [0, 1])
def test_batches_equal_single_calls(S, mask):
    """four different pairs: in one group of 4, in two groups of 2, and again in another order on the same lanes"""
    prm = H.robotics(**(MASK[0] if mask else {}))
    w, h = 320, 117
    prs = [_pair(960 + i, w, h) for i in range(4)]
    single = []
    for l, r in prs:
        rc, D1, D2 = S.Elas(prm).process(l, r)
        assert rc == 0
        single.append((D1.copy(), D2.copy()))
    S.set_stage(1)
    S.set_lanes(1)
    for group in (4, 2):
        S.trim()
        S.set_group(group)
        e = S.Elas(prm)
        for order in ([0, 1, 2, 3], [2, 3, 1, 0], [3, 0, 2, 1]):
            st, B1, B2 = e.process_batch(np.stack([prs[i][0] for i in order]), np.stack([prs[i][1] for i in order]))
            assert list(st) == [0, 0, 0, 0]
            for k, i in enumerate(order):
                assert np.array_equal(B1[k].view(np.uint32), single[i][0].view(np.uint32)), (group, order, k)
                assert np.array_equal(B2[k].view(np.uint32), single[i][1].view(np.uint32)), (group, order, k)


if __name__ == "__main__":
    child_main(sys.argv[1])

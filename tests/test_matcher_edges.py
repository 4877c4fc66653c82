"""CPU: the proof, on the oracle's output alone, that every generated scene of tests/matcher_scenes.py reaches the
edge it is named for -- a size at which a launcher of csrc/matcher_kernels.hip takes another kernel or another
branch, a tie that only the reference's first-minimum rules decide, a saturated filter, a starved frame.
tests/test_matcher_edges_gpu.py compares the device with the oracle on the same scenes; that comparison is only worth
what the scenes reach, so a scene that stops reaching its edge fails here.

The thresholds are restated from the launchers as constants (never imported from the code under test).  The shapes
are the smallest found by a search that is not part of this file.  Slowest test: the 640 x 480 noise scene, one
oracle pass of about 1.2 s."""
import numpy as np
import pytest

import helpers as H
import matcher_scenes as MS

pytestmark = pytest.mark.skipif(not H.have_ref_viso(), reason="the oracle needs the real Triangle (oracle/_ref)")

# ---- thresholds of csrc/matcher_kernels.hip ------------------------------------------------------------------------
LDS_BIN_INDEX = 56 * 1024        # mlaunch_bin_index: `t_rec || lds <= 56 * 1024` -> k_bin_index_lds, else k_bin_index
LDS_RECORDED = 156 * 1024        # mlaunch_bin_index: `t_rec && lds > 156 * 1024` -> the recorded batch is broken
COMPACT_LDS = 8192               # kCompactLds: survivors whose slot numbers fit d_compact_matches' LDS list
COMPACT_MASKED_QUERIES = 32768   # d_compact_matches: `masked = chunk <= 32`, chunk = ceil(nslots / 1024)
COPY_KERNEL_BYTES = 1 << 20      # mlaunch_copy: by kernel while `bytes <= 1 << 20`, else hipMemcpyAsync
MATCH_BYTES = 48                 # sizeof(svh_p_match)
RANKED_BINS = 2048               # d_bin_index_lds: `ranked = nb < 2048 && ...`
LANES_PER_QUERY = 16             # kQ: a bin with more entries of one class takes find_match's `q4 + kQ` loop
SLOTS_MASKED = 65536             # d_compact_slots: `masked = chunk <= 64`, chunk = ceil(nslots / 1024) rounded up to 4
SLOT_THREADS = 1024              # d_compact_slots: one workgroup of 1024 threads
F1_EXTREME = 4080                # blob5x5 on 0 / 255: -(25 - 9) * 255 + ... = +-16 * 255


def bin_grid(case, prm):
    """(ub, vb) of Matcher::createIndexVector (matcher.cpp:1036-1040)"""
    bs = prm.match_binsize
    return int(np.ceil(np.float32(case.w) / np.float32(bs))), int(np.ceil(np.float32(case.h) / np.float32(bs)))


def lds_need(nb, n):
    """mlaunch_bin_index: (2 nb + 1 + n) ints"""
    return (2 * nb + 1 + n) * 4


_cache = {}


def oracle_run(name, method=2, **more):
    """the oracle's matcher after the case's quad, kept for the tests that look at the same scene"""
    key = (name, method, tuple(sorted(more.items())))
    if key not in _cache:
        c = MS.CASES[name]
        _cache[key] = MS.run(H.OracleMatcher(c.params(**more)), c.quad(), method)
    return _cache[key]


def counts(m):
    return [len(m.features(tb)) for tb in range(8)]


def dense_tables(m):
    return [m.features(tb) for tb in (1, 3, 5, 7)]


def path_figures(name):
    c = MS.CASES[name]
    m = oracle_run(name)
    ub, vb = bin_grid(c, c.params())
    n = counts(m)
    return {"nb": 4 * ub * vb, "n_dense": n[1::2], "nq": n[1], "raw": len(m.stage(H.M_DENSE_RAW)),
            "lds": lds_need(4 * ub * vb, max(n[1::2])), "lds_min": lds_need(4 * ub * vb, min(n[1::2]))}


# ---- size-switched paths -------------------------------------------------------------------------------------------
def test_big_reaches_global_index_broken_recording_unmasked_compaction_and_memcpy():
    """640 x 480 noise: every dense table needs more LDS than k_bin_index_lds gets alone (56 KiB) and than a recorded
    batch gets (156 KiB); more than 32 768 queries (d_compact_matches unmasked); more than 8 192 raw matches; the
    match download is above 1 MiB (hipMemcpyAsync)"""
    f = path_figures("big")
    assert f["lds_min"] > LDS_RECORDED > LDS_BIN_INDEX, f
    assert f["nq"] > COMPACT_MASKED_QUERIES, f
    assert f["raw"] > COMPACT_LDS, f
    assert f["nq"] * MATCH_BYTES > COPY_KERNEL_BYTES, f
    # (one launch decides for all tables of a call by the largest, so the global kernel builds the sparse indices too:
    # eight tables share `cursor`)
    assert len(oracle_run("big").stage(H.M_SPARSE_RAW)) > 1000


def test_middle_reaches_global_index_and_masked_direct_compaction():
    """480 x 320 noise (smallest found around 448 x 320; 464 x 328 has 21 647 queries, 199 short of 1 MiB): global
    k_bin_index, at most 32 768 queries (masked compaction) with more than 8 192 survivors (direct writes), download
    above 1 MiB"""
    f = path_figures("middle")
    assert LDS_BIN_INDEX < f["lds"] <= LDS_RECORDED, f
    assert f["nq"] <= COMPACT_MASKED_QUERIES, f
    assert f["raw"] > COMPACT_LDS, f
    assert f["nq"] * MATCH_BYTES > COPY_KERNEL_BYTES, f


def test_natural_reaches_global_index():
    """the KITTI quad at 640 x 480: a natural image's features come in clumps, so the arrival order of the global
    k_bin_index's atomics is far from the index order its insertion sort restores (on noise the two nearly agree)"""
    f = path_figures("natural")
    assert LDS_BIN_INDEX < f["lds_min"] and f["lds"] <= LDS_RECORDED, f
    assert f["raw"] > COMPACT_LDS, f


def test_small_reaches_lds_index_with_masked_direct_compaction():
    """320 x 200 noise (304 x 208 has 8 077 raw matches): the LDS bin index still holds, more than 8 192 survivors,
    download by kernel"""
    f = path_figures("small")
    assert f["lds"] <= LDS_BIN_INDEX, f
    assert COMPACT_LDS < f["raw"] and f["nq"] <= COMPACT_MASKED_QUERIES, f
    assert f["nq"] * MATCH_BYTES <= COPY_KERNEL_BYTES, f


def test_under_is_the_largest_lds_list():
    """default parameters on 1024 x 512 noise of 2 x 2 cells: a raw dense match count in (7 000, 8 192], the upper
    end of d_compact_matches' LDS list"""
    f = path_figures("under")
    assert 7000 < f["raw"] <= COMPACT_LDS, f
    assert f["lds"] <= LDS_BIN_INDEX, f


def fullest_bin(case, prm, table):
    """largest number of entries one (class, v_bin, u_bin) holds: matcher.cpp:1043-1056"""
    ub, vb = bin_grid(case, prm)
    bs = np.float32(prm.match_binsize)
    u = np.minimum(np.floor(table[:, 0].astype(np.float32) / bs).astype(int), ub - 1)
    v = np.minimum(np.floor(table[:, 1].astype(np.float32) / bs).astype(int), vb - 1)
    return int(np.bincount((table[:, 3] * vb + v) * ub + u, minlength=4 * ub * vb).max())


@pytest.mark.parametrize("name,ranked", [("ranked_off", False), ("ranked_on", True)])
def test_ranked_switch_with_bins_above_one_pass_of_lanes(name, ranked):
    """d_bin_index_lds ranks entries by packed (bin, id) while nb < 2048 and insertion-sorts above; both cases have a
    bin with more than kQ = 16 entries of one class, so find_match's second pass over a bin runs"""
    c = MS.CASES[name]
    f = path_figures(name)
    assert (f["nb"] < RANKED_BINS) == ranked, f
    assert f["lds"] <= LDS_BIN_INDEX, f
    m = oracle_run(name)
    assert max(fullest_bin(c, c.params(), t) for t in dense_tables(m)) > LANES_PER_QUERY
    assert len(m.stage(H.M_DENSE)) > 1000


# ---- slot compaction -----------------------------------------------------------------------------------------------
def test_slot_sizes_sit_on_the_compaction_boundaries():
    """nslots = 4 ni nj of d_compact_slots for the committed sizes: 1, 2, 3 blocks (dense and sparse), just under
    1 024 (threads with an empty chunk), ceil(nslots / 1024) no multiple of 4 (the chunk is rounded up), exactly
    65 536 (the last masked size) and 66 048 = 4 x 129 x 128, one more column of blocks.  nslots and the chunk are
    both multiples of 4, so the scalar tail of the masked branch's 16-byte flag loads is never taken by a table"""
    got = {}
    for (w, h, n, what) in MS.SLOT_SIZES:
        dense, sparse = MS.nslots(w, h, n), MS.nslots(w, h, MS.sparse_n(n))
        got[what] = (dense, sparse)
    assert [got[k][0] for k in ("dense1", "dense2", "dense3")] == [4, 8, 12]
    assert [got[k][1] for k in ("dense1", "dense2", "dense3")] == [0, 0, 0]
    assert [got[k][1] for k in ("sparse1", "sparse2", "sparse3")] == [4, 8, 12]
    assert SLOT_THREADS - 8 <= got["under1024"][0] < SLOT_THREADS
    chunks = -(-got["ragged_chunk"][0] // SLOT_THREADS)
    assert chunks % 4 != 0 and chunks > 1
    assert got["masked_last"][0] == SLOTS_MASKED
    assert got["unmasked_first"][0] == SLOTS_MASKED + 4 * 128


@pytest.mark.parametrize("size", MS.SLOT_SIZES, ids=lambda s: s[3])
def test_slot_sizes_have_features(size):
    """the oracle finds features in the table the size is named for (an empty table would compact nothing)"""
    w, h, n, what = size
    c = MS.slot_case(size)
    m = H.OracleMatcher(c.params())
    q = c.quad()
    m.push_back(q[0], q[1])
    t = m.features(4 if what.startswith("sparse") else 5)
    assert 0 < len(t) <= (MS.nslots(w, h, MS.sparse_n(n)) if what.startswith("sparse") else MS.nslots(w, h, n))


# ---- ties ----------------------------------------------------------------------------------------------------------
def duplicated(table):
    """features that share class and descriptor with another feature of the table"""
    key = np.ascontiguousarray(table[:, 3:12]).view(np.dtype((np.void, 36))).ravel()
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return int((cnt[inv.ravel()] > 1).sum())


def tied_queries(t1, t2, radius, vtol, sample):
    """queries of t1 (every `sample`-th) whose minimum cost over the candidates of t2 inside the window of a pass
    without a prior (matcher.cpp:1075-1090: u +- match_radius, v +- match_disp_tolerance) is attained twice or more"""
    d2 = np.ascontiguousarray(t2[:, 4:12]).view(np.uint8).reshape(len(t2), 32).astype(np.int32)
    tied = 0
    for q in t1[::sample]:
        ok = (t2[:, 3] == q[3]) & (np.abs(t2[:, 0] - q[0]) <= radius) & (np.abs(t2[:, 1] - q[1]) <= vtol)
        if ok.sum() < 2:
            continue
        d1 = np.ascontiguousarray(q[4:12]).view(np.uint8).astype(np.int32)
        cost = np.abs(d2[ok] - d1).sum(axis=1)
        tied += int((cost == cost.min()).sum() >= 2)
    return tied


@pytest.mark.parametrize("name", ["periodic", "periodic16"])
def test_periodic_tables_repeat_descriptors_and_ties_decide(name):
    """one random tile repeated: thousands of features share their 32-byte descriptor, and in the first stage of a
    pass without a prior (multi_stage = 0) the minimum SAD of a query is attained by several candidates, so the match
    index is whatever the walk order (u-bin outer, v-bin inner, list order) meets first"""
    c = MS.CASES[name]
    m = oracle_run(name, multi_stage=0)
    t1p, t2p = m.features(1), m.features(3)
    assert duplicated(t1p) >= 1000 and duplicated(t2p) >= 1000
    prm = c.params()
    assert tied_queries(t1p, t2p, prm.match_radius, prm.match_disp_tolerance, 8) >= 100


def test_binary8_repeats_descriptors():
    """cells of 8 x 8: long flat runs, where the Sobel planes are 128 and whole descriptors repeat"""
    assert min(duplicated(t) for t in dense_tables(oracle_run("binary8"))) >= 1000


def nms_ties(f, n, tau, w, h, margin=MS.MARGIN):
    """(blocks whose extremum passes tau and is attained at two or more pixels of the block,
        blocks whose extremum passes tau, meets an EQUAL value outside the block inside its +-n neighbourhood and no
        value that beats it: the strict vote of matcher.cpp:437-452 keeps these)  -- minima and maxima of one plane"""
    n1 = n + 1
    inside = voted = 0
    for i in range(n + margin, w - n - margin, n1):
        for j in range(n + margin, h - n - margin, n1):
            blk = f[j:j + n1, i:i + n1].T          # [di][dj]: the scan is i outer, j inner
            for sign in (1, -1):
                v = sign * blk
                l = int(np.argmin(v))              # first minimum in scan order
                ext = int(v.flat[l])
                if ext > -tau:
                    continue
                inside += int((v == ext).sum() >= 2)
                ci, cj = i + l // n1, j + l % n1
                ie, je = min(ci + n, w - 1 - margin), min(cj + n, h - 1 - margin)
                nb = sign * f[cj - n:je + 1, ci - n:ie + 1].astype(np.int32)
                out = np.ones(nb.shape, bool)
                out[max(j - (cj - n), 0):j + n - (cj - n) + 1, max(i - (ci - n), 0):i + n - (ci - n) + 1] = False
                if (nb[out] < ext).any():
                    continue
                voted += int((nb[out] == ext).any())
    return inside, voted


@pytest.mark.parametrize("name", ["levels3", "levels4c2"])
def test_levels_put_ties_into_the_nms(name):
    """few grey levels: equal f1 / f2 inside one (n+1)^2 block (d_nms' scan-order key decides which pixel is the
    feature) and equal values just outside it (the vote is strict: an equal value must not suppress)"""
    c = MS.CASES[name]
    prm = c.params()
    m = oracle_run(name)
    inside = voted = 0
    for which in (4, 5):
        f, dims = m.filter_image(which)
        a, b = nms_ties(f.astype(np.int32), prm.nms_n, prm.nms_tau, dims[0], dims[1])
        inside, voted = inside + a, voted + b
    assert inside >= 100 and voted >= 20, (inside, voted)


# ---- saturation ----------------------------------------------------------------------------------------------------
def test_binary3_saturates_the_blob_filter():
    """cells of 0 / 255, 3 x 3: f1 reaches both ends of its range, the largest magnitudes the packed 16-bit
    arithmetic of d_filters ever holds"""
    f1, _ = oracle_run("binary3").filter_image(4)
    assert f1.min() == -F1_EXTREME and f1.max() == F1_EXTREME


@pytest.mark.parametrize("vertical", [True, False])
def test_sobel_cannot_reach_its_clamp(vertical):
    """a 0 | 255 | 0 bar: the 5x5 Sobel sums to at most (1 + 2) * 16 * 255 = 12 240, >> 7 that is 95 (-96 for the
    negative sum), so du / dv stay in [128 - 96, 128 + 95] = [32, 223] and the clamp to [0, 255] of filter.cpp is
    unreachable for 8-bit input.  The bar attains both ends; the plane across it stays at 128.  Noise and the 0 / 255
    cells stay inside the same range"""
    q = MS.bar_quad(64, 48, vertical, 24)
    m = H.OracleMatcher(H.matcher_defaults(half_resolution=0))
    m.push_back(q[0], q[1])
    d = m.filter_image(0 if vertical else 1)[0][2:-2, 2:-2]
    o = m.filter_image(1 if vertical else 0)[0][2:-2, 2:-2]
    assert (int(d.min()), int(d.max())) == (32, 223)
    assert (int(o.min()), int(o.max())) == (128, 128)
    for name in ("big", "binary3"):
        for which in (0, 1):
            p = oracle_run(name).filter_image(which)[0][2:-2, 2:-2]
            assert 32 <= p.min() < 128 < p.max() <= 223, (name, which, p.min(), p.max())


# ---- degenerate frames ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["constant", "tiny16", "tiny16h", "tiny24", "tiny24h", "half_of_33x31"])
def test_empty_tables(name):
    """a constant image, and images too small for one NMS block at either resolution: eight empty tables, no match"""
    m = oracle_run(name)
    assert counts(m) == [0] * 8 and len(m.matches()) == 0


def test_dense_without_sparse():
    """33 x 31 at full resolution: room for dense NMS blocks (n = 3) and for no sparse one (n = 9), so matchFeatures
    returns silently (matcher.cpp:216-259)"""
    n = counts(oracle_run("dense_only"))
    assert n[0::2] == [0] * 4 and min(n[1::2]) > 0 and len(oracle_run("dense_only").matches()) == 0


def test_handful():
    """64 x 48 at full resolution: a handful of sparse matches carry the whole prior"""
    m = oracle_run("handful")
    assert 0 < len(m.stage(H.M_SPARSE)) <= 16 and 0 < len(m.matches())


def test_blank_right_camera_has_one_empty_side():
    c = MS.CASES["ranked_on"]
    m = MS.run(H.OracleMatcher(c.params()), MS.blank_right(c))
    n = counts(m)
    assert n[2] == n[3] == n[6] == n[7] == 0 and min(n[0], n[1], n[4], n[5]) > 0 and len(m.matches()) == 0


def test_filter_sizes_cover_the_block_geometry():
    """(a parameter list, not a property: d_filters' block is 256 x 32, a thread 4 x 8, bpl = w rounded up to 16)"""
    ws = {w for w, h, half in MS.FILTER_SIZES}
    hs = {h for w, h, half in MS.FILTER_SIZES if not half}
    assert {255, 256, 257, 1025} <= ws and {w % 16 for w in ws} >= {0, 1, 15}
    assert {31, 32, 33} <= hs and {h % 8 for h in hs} >= {0, 1, 7}
    assert any(half and w % 2 and h % 2 for w, h, half in MS.FILTER_SIZES)


# ---- refinement ties -----------------------------------------------------------------------------------------------
def sobel_planes(img, half):
    """(du, dv) at full resolution of one frame, from the oracle"""
    m = H.OracleMatcher(H.matcher_defaults(half_resolution=half))
    m.push_back(img, img)
    return m.filter_image(2 if half else 0)[0].astype(np.int32), m.filter_image(3 if half else 1)[0].astype(np.int32)


def small_desc(du, dv, u, v):
    """Matcher::computeSmallDescriptor (matcher.cpp:583-611), u and v arrays"""
    return np.stack([du[v - 2, u], du[v - 1, u - 2], du[v - 1, u], du[v - 1, u + 2], du[v, u - 1], du[v, u], du[v, u],
                     du[v, u + 1], du[v + 1, u - 2], du[v + 1, u], du[v + 1, u + 2], du[v + 2, u],
                     dv[v - 1, u], dv[v, u - 1], dv[v, u + 1], dv[v + 1, u]], axis=-1)


def search_costs(ref, tgt, u1, v1, u2, v2, r, w, h, margin=MS.MARGIN):
    """cost grids [match][dv][du] of the (2r+1)^2 search of relocateMinimum (r = 2) / parabolicFitting (r = 3) for the
    matches that pass the border test (matcher.cpp:1586-1590, 1676-1680), and their indices"""
    ok = (u2 - r >= margin) & (u2 + r <= w - 1 - margin) & (v2 - r >= margin) & (v2 + r <= h - 1 - margin)
    idx = np.nonzero(ok)[0]
    d1 = small_desc(ref[0], ref[1], u1[idx], v1[idx])
    k = 2 * r + 1
    cost = np.zeros((len(idx), k, k), np.int32)
    for dy in range(k):
        for dx in range(k):
            d2 = small_desc(tgt[0], tgt[1], u2[idx] + dx - r, v2[idx] + dy - r)
            cost[:, dy, dx] = np.abs(d1 - d2).sum(axis=-1)
    return cost, idx


def refinement_figures(name, r):
    """over the raw dense matches of the case and the three searched frames: (searches whose first and last minimum
    differ, searches whose first minimum lies on the border of the window, searches with an interior first minimum
    whose quadratic fit is degenerate: |divisor| or |b2| < 1e-8 as in matcher.cpp:1747)"""
    c = MS.CASES[name]
    m = oracle_run(name)
    raw = m.stage(H.M_DENSE_RAW)
    q = c.quad()
    half = c.params().half_resolution
    planes = [sobel_planes(img, half) for img in q]          # 1p, 2p, 1c, 2c
    iv = lambda f: raw[f].astype(np.int64)
    two = border = flat = 0
    A = np.array([[1, 1, 1, -1, -1, 1], [0, 1, 0, 0, -1, 1], [1, 1, -1, 1, -1, 1], [1, 0, 0, -1, 0, 1],
                  [0, 0, 0, 0, 0, 1], [1, 0, 0, 1, 0, 1], [1, 1, -1, -1, 1, 1], [0, 1, 0, 0, 1, 1],
                  [1, 1, 1, 1, 1, 1]], np.float64)          # matcher.cpp:1725-1733
    for tgt, fu, fv in ((planes[0], "u1p", "v1p"), (planes[3], "u2c", "v2c"), (planes[1], "u2p", "v2p")):
        cost, idx = search_costs(planes[2], tgt, iv("u1c"), iv("v1c"), iv(fu), iv(fv), r, c.w, c.h)
        k = 2 * r + 1
        flatc = cost.reshape(len(idx), -1)
        first = flatc.argmin(axis=1)
        last = k * k - 1 - flatc[:, ::-1].argmin(axis=1)
        two += int((first != last).sum())
        fx, fy = first % k, first // k
        on_border = (fx == 0) | (fx == k - 1) | (fy == 0) | (fy == k - 1)
        border += int(on_border.sum())
        for i in np.nonzero(~on_border)[0][:4000]:
            c9 = cost[i, fy[i] - 1:fy[i] + 2, fx[i] - 1:fx[i] + 2].astype(np.float64).ravel()
            x = np.linalg.solve(A.T @ A, A.T @ c9)
            flat += int(abs(np.float32(x[2] * x[2] - 4 * x[0] * x[1])) < 1e-8 or abs(x[2]) < 1e-8)
    return two, border, flat


def test_relocation_minimum_is_attained_twice():
    """0 / 255 cells: the 5 x 5 search of relocateMinimum meets its minimum cost at several positions (8 x 8 cells:
    flat Sobel planes, over a thousand searches; 3 x 3 cells: a few dozen), so relocate_group's (cost << 5) | lane key
    decides where the match moves"""
    assert refinement_figures("binary8", 2)[0] >= 1000
    assert refinement_figures("binary3", 2)[0] >= 20


def test_parabolic_search_reaches_border_drop_and_degenerate_fit():
    """the 7 x 7 search of parabolicFitting on the same scenes: first minima that differ from the last ones, first
    minima on the window's border (match dropped), and interior minima whose fit is degenerate (match dropped).  A
    first minimum cannot sit in a flat 3 x 3 patch (the equal cost above it would have come first), so the degenerate
    fits are those whose mixed term vanishes: c(-1,-1) + c(1,1) == c(-1,1) + c(1,-1) makes b2 = 0 up to rounding"""
    two, border, flat = refinement_figures("binary3", 3)
    assert two >= 20 and border >= 20 and flat >= 20, (two, border, flat)
    two, border, _ = refinement_figures("binary8", 3)
    assert two >= 1000 and border >= 1000, (two, border)
    for name in ("binary3", "binary8"):
        m = oracle_run(name, refinement=2)
        assert len(m.stage(H.M_DENSE_REFINED)) < len(m.stage(H.M_DENSE_RAW))

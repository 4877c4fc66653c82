"""CPU: the inputs of tests/test_map_edges_gpu.py and the proof, on the oracle's output alone, that each of them meets
the edge it is named for.  The map fusion (include/svh_map.h, csrc/map_kernels.hip) is compared with
oracle/map_oracle.cpp bit for bit; a comparison is only worth what its inputs reach, so this file builds them and
asserts on what the ORACLE makes of them:

 * sizes: the 64 x 4 tiles of k_map_create, the 1024-element blocks of k_map_count / k_map_scatter (scan order is column
   by column, so 683 x 3 and 89 x 23 differ strongly from raster order), the 1024-block chunks of k_map_scan (1024 x 1024:
   one chunk; 1025 x 1024: one carry; 2049 x 1024: two), the gain margin min(200, w/2, h/2) at 0, 1, 2, where w/2
   decides (portrait) and at its cap;
 * hand-built geometry (f = 64, cu = 32, cv = 16 on a 64 x 32 frame, pure translations, disparities that keep x, y, z
   and the re-projection exact): z == float32(0.1), z == max_dist and the float below it, for the current frame's z and
   for the previous map's z2; a closeness sum of exactly float32(0.2) and of the float below; re-projections into
   (-1, 0), onto 0, into (cw - 1, cw) and onto cw; points on and behind the second camera's plane; three previous
   points of different 256-blocks on one target, whose result depends on the replay order; NaN, +-inf, -0.0, a denormal
   and FLT_MAX as disparities; gains that take the lower and the upper clamp of the ramp.

Every builder is deterministic (a seed or hand-written cells).  The GPU file imports this one as a module."""
import numpy as np
import pytest

import test_map as M

F32 = np.float32
EYE = np.eye(4)


class Case:
    def __init__(self, name, prm, frames, **cells):
        self.name, self.prm, self.frames, self.cells = name, tuple(F32(v) for v in prm), frames, cells


def shift(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, tz)
    return T


# ---- A: sizes -------------------------------------------------------------------------------------------------------
TILE_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 2), (5, 4), (63, 3), (64, 4), (65, 5), (33, 65)]
BLOCK_SIZES = [(1023, 1), (32, 32), (41, 25), (89, 23), (683, 3)]
CHUNK_SIZES = [(1024, 1024), (1025, 1024), (2049, 1024)]
MARGIN = {(1, 1): 0, (1, 7): 0, (7, 1): 0, (2, 2): 1, (3, 2): 1, (5, 4): 2, (63, 3): 1, (64, 4): 2, (65, 5): 2,
          (33, 65): 16, (1023, 1): 0, (32, 32): 16, (41, 25): 12, (89, 23): 11, (683, 3): 1,
          (1024, 1024): 200, (1025, 1024): 200, (2049, 1024): 200}


def thin_frames(w, h, n, seed, step=0.12, valid=0.8):
    """synth_frames' scene for frames thinner than three pixels (it writes three marker cells up to [2, 2]):
    the principal point in the middle, so that a 1-pixel-wide frame still sees its own points again"""
    rng = np.random.default_rng(seed)
    f, cu, cv, base = 0.9 * max(w, h, 8), w / 2, h / 2, 0.54
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = []
    for k in range(n):
        # no rotation: one about the long axis would move every point off a frame that is one pixel high
        Ht = shift(0.02 * k if w >= h else 0.0, 0.0 if w >= h else -0.01 * k, step * k)
        depth = 4.0 + 3.0 * np.sin(xx / w * 3 + 0.3) + 2.0 * (yy / h) - step * k
        d = (f * base / depth).astype(np.float32)
        d *= rng.uniform(0.99, 1.01, d.shape).astype(np.float32)
        d[rng.random(d.shape) > valid] = -1
        img = rng.integers(0, 256, (h, w)).astype(np.uint8)
        frames.append((d, img, Ht, np.float32([0.0, 1.07][k % 2])))
    return (F32(f), F32(cu), F32(cv), F32(base)), frames


def size_case(w, h, seed=11, valid=0.8):
    gen = M.synth_frames if (w >= 3 and h >= 3) else thin_frames
    (f, cu, cv, base), frames = gen(w, h, 2, seed, valid=valid)
    return Case("size_%dx%d" % (w, h), (f, cu, cv, base, 20), frames)


def scan_index(w, h):
    """[h, w] array of every pixel's position in the reference's scan order (columns left to right)"""
    return (np.arange(w)[None, :] * h + np.arange(h)[:, None]).astype(np.int64)


def last_block_case():
    """89 x 23 = 2047 pixels, two scan-order blocks.  Frame 0 has no valid pixel (both lists empty), frame 1 has
    valid pixels in the last scan-order block only, frame 2 is an ordinary frame from a moved camera"""
    w, h = 89, 23
    (f, cu, cv, base), fr = M.synth_frames(w, h, 3, seed=12)
    d0 = np.full((h, w), -1, F32)
    d0[::3, ::2] = 0.0
    d1 = fr[1][0].copy()
    d1[scan_index(w, h) < 1024] = -1
    frames = [(d0, fr[0][1], fr[0][2], fr[0][3]), (d1, fr[1][1], fr[1][2], fr[1][3]), fr[2]]
    return Case("last_block_89x23", (f, cu, cv, base, 20), frames)


def chunk_case(w, h):
    c = size_case(w, h, seed=13, valid=0.5)
    c.name = "chunk_%dx%d" % (w, h)
    return c


def second_chunk_only_case():
    """1025 x 1024: only the pixels of scan-order block 1024 -- the last column -- are valid, so k_map_scan's first
    chunk sums to 0 and the whole total comes from its one-element second chunk"""
    w, h = 1025, 1024
    (f, cu, cv, base), fr = M.synth_frames(w, h, 2, seed=14, valid=0.5)
    frames = []
    for d, img, Ht, gain in fr:
        d = d.copy()
        d[:, :1024] = -1
        frames.append((d, img, Ht, gain))
    return Case("second_chunk_only_1025x1024", (f, cu, cv, base, 20), frames)


# ---- B: hand-built geometry ------------------------------------------------------------------------------------------
W, HH = 64, 32          # cu = 32 and cv = 16 are powers of two: cu * z is exact whatever z's mantissa is


def blank():
    return np.full((HH, W), -1, F32)


def image(seed):
    return np.random.default_rng(seed).integers(0, 256, (HH, W)).astype(np.uint8)


def z_min_case():
    """base = float32(0.1) * 16, so f * base = float32(0.1) * 1024 and d = 1024 gives z == float32(0.1), which the
    double comparison z > 0.1 accepts (a float comparison z > 0.1f would not).  One ulp up in d: rejected.
    Frame 2 repeats frame 1 (z2 == float32(0.1) passes, the point merges with itself), frame 3 is empty (it fills)"""
    base = F32(0.1) * F32(16)
    D = blank()
    D[16, 32] = 1024                                   # x = y = 0, z = float32(0.1)
    D[16, 16] = np.nextafter(F32(1024), F32(np.inf))   # z below 0.1
    D[8, 32] = 512                                     # z = 2 * float32(0.1): an ordinary point
    frames = [(D, image(1), EYE, F32(0)), (D.copy(), image(2), EYE, F32(1.07)), (blank(), image(3), EYE, F32(0))]
    return Case("z_min", (64, 32, 16, base, 20), frames, keep=(32, 16), drop=(16, 16), plain=(32, 8))


def z_max_case():
    """base = the float below 0.5, max_dist = 16: f * base is the float below 32, so d = 2 gives the float below 16
    (kept) and d = the float below 2 gives exactly 16 (rejected: z < max_dist is strict).  Frame 2 (empty, same
    pose): z2 is that float below 16 and passes, the point fills its own pixel.  Frame 3 (empty, camera 2^-20 back):
    z2 = 16 exactly, the point stays in the previous list"""
    base = np.nextafter(F32(0.5), F32(0))
    D = blank()
    D[16, 32] = 2
    D[16, 16] = np.nextafter(F32(2), F32(0))
    frames = [(D, image(4), EYE, F32(0)), (blank(), image(5), EYE, F32(0)),
              (blank(), image(6), shift(tz=-2.0 ** -20), F32(0))]
    return Case("z_max", (64, 32, 16, base, 16), frames, keep=(32, 16), drop=(16, 16))


def closeness(x1, y1, z1, x2, y2, z2):
    """fabs(float) + fabs(float) + fabs(float), left to right, in float32"""
    return (np.abs(F32(x1) - x2) + np.abs(F32(y1) - y2)) + np.abs(F32(z1) - z2)


def find_d2(u, v, d1, want):
    """a frame-2 disparity at pixel (u, v) whose point is at closeness `want` (a float32) from the frame-1 point of
    disparity d1 at that pixel (identity poses, f = 64, base = 0.5); None when the scanned floats hold none"""
    du, dv, b, fb = F32(u - 32), F32(v - 16), F32(0.5), F32(64) * F32(0.5)
    d1 = F32(d1)
    x1, y1, z1 = du * b / d1, dv * b / d1, fb / d1
    k = (abs(float(du)) + abs(float(dv))) * 0.5 + 32.0
    guess = F32(1.0 / (1.0 / float(d1) + float(want) / k))          # the farther of the two solutions
    cand = (guess + np.arange(-30000, 30001, dtype=np.float64) * float(np.spacing(guess))).astype(F32)
    dist = closeness(x1, y1, z1, du * b / cand, dv * b / cand, fb / cand)
    hit = np.flatnonzero(dist == want)
    return None if len(hit) == 0 else cand[hit[len(hit) // 2]]


DIST_AT = F32(0.2)                                   # > 0.2 as a double: does not merge
DIST_BELOW = np.nextafter(F32(0.2), F32(0))           # < 0.2: merges
DIST_CELLS = dict(at=(4, 0), below=(60, 30), zero=(48, 8), fill=(8, 24))
DIST_D1 = 256        # z = 0.125: both z and the sum lie where floats are 2^-26 apart, as float32(0.2) needs


def dist_case():
    """one previous and one current point per named pixel (identity poses, so a previous point with d = 256
    re-projects onto its own pixel exactly): closeness exactly float32(0.2) -> not merged, the previous point stays
    in list 0; the float below -> merged; the same point again (0) -> averages to itself; no current point -> fills"""
    D1, D2 = blank(), blank()
    for name, (u, v) in DIST_CELLS.items():
        D1[v, u] = DIST_D1
    found = {}
    for name, want in (("at", DIST_AT), ("below", DIST_BELOW)):
        u, v = DIST_CELLS[name]
        found[name] = find_d2(u, v, DIST_D1, want)
        if found[name] is not None:
            D2[v, u] = found[name]
    u, v = DIST_CELLS["zero"]
    D2[v, u] = DIST_D1
    frames = [(D1, image(7), EYE, F32(0)), (D2, image(8), EYE, F32(0))]
    return Case("dist", (64, 32, 16, 0.5, 20), frames, found=found, **DIST_CELLS)


# previous points (u, v, d) -> where the second pose puts them: a cell (u2, v2) or None = outside, stays in list 0.
# base = 0.5 and a camera moved by (t, t, 0): u2 = u - 2 t d, v2 = v - 2 t d, all exact
BORDER = {
    "lo": (0.25, [((0, 10, 1), (0, 9)),       # u2 = -0.5 -> column 0 (a floor would say -1)
                  ((10, 0, 1), (9, 0)),       # v2 = -0.5 -> row 0
                  ((0, 0, 1), (0, 0)),        # both
                  ((1, 12, 2), (0, 11)),      # u2 = 0 exactly
                  ((12, 1, 2), (11, 0)),      # v2 = 0 exactly
                  ((0, 20, 2), None),         # u2 = -1
                  ((20, 0, 2), None)]),       # v2 = -1
    "hi": (-0.25, [((63, 10, 1), (63, 10)),   # u2 = 63.5 -> last column
                   ((20, 31, 1), (20, 31)),   # v2 = 31.5 -> last row
                   ((63, 31, 1), (63, 31)),   # both
                   ((62, 5, 2), (63, 6)),     # u2 = 63 exactly
                   ((63, 14, 2), None),       # u2 = 64 = cw: outside
                   ((24, 31, 2), None)]),     # v2 = 32 = chh: outside
}


def border_case(side):
    t, pts = BORDER[side]
    D = blank()
    for (u, v, d), _ in pts:
        D[v, u] = d
    frames = [(D, image(9), EYE, F32(0)), (blank(), image(10), shift(t, t, 0), F32(0))]
    return Case("border_" + side, (64, 32, 16, 0.5, 64), frames)


def behind_case():
    """w2 == 0 and w2 < 0.  The third row of K is (0, 0, 1), so pfc[8..11] == hfc[0..3] and w2 is z2 bit for bit:
    whatever the pose, a point with w2 <= 0 has already failed z2 > 0.1, and the division by w2 == 0 (inf or NaN ->
    INT_MIN) cannot be reached.  Kept is the case that comes closest: a point exactly on the second camera's plane
    (z2 = 0), one behind it (z2 = -4) -- both must stay in list 0 -- and one in front that moves on"""
    D = blank()
    D[16, 32] = 4         # z = 8
    D[16, 16] = 8         # z = 4
    D[20, 40] = 2         # z = 16
    frames = [(D, image(11), EYE, F32(0)), (blank(), image(12), shift(tz=8.0), F32(0))]
    return Case("behind", (64, 32, 16, 0.5, 64), frames, on=(32, 16), behind=(16, 16), front=(40, 20))


TIE_PTS = [(32, 24, 64.0), (33, 20, 32 / 0.65), (34, 16, 40.0)]     # in scan order; z = 0.5, 0.65, 0.8


def ties_case():
    """three previous points of three different 256-thread blocks of k_map_project (pixel indices 1568, 1313, 1058:
    blocks 6, 5, 4 -- scan order is the reverse of index order) seen from 15.5 m further back, where all land on
    pixel (32, 16), which is empty.  In scan order the first fills, the second is within 0.2 and merges, the third is
    too far from the average and stays; in the reverse order the first fills and nothing merges"""
    D = blank()
    for u, v, d in TIE_PTS:
        D[v, u] = d
    frames = [(D, image(13), EYE, F32(0)), (blank(), image(14), shift(tz=-15.5), F32(0))]
    return Case("ties", (64, 32, 16, 0.5, 64), frames, target=(32, 16))


def replay(pts):
    """k_map_fuse / stereothread.cpp:340-375 for one empty target pixel: pts = (x, y, z, val) rows in replay order.
    Returns the cell and the indices of the points that stay"""
    cell, stay = None, []
    for i, p in enumerate(np.asarray(pts, F32)):
        if cell is None:
            cell = p.copy()
        elif float(closeness(p[0], p[1], p[2], cell[0], cell[1], cell[2])) < 0.2:
            cell = ((cell + p).astype(np.float64) / 2.0).astype(F32)
        else:
            stay.append(i)
    return cell, stay


NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(F32)[0]
ODD = [("nan", NAN_PAYLOAD), ("pinf", F32(np.inf)), ("ninf", F32(-np.inf)), ("nzero", F32(-0.0)),
       ("denormal", F32(1e-40)), ("fltmax", np.finfo(F32).max)]


def nonfinite_case():
    """frame 1: the odd disparities in row 4, ordinary points (d = 4, z = 8, re-projecting onto themselves) in row 20;
    frame 2 (same pose) the other way round, so every odd cell is also the target of a previous point; frame 3 empty"""
    D1, D2 = blank(), blank()
    for k, (_, val) in enumerate(ODD):
        D1[4, 4 + 8 * k] = val
        D2[20, 4 + 8 * k] = val
        D1[20, 4 + 8 * k] = 4
        D2[4, 4 + 8 * k] = 4
    frames = [(D1, image(15), EYE, F32(0)), (D2, image(16), EYE, F32(0.93)), (blank(), image(17), EYE, F32(0))]
    return Case("nonfinite", (64, 32, 16, 0.5, 20), frames)


GAINS = [-0.5, -0.0, 1e-30, 1e30, 0.93]


def gain_case():
    """one frame per gain over a static scene (every point merges with itself, so I is averaged too).  The image has
    0, 255 and values between inside the 16-pixel margin; the last frame (0.93) is all 255"""
    rng = np.random.default_rng(18)
    frames = []
    for k, g in enumerate(GAINS):
        img = rng.choice(np.array([0, 255, 1, 77, 254], np.uint8), (HH, W)).astype(np.uint8)
        if k == len(GAINS) - 1:
            img[:] = 255
        frames.append((np.full((HH, W), 4, F32), img, EYE, F32(g)))
    return Case("gain", (64, 32, 16, 0.5, 20), frames)


HAND_CASES = {"z_min": z_min_case, "z_max": z_max_case, "dist": dist_case, "border_lo": lambda: border_case("lo"),
              "border_hi": lambda: border_case("hi"), "behind": behind_case, "ties": ties_case,
              "nonfinite": nonfinite_case, "gain": gain_case}

_results = {}


def run_oracle(L, case):
    """[(list 0, list 1, planes)] after every frame; cached per case name, never modified by a test"""
    if case.name not in _results:
        o = M.OracleMapper(M.oracle_map(L), M.MapParams(*case.prm))
        out = []
        for d, img, Ht, gain in case.frames:
            o.add(d, img, Ht, gain)
            out.append((o.points(0), o.points(1), o.planes()))
        _results[case.name] = out
    return _results[case.name]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def at(planes, cell):
    u, v = cell
    return planes[:, v, u]          # I, D, X, Y, Z


def xyz_rows(p):
    return {tuple(bits(r[:3]).tolist()) for r in p}


def xyz_key(pl):
    return tuple(bits(pl[2:5]).tolist())


# ---- A on the oracle -------------------------------------------------------------------------------------------------
def margin_mask(w, h, m):
    """the pixels createCurrentMap's gain ramp touches"""
    mask = np.zeros((h, w), bool)
    if m > 0:
        mask[:m, m:w - m] = True
        mask[h - m:, m:w - m] = True
        mask[m:h - m, :m] = True
        mask[m:h - m, w - m:] = True
    return mask


@pytest.mark.parametrize("w,h", TILE_SIZES + BLOCK_SIZES + CHUNK_SIZES)
def test_margin_is_the_named_value(w, h, oracle_lib):
    """gain 0.5 doubles a mid-grey image at the border and leaves it alone elsewhere: the touched pixels are those of
    the named margin, and the outermost ring is exactly doubled"""
    m = MARGIN[(w, h)]
    assert m == min(200, w // 2, h // 2)
    img = np.full((h, w), 100, np.uint8)
    one = Case("margin_%dx%d" % (w, h), (64, 32, 16, 0.5, 20), [(np.full((h, w), -1, F32), img, EYE, F32(0.5))])
    planes = run_oracle(oracle_lib, one)[0][2]
    del _results[one.name]
    raw = F32(np.float64(F32(100)) / 255.0)
    touched = planes[0] != raw
    assert np.array_equal(touched, margin_mask(w, h, m)), (w, h, m)
    assert np.all(planes[0][~touched] == raw)
    if touched.any():
        assert planes[0].max() == F32(2) * raw          # ring 0 exists and has the gain's inverse itself
    if (w, h) in CHUNK_SIZES:
        assert touched[199, 500] and not touched[200, 500] and touched[500, 199] and not touched[500, 200]


@pytest.mark.parametrize("w,h", TILE_SIZES + BLOCK_SIZES)
def test_size_cases_fuse(w, h, oracle_lib):
    r = run_oracle(oracle_lib, size_case(w, h))
    assert len(r[0][0]) == 0
    if w * h >= 9:
        assert len(r[0][1]) > 0 and len(r[1][1]) > 0, (w, h)
    if w * h >= 1023:
        assert len(r[1][0]) > 0 and len(r[1][1]) > len(r[0][1]) * 0.5


def test_last_block_case(oracle_lib):
    c = last_block_case()
    r = run_oracle(oracle_lib, c)
    assert len(r[0][0]) == 0 and len(r[0][1]) == 0
    valid = r[1][2][1] > 0
    assert valid.any() and not valid[scan_index(89, 23) < 1024].any() and len(r[1][0]) == 0
    assert len(r[2][0]) > 0 and len(r[2][1]) > 1024


def block_counts(D):
    """per-1024 counts of list 1 in scan order"""
    taken = (D.T.ravel() > 0).astype(np.int64)
    pad = (-len(taken)) % 1024
    return np.concatenate([taken, np.zeros(pad, np.int64)]).reshape(-1, 1024).sum(1)


@pytest.mark.parametrize("w,h", CHUNK_SIZES)
def test_chunk_cases_carry(w, h, oracle_lib):
    """list 1 has points in the first and in the last 1024-block chunk of k_map_scan, the block counts differ, and
    what is carried into the last chunk is neither 0 nor a multiple of 1024; list 0 of frame 2 is longer than one block"""
    r = run_oracle(oracle_lib, chunk_case(w, h))
    for k in (0, 1):
        cnt = block_counts(r[k][2][1])
        assert len(cnt) == (w * h + 1023) // 1024 == w and cnt.sum() == len(r[k][1])
        last = (len(cnt) - 1) // 1024 * 1024
        assert cnt[:1024].sum() > 0 and cnt[last:].sum() > 0 and len(np.unique(cnt)) > 10
        if last:
            assert cnt[:last].sum() % 1024 != 0
    assert len(r[1][0]) > 1024


def test_second_chunk_only_case(oracle_lib):
    r = run_oracle(oracle_lib, second_chunk_only_case())
    cnt = block_counts(r[0][2][1])
    assert len(cnt) == 1025 and cnt[:1024].sum() == 0 and cnt[1024] == len(r[0][1]) > 100
    assert len(r[1][0]) + len(r[1][1]) > 100


# ---- B on the oracle -------------------------------------------------------------------------------------------------
def test_z_min_is_met_exactly(oracle_lib):
    c = z_min_case()
    base = c.prm[3]
    assert F32(64) * base == F32(0.1) * F32(1024)
    z = (F32(64) * base) / F32(1024)
    assert z == F32(0.1) and float(z) > 0.1 and not (z > F32(0.1))
    z_dn = (F32(64) * base) / c.frames[0][0][16, 16]
    assert z_dn < z and not float(z_dn) > 0.1
    r = run_oracle(oracle_lib, c)
    keep, drop = at(r[0][2], c.cells["keep"]), at(r[0][2], c.cells["drop"])
    assert keep[1] == 1024 and bits(keep[4]) == bits(F32(0.1)) and keep[2] == 0 and keep[3] == 0
    assert drop[1] == -1 and len(r[0][1]) == 2
    # frame 2: z2 == float32(0.1) passes (else the point would stay in list 0) and merges with itself
    assert len(r[1][0]) == 0 and len(r[1][1]) == 2 and bits(at(r[1][2], c.cells["keep"])[4]) == bits(F32(0.1))
    # frame 3: it fills the empty cell
    cell = at(r[2][2], c.cells["keep"])
    assert len(r[2][0]) == 0 and cell[1] == 1 and bits(cell[4]) == bits(F32(0.1))


def test_z_max_is_met_exactly(oracle_lib):
    c = z_max_case()
    fb = F32(64) * c.prm[3]
    assert fb == np.nextafter(F32(32), F32(0))
    below = np.nextafter(F32(16), F32(0))
    assert fb / F32(2) == below and fb / c.frames[0][0][16, 16] == F32(16) == c.prm[4]
    r = run_oracle(oracle_lib, c)
    keep, drop = at(r[0][2], c.cells["keep"]), at(r[0][2], c.cells["drop"])
    assert keep[1] == 2 and keep[4] == below and drop[1] == -1 and len(r[0][1]) == 1
    cell = at(r[1][2], c.cells["keep"])                     # z2 = the float below max_dist: moved on
    assert len(r[1][0]) == 0 and cell[1] == 1 and cell[4] == below
    assert below + F32(2.0 ** -20) == F32(16)              # z2 == max_dist: stays
    assert len(r[2][0]) == 1 and r[2][0][0][2] == below and len(r[2][1]) == 0


def test_closeness_threshold_is_met_exactly(oracle_lib):
    c = dist_case()
    assert c.cells["found"]["at"] is not None and c.cells["found"]["below"] is not None
    assert float(DIST_AT) > 0.2 > float(DIST_BELOW) and np.nextafter(DIST_BELOW, F32(1)) == DIST_AT
    r = run_oracle(oracle_lib, c)
    alone = run_oracle(oracle_lib, Case("dist_frame2_alone", c.prm, c.frames[1:]))[0][2]
    prev, fused = r[0][2], r[1][2]

    def dist(name):
        p, q = at(prev, c.cells[name]), at(alone, c.cells[name])
        return closeness(p[2], p[3], p[4], q[2], q[3], q[4])

    assert dist("at") == DIST_AT and dist("below") == DIST_BELOW and dist("zero") == 0
    # exactly float32(0.2): not merged
    assert xyz_rows(r[1][0]) == {xyz_key(at(prev, c.cells["at"]))} and len(r[1][0]) == 1
    assert np.array_equal(bits(at(fused, c.cells["at"])), bits(at(alone, c.cells["at"])))
    # the float below: merged
    p, q, m = (at(x, c.cells["below"]) for x in (prev, alone, fused))
    assert np.array_equal(bits(m[[0, 2, 3, 4]]), bits(((p + q).astype(np.float64) / 2.0).astype(F32)[[0, 2, 3, 4]]))
    assert m[1] == q[1] and not np.array_equal(bits(m[2:]), bits(q[2:]))
    # the same point: itself
    assert np.array_equal(bits(at(fused, c.cells["zero"])[1:]), bits(at(prev, c.cells["zero"])[1:]))
    # no current point: filled
    p, m = at(prev, c.cells["fill"]), at(fused, c.cells["fill"])
    assert at(alone, c.cells["fill"])[1] == -1 and m[1] == 1 and np.array_equal(bits(m[[0, 2, 3, 4]]), bits(p[[0, 2, 3, 4]]))
    assert len(r[1][1]) == 4


@pytest.mark.parametrize("side", ["lo", "hi"])
def test_border_truncation(side, oracle_lib):
    c = border_case(side)
    t, pts = BORDER[side]
    r = run_oracle(oracle_lib, c)
    prev, fused = r[0][2], r[1][2]
    assert len(r[0][1]) == len(pts)
    stays = set()
    for (u, v, d), to in pts:
        p = at(prev, (u, v))
        z = F32(32) / F32(d)
        assert p[1] == d and p[4] == z
        # the re-projection in float32, as both sides evaluate it
        w2 = p[4]
        u2 = (F32(64) * p[2] + F32(32) * p[4] + F32(-64 * t)) / w2
        v2 = (F32(64) * p[3] + F32(16) * p[4] + F32(-64 * t)) / w2
        assert u2 == u - 2 * t * d and v2 == v - 2 * t * d
        if to is None:
            assert u2 in (-1, W) or v2 in (-1, HH)
            stays.add(xyz_key(p))
        else:
            assert to == (int(u2), int(v2))               # int() truncates toward zero
            m = at(fused, to)
            assert m[1] == 1 and np.array_equal(bits(m[[0, 2, 3, 4]]), bits(p[[0, 2, 3, 4]])), (u, v, d)
    assert xyz_rows(r[1][0]) == stays and len(r[1][0]) == len(stays)
    assert len(r[1][1]) == len(pts) - len(stays)
    if side == "lo":
        assert any(-1 < u - 2 * t * d < 0 for (u, v, d), to in pts if to) and any(u - 2 * t * d == 0 for (u, v, d), to in pts)
    else:
        assert any(W - 1 < u - 2 * t * d < W for (u, v, d), to in pts if to) and any(u - 2 * t * d == W for (u, v, d), to in pts)


def test_points_on_and_behind_the_camera_plane_stay(oracle_lib):
    c = behind_case()
    r = run_oracle(oracle_lib, c)
    prev = r[0][2]
    on, behind, front = (at(prev, c.cells[k]) for k in ("on", "behind", "front"))
    assert on[4] - F32(8) == 0 and behind[4] - F32(8) == -4 and front[4] - F32(8) == 8
    assert xyz_rows(r[1][0]) == {xyz_key(on), xyz_key(behind)} and len(r[1][0]) == 2
    assert len(r[1][1]) == 1 and np.array_equal(bits(r[1][1][0][:3]), bits(front[2:]))


def test_replay_order_decides_the_tie_pixel(oracle_lib):
    c = ties_case()
    r = run_oracle(oracle_lib, c)
    prev = r[0][2]
    idx = [v * W + u for u, v, _ in TIE_PTS]
    assert sorted(i // 256 for i in idx) == [4, 5, 6] and idx == sorted(idx, reverse=True)
    assert [u * HH + v for u, v, _ in TIE_PTS] == sorted(u * HH + v for u, v, _ in TIE_PTS)
    pts = np.array([at(prev, (u, v))[[2, 3, 4, 0]] for u, v, _ in TIE_PTS], F32)
    assert np.array_equal(bits(pts), bits(r[0][1]))              # list 1 of frame 1, in scan order
    fwd, fwd_stay = replay(pts)
    rev, rev_stay = replay(pts[::-1])
    assert fwd_stay == [2] and rev_stay == [1, 2] and not np.array_equal(bits(fwd), bits(rev))
    cell = at(r[1][2], c.cells["target"])
    assert cell[1] == 1 and np.array_equal(bits(cell[[2, 3, 4, 0]]), bits(fwd))
    assert len(r[1][1]) == 1 and len(r[1][0]) == 1 and np.array_equal(bits(r[1][0][0]), bits(pts[2]))


def test_odd_disparities(oracle_lib):
    c = nonfinite_case()
    r = run_oracle(oracle_lib, c)
    want = {"nan": NAN_PAYLOAD, "pinf": F32(-1), "ninf": F32(-np.inf), "nzero": F32(-0.0), "denormal": F32(-1),
            "fltmax": F32(-1)}
    D = r[0][2][1]
    for k, (name, val) in enumerate(ODD):
        assert bits(D[4, 4 + 8 * k]) == bits(want[name]), name
        assert D[20, 4 + 8 * k] == 4
    assert bits(F32(1e-40)) < 0x00800000 and F32(1e-40) > 0
    assert len(r[0][1]) == 6 and len(r[0][0]) == 0
    D = r[1][2][1]
    assert np.all(D[20, 4:48:8] == 1) and np.all(D[4, 4:48:8] == 4)     # every odd cell took a previous point
    assert np.array_equal(bits(r[1][2][4][20, 4:48:8]), bits(r[0][2][4][20, 4:48:8]))
    assert len(r[1][0]) == 0 and len(r[1][1]) == 12
    assert len(r[2][0]) == 0 and len(r[2][1]) == 12


def test_gain_clamps_are_taken(oracle_lib):
    c = gain_case()
    mask = margin_mask(W, HH, 16)
    seen = {}
    for k, (d, img, Ht, g) in enumerate(c.frames):
        I = run_oracle(oracle_lib, Case("gain_alone_%d" % k, c.prm, [c.frames[k]]))[0][2][0]
        raw = (img.astype(F32).astype(np.float64) / 255.0).astype(F32)
        assert np.array_equal(bits(I[~mask]), bits(raw[~mask]))
        seen[float(g)] = (I, raw, img)
    I, raw, img = seen[-0.5]
    low = mask & (img > 0) & (bits(I) == 0)                     # the lower clamp: a negative product became +0
    mzero = mask & (img == 0) & (bits(I) == 0x80000000)         # std::max(-0.0f, 0.0f) is -0.0f
    assert low.sum() > 50 and mzero.sum() > 20 and not (bits(I)[mask & (img == 0)] == 0).all()
    assert (mask & (I > 0) & (I < 1)).any()                     # the inner third of the ramp is positive again
    I, raw, img = seen[0.0]                                     # -0.0 is "no gain"
    assert np.array_equal(bits(I), bits(raw))
    I, raw, img = seen[float(F32(1e-30))]
    assert (mask & (raw > 0) & (raw < 1) & (I == 1)).sum() > 50 and np.all(I[mask & (img == 0)] == 0)
    I, raw, img = seen[float(F32(1e30))]
    assert np.all(I[0, 16:48] < 1e-25) and (I[0, 16:48] > 0).any()       # ring 0 has the gain's inverse itself
    I, raw, img = seen[float(F32(0.93))]
    assert np.all(img == 255) and np.all(I == 1) and 1.0 / float(F32(0.93)) > 1
    # and in the sequence the averaged I keeps a -0.0 only in frame 1
    r = run_oracle(oracle_lib, c)
    assert (bits(r[0][2][0]) == 0x80000000).any() and len(r[4][1]) == W * HH and len(r[4][0]) == 0

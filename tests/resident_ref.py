"""numpy restatement of Matcher::getGain (matcher.cpp:347-389 with `mean`, :1825-1837) as svh_matcher_get_gain states
it, and the inputs the device-frame tests share (tests/test_resident.py checks them on the CPU,
tests/test_resident_gpu.py runs the library against them).

The engine clamps both 7x7 windows INCLUSIVELY to [0, W] x [0, H]: column W is the first padding byte of the packed
row (zero) and row H is one row past the image (zero).  A window holds at most 49 bytes, so its sum is exact; the mean
is one float32 division by the clamped window's pixel count, a match counts where mean_prev > 10, and the ratios
mean_curr / mean_prev are added ONE AFTER THE OTHER in float32, in inlier order."""
import numpy as np

P_MATCH = np.dtype([("u1p", "f4"), ("v1p", "f4"), ("i1p", "i4"), ("u2p", "f4"), ("v2p", "f4"), ("i2p", "i4"),
                    ("u1c", "f4"), ("v1c", "f4"), ("i1c", "i4"), ("u2c", "f4"), ("v2c", "f4"), ("i2c", "i4")])


def bpl_of(w):
    return w + 16 - w % 16      # matcher.cpp:173


def padded(I):
    """[h, w] -> [h + 1, bpl]: the packed image with its zero padding and the zero row"""
    h, w = I.shape
    P = np.zeros((h + 1, bpl_of(w)), np.uint8)
    P[:h, :w] = I
    return P


def window_mean(P, W, H, u, v):
    cl = lambda x, hi: min(max(x, 0), hi)
    iu, iv = int(np.float32(u)), int(np.float32(v))          # C's float -> int: towards zero
    u0, u1, v0, v1 = cl(iu - 3, W), cl(iu + 3, W), cl(iv - 3, H), cl(iv + 3, H)
    s = int(P[v0:v1 + 1, u0:u1 + 1].astype(np.int64).sum())
    return np.float32(s) / np.float32((u1 - u0 + 1) * (v1 - v0 + 1))


def ratios(Ip, Ic, matches, inliers):
    """(ratio, counted) of every inlier that names a match, in inlier order"""
    assert Ip.shape == Ic.shape
    H, W = Ip.shape
    Pp, Pc = padded(Ip), padded(Ic)
    out = []
    for q in inliers:
        if q >= len(matches):
            continue
        m = matches[q]
        mp = window_mean(Pp, W, H, m["u1p"], m["v1p"])
        mc = window_mean(Pc, W, H, m["u1c"], m["v1c"])
        out.append((np.float32(mc) / np.float32(mp) if mp > 10 else np.float32(0), bool(mp > 10)))
    return out


def sequential_sum(values):
    s = np.float32(0)
    for x in values:
        s = np.float32(s + np.float32(x))
    return s


def gain(Ip, Ic, matches, inliers):
    if len(inliers) == 0:
        return np.float32(1)
    r = [x for x, used in ratios(Ip, Ic, matches, inliers) if used]
    return np.float32(sequential_sum(r) / np.float32(len(r))) if r else np.float32(1)


def make_matches(coords):
    """rows of (u1p, v1p, u1c, v1c)"""
    m = np.zeros(len(coords), P_MATCH)
    for k, (a, b, c, d) in enumerate(coords):
        m[k]["u1p"], m[k]["v1p"], m[k]["u1c"], m[k]["v1c"] = a, b, c, d
    return m


# ---- the painted pair of the gain tests: constant regions of 10 (mean exactly 10: excluded) and 11, a ramp elsewhere
GAIN_W, GAIN_H = 608, 230


def painted_pair():
    y, x = np.mgrid[0:GAIN_H, 0:GAIN_W].astype(np.int64)
    Ip = ((3 * x + 5 * y) % 200 + 20).astype(np.uint8)
    Ic = ((7 * x + 3 * y) % 230 + 15).astype(np.uint8)
    Ip[:60, :100] = 10
    Ip[:60, 100:200] = 11
    Ic[:60, :200] = 23
    return Ip, Ic


def crafted_matches():
    """the border cases first (window clamped at 0, truncation of 2.9, the last pixel, past the image, -0.5 -> 0), then
    seeded matches all over the image, a few pixels outside it included"""
    W, H = GAIN_W, GAIN_H
    edge = [(0, 0, 0, 0), (2.9, 2.9, 2.9, 2.9), (W - 1, H - 1, W - 1, H - 1), (W + 5, H + 5, W + 5, H + 5),
            (-0.5, -0.5, -0.5, -0.5), (150, 30, W - 1, H - 1), (W - 1, H - 1, 0, 0), (300.5, 100.25, W + 5, 3),
            (50, 30, 300, 100), (99, 30, 10, 10), (103, 57, 5, H + 5)]
    rng = np.random.default_rng(20241)
    rnd = np.stack([rng.uniform(-8, W + 8, 1100), rng.uniform(-8, H + 8, 1100),
                    rng.uniform(-8, W + 8, 1100), rng.uniform(-8, H + 8, 1100)], 1).astype(np.float32)
    return make_matches(edge + [tuple(r) for r in rnd])


def inlier_list(n, nm, seed=7):
    """n inlier indices into nm matches: the border cases first, then seeded ones; every 17th names no match"""
    rng = np.random.default_rng(seed + n)
    idx = np.concatenate([np.arange(min(n, 11)), rng.integers(0, nm, max(n - 11, 0))]).astype(np.int32)[:n]
    idx[16::17] = nm + np.arange(len(idx[16::17]))
    return idx


ORDERED_SEED = 3


def ordered_sum_case():
    """1025 inliers on the painted pair whose ratios a pairwise (tree) sum adds up to another float32 than the
    sequential sum does: a device sum in another order would be caught"""
    Ip, Ic = painted_pair()
    m = crafted_matches()
    every = ratios(Ip, Ic, m, np.arange(len(m)))
    counted = np.array([k for k, (_, used) in enumerate(every) if used], np.int32)
    idx = np.random.default_rng(ORDERED_SEED).choice(counted, 1025).astype(np.int32)
    r = np.array([every[k][0] for k in idx], np.float32)
    return Ip, Ic, m, idx, r

"""Edge cases of VisualOdometryStereo::estimateMotion (k_vo_ransac, k_vo_refine), shared by test_vo_edges.py
(CPU: is each case a fair parity case?) and test_vo_edges_gpu.py (device against oracle).

The structural switches of the kernels the sizes sit on:
  N <= 656 / N >= 657   refinement rows in LDS (column-major, reads one turn ahead) / in global scratch (row-major,
                        clamped tail): lds_rows = roundup8(4 N) + 8 rows of 56 bytes, at most 144 KB
  4 nin mod 8           wave_gn_step sums the rows in turns of 8: an odd inlier count leaves half a turn
  N = 256/257, 512/513  the ordered inlier compaction gives ceil(N / 256) matches to each of 256 threads
  N = 63/64/65          the vote loop walks 64 matches per trip

Fairness.  The device's sine and cosine may differ from glibc's in the last bit; TOL = 1e-9 of the parity tests is
there for that alone.  The oracle can imitate it (orc_vo_set_trig_mode: every sine / cosine of the linearisation one
ulp up, down, or a seeded mix).  A case is ADMITTED for final-answer parity if status and inlier list are identical in
all four modes and the motion moves by less than ADMIT = 1e-10, a tenth of TOL.  A hypothesis is STABLE if its vote is
identical in the four modes and its vector stays finite and moves by less than ADMIT; the others are masked out of the
per-hypothesis comparison, and the mask may hide at most CAP_PLAIN (size and parameter cases) or CAP_DEGENERATE of
them.  Everything here comes from the oracle alone."""
import ctypes as C
import functools
import os

import numpy as np

import helpers as H

TOL = 1e-9
ADMIT = 1e-10
CAP_PLAIN = 0.05
CAP_DEGENERATE = 0.20
TRIG_SEED = 20261020        # the generator of mode 3
LDS_MAX_N = 656             # vlaunch_estimate: (roundup8(4 N) + 8) * 56 bytes <= 144 KB
MODES = (0, 1, 2, 3)

# Named seeds of H.synth_vo_matches.  Where the first choice (1000 + N, 4257 / 4657, 64) left a case outside the
# admission rule or the mask caps, or -- for the parameter sets -- gave the threshold-1e6 case a FAILED hypothesis, so
# that its 200 votes were not all equal, the seed was replaced by the next one that the ORACLE's four modes accept;
# no seed was chosen by looking at the device.
SEED_SIZE = 1000            # size case N uses SEED_SIZE + N ...
SEED_SIZE_OTHER = {7: 1012}  # ... but N = 7: 1007 hides 8.5 % of the hypotheses
SEED_ALL_INLIER = 3000      # + N
SEED_PARAM = 4001           # both parameter sizes: no FAILED hypothesis at the default parameters
SEED_BASE64 = 65            # the N = 64 base set of the degenerate cases (64: the zero-disparity case hides 20.5 %)
SEED_OUTLIERS97 = 5
SEED_NOISE3 = 6
SEED_EXACT = 80
SEED_ZERO = 81
SEED_LARGE = 82
SEED_SEQ = 7080             # + position in the sequence (7000: the N = 6 step hides 12 % of its hypotheses)

SIZES = (6, 7, 63, 64, 65, 255, 256, 257, 511, 512, 513, 655, 656, 657, 658, 1025)
PARAM_SIZES = (257, 657)    # one LDS size, one global size
PARAM_SETS = (
    ("iters0", {"ransac_iters": 0}), ("iters1", {"ransac_iters": 1}), ("iters3", {"ransac_iters": 3}),
    ("reweight0", {"reweighting": 0}), ("reweight1", {"reweighting": 1}),
    ("thr1e-6", {"inlier_threshold": 1e-6}),      # every vote 0: no winner
    ("thr1e6", {"inlier_threshold": 1e6}),        # every vote N: hypothesis 0 must win
    ("cu0", {"cu": 0.0}),                         # weight 1 / (|u| / 0 + 0.05) = 0: every pivot search sees zeros
)
SEQUENCE = (657, 64, 656, 3000, 6, 5, 257)
LARGE_MOTION = (0.3, -0.4, 0.5, 1.0, -0.5, -3.0)


class Case:
    def __init__(self, name, kind, build, params=None, hypotheses=True, parity=True):
        self.name, self.kind, self.build, self.params = name, kind, build, dict(params or {})
        self.hypotheses = hypotheses      # False: final answer only (nearly every hypothesis moves with the last bit)
        self.parity = parity              # False: not even the final answer is a fair parity case
        self.cap = CAP_DEGENERATE if kind == "degenerate" else CAP_PLAIN

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def matches(self):
        m = self.build()
        m.setflags(write=False)
        return m

    def prm(self):
        return H.vo_defaults(**self.params)


def _base64():
    return H.synth_vo_matches(64, seed=SEED_BASE64)


def _copy_of_first_half():
    m = _base64()
    return np.concatenate([m, m[:32]])


def _zero_disparity_every_second():
    m = _base64()
    m["u2p"][::2] = m["u1p"][::2]                 # d = 0 -> the 0.0001 clamp
    return m


def _negative_disparity():
    m = _base64()
    m["u2p"] = m["u1p"] + 3
    return m


def _one_row():
    m = _base64()
    for k in ("v1p", "v2p", "v1c", "v2c"):
        m[k] = np.float32(H.vo_defaults().cv)
    return m


def _two_matches():
    # (matches 10 and 50 of the base set; with 3 and 11, the first pair tried, the oracle's own winner is hypothesis 0
    # in three trig modes and 6 in the fourth, so the winner's index could not be held against the device)
    m = _base64()
    return np.concatenate([np.repeat(m[10:11], 20), np.repeat(m[50:51], 20)])


def _one_match():
    return np.repeat(_base64()[3:4], 40)


def _cases():
    out = []
    for n in SIZES:
        out.append(Case("n%d" % n, "size", functools.partial(H.synth_vo_matches, n, seed=SEED_SIZE_OTHER.get(n, SEED_SIZE + n))))
    for n in (656, 657):   # 4 nin reaches the last LDS row / the odd global tail
        out.append(Case("all_inliers_n%d" % n, "size",
                        functools.partial(H.synth_vo_matches, n, seed=SEED_ALL_INLIER + n, outliers=0, noise=0.05)))
    for n in PARAM_SIZES:
        for tag, kw in PARAM_SETS:
            out.append(Case("%s_n%d" % (tag, n), "param",
                            functools.partial(H.synth_vo_matches, n, seed=SEED_PARAM), kw))
    D = "degenerate"
    out += [
        Case("copy_of_first_half", D, _copy_of_first_half),
        Case("zero_disparity_every_second", D, _zero_disparity_every_second),
        Case("negative_disparity", D, _negative_disparity, hypotheses=False),
        Case("one_row", D, _one_row),
        Case("two_matches_x20", D, _two_matches, hypotheses=False),
        Case("outliers97_n300", D, functools.partial(H.synth_vo_matches, 300, seed=SEED_OUTLIERS97, outliers=0.97)),
        Case("noise3_n200", D, functools.partial(H.synth_vo_matches, 200, seed=SEED_NOISE3, noise=3.0)),
        Case("exact_n80", D, functools.partial(H.synth_vo_matches, 80, seed=SEED_EXACT, outliers=0, noise=0)),
        Case("zero_motion", D, functools.partial(H.synth_vo_matches, 64, seed=SEED_ZERO, motion=(0,) * 6, outliers=0,
                                                 noise=0)),
        Case("large_motion", D, functools.partial(H.synth_vo_matches, 64, seed=SEED_LARGE, motion=LARGE_MOTION)),
        Case("one_match_x40", D, _one_match, hypotheses=False, parity=False),
    ]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
PARITY_CASES = [c for c in CASES if c.parity]
HYP_CASES = [c for c in CASES if c.parity and c.hypotheses]


def sequence_matches():
    return [H.synth_vo_matches(n, seed=SEED_SEQ + i) for i, n in enumerate(SEQUENCE)]


def new_oracle(prm):
    """an oracle object for estimateMotion alone: no Triangle needed, so none is demanded"""
    tri = None if H.have_ref_viso() else C.c_void_p(0)
    return H.OracleVo(prm, tri_fn=tri)


class Result:
    """what one estimateMotion call leaves behind"""

    def __init__(self, vo, ret):
        self.ok, self.tr = ret[0], ret[1].copy()
        self.inliers = vo.inliers().copy()
        self.votes, self.hyp = vo.hypotheses()

    def winner(self):
        """first hypothesis with the most votes, -1 if none has any (viso_stereo.cpp:107-117)"""
        if len(self.votes) == 0 or self.votes.max() <= 0:
            return -1
        return int(np.argmax(self.votes))


def run_steps(vo, steps):
    return [Result(vo, vo.estimate_motion(m)) for m in steps]


@functools.lru_cache(maxsize=None)
def oracle_modes(name):
    """the case on a fresh oracle object (srand(0)) in each trig mode; name 'sequence': the list of steps"""
    out = []
    for mode in MODES:
        if name == "sequence":
            vo = new_oracle(H.vo_defaults())
            vo.set_trig_mode(mode, TRIG_SEED)
            out.append(run_steps(vo, sequence_matches()))
        else:
            c = BY_NAME[name]
            vo = new_oracle(c.prm())
            vo.set_trig_mode(mode, TRIG_SEED)
            out.append(run_steps(vo, [c.matches()])[0])
    return out


def final_shift(rs):
    """(status and inlier list identical in all modes, largest move of the motion vector)"""
    same = all(r.ok == rs[0].ok and np.array_equal(r.inliers, rs[0].inliers) for r in rs)
    move = max([np.abs(r.tr - rs[0].tr).max() for r in rs]) if rs[0].ok and same else 0.0
    return same, float(move)


def admitted(rs):
    same, move = final_shift(rs)
    return same and move < ADMIT


def stable_mask(rs):
    """bool [n_hyp]: vote identical in all modes, vector finite and within ADMIT of mode 0's in all modes"""
    v0, h0 = rs[0].votes, rs[0].hyp
    ok = np.ones(len(v0), bool)
    for r in rs:
        assert len(r.votes) == len(v0)
        ok &= r.votes == v0
        ok &= np.isfinite(r.hyp).all(axis=1)
        with np.errstate(invalid="ignore"):
            ok &= np.abs(r.hyp - h0).max(axis=1) < ADMIT
    return ok


def uses_lds(n):
    return n <= LDS_MAX_N


# ---- the lockstep trio: three objects, three frame variants, N on both sides of the LDS limit -------------------
TRIO_PARAMS = {"bucket_max_features": 3, "bucket_width": 30.0, "bucket_height": 30.0}
TRIO_CUTS = (None, 900, 800)          # columns >= cut are set to 128
TRIO_SRAND = 7                        # srand() after the objects exist (their constructors call srand(0))


def trio_frames():
    """[object][I1p, I2p, I1c, I2c]"""
    quad = [H.read_pgm(os.path.join(H.GOLDEN, "viso_%s.pgm" % k)) for k in ("I1p", "I2p", "I1c", "I2c")]
    out = []
    for cut in TRIO_CUTS:
        q = [im.copy() for im in quad]
        if cut is not None:
            for im in q:
                im[:, cut:] = 128
        out.append(q)
    return out

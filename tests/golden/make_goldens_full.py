"""Generate the full-size fixtures.  RUNS ONLY IN THE BUILD CONTAINER.

Inputs : the reference's seven stereo pairs at full size (/root/reference/libelas/img/*.pgm, the
         pairs its `main.cpp demo` runs) and its mono sequence I1_000000..6
         (/root/reference/libviso2/img/*.png, converted to gray), stored under full/ as one
         compressed .npz per image.  Each row is stored as its horizontal differences mod 256
         (helpers.full_image undoes that): it keeps every file well under 1 MiB.
Outputs: results of the REFERENCE itself (oracle/_ref/libref_{elas,viso}.so), per case:
   ELAS   support list and both triangle lists exact (int16), a sha256 per tapped stage
          (float stages with -0.0 taken as +0.0, helpers.stage_sha256) and the valid-pixel
          counts of D1 and D2;
   mono   per step (pushBack(I1_k) + matchFeatures(0), k = 1..6): the match list (in full for
          the default parameters, sha256 + count otherwise) and the hashes of the 1p1 / 1c1
          feature tables.

    python tests/golden/make_goldens_full.py

The GPU box never runs this; tests only read the committed files.
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "full")
sys.path.insert(0, os.path.dirname(HERE))
import helpers as H  # noqa: E402

ELAS_IMG = "/root/reference/libelas/img"
VISO_IMG = "/root/reference/libviso2/img"
PAIRS = ["urban1", "urban2", "urban3", "urban4", "cones", "aloe", "raindeer"]

# libelas/src/main.cpp:61-63: Elas::parameters() (ROBOTICS) with both maps post-processed
DEMO = H.robotics(postprocess_only_left=0)
ELAS_CASES = {}
for _p in PAIRS:
    ELAS_CASES[_p + "_demo"] = (_p, DEMO)
for _p in ("urban1", "urban2", "urban3", "urban4"):
    ELAS_CASES[_p + "_robotics"] = (_p, H.robotics())
for _p in ("cones", "aloe", "raindeer"):
    ELAS_CASES[_p + "_middlebury"] = (_p, H.middlebury())
ELAS_CASES["urban1_robotics_sub"] = ("urban1", H.robotics(subsampling=1))

# mono Matcher parameter sets (matchFeatures(0) after every pushBack(I1))
MONO_SETS = {
    "default": H.matcher_defaults(),
    "full_res": H.matcher_defaults(half_resolution=0),
    "refine2": H.matcher_defaults(refinement=2),
}
T1P1, T1C1 = H.M_TABLES.index("1p1"), H.M_TABLES.index("1c1")


def save_image(name, img):
    img = np.ascontiguousarray(img, np.uint8)
    rows = np.diff(img, axis=1, prepend=np.zeros((img.shape[0], 1), np.uint8)).astype(np.uint8)
    assert np.array_equal(H._unfilter_rows(rows), img)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), rows=rows)


def elas_record(prm, pair, run):
    out = {"params": np.frombuffer(bytes(prm), np.uint8), "pair": np.array(pair)}
    for s in (H.SUPPORT, H.TRI1, H.TRI2):
        a = run[s]
        assert np.abs(a).max() < 2 ** 15
        out[H.STAGE_NAMES[s]] = a.astype(np.int16)
    hashed = [s for s in sorted(H.STAGE_NAMES) if s in run]
    out["hashed"] = np.array([H.STAGE_NAMES[s] for s in hashed])
    for s in hashed:
        out[H.STAGE_NAMES[s] + "_sha256"] = np.array(H.stage_sha256(run[s]))
    out["d1_valid"] = np.array(int((run[H.D1_FINAL] >= 0).sum()))
    out["d2_valid"] = np.array(int((run[H.D2_FINAL] >= 0).sum()))
    return out


def mono_record(prm, frames, full):
    m = H.RefMatcher(prm)
    out = {"params": np.frombuffer(bytes(prm), np.uint8)}
    n, sha, t1p1, t1c1 = [], [], [], []
    for k, img in enumerate(frames):
        m.push_back(img)
        if k == 0:
            continue
        m.match(0, None, staged=True)
        got = m.matches()
        n.append(len(got))
        sha.append(H.stage_sha256(got))
        t1p1.append(H.stage_sha256(m.features(T1P1)))
        t1c1.append(H.stage_sha256(m.features(T1C1)))
        if full:
            out["matches_%d" % k] = got
    out.update(n=np.array(n), sha256=np.array(sha), t1p1_sha256=np.array(t1p1), t1c1_sha256=np.array(t1c1))
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    pairs = {}
    for p in PAIRS:
        pairs[p] = tuple(H.read_pgm(os.path.join(ELAS_IMG, "%s_%s.pgm" % (p, side))) for side in ("left", "right"))
        for side, img in zip(("left", "right"), pairs[p]):
            save_image("%s_%s" % (p, side), img)
    frames = []
    for k in range(7):
        img = np.array(Image.open(os.path.join(VISO_IMG, "I1_%06d.png" % k)).convert("L"))
        save_image("I1_%06d" % k, img)
        frames.append(img)
    for case, (pair, prm) in ELAS_CASES.items():
        l, r = pairs[pair]
        run = H.ref_elas_run(prm, l, r)
        assert run.status == 0, case
        np.savez_compressed(os.path.join(OUT, "elas_" + case + ".npz"), **elas_record(prm, pair, run))
        print(case, "support", len(run[H.SUPPORT]) // 3, "tri", len(run[H.TRI1]) // 3, len(run[H.TRI2]) // 3)
    for name, prm in MONO_SETS.items():
        rec = mono_record(prm, frames, full=(name == "default"))
        np.savez_compressed(os.path.join(OUT, "mono_" + name + ".npz"), **rec)
        print("mono", name, list(rec["n"]))


if __name__ == "__main__":
    main()

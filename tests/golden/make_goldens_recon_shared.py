"""Generate tests/golden/recon_shared.npz: one more Reconstruction scene, `shared`, in the layout of recon.npz
(make_goldens_recon.py).  RUNS ONLY IN THE BUILD CONTAINER.

recon.npz has two matches with one i1c (scene edge, update 6), so two tracks end on one feature index, but no match
of the following update has that index as its i1p: which of the two tracks owns the slot of track_idx
(reconstruction.cpp:86-87, "a later track overwrites the slot") is never asked.  This scene asks it.  It is a short
drive of recon_ref.synth_scene in which, in several updates, a match b is given the i1c of a match a whose feature is
matched again in the next update.  The tracks of a and b then share a last_idx; the next update's match extends the
HIGHER-indexed of the two and the other is lost.  The pairs are chosen so that the two tracks have different lengths
(tracks are stored in the order of their creation, so the lower-indexed, lost one is the longer; under
min_track_length = 3 a wrong owner would lose a track of two frames instead and show as outcome 0), and so that the
track of the match that is matched again is once the lower and once the higher of the two.  In one update the shared index is also the i1p of two matches (the first
extends, the second creates).  The script checks all of that on its own serial replay before it records the
reference's results.

The reference's own Reconstruction is built through recon_ref.build_harness into a temporary directory and never
committed.

    python tests/golden/make_goldens_recon_shared.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import recon_ref as R  # noqa: E402

LIMIT = 1024 * 1024
OUT = os.path.join(HERE, "recon_shared.npz")
SETTINGS = [(0, 2, 30, 2), (0, 3, 30, 2), (1, 3, 30, 2)]
SHARE_AT = (2, 3, 5, 6, 8)       # updates in which two matches get one i1c
DOUBLE_AT = 6                    # ... and the next update has the shared index as i1p twice


def replay(scene):
    """the track table (last_idx, length per track) before every update, by the reference's sequential rule"""
    last, length, before = [], [], []
    for _, m in scene:
        before.append((list(last), list(length)))
        slot = {}
        for t, li in enumerate(last):
            slot[li] = t
        extended = set()
        new_last, new_len = list(last), list(length)
        for q in m:
            t = slot.get(int(q["i1p"]), -1)
            if t >= 0 and t not in extended:
                extended.add(t)
                new_last[t], new_len[t] = int(q["i1c"]), length[t] + 1
            else:
                new_last.append(int(q["i1c"]))
                new_len.append(2)
        keep = [t for t in range(len(new_last)) if t >= len(last) or t in extended]
        last, length = [new_last[t] for t in keep], [new_len[t] for t in keep]
    return before


def shared_cases(scene):
    """(update, lower track, higher track, their lengths) wherever a match's i1p reaches a last_idx two tracks share"""
    out = []
    for k, ((last, length), (_, m)) in enumerate(zip(replay(scene), scene)):
        for idx in sorted(set(int(p) for p in m["i1p"])):
            owners = [t for t, li in enumerate(last) if li == idx]
            if len(owners) >= 2:
                out.append((k, owners[0], owners[-1], length[owners[0]], length[owners[-1]]))
    return out


def shared_scene():
    scene = [(T, m.copy()) for T, m in R.synth_scene(n_points=400, n_updates=10, seed=21, drop=0.0)]
    for k in SHARE_AT:
        m, nxt = scene[k][1], scene[k + 1][1]
        last, length = replay(scene)[k]
        track_of = {li: t for t, li in enumerate(last)}
        again = set(int(p) for p in nxt["i1p"])
        # a: continues an old track and is matched again; b: another match whose track differs in length from a's
        # b's track: created now (always above a's), or an old one below a's, or an old one above a's
        want = {0: "new", 1: "below", 2: "above"}[SHARE_AT.index(k) % 3]
        done = False
        for a in range(len(m)):
            ta = track_of.get(int(m["i1p"][a]), -1)
            if ta < 0 or int(m["i1c"][a]) not in again:
                continue
            for b in range(len(m)):
                tb = track_of.get(int(m["i1p"][b]), -1)
                if b == a or (tb < 0) != (want == "new") or (tb >= 0 and length[tb] == length[ta]):
                    continue
                if (want == "below" and tb > ta) or (want == "above" and tb < ta):
                    continue
                m["i1c"][b] = m["i1c"][a]
                done = True
                break
            if done:
                break
        assert done, k
        if k == DOUBLE_AT:
            hit = int(np.flatnonzero(nxt["i1p"] == m["i1c"][a])[0])
            extra = nxt[hit:hit + 1].copy()
            extra["i1c"] = int(nxt["i1c"].max()) + 1
            extra["u1c"] += 2.0
            scene[k + 1] = (scene[k + 1][0], np.concatenate([nxt[:hit + 3], extra, nxt[hit + 3:]]))
    return scene


def main():
    scene = shared_scene()
    cases = shared_cases(scene)
    print("shared last_idx reached by a match:", cases)
    assert len(cases) >= len(SHARE_AT), cases
    assert all(la != lb for _, _, _, la, lb in cases), cases
    out = {"calib": np.array(R.CALIB, np.float64), "scene_names": np.array(["shared"])}
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        R.pack_scene(out, "shared", scene)
        out["shared_settings"] = np.array(SETTINGS, np.float64)
        path = os.path.join(tmp, "shared.bin")
        R.write_scene(path, scene)
        for j, s in enumerate(SETTINGS):
            res = R.run_scene(exe, path, len(scene), s)
            R.pack_result(out, "shared_%d" % j, res)
            codes = np.concatenate([r[2] for r in res])
            print(s, "updates", len(scene), "lost", len(codes), dict(zip(R.CODE_NAMES, np.bincount(codes, minlength=7).tolist())))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("recon_shared.npz", size // 1024, "KiB")
    if size > LIMIT:
        raise SystemExit("recon_shared.npz is larger than %d bytes" % LIMIT)


if __name__ == "__main__":
    main()

"""The reference's Reconstruction, built from the reference sources into a temporary directory, and the scenes of
the reconstruction golden fixture (tests/golden/recon.npz).  Used by tests/golden/make_goldens_recon.py and by the
live check in tests/test_recon.py; the GPU tests read only the committed fixture.

The driver (tests/recon/ref_recon_harness.cpp) is this project's text.  It is linked against the reference's
libviso2/src/matrix.cpp, built with the flags of oracle/Makefile, and against reconstruction.cpp, built with
tests/recon/recon_prelude.h force-included (see there)."""
import os
import struct
import subprocess

import numpy as np

import helpers as H

REF = os.environ.get("REF", "/root/reference")
HERE = os.path.join(H.ROOT, "tests", "recon")
REFFLAGS = ["-O3", "-DNDEBUG", "-msse3", "-fPIC", "-w", "-std=c++11"]   # oracle/Makefile
GOLDEN = os.path.join(H.GOLDEN, "recon.npz")
CALIB = (645.2, 635.9, 194.1)           # demo_structure_from_motion.m: f, cu, cv
CODE_NAMES = ["TOO_SHORT", "INIT_FAILED", "TYPE_BELOW", "REFINE_FAILED", "TOO_FAR", "ANGLE_SMALL", "ACCEPTED"]
ACCEPTED = 6
# what a scene stores of a match (the fields Reconstruction::update reads), in the driver's file order
M6 = np.dtype([("u1p", "f4"), ("v1p", "f4"), ("i1p", "i4"), ("u1c", "f4"), ("v1c", "f4"), ("i1c", "i4")])
# (point_type, min_track_length, max_dist, min_angle) per scene
SETTINGS = {
    "frames": [(1, 2, 30, 2), (2, 2, 30, 3)],
    "synth": [(0, 2, 30, 2), (1, 2, 30, 2), (2, 2, 30, 3), (1, 4, 30, 2)],
    "edge": [(0, 2, 30, 2), (1, 3, 30, 2)],
}
SYNTH_POINTS = 6000


def have_ref():
    return os.path.isfile(os.path.join(REF, "libviso2", "src", "reconstruction.cpp"))


def build_harness(tmp):
    """compile the reference objects and the driver into tmp; returns the program's path"""
    src = os.path.join(REF, "libviso2", "src")
    objs = [os.path.join(tmp, "matrix.o"), os.path.join(tmp, "reconstruction.o")]
    subprocess.check_call(["g++"] + REFFLAGS + ["-I" + src, "-c", os.path.join(src, "matrix.cpp"), "-o", objs[0]])
    subprocess.check_call(["g++"] + REFFLAGS + ["-I" + src, "-include", os.path.join(HERE, "recon_prelude.h"), "-c",
                           os.path.join(src, "reconstruction.cpp"), "-o", objs[1]])
    exe = os.path.join(tmp, "ref_recon_harness")
    subprocess.check_call(["g++"] + REFFLAGS + ["-I" + src, os.path.join(HERE, "ref_recon_harness.cpp")] + objs +
                          ["-o", exe])
    return exe


def write_scene(path, scene):
    """scene: list of (Tr 4x4, matches M6)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(scene)))
        for Tr, m in scene:
            f.write(np.ascontiguousarray(Tr, np.float64).tobytes())
            f.write(struct.pack("<i", len(m)))
            f.write(np.ascontiguousarray(m, M6).tobytes())


def setting_args(s):
    return [str(int(s[0])), str(int(s[1])), repr(float(s[2])), repr(float(s[3]))]


def run_scene(exe, path, n_updates, setting, calib=CALIB):
    """per update: (active tracks, appended points (k,3) float32, codes of the lost tracks int32, their points)"""
    b = subprocess.run([exe, "run", path] + [repr(float(c)) for c in calib] + setting_args(setting), check=True,
                       capture_output=True).stdout
    return parse_run(b, n_updates)


def parse_run(b, n_updates):
    """the driver's output (also written by tests/recon/recon_core_check.cpp and tests/recon/recon_dropin.cpp)"""
    at, out = 0, []
    for _ in range(n_updates):
        active, napp = struct.unpack_from("<ii", b, at)
        at += 8
        pts = np.frombuffer(b, np.float32, 3 * napp, at).reshape(-1, 3).copy()
        at += 12 * napp
        nlost = struct.unpack_from("<i", b, at)[0]
        at += 4
        codes = np.frombuffer(b, np.int32, nlost, at).copy()
        at += 4 * nlost
        xyz = np.frombuffer(b, np.float32, 3 * nlost, at).reshape(-1, 3).copy()
        at += 12 * nlost
        out.append((active, pts, codes, xyz))
    assert at == len(b)
    return out


def run_bench(exe, path, setting, reps, calib=CALIB):
    return subprocess.run([exe, "bench", path] + [repr(float(c)) for c in calib] + setting_args(setting) +
                          [str(reps)], check=True, capture_output=True, text=True).stdout.strip()


# ---------------------------------------------------------------------------------------------------------- scenes
def to_m6(m):
    out = np.zeros(len(m), M6)
    for k in M6.names:
        out[k] = m[k]
    return out


def rot(rx, ry, rz):
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def project(W2C, X, calib=CALIB):
    f, cu, cv = calib
    Xc = X @ W2C[:3, :3].T + W2C[:3, 3]
    return f * Xc[:, 0] / Xc[:, 2] + cu, f * Xc[:, 1] / Xc[:, 2] + cv, Xc[:, 2]


def synth_scene(n_points=SYNTH_POINTS, n_updates=40, seed=11, noise=0.2, drop=0.05):
    """a drive forward (0.5-1.1 m per frame, small random rotation) past random points with geometric lifetimes
    (mean 4 frames, a few as long as the whole drive), pixel noise, dropped matches, feature indices permuted per
    frame, matches in random order"""
    rng = np.random.default_rng(seed)
    nf = n_updates + 1
    Trs = [rigid(rot(*rng.normal(0, 0.004, 3)), [rng.normal(0, 0.03), rng.normal(0, 0.02), -rng.uniform(0.5, 1.1)])
           for _ in range(n_updates)]
    W2C = [np.eye(4)]
    for T in Trs:
        W2C.append(T @ W2C[-1])
    birth = rng.integers(0, nf - 1, n_points)
    life = rng.geometric(0.25, n_points) + 1           # frames observed: at least two
    whole = rng.random(n_points) < 0.01
    birth[whole], life[whole] = 0, nf
    Xc = np.stack([rng.uniform(-15, 15, n_points), rng.uniform(-6, 1.6, n_points), rng.uniform(4, 60, n_points)], 1)
    Xc[whole, 2] = rng.uniform(60, 150, int(whole.sum()))
    X = np.empty_like(Xc)
    for i in range(n_points):
        C2W = np.linalg.inv(W2C[birth[i]])
        X[i] = C2W[:3, :3] @ Xc[i] + C2W[:3, 3]
    u = np.full((nf, n_points), np.nan, np.float32)
    v = np.full((nf, n_points), np.nan, np.float32)
    idx = np.full((nf, n_points), -1, np.int64)
    for k in range(nf):
        uu, vv, z = project(W2C[k], X)
        vis = (birth <= k) & (k < birth + life) & (z > 1.5) & (uu > 0) & (uu < 1242) & (vv > 0) & (vv < 375)
        u[k, vis] = (uu[vis] + rng.normal(0, noise, int(vis.sum()))).astype(np.float32)
        v[k, vis] = (vv[vis] + rng.normal(0, noise, int(vis.sum()))).astype(np.float32)
        which = np.flatnonzero(vis)
        idx[k, which] = rng.permutation(len(which))
    scene = []
    for k in range(1, nf):
        both = np.flatnonzero((idx[k - 1] >= 0) & (idx[k] >= 0))
        both = both[rng.random(len(both)) >= drop]
        both = rng.permutation(both)
        m = np.zeros(len(both), M6)
        m["u1p"], m["v1p"], m["i1p"] = u[k - 1, both], v[k - 1, both], idx[k - 1, both]
        m["u1c"], m["v1c"], m["i1c"] = u[k, both], v[k, both], idx[k, both]
        scene.append((Trs[k - 1], m))
    return scene


def edge_scene(seed=12):
    """a camera drifting sideways (5 cm per frame, no rotation) with, by update:
       3   two matches with the same i1p (the first extends the track, the second starts one);
       5   Tr = identity (two identical poses): tracks that live only in frames 4-5 have no baseline;
       6/7 two tracks ending on the same feature index (the later one owns the slot of track_idx);
       10  an empty update: every track is lost;
       11..85  tracks of 76 frames; 86 empty again (flushes them).
    All along: points behind the camera, tracks with the same pixel in both frames (rays parallel: the point is at
    infinity), tracks of random pixels, points too far and on / below the road."""
    rng = np.random.default_rng(seed)
    n_updates = 87
    nf = n_updates + 1
    Trs = [rigid(np.eye(3), [-0.05, 0, 0]) for _ in range(n_updates)]
    Trs[5] = np.eye(4)
    W2C = [np.eye(4)]
    for T in Trs:
        W2C.append(T @ W2C[-1])
    tracks = []   # (first frame, last frame, world point or None, kind)

    def add(first, last, X, kind="point"):
        tracks.append((first, last, None if X is None else np.asarray(X, float), kind))

    for first in range(0, 9):
        for _ in range(12):   # ordinary points, two to five frames
            add(first, min(first + int(rng.integers(1, 5)), 10), [rng.uniform(-4, 6), rng.uniform(-3, 1.6), rng.uniform(3, 50)])
        add(first, first + 1, [rng.uniform(-3, 3), rng.uniform(-2, 1), -rng.uniform(3, 20)])   # behind the camera
        add(first, first + 1, None, "same_pixel")
        add(first, min(first + 3, 10), None, "random")
    for _ in range(10):
        add(4, 5, [rng.uniform(-4, 6), rng.uniform(-3, 1.6), rng.uniform(3, 30)])              # zero baseline
        add(4, 5, None, "same_pixel")
    for _ in range(30):
        add(11, 86, [rng.uniform(0, 4), rng.uniform(-3, 1.6), rng.uniform(5, 14)])             # 76 frames
    for first in range(11, 80, 4):
        for _ in range(4):
            add(first, first + int(rng.integers(1, 8)), [rng.uniform(-4, 8), rng.uniform(-3, 1.6), rng.uniform(3, 60)])
        add(first, first + 2, None, "random")
    n = len(tracks)
    u = np.full((nf, n), np.nan, np.float32)
    v = np.full((nf, n), np.nan, np.float32)
    idx = np.full((nf, n), -1, np.int64)
    for i, (first, last, X, kind) in enumerate(tracks):
        fixed = (rng.uniform(100, 1100), rng.uniform(50, 330))
        for k in range(first, last + 1):
            if kind == "same_pixel":
                uu, vv = fixed
            elif kind == "random":
                uu, vv = rng.uniform(0, 1242), rng.uniform(0, 375)
            else:
                a, b, _ = project(W2C[k], X[None])
                uu, vv = a[0] + rng.normal(0, 0.1), b[0] + rng.normal(0, 0.1)
            u[k, i], v[k, i] = uu, vv
    for k in range(nf):
        which = np.flatnonzero(~np.isnan(u[k]))
        idx[k, which] = rng.permutation(len(which))
    scene = []
    for k in range(1, nf):
        both = np.flatnonzero((idx[k - 1] >= 0) & (idx[k] >= 0))
        both = rng.permutation(both)
        if k - 1 in (10, 86):
            both = both[:0]
        m = np.zeros(len(both), M6)
        m["u1p"], m["v1p"], m["i1p"] = u[k - 1, both], v[k - 1, both], idx[k - 1, both]
        m["u1c"], m["v1c"], m["i1c"] = u[k, both], v[k, both], idx[k, both]
        if k - 1 == 3 and len(m) > 4:      # the same previous feature twice
            extra = m[2:3].copy()
            extra["i1c"] = int(m["i1c"].max()) + 1
            extra["u1c"] += 1.5
            m = np.concatenate([m[:4], extra, m[4:]])
        if k - 1 == 6 and len(m) > 6:      # two matches end on the same current feature
            m["i1c"][5] = m["i1c"][1]
        scene.append((Trs[k - 1], m))
    return scene


def frames_scene(tmp):
    """the seven mono frames through the reference's VisualOdometryMono with bucketing disabled and motion_threshold
    1e6 (every estimate runs to the end): its matches and getDeltaMotion() per successful frame"""
    import mono_ref
    exe = mono_ref.build_harness(tmp)
    mono_ref.write_frames(tmp)
    p = dict(mono_ref.DEMO, motion_threshold=1e6, max_features=1000)
    scene = []
    for k, (ok, m, inl, T) in enumerate(mono_ref.run_sequence(exe, tmp, p, True)):
        if k > 0 and ok:                   # demo_structure_from_motion.m:40-67
            scene.append((T, to_m6(m)))
    return scene


# --------------------------------------------------------------------------------------------------------- fixture
def pack_scene(out, name, scene):
    out[name + "_Tr"] = np.stack([np.asarray(T, np.float64) for T, _ in scene])
    out[name + "_n"] = np.array([len(m) for _, m in scene], np.int32)
    allm = np.concatenate([m for _, m in scene]) if scene else np.zeros(0, M6)
    for k in M6.names:
        out[name + "_" + k] = np.ascontiguousarray(allm[k])


def unpack_scene(Z, name):
    n = Z[name + "_n"]
    o = np.concatenate([[0], np.cumsum(n)])
    allm = np.zeros(int(o[-1]), M6)
    for k in M6.names:
        allm[k] = Z[name + "_" + k]
    return [(Z[name + "_Tr"][i], allm[o[i]:o[i + 1]]) for i in range(len(n))]


def pack_result(out, key, res):
    out[key + "_active"] = np.array([r[0] for r in res], np.int32)
    out[key + "_napp"] = np.array([len(r[1]) for r in res], np.int32)
    out[key + "_points"] = np.concatenate([r[1] for r in res]).astype(np.float32).reshape(-1, 3)
    out[key + "_nlost"] = np.array([len(r[2]) for r in res], np.int32)
    out[key + "_codes"] = np.concatenate([r[2] for r in res]).astype(np.int8)


def unpack_result(Z, key):
    """per update: (active, appended points, codes of the lost tracks)"""
    napp, nlost = Z[key + "_napp"], Z[key + "_nlost"]
    oa, ol = np.concatenate([[0], np.cumsum(napp)]), np.concatenate([[0], np.cumsum(nlost)])
    return [(int(Z[key + "_active"][i]), Z[key + "_points"][oa[i]:oa[i + 1]],
             Z[key + "_codes"][ol[i]:ol[i + 1]].astype(np.int32)) for i in range(len(napp))]


def to_p_match(m):
    out = np.zeros(len(m), H.P_MATCH)
    for k in M6.names:
        out[k] = m[k]
    return out


# ---------------------------------------------------------------------------------------------------------- collide
# Scene `collide` (tests/golden/recon_collide.npz, make_goldens_recon_collide.py): the sizes and collisions at which the
# resident track table's kernels (recon_track_kernels.hip) can go wrong.  The number of active tracks after an update is
# that update's number of matches, so COLLIDE_N is also the n_old of the following update.
COLLIDE_N = [1023, 1024, 1025, 2048, 2049, 3000, 0, 1, 1025, 2049, 1024, 2048, 0]
COLLIDE_SETTINGS = [(0, 2, 30, 2), (1, 3, 30, 2), (2, 3, 30, 3)]
COLLIDE_SHARE_AT = (1, 2, 3, 9, 10)  # updates in which matches are given the i1c of another match
COLLIDE_QUIET = 5                       # the update in which every old track is extended
COLLIDE_GROUPS = 16                     # collisions of either kind per update
COLLIDE_SPARSE = 60000                  # feature indices of a sparse frame are drawn below this


def sequential_update(last, length, m):
    """reconstruction.cpp:75-145 on (last_idx, length) per track: the new table, the lost tracks' lengths, and per
    match the number of its track in the new table"""
    n_old = len(last)
    slot = {}
    for t, li in enumerate(last):
        slot[li] = t                                  # a later track overwrites the slot
    new_last, new_len, owner = list(last), list(length), [-1] * len(m)
    extended = set()
    for i, q in enumerate(m):
        t = slot.get(int(q["i1p"]), -1)
        if t >= 0 and t not in extended:
            extended.add(t)
            new_last[t], new_len[t] = int(q["i1c"]), length[t] + 1
            owner[i] = t
        else:
            owner[i] = len(new_last)
            new_last.append(int(q["i1c"]))
            new_len.append(2)
    keep = [t for t in range(len(new_last)) if t >= n_old or t in extended]
    at = {t: j for j, t in enumerate(keep)}
    return ([new_last[t] for t in keep], [new_len[t] for t in keep],
            [length[t] for t in range(n_old) if t not in extended], [at[t] for t in owner])


def collide_scene(seed=31, noise=0.2):
    """a drive as synth_scene's whose updates have exactly COLLIDE_N matches, with, by construction:
       * after each update of COLLIDE_SHARE_AT, COLLIDE_GROUPS feature indices on which two (every fourth: three)
         tracks end whose numbers lie in different blocks of 256, each the i1p of a match of the following update;
       * in each following update, COLLIDE_GROUPS i1p values named by two to four matches whose positions lie in
         different blocks of 256, every third of them one of the shared indices above;
       * update COLLIDE_QUIET extends every one of its 2049 old tracks; the update after it is empty (3000 lost);
       * feature indices drawn below COLLIDE_SPARSE in frames 0, 1, 4, 5, ... and below the frame's number of
         features in frames 2, 3, 6, 7, ...: the index table is far larger than n in some updates, about n in others."""
    rng = np.random.default_rng(seed)
    N, K = COLLIDE_N, len(COLLIDE_N)
    nf = K + 1
    Trs = [rigid(rot(*rng.normal(0, 0.004, 3)), [rng.normal(0, 0.03), rng.normal(0, 0.02), -rng.uniform(0.5, 1.1)])
           for _ in range(K)]
    W2C = [np.eye(4)]
    for T in Trs:
        W2C.append(T @ W2C[-1])
    # which point is matched in which update, in match order
    sets, prev, n_points = [], np.zeros(0, np.int64), 0
    for k, n in enumerate(N):
        c = len(prev) if k == COLLIDE_QUIET else min(len(prev), n) * 7 // 10
        new = np.arange(n_points, n_points + n - c)
        n_points += n - c
        prev = rng.permutation(np.concatenate([rng.permutation(prev)[:c], new]))
        sets.append(prev)
    first, last = np.full(n_points, -1), np.full(n_points, -1)
    for k, s in enumerate(sets):
        first[s] = np.where(first[s] < 0, k, first[s])
        last[s] = k
    # a point inside the image of its first frame, far enough ahead to stay in front for its whole life
    f, cu, cv = CALIB
    z = rng.uniform(3, 28, n_points) + 1.2 * (last - first + 2)
    uu, vv = rng.uniform(50, 1190, n_points), rng.uniform(20, 355, n_points)
    Xc = np.stack([(uu - cu) / f * z, (vv - cv) / f * z, z], 1)
    X = np.empty_like(Xc)
    for k in range(K):
        C2W = np.linalg.inv(W2C[k])
        w = first == k
        X[w] = Xc[w] @ C2W[:3, :3].T + C2W[:3, 3]
    u = np.zeros((nf, n_points), np.float32)
    v = np.zeros((nf, n_points), np.float32)
    idx = np.full((nf, n_points), -1, np.int64)
    for fr in range(nf):
        seen = np.unique(np.concatenate([sets[k] for k in (fr - 1, fr) if 0 <= k < K]))
        a, b, _ = project(W2C[fr], X[seen])
        u[fr, seen] = (a + rng.normal(0, noise, len(seen))).astype(np.float32)
        v[fr, seen] = (b + rng.normal(0, noise, len(seen))).astype(np.float32)
        top = COLLIDE_SPARSE if fr % 4 < 2 else len(seen) + 7
        idx[fr, seen] = rng.choice(top, len(seen), replace=False)
    scene = []
    for k, s in enumerate(sets):
        m = np.zeros(len(s), M6)
        m["u1p"], m["v1p"], m["i1p"] = u[k, s], v[k, s], idx[k, s]
        m["u1c"], m["v1c"], m["i1c"] = u[k + 1, s], v[k + 1, s], idx[k + 1, s]
        scene.append((Trs[k], m))

    def pick(rng, pools, used, blocks=()):
        """one index out of each pool, not used before, each in another block of 256 than the first of the group and,
        while blocks last, than every other one of it (pools: (index, block); blocks: those the group has already)"""
        got, blocks = [], list(blocks)
        for pool in pools:
            free = [pool[j] for j in rng.permutation(len(pool)) if pool[j][0] not in used]
            hit = [c for c in free if c[1] not in blocks] or [c for c in free if c[1] != blocks[0]]
            assert hit, "no candidate left"
            got.append(hit[0][0])
            blocks.append(hit[0][1])
            used.add(hit[0][0])
        return got

    tbl_last, tbl_len, asked = [], [], []
    for k, (T, m) in enumerate(scene):
        goes_on = np.isin(sets[k], sets[k + 1]) if k + 1 < K else np.zeros(len(m), bool)
        born = first[sets[k]] == k
        used = set()
        if k - 1 in COLLIDE_SHARE_AT:
            # the same i1p in several matches: a match that extends a track and goes on, and matches of points seen
            # for the first time that do not go on (whether they go on is not asked before an update in which every point does, or none)
            old = [(i, i // 256) for i in np.flatnonzero(~born & (goes_on | ~goes_on.any()))]
            fresh = [(i, i // 256) for i in np.flatnonzero(born & (~goes_on | goes_on.all()))]
            for g in range(COLLIDE_GROUPS):
                extra = 1 + g % 3
                if g % 3 == 0:
                    a = asked[g]                          # ... the match that asks for a shared index
                    assert a not in used
                    used.add(a)
                    got = [a] + pick(rng, [fresh] * extra, used, [a // 256])
                else:
                    got = pick(rng, [old] + [fresh] * extra, used)
                assert all(i // 256 != got[0] // 256 for i in got[1:])
                m["i1p"][got[1:]] = m["i1p"][got[0]]
        _, new_len, _, track = sequential_update(tbl_last, tbl_len, m)
        track = np.array(track)
        asked = []
        if k in COLLIDE_SHARE_AT:
            # the same i1c in several matches: one whose point goes on (the next update asks for the index) and one or
            # two whose points do not; alternately the one that goes on is the longer track and the shorter
            long_on = [(i, track[i] // 256) for i in np.flatnonzero(~born & goes_on) if i not in used]
            short_on = [(i, track[i] // 256) for i in np.flatnonzero(born & goes_on) if i not in used]
            long_off = [(i, track[i] // 256) for i in np.flatnonzero(~born & ~goes_on) if i not in used]
            short_off = [(i, track[i] // 256) for i in np.flatnonzero(born & ~goes_on) if i not in used]
            nxt = scene[k + 1][1]
            for g in range(COLLIDE_GROUPS):
                pools = [[long_on, short_off], [short_on, long_off], [long_on, long_off]][g % 3]
                if g % 4 == 0:
                    pools = pools + [short_off if g % 8 else long_off]
                got = pick(rng, pools, used)
                m["i1c"][got[1:]] = m["i1c"][got[0]]
                hit = np.flatnonzero(sets[k + 1] == sets[k][got[0]])
                assert len(hit) == 1 and nxt["i1p"][hit[0]] == m["i1c"][got[0]]
                asked.append(int(hit[0]))
        tbl_last, tbl_len, _, _ = sequential_update(tbl_last, tbl_len, m)
    assert [len(m) for _, m in scene] == COLLIDE_N
    return scene


COLLIDE_GOLDEN = os.path.join(H.GOLDEN, "recon_collide.npz")
COLLIDE_BOUNDARIES = (0, 1, 1023, 1024, 1025, 2048, 2049, 3000)


def collide_properties(scene, update):
    """what scene `collide` is there for, recomputed from its matches by `update` (sequential_update above, or the
    parallel form of tests/test_recon_resident.py: the first three values of what it returns are used)"""
    out = {"n": [], "n_old": [], "lost": [], "tbl": [], "shared": [], "three_way": [], "named": [], "both": []}
    last, length = [], []
    for k, (_, m) in enumerate(scene):
        i1p = m["i1p"].astype(np.int64)
        out["n"].append(len(m))
        out["n_old"].append(len(last))
        out["tbl"].append(int(max([-1] + list(last) + i1p.tolist() + m["i1c"].tolist())) + 1)
        owners = {}
        for t, li in enumerate(last):
            owners.setdefault(li, []).append(t)
        asked = set(i1p.tolist())
        shared = {li for li, ts in owners.items() if li in asked and len({t // 256 for t in ts}) >= 2}
        out["shared"] += [(k, li) for li in sorted(shared)]
        out["three_way"] += [(k, li) for li in sorted(shared) if len({t // 256 for t in owners[li]}) >= 3]
        at = {}
        for i, p in enumerate(i1p.tolist()):
            at.setdefault(p, []).append(i)
        named = {p for p, ii in at.items() if 2 <= len(ii) <= 4 and len({i // 256 for i in ii}) >= 2}
        out["named"] += [(k, p) for p in sorted(named)]
        out["both"] += [(k, p) for p in sorted(named & shared)]
        res = update(last, length, m)
        last, length = res[0], res[1]
        out["lost"].append(len(res[2]))
    return out


def check_collide_properties(p):
    """conditions, not measurements: a scene that loses one of them is not `collide`"""
    assert p["n"] == COLLIDE_N and p["n_old"] == [0] + COLLIDE_N[:-1]
    for b in COLLIDE_BOUNDARIES:
        assert b in p["n"] and b in p["n_old"], b
    k = COLLIDE_QUIET
    assert p["n_old"][k] >= 2049 and p["lost"][k] == 0 and p["n"][k] >= 3000           # a large update, nothing lost
    assert p["n"][k + 1] == 0 and p["lost"][k + 1] == p["n_old"][k + 1] >= 12 * 250    # every track lost: 12 rounds of 256
    assert p["n"][k + 2] == 1 and p["n_old"][k + 2] == 0
    assert len(p["shared"]) >= 50 and len(p["three_way"]) >= 10, (len(p["shared"]), len(p["three_way"]))
    assert len(p["named"]) >= 50 and len(p["both"]) >= 5, (len(p["named"]), len(p["both"]))
    ratio = [t / n for t, n in zip(p["tbl"], p["n"]) if n >= 1000]
    assert min(ratio) < 3 and max(ratio) > 20, ratio                                   # the index table: about n, far above n
    assert max(p["tbl"]) > 50000

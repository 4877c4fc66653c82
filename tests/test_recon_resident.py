"""CPU: the resident form of Reconstruction (svh_recon_create_resident, svh_recon_update_device,
svh_recon_update_batch; include/svh.h) at the boundary, and the parallel form of the track association it runs.

The entries are exported and declared; their argument checks answer SVH_ERR_BAD_ARG, a batch with a host-table object
among them; without a device every compute entry of a resident object returns SVH_ERR_NO_DEVICE.  What they compute
is checked on the GPU (tests/test_recon_resident_gpu.py).

The association of reconstruction.cpp:75-145 looks sequential.  The kernels run this form of it (recon_internal.h):
track_idx[last_idx[t]] = the largest t; claim[idx] = the smallest match i with track_idx[i1p] == idx; match i extends
its track iff claim[idx] == i and creates one otherwise; new order = extended old tracks in old order, then created
tracks in match order; lost tracks in old order.  parallel_update() below is a RESTATEMENT of that form in Python,
written serially -- it pins the derivation, not the kernels' code -- and is run over every update of
tests/golden/recon.npz and tests/golden/recon_shared.npz: the number of active tracks, the number of lost tracks and
which of them are shorter than min_track_length (outcome code 0) must equal the reference's record.

recon.npz has two matches with the same i1p, and two matches with the same i1c (two tracks then end on one feature
index) -- but no match of the following update has that index as its i1p, so which of the two tracks owns the slot is
never asked there.  recon_shared.npz (make_goldens_recon_shared.py) asks it five times: the match extends the
higher-indexed track and the other is lost.  The same restatement with the owner rule turned round (the lowest t) must
NOT reproduce the reference on that scene: the fixture tells the two rules apart."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import recon_ref as R

NAMES = ["svh_recon_create_resident", "svh_recon_update_device", "svh_recon_update_batch"]
NONE = 1 << 30


@pytest.fixture(scope="module")
def S():
    import svhip
    return svhip


SHARED = os.path.join(H.GOLDEN, "recon_shared.npz")


@pytest.fixture(scope="module")
def Z():
    """both fixtures as one: the scenes of recon.npz, then `shared`"""
    with np.load(R.GOLDEN) as z, np.load(SHARED) as y:
        out = {k: z[k] for k in z.files}
        assert np.array_equal(y["calib"], z["calib"])
        out.update({k: y[k] for k in y.files if k not in ("calib", "scene_names")})
        out["scene_names"] = np.concatenate([z["scene_names"], y["scene_names"]])
        return out


def parallel_update(last_idx, length, m, owner=max, claim=min):
    """one update of the track table (last_idx, length per track) by the matches m: the new table and the lengths of
    the lost tracks, in order.  owner / claim: the two rules, to be turned round by tests that show a scene tells
    them apart"""
    n_old, claim_rule = len(last_idx), claim
    table = {}
    for t in range(n_old):                                    # k_rt_scatter: atomicMax
        table[last_idx[t]] = owner(table.get(last_idx[t], t), t)
    idx = [table.get(int(p), -1) for p in m["i1p"]]
    claim = [NONE] * n_old
    for i, t in enumerate(idx):                               # k_rt_associate: atomicMin
        if t >= 0:
            claim[t] = i if claim[t] == NONE else claim_rule(claim[t], i)
    extended = [t for t in range(n_old) if claim[t] != NONE]  # k_rt_scan
    lost = [t for t in range(n_old) if claim[t] == NONE]
    created = [i for i, t in enumerate(idx) if not (t >= 0 and claim[t] == i)]
    new_last = [int(m["i1c"][claim[t]]) for t in extended] + [int(m["i1c"][i]) for i in created]
    new_len = [length[t] + 1 for t in extended] + [2] * len(created)
    return new_last, new_len, [length[t] for t in lost]


def test_symbols_are_exported_and_declared(S):
    hdr = open(os.path.join(H.ROOT, "include", "svh.h")).read()
    for name in NAMES:
        assert hasattr(S.lib(), name), name
        assert (name + "(") in hdr, name


def test_fixture_has_shared_previous_and_shared_current_features(Z):
    edge = R.unpack_scene(Z, "edge")
    assert len(edge[3][1]) != len(np.unique(edge[3][1]["i1p"]))   # the first extends, the second creates
    assert len(edge[6][1]) != len(np.unique(edge[6][1]["i1c"]))   # two tracks end on one feature index


def shared_slots_asked(scene):
    """(update, lower track, higher track, their lengths) wherever a match's i1p is a last_idx that two tracks share"""
    out, last, length = [], [], []
    for k, (_, m) in enumerate(scene):
        for idx in sorted(set(int(p) for p in m["i1p"])):
            owners = [t for t, li in enumerate(last) if li == idx]
            if len(owners) >= 2:
                out.append((k, owners[0], owners[-1], length[owners[0]], length[owners[-1]]))
        last, length, _ = parallel_update(last, length, m)
    return out


def test_shared_fixture_asks_who_owns_a_shared_slot(Z):
    assert os.path.getsize(SHARED) <= 1024 * 1024
    for name in ("frames", "synth", "edge"):
        assert shared_slots_asked(R.unpack_scene(Z, name)) == [], name     # recon.npz never asks
    scene = R.unpack_scene(Z, "shared")
    asked = shared_slots_asked(scene)
    assert len(asked) >= 5 and len({k for k, _, _, _, _ in asked}) >= 5, asked
    assert all(la != lb for _, _, _, la, lb in asked), asked               # the two tracks can be told apart
    assert any(lb == 2 for _, _, _, _, lb in asked)                        # a wrong owner loses a 2-frame track
    # in one of those updates the shared index is the i1p of two matches: the first extends, the second creates
    twice = [k for k, _, _, _, _ in asked
             if any(np.count_nonzero(scene[k][1]["i1p"] == i) >= 2 for i in set(scene[k][1]["i1p"].tolist()))]
    assert twice, asked
    assert 3.0 in Z["shared_settings"][:, 1]                               # a setting under which lengths 2 and 3 differ


def model_matches(Z, name, owner, claim=min):
    scene = R.unpack_scene(Z, name)
    for j, s in enumerate(Z["%s_settings" % name]):
        want = R.unpack_result(Z, "%s_%d" % (name, j))
        last, length = [], []
        for k, (_, m) in enumerate(scene):
            last, length, lost_len = parallel_update(last, length, m, owner, claim)
            active, _, codes = want[k]
            if len(last) != active or len(lost_len) != len(codes):
                return (name, j, k, "counts")
            if not np.array_equal(np.array(lost_len, np.int64) < int(s[1]), codes == 0):
                return (name, j, k, "too-short codes")
    return None


def test_parallel_association_reproduces_reference(Z):
    for name in Z["scene_names"]:
        assert model_matches(Z, str(name), max) is None
    # the owner rule matters on `shared` and nowhere in recon.npz
    assert model_matches(Z, "shared", min) is not None
    for name in ("frames", "synth", "edge"):
        assert model_matches(Z, name, min) is None


def bind(S):
    L = S.lib()
    v = C.c_void_p
    L.svh_recon_create.restype = v
    L.svh_recon_create_resident.restype = v
    L.svh_recon_destroy.argtypes = [v]
    L.svh_recon_set_calibration.argtypes = [v, C.c_double, C.c_double, C.c_double]
    L.svh_recon_update.argtypes = [v, v, C.c_int32, v, C.c_int32, C.c_int32, C.c_double, C.c_double]
    L.svh_recon_update_device.argtypes = [v, v, C.c_int32, C.c_int32, v, C.c_int32, C.c_int32, C.c_double, C.c_double]
    L.svh_recon_update_batch.argtypes = [v, v, v, v, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, v]
    L.svh_recon_num_points.argtypes = [v]
    L.svh_recon_num_tracks.argtypes = [v]
    L.svh_recon_get_outcomes.argtypes = [v, v, v, C.c_int32]
    return L


def test_argument_checks_and_no_device(S):
    L = bind(S)
    a, b, fresh, host = (L.svh_recon_create_resident(), L.svh_recon_create_resident(), L.svh_recon_create_resident(),
                         L.svh_recon_create())
    assert a and b and fresh and host
    for r in (a, b, host):
        assert L.svh_recon_set_calibration(r, *R.CALIB) == S.OK
    assert L.svh_recon_set_calibration(a, *R.CALIB) == S.ERR_BAD_ARG            # once per object, as before
    Tr = np.stack([np.eye(4), np.eye(4)])
    m = np.zeros(4, S.P_MATCH)
    m["i1p"], m["i1c"] = np.arange(4), np.arange(4)
    mp = (C.c_void_p * 2)(m.ctypes.data, m.ctypes.data)
    n = (C.c_int32 * 2)(4, 4)
    st = (C.c_int32 * 2)()

    def batch(hs, K=2, mp=mp, n=n, Tr=Tr):
        return L.svh_recon_update_batch(hs, mp, n, None if Tr is None else Tr.ctypes.data, K, 1, 2, 30.0, 2.0, st)

    bad = {
        "null object": (C.c_void_p * 2)(a, None),
        "host-table object": (C.c_void_p * 2)(a, host),
        "duplicate": (C.c_void_p * 2)(a, a),
        "not calibrated": (C.c_void_p * 2)(a, fresh),
    }
    for why, hs in bad.items():
        assert batch(hs) == S.ERR_BAD_ARG, why
    good = (C.c_void_p * 2)(a, b)
    assert batch(good, K=-1) == S.ERR_BAD_ARG
    assert batch(None) == S.ERR_BAD_ARG
    assert batch(good, mp=None) == S.ERR_BAD_ARG
    assert batch(good, n=None) == S.ERR_BAD_ARG
    assert batch(good, Tr=None) == S.ERR_BAD_ARG
    assert batch(good, n=(C.c_int32 * 2)(4, -1)) == S.ERR_BAD_ARG
    assert batch(good, K=0) == S.OK
    # the single entries
    T = np.eye(4)
    upd = lambda r, mm, k: L.svh_recon_update(r, mm, k, T.ctypes.data, 1, 2, 30.0, 2.0)
    dev = lambda r, p, k, top: L.svh_recon_update_device(r, p, k, top, T.ctypes.data, 1, 2, 30.0, 2.0)
    assert upd(fresh, None, 0) == S.ERR_BAD_ARG                                  # before set_calibration
    assert dev(fresh, None, 0, 0) == S.ERR_BAD_ARG
    assert dev(host, None, 0, 0) == S.ERR_BAD_ARG                                # needs a resident object
    assert dev(a, None, 3, 10) == S.ERR_BAD_ARG                                  # matches missing
    assert dev(a, None, 0, -1) == S.ERR_BAD_ARG
    assert upd(a, None, 3) == S.ERR_BAD_ARG
    neg = m.copy()
    neg["i1c"][2] = -1
    assert upd(a, neg.ctypes.data, 4) == S.ERR_BAD_ARG
    big = m.copy()
    big["i1p"][1] = 1 << 26
    assert upd(a, big.ctypes.data, 4) == S.ERR_BAD_ARG
    for r in (a, b, fresh):
        assert L.svh_recon_num_points(r) == 0 and L.svh_recon_num_tracks(r) == 0
        assert L.svh_recon_get_outcomes(r, None, None, 0) == 0
    if S.device_count() == 0:
        # no device: every compute entry of a resident object says so, and nothing has changed
        assert upd(a, m.ctypes.data, 4) == S.ERR_NO_DEVICE
        assert "no HIP device" in S.last_error()
        assert upd(a, None, 0) == S.ERR_NO_DEVICE
        assert dev(a, None, 0, 0) == S.ERR_NO_DEVICE
        assert batch(good) == S.ERR_NO_DEVICE
        assert batch(good, K=1) == S.ERR_NO_DEVICE
        assert L.svh_recon_num_tracks(a) == 0 and L.svh_recon_num_tracks(b) == 0
    for r in (a, b, fresh, host):
        L.svh_recon_destroy(r)


def test_wrapper_takes_resident_argument(S):
    r = S.Reconstruction(resident=True)
    assert r.resident and r.num_tracks() == 0 and r.num_points() == 0
    h = S.Reconstruction()
    assert not h.resident
    h.set_calibration(*R.CALIB)
    r.set_calibration(*R.CALIB)
    with pytest.raises(S.SvhError) as e:
        S.Reconstruction.update_batch([r, h], [np.zeros(0, S.P_MATCH)] * 2, [np.eye(4)] * 2)
    assert e.value.code == S.ERR_BAD_ARG
    r.close()
    h.close()

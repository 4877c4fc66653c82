"""GPU: the prediction of the ground grid on the device (include/svh_grid_pred.h, "PREDICTION";
stereo-vision_amd/csrc/grid_pred_kernels.hip) against the restatement tests/grid_pred_ref.py, byte for byte: PRED, its statistics,
the footprint masks, the records, the scores, the best and the image.  First the kernels of PRED on a caller's ID plane and track
table (svh_test_grid_pred_device) at the sizes where they take another path -- frames round the tiles of both inflation passes, the
radii 0 (the skipped form), 1 and 16, track tables round a wave and at their largest --, then the object: frames played on it, a step
each, and everything it reports compared with the restatement of its own track state and planes (tests/grid_pred_cases.py).
tests/test_grid_pred.py pins the restatement by hand."""
import ctypes as C

import numpy as np
import pytest

import grid_obj_cases as OC
import grid_obj_ref as OR
import grid_pred_cases as PC
import grid_pred_ref as PR
import grid_roll_ref as RR
import helpers as H   # puts the package on the path
from test_view_gpu import Dev

pytestmark = pytest.mark.gpu
T = OR.T
BAD_ARG = -1


@pytest.fixture(scope="module")
def G():
    import svhip
    from svhip import grid
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    grid._bind()
    return grid


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


# ---- PRED on a caller's plane and table ------------------------------------------------------------------------------------------
def table(rng, n, vmax=40, gaps=True):
    """n track records with ascending ids that are not contiguous, random velocities, some without the MOVING flag, some missed"""
    ids = np.cumsum(rng.integers(1, 4 if gaps else 2, n)).astype(np.int32)
    t = np.zeros((n, 14), np.int32)
    t[:, T["id"]], t[:, T["label"]] = ids, np.where(rng.random(n) < 0.1, -1, 5)
    t[:, T["flags"]] = np.where(rng.random(n) < 0.8, OR.MOVING | OR.BY_OVERLAP, OR.BY_OVERLAP)
    t[:, T["v16_a"]], t[:, T["v16_b"]] = rng.integers(-vmax, vmax + 1, n), rng.integers(-vmax, vmax + 1, n)
    return t


def plane_of(rng, nx, nz, tracks, border=True):
    """an ID plane: a small block per track with a label, the first four on the four borders; ids the table does not hold among them"""
    ids = np.full((nz, nx), -1, np.int32)
    spots = [(0, nz // 2), (nx - 1, nz // 2), (nx // 2, 0), (nx // 2, nz - 1)] if border else []
    for k, t in enumerate(tracks):
        if t[T["label"]] < 0:
            continue
        a, b = spots[k] if k < len(spots) else (int(rng.integers(0, nx)), int(rng.integers(0, nz)))
        w, h = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        ids[b:b + h, a:a + w] = t[T["id"]]
    ids[nz // 3, nx // 3] = 0x7FFFFFF0                                         # a stranger
    return ids


def same(G, kw, ids, tracks, tag=""):
    want, wstats = PR.plane(PR.PredParams(**kw), ids, tracks)
    got, gstats = G.device_pred(G.default_pred(**kw), ids, tracks)
    assert np.array_equal(got, want), (tag, kw, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])
    assert gstats == wstats + (PR.launches(PR.PredParams(**kw), len(tracks)),), (tag, gstats, wstats)
    return want, wstats


FRAMES = [(16, 16), (17, 17), (33, 31), (64, 64), (257, 130)]
RADII = [dict(margin=0, grow16=0), dict(margin=1, grow16=0), dict(margin=16, grow16=0), dict(margin=0, grow16=24)]


@pytest.mark.parametrize("nx,nz", FRAMES)
@pytest.mark.parametrize("r", range(len(RADII)))
def test_frames_round_the_tiles_at_every_radius(G, nx, nz, r):
    rng = np.random.default_rng(100 * nx + r)
    tracks = table(rng, 12)
    tracks[:4, T["label"]], tracks[:4, T["flags"]] = 5, OR.MOVING
    tracks[:4, T["v16_a"]], tracks[:4, T["v16_b"]] = [-24, 24, 3, -3], [3, -3, -24, 24]      # the border blocks leave through their border
    ids = plane_of(rng, nx, nz, tracks)
    for slots, only in ((8, 1), (32, 0)):
        pred, stats = same(G, dict(RADII[r], slots=slots, only_moving=only), ids, tracks)
        assert stats[2] > 0 and (pred[:, 0] != 0).any() and (pred[:, -1] != 0).any() and (pred[0] != 0).any() and (pred[-1] != 0).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_track_tables_round_a_wave_and_at_their_largest(G, n):
    rng = np.random.default_rng(n)
    nx = nz = 128
    tracks = table(rng, n, vmax=64)
    ids = np.full((nz, nx), -1, np.int32)                                      # one cell per track on every second cell of every second row
    k = rng.permutation(4096)[:n]
    ids[2 * (k // 64), 2 * (k % 64)] = tracks[:, T["id"]]
    for kw in (dict(margin=0, slots=8), dict(margin=2, slots=32, stride=2)):
        _, stats = same(G, dict(kw, only_moving=1), ids, tracks)
        assert stats[0] == ((tracks[:, T["label"]] >= 0) & ((tracks[:, T["flags"]] & OR.MOVING) != 0)).sum() == stats[1]


def test_slow_fast_and_meeting_tracks_and_the_ends_of_the_slots(G):
    tracks = np.zeros((4, 14), np.int32)
    tracks[:, T["id"]], tracks[:, T["flags"]] = [2, 5, 6, 9], OR.MOVING
    tracks[:, T["v16_a"]], tracks[:, T["v16_b"]] = [0, 1, 16, -16], [0, 0, 16, 0]
    ids = np.full((40, 70), -1, np.int32)
    ids[30:32, 3:5], ids[20, 3], ids[2, 1], ids[33, 64] = 2, 5, 6, 9
    for slots in (1, 31, 32):
        pred, _ = same(G, dict(slots=slots, margin=0), ids, tracks)
        every = (1 << slots) - 1
        assert (pred[30:32, 3:5] == every).all()                              # a standing block: all slots collapse onto its own cells
        assert pred[20, 3] == every & 0xFF and pred[20, 4] == every & 0xFFFF00 and pred[20, 5] == every & 0xFF000000    # three targets
        assert [int(pred[2 + s, 1 + s]) for s in range(min(slots, 32))] == [1 << s for s in range(slots)]              # every slot another
    # two tracks onto one cell: at (33, 32) the squares of radius 2 of track 6, at (31, 32) and (32, 33) in slots 30 and 31, and of
    # track 9, at (35, 33), (34, 33) and (33, 33) in slots 29 to 31
    pred, _ = same(G, dict(slots=32, margin=2), ids, tracks)
    assert pred[32, 33] == 0xE0000000
    # int32 extremes of the velocity: the 64-bit path
    tracks[:, T["v16_a"]], tracks[:, T["v16_b"]] = [2 ** 31 - 1, -2 ** 31, 1, -1], [-2 ** 31, 2 ** 31 - 1, -1, 1]
    same(G, dict(slots=32, stride=64, margin=1), ids, tracks)


def test_an_empty_table_and_a_table_that_predicts_nothing(G):
    pred, stats = G.device_pred(G.default_pred(), None, np.zeros((0, 14), np.int32), shape=(17, 33))
    assert not pred.any() and stats == (0, 0, 0, 0)
    rng = np.random.default_rng(5)
    tracks = table(rng, 9)
    tracks[:, T["flags"]] = OR.BY_OVERLAP
    _, stats = same(G, dict(), plane_of(rng, 33, 17, tracks), tracks)
    assert stats == (0, 0, 0)


# ---- the object ------------------------------------------------------------------------------------------------------------------
def crossing(nx=64, nz=48):
    """a 2 x 2 block that crosses from the left at one cell per step, a 1 x 3 block that comes down at two, a block that stands"""
    return PC.merged(PC.moving_block(nx, nz, 4, 20, 2, 2, 1, 0), PC.moving_block(nx, nz, 40, 40, 1, 3, 0, -2), PC.moving_block(nx, nz, 50, 8, 3, 3, 0, 0))


def straight(K, T, b0=0, step=1):
    """K candidates of T poses along +a (heading 0), candidate c on row b0 + c"""
    tab = np.zeros((1, K, T, 3), np.int32)
    tab[0, :, :, 0] = step * (np.arange(T) + 1)
    tab[0, :, :, 1] = b0 + np.arange(K)[:, None]
    return tab


def test_before_the_first_step_and_after_a_reset(G):
    g = PC.new_grid(G, 33, 31)
    pred, stats, off = PC.check_pred(g, "no step yet")
    assert not pred.any() and stats == (0, 0, 0, 0) and off == (0, 0)
    PC.play(g, crossing(33, 31)[:2])
    g.set_predict(only_moving=0)
    assert PC.check_pred(g, "two steps")[1][0] >= 1
    g.objects_reset()
    assert PC.check_pred(g, "reset")[1] == (0, 0, 0, 0)
    g.close()


def test_refusals_change_nothing(G):
    g = PC.new_grid(G, 17, 17, pred=dict(slots=5, stride=2, margin=3))
    before = g.get_predict().asdict()
    for kw in (dict(slots=0), dict(slots=33), dict(stride=0), dict(stride=65), dict(poses_per_step=0), dict(poses_per_step=1025), dict(margin=-1),
               dict(margin=17), dict(grow16=-1), dict(grow16=257), dict(only_moving=-1), dict(only_moving=2)):
        with pytest.raises(G.SvhError) as e:
            g.set_predict(**kw)
        assert e.value.code == BAD_ARG and g.get_predict().asdict() == before, kw
    with pytest.raises(G.SvhError):
        g.footprint_pred(np.array([[0, 0, 64]], np.int32))                     # a heading that does not exist, host path
    with pytest.raises(G.SvhError):
        g.render_pred(mode=3)
    g.set_candidates(straight(1, 1))
    with pytest.raises(G.SvhError):
        g.roll_score_pred(PC.centre(0, 0), 1)                                  # no such set
    g.close()


@pytest.mark.parametrize("kw", [dict(), dict(margin=0), dict(margin=16, slots=32), dict(slots=1, only_moving=0), dict(slots=31, stride=3, grow16=20),
                                dict(poses_per_step=3, only_moving=0)])
def test_crossing_objects_scored_with_the_default_car(G, kw):
    nx, nz = 64, 48
    g = PC.new_grid(G, nx, nz, pred=kw)
    PC.play(g, crossing())
    moving = (g.tracks()[:, T["flags"]] & OR.MOVING) != 0
    assert moving.tolist() == [False, True, True]                              # by label: the standing block, the crossing one, the one that comes down
    tab = G.arc_candidates(PC.CELL, 8, [-0.2, -0.05, 0.0, 0.05, 0.2], 0.5, 24)
    g.set_candidates(tab)
    seen = set()
    for set_, at in ((16, (12, 4)), (0, (2, 21)), (32, (41, 20)), (16, (7, 2))):
        best, recs, scores = PC.check_score(G, g, tab, PC.centre(*at), set_, "set %d at %r" % (set_, at), image=set_ == 16)
        seen |= set(recs[:, 1].tolist())
    if not kw:                                                                 # the car that drives straight up column 12 meets the crossing block's slot 7
        assert PR.CUT_OBJECT in seen, seen
    g.close()


def test_a_scroll_between_the_step_and_the_query(G):
    nx, nz = 64, 48
    g = PC.new_grid(G, nx, nz, pred=dict(only_moving=0, margin=2))
    PC.play(g, crossing())
    tab = G.arc_candidates(PC.CELL, 8, [-0.1, 0.0, 0.1], 0.5, 20)
    g.set_candidates(tab)
    pred, stats, off = PC.check_pred(g)
    rng = np.random.default_rng(3)
    for move in ((3, -5), (70, 60)):                                           # a few cells; more than the window
        g.scroll(*move)
        assert g.pred_plane()[1] == off and np.array_equal(g.pred_plane()[0], pred)       # the frame stays where the step left it
        oa, ob = g.window()
        for at in ((oa + 5, ob + 20), (off[0] + 5, off[1] + 25), (oa - 3, ob + 5)):      # in the window, in the frame, outside the window
            PC.check_score(G, g, tab, PC.centre(*at), 0, "after scrolling %r at %r" % (move, at))
        # footprints that straddle the frame's edge inside the window and the reverse, and bad headings on the device path
        rp, lists = PC.roll_of(g)
        poses = np.stack([rng.integers(min(oa, off[0]) - 9, max(oa, off[0]) + nx + 9, 400), rng.integers(min(ob, off[1]) - 9, max(ob, off[1]) + nz + 9, 400),
                          rng.integers(0, 64, 400)], 1).astype(np.int32)
        assert np.array_equal(g.footprint_pred(poses), PR.footprint_masks(lists, pred, off, poses))
    g.close()


def test_device_pointers_and_null_outputs(G, hip):
    nx, nz = 64, 48
    g = PC.new_grid(G, nx, nz, pred=dict(only_moving=0))
    PC.play(g, crossing())
    tab = G.arc_candidates(PC.CELL, 8, [-0.1, 0.0, 0.1], 0.5, 20)
    g.set_candidates(tab)
    at = PC.centre(2, 21)
    best, recs, scores = PC.check_score(G, g, tab, at, 0)
    K = tab.shape[1]
    d_recs, d_scores, d_plane = Dev(hip, 24 * K + 16), Dev(hip, 8 * K + 16), Dev(hip, 4 * nx * nz + 16)
    assert g.roll_score_pred(at, 0, device_ptrs=(d_recs.addr, d_scores.addr)) == best
    out = d_recs.get()
    assert np.array_equal(out[:24 * K].view(np.int32).reshape(K, 6), recs) and (out[24 * K:] == 0xEE).all()
    out = d_scores.get()
    assert np.array_equal(out[:8 * K].view(np.int64), scores) and (out[8 * K:] == 0xEE).all()
    for ptrs in ((None, d_scores.addr), (d_recs.addr, None), (None, None)):
        assert g.roll_score_pred(at, 0, device_ptrs=ptrs) == best
    for want in ((False, True), (True, False), (False, False)):
        got = g.roll_score_pred(at, 0, want=want)
        assert got[0] == best and (got[1] is None or np.array_equal(got[1], recs)) and (got[2] is None or np.array_equal(got[2], scores))
    pred, off = g.pred_plane()
    assert g.pred_plane(device_ptr=d_plane.addr) == (None, off)
    out = d_plane.get()
    assert np.array_equal(out[:4 * nx * nz].view(np.uint32).reshape(nz, nx), pred) and (out[4 * nx * nz:] == 0xEE).all()
    # free poses on the device: a heading that does not exist gives the mask 0
    rp, lists = PC.roll_of(g)
    poses = np.stack([np.arange(300) % nx, (np.arange(300) * 7) % nz, np.arange(300) % 64], 1).astype(np.int32)
    poses[7, 2], poses[9, 2] = 64, -1
    d_in, d_out = Dev(hip, poses), Dev(hip, 4 * 300 + 16)
    g.footprint_pred(device_ptrs=(d_in.addr, d_out.addr), n=300)
    out = d_out.get()
    want = PR.footprint_masks(lists, pred, off, poses)
    assert want[7] == want[9] == 0 and want.any() and np.array_equal(out[:1200].view(np.uint32), want) and (out[1200:] == 0xEE).all()
    d_img = Dev(hip, 3 * nx * nz + 16)
    g.render_pred(device_ptr=d_img.addr)
    out = d_img.get()
    assert np.array_equal(out[:3 * nx * nz].reshape(nz, nx, 3), g.render_pred()) and (out[3 * nx * nz:] == 0xEE).all()
    assert len(g.footprint_pred(np.zeros((0, 3), np.int32))) == 0
    g.close()


@pytest.mark.parametrize("K,T", [(1, 1), (1, 64), (65, 64), (65, 1), (3, 1024)])
def test_k_and_t_with_a_point_vehicle(G, K, T):
    """a wide, low window; the candidates run along +a on rows of their own, a cell per pose; a wall that comes towards them at two
    cells per step is met in some slot, a small block stands in the way of two of them"""
    nx, nz = (1100 if T == 1024 else 140), 70
    step = 1
    g = PC.new_grid(G, nx, nz, roll=dict(front=0.0, rear=0.0, half_width=0.0, w_cut=1), pred=dict(slots=16, margin=0))
    a_end = 1 + step * T                                                       # the cell of the last pose
    PC.play(g, PC.merged(PC.moving_block(nx, nz, min(a_end + 6, nx - 8), 0, 3, nz, -2, 0), PC.moving_block(nx, nz, 30, 0, 1, 3, 0, 0)))
    tab = straight(K, T, 0, step)
    g.set_candidates(tab)
    for kw in (dict(), dict(only_moving=0), dict(poses_per_step=64, slots=32), dict(stride=64, poses_per_step=16)):
        g.set_predict(**kw)
        best, recs, scores = PC.check_score(G, g, tab, PC.centre(1, 1), 0, "K %d T %d %r" % (K, T, kw), image=False)
    g.close()


def test_the_cut_at_pose_0_at_the_last_pose_and_beyond_the_last_slot(G):
    """standing one-cell objects, which hold every slot on their own cell, and a point vehicle that no cost stops (stop_cost 255 is
    above every cost there is): only the prediction cuts"""
    nx, nz = 80, 24
    g = PC.new_grid(G, nx, nz, roll=dict(front=0.0, rear=0.0, half_width=0.0, w_cut=1, stop_cost=255), pred=dict(slots=4, margin=0, only_moving=0))
    PC.play(g, [OC.Frame(nx, nz, [(9, 2), (20, 5), (40, 8), (71, 11)])] * 2)
    tab = straight(16, 12, 0, 1)                                               # candidate c runs along row c, pose t at column 9 + t
    g.set_candidates(tab)
    best, recs, scores = PC.check_score(G, g, tab, PC.centre(8, 0), 0, image=False)
    assert recs[2].tolist() == [0, PR.CUT_OBJECT, -1, 0, RR.FAR, 1] and scores[2] == RR.INFEASIBLE          # at pose 0, which is at slot 1
    assert recs[5, :2].tolist() == [11, PR.CUT_OBJECT] and recs[5, 5] == 3                                   # at the last pose, 12 steps ahead: the last slot
    assert recs[0, :2].tolist() == recs[8, :2].tolist() == [12, RR.COMPLETE] and recs[8, 5] == -1 and best >= 0
    g.close()


def test_a_footprint_longer_than_a_wave_and_equal_scores(G):
    nx, nz = 96, 64
    g = PC.new_grid(G, nx, nz, roll=dict(front=4.0, rear=2.0, half_width=1.5, w_cost=0, w_cut=1), pred=dict(margin=1))
    PC.play(g, crossing(nx, nz))
    rp, lists = PC.roll_of(g)
    assert max(len(l) for l in lists) > 64
    tab = np.repeat(G.arc_candidates(PC.CELL, 8, [0.0], 0.5, 30), 5, axis=1)    # five times the same arc: equal scores, the index decides
    g.set_candidates(tab)
    for set_, at in ((0, (10, 21)), (16, (20, 10)), (48, (40, 50))):
        best, recs, scores = PC.check_score(G, g, tab, PC.centre(*at), set_, "set %d" % set_, image=False)
        assert (scores == scores[0]).all() and best == (0 if scores[0] != RR.INFEASIBLE else -1)
    g.close()


def test_empty_tracks_score_as_roll_score(G):
    nx, nz = 64, 48
    g = PC.new_grid(G, nx, nz)
    PC.play(g, crossing())
    g.objects_reset()                                                          # the obstacles stay in COST; nothing predicts
    tab = G.arc_candidates(PC.CELL, 8, [-0.2, -0.05, 0.0, 0.05, 0.2], 0.5, 24)
    g.set_candidates(tab)
    for set_, at in ((16, (12, 4)), (0, (2, 21)), (32, (41, 20))):
        plain = g.roll_score(PC.centre(*at), set_)
        got = g.roll_score_pred(PC.centre(*at), set_)
        assert got[0] == plain[0] and np.array_equal(got[1][:, :5], plain[1]) and (got[1][:, 5] == -1).all() and np.array_equal(got[2], plain[2])
    assert g.pred_stats() == (0, 0, 0, 0)
    g.close()


def test_render_roll_keeps_drawing_the_last_roll_score(G):
    nx, nz = 64, 48
    g = PC.new_grid(G, nx, nz, pred=dict(only_moving=0))
    PC.play(g, crossing())
    tab = G.arc_candidates(PC.CELL, 8, [-0.1, 0.0, 0.1], 0.5, 20)
    g.set_candidates(tab)
    g.roll_score(PC.centre(2, 21), 0)
    img = g.render_roll()
    got = g.roll_score_pred(PC.centre(12, 4), 16)
    assert np.array_equal(g.render_roll(), img) and (got[1][:, 1] == PR.CUT_OBJECT).any()
    g.close()


def test_the_same_bytes_twice(G):
    nx, nz = 96, 64
    g = PC.new_grid(G, nx, nz, pred=dict(margin=2, grow16=8, only_moving=0))
    PC.play(g, crossing(nx, nz))
    tab = G.arc_candidates(PC.CELL, 8, [-0.2, -0.1, -0.05, 0.0, 0.05, 0.1, 0.2], 0.5, 40)
    other = straight(3, 5)
    at = PC.centre(12, 4)
    g.set_candidates(tab)
    a, plane_a = g.roll_score_pred(at, 16), g.pred_plane()[0]
    g.set_candidates(other)
    g.roll_score_pred(at, 0)
    g.set_predict(margin=2)                                                    # PRED is computed again, from the same state
    g.set_candidates(tab)
    b, plane_b = g.roll_score_pred(at, 16), g.pred_plane()[0]
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and plane_a.tobytes() == plane_b.tobytes()
    assert (a[1][:, 1] == PR.CUT_OBJECT).any() and plane_a.any()
    g.close()


def test_4096_tracks_through_the_object(G):
    """one-cell objects on every second cell of every second row of 128 x 128 cells; every 40th is absent in the first frame, the next
    of every 40 in the second, none in the third: the table is full and its ids are not contiguous"""
    nx = nz = 128
    g = PC.new_grid(G, nx, nz, obj=dict(max_tracks=4096), pred=dict(only_moving=0, margin=0, slots=32))
    k = np.arange(4096)
    frames = []
    for absent in (0, 1, None):
        f = OC.Frame(nx, nz)
        kk = k if absent is None else k[k % 40 != absent]
        f.state[2 * (kk // 64), 2 * (kk % 64)], f.hmax[2 * (kk // 64), 2 * (kk % 64)], f.count[2 * (kk // 64), 2 * (kk % 64)] = OR.OBSTACLE, 0.5, 1
        frames.append(f)
    PC.play(g, frames)
    ids = g.tracks()[:, 0]
    assert len(ids) == 4096 and ids[-1] > 4095 and (np.diff(ids) > 1).any()
    pred, stats, _ = PC.check_pred(g, "4096 tracks")
    assert stats == (4096, 4096, 4096, 2) and (pred[pred != 0] == 0xFFFFFFFF).all()
    g.set_predict(margin=1)
    assert PC.check_pred(g, "4096 tracks, radius 1")[1] == (4096, 4096, 128 * 128, 4)
    g.close()


def test_pipeline_grid_predict(G, tmp_path, monkeypatch, capsys):
    """--grid-predict DIR with --grid-objects and --grid-roll on the two golden frames: one image and one line of predict.jsonl per
    frame.  Two frames make no MOVING track (min_age is 3), so nothing predicts yet: the line's two bests and scores agree and the
    statistics of PRED say so; what a prediction does to a scoring is compared with the restatement above"""
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import stereomapper_pipeline as SP
    import test_rectify
    from test_grid_gpu import read_ppm
    from test_view_gpu import two_frame_drive
    drive = str(two_frame_drive(tmp_path / "drive"))
    calib = tmp_path / "calib_cam_to_cam.txt"
    calib.write_text(test_rectify.rig_calib_text())
    d, d2, d3, d4, d5, d6 = (str(tmp_path / n) for n in ("loc", "cost", "plan", "roll", "obj", "pred"))
    common = ["--grid-slope", "2.0", "--grid-inscribed", "0.1", "--grid-inflate", "0.5", "--grid-cell", "0.25", "--grid-size", "96x160", drive, str(calib)]
    monkeypatch.setattr(sys, "argv", ["stereomapper_pipeline.py", "--grid-local", d, "--grid-cost", d2, "--grid-plan", d3, "--grid-roll", d4,
                                      "--grid-roll-vehicle", "0,0,0", "--grid-roll-unknown", "0", "--grid-objects", d5, "--grid-objects-params",
                                      "2,300,0.4,3,1", "--grid-predict", d6, "--grid-predict-params", "12,2,2,8"] + common)
    SP.main()
    out = capsys.readouterr().out.splitlines()
    assert any(l.startswith("prediction: 12 slots of 2 steps, margin 2 cells growing 8/16 per slot:") and "2 images and predict.jsonl" in l for l in out), out[-6:]
    assert sorted(os.listdir(d6)) == ["predict.jsonl"] + ["predict_%06d.ppm" % k for k in range(2)]
    lines = [json.loads(l) for l in open(os.path.join(d6, "predict.jsonl"))]
    rolls = [json.loads(l) for l in open(os.path.join(d4, "roll.jsonl"))]
    assert [l["frame"] for l in lines] == [0, 1]
    for l, r in zip(lines, rolls):
        assert set(l) == {"frame", "set", "best", "best_pred", "cut_by_object", "score", "score_pred", "pred_stats"}
        assert (l["set"], l["best"], l["score"]) == (r["set"], r["best"], r["score"]) and len(l["pred_stats"]) == 4
        if l["cut_by_object"] == 0:
            assert (l["best_pred"], l["score_pred"]) == (l["best"], l["score"])
        assert l["pred_stats"][0] == 0 and l["pred_stats"][2] == 0               # two frames make no MOVING track: nothing predicts yet
    img = read_ppm(os.path.join(d6, "predict_%06d.ppm" % 1))
    assert img.shape == (160, 96, 3)

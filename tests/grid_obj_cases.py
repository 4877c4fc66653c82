"""The scenes behind tests/test_grid_obj.py (header against restatement) and tests/test_grid_obj_gpu.py (device against restatement): a
SCENARIO is a set of object parameters and a list of FRAMES; a frame is the obstacle cells of a window with their heights and point
counts, and the window's offsets.  The grid is rebuilt per frame, as a caller who tracks would do.  Three runners play a scenario
and return the same read-out per frame: the restatement (tests/grid_obj_ref.py), the header through the library's host test entries,
and the device through the Grid object.  Planes are indexed [ib, ia]."""
import numpy as np

import grid_obj_ref as OR

F = np.float32
CELL = 0.5


class Frame:
    def __init__(self, nx, nz, cells=(), off=(0, 0), height=0.5, count=3):
        """cells: (ia, ib) or (ia, ib, height) or (ia, ib, height, count)"""
        self.off = (int(off[0]), int(off[1]))
        self.state, self.hmax, self.count = np.zeros((nz, nx), np.uint8), np.full((nz, nx), np.nan, F), np.zeros((nz, nx), np.int32)
        for c in cells:
            self.put(*c) if len(c) > 2 else self.put(c[0], c[1], height, count)

    def put(self, ia, ib, height=0.5, count=3):
        self.state[ib, ia], self.hmax[ib, ia], self.count[ib, ia] = OR.OBSTACLE, F(height), count if count is not None else 3
        return self

    def block(self, a0, b0, w, h, height=0.5, count=3):
        for ib in range(b0, b0 + h):
            for ia in range(a0, a0 + w):
                self.put(ia, ib, height, count)
        return self

    @staticmethod
    def of_mask(mask, off=(0, 0), height=0.5, count=3):
        mask = np.asarray(mask, bool)
        f = Frame(mask.shape[1], mask.shape[0], off=off)
        f.state[mask], f.hmax[mask], f.count[mask] = OR.OBSTACLE, F(height), count
        return f


class Scenario:
    def __init__(self, name, frames, **params):
        self.name, self.frames, self.kw = name, frames, dict(dict(min_size=1, min_height=0.0), **params)
        self.nz, self.nx = frames[0].state.shape


def read_out(flags, label, recs, stats, assign, tracks, ids, ids_off, tstats):
    return dict(flags=np.asarray(flags, np.uint8), label=np.asarray(label, np.int32), recs=np.asarray(recs, np.int32).reshape(-1, 10),
                stats=tuple(int(v) for v in stats[:6]), assign=np.asarray(assign, np.int32), tracks=np.asarray(tracks, np.int32).reshape(-1, 14),
                ids=np.asarray(ids, np.int32), ids_off=tuple(ids_off), tstats=tuple(int(v) for v in tstats))


def run_ref(sc):
    p, trk, out = OR.ObjParams(**sc.kw), OR.Tracker(), []
    for f in sc.frames:
        flags, label, recs, stats = OR.objects(p, f.state, f.hmax, f.count, *f.off)
        assign = trk.step(p, recs, label, f.off)
        out.append(read_out(flags, label, recs, stats, assign, trk.tracks, trk.ids, trk.off, trk.track_stats()))
    return out


def run_header(G, sc):
    """the same through svh_test_grid_obj and svh_test_grid_obj_step, the state kept here"""
    p, out = G.default_obj(**sc.kw), []
    tracks, ids, ids_off, next_id, steps = np.zeros((0, 14), np.int32), None, (0, 0), 0, 0
    for f in sc.frames:
        flags, label, recs, stats = G.core_obj(p, f.state, f.hmax, f.count, *f.off)
        tracks, assign, ids, st, next_id = G.core_obj_step(p, recs, label, f.off, ids, ids_off, tracks if ids is not None else tracks[:0], next_id)
        ids_off, steps = f.off, steps + 1
        out.append(read_out(flags, label, recs, stats, assign, tracks, ids, ids_off, (steps,) + st[1:]))
    return out


def grid_kw(nx, nz):
    import grid_ref as R
    return dict(nx=nx, nz=nz, cell=CELL, x0=0.0, z0=0.0, T=np.asarray(R.frame_camera(1.5), np.float64), min_points=1, step=0.2, drop=0.3,
                clearance=1000.0)


def frame_points(f):
    """count points at the cell's height in the middle of every obstacle cell of the frame: float32 [n, 4].  Cell centres are multiples of
    0.25 and exact in fp32; a = x, b = z, h = 1.5 - y"""
    ib, ia = np.nonzero(f.state == OR.OBSTACLE)
    n = f.count[ib, ia]
    p = np.zeros((len(ia), 4), F)
    p[:, 0], p[:, 2] = (f.off[0] + ia + 0.5) * CELL, (f.off[1] + ib + 0.5) * CELL
    p[:, 1], p[:, 3] = F(1.5) - f.hmax[ib, ia], 0.5
    return np.repeat(p, n, axis=0)


def run_device(G, sc, g=None):
    """through the Grid object: clear, scroll to the frame's offsets, add the frame's points, step"""
    own = g is None
    g = g if g is not None else G.Grid(G.default_params(**grid_kw(sc.nx, sc.nz)))
    out = []
    try:
        g.set_objects(G.default_obj(**sc.kw))
        for f in sc.frames:
            g.clear()
            oa, ob = g.window()
            g.scroll(f.off[0] - oa, f.off[1] - ob)
            pts = frame_points(f)
            if len(pts):
                g.add_points(pts)
            assign = g.objects_step()
            ids, ids_off = g.track_plane()
            out.append(read_out(g.obj_plane(G.OBJ_FLAGS), g.obj_plane(G.OBJ_LABEL), g.objects(), g.object_stats(), assign, g.tracks(), ids, ids_off,
                                g.track_stats()))
            out[-1]["image"] = g.render_objects()
            out[-1]["class_image"] = g.render(G.RENDER_CLASS)
    finally:
        if own:
            g.close()
    return out


def same(got, want, tag=""):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        for name in ("flags", "label", "recs", "assign", "tracks", "ids"):
            assert a[name].shape == b[name].shape, (tag, k, name, a[name].shape, b[name].shape)
            assert np.array_equal(a[name], b[name]), (tag, k, name, a[name].ravel()[:40], b[name].ravel()[:40])
        for name in ("stats", "ids_off", "tstats"):
            assert a[name] == b[name], (tag, k, name, a[name], b[name])


# ---- the scenarios of the issue --------------------------------------------------------------------------------------------------
def moving_block(steps=9):
    """a 3 x 3 block that moves one cell per step along a, the grid rebuilt per step"""
    return Scenario("moving block", [Frame(24, 10).block(2 + k, 4, 3, 3) for k in range(steps)], min_age=3, move_cells=2, gate=0)


def merge_and_split(gate):
    """A (3 x 2, columns 2..4) and B (2 x 2, columns 6..7) apart; B one cell closer, touching A; apart again"""
    apart = lambda: Frame(16, 8).block(2, 2, 3, 2).block(6, 2, 2, 2)
    joined = Frame(16, 8).block(2, 2, 3, 2).block(5, 2, 2, 2)
    return Scenario("merge and split", [apart(), joined, apart()], gate=gate, max_missed=2)


def jump(gate):
    """a 2 x 2 block that moves 5 cells, further than its own length"""
    return Scenario("jump", [Frame(20, 8).block(2, 3, 2, 2), Frame(20, 8).block(7, 3, 2, 2)], gate=gate)


def scrolled():
    """two blocks that stand still in the world while the window scrolls under them"""
    offs = [(0, 0), (3, -2), (3, -2), (-1, 1)]
    return Scenario("scroll", [Frame(24, 16, off=o).block(8 - o[0], 6 - o[1], 2, 3).block(14 - o[0], 9 - o[1], 3, 1) for o in offs], gate=0)


def leaving():
    """a block that leaves the window by its side, and the track that is dropped after max_missed steps"""
    frames = [Frame(12, 6).block(min(8 + k, 12), 2, min(2, max(0, 12 - 8 - k)), 2).block(1, 1, 2, 2) for k in range(7)]
    return Scenario("leaving", frames, gate=2, max_missed=1)


def full_table():
    return Scenario("full table", [Frame(12, 4, [(1, 1), (4, 1), (7, 1)]), Frame(12, 4, [(1, 1), (4, 1), (7, 1)])], max_tracks=2, gate=0)


def missed(max_missed):
    """a block that is there, gone for two steps, there again.  The ID plane of an empty step holds no id, so only the gate can find the
    track again"""
    there, gone = lambda: Frame(10, 6).block(3, 2, 2, 2), lambda: Frame(10, 6)
    return Scenario("missed %d" % max_missed, [there(), gone(), gone(), there()], max_missed=max_missed, gate=2)


def overlap_bound(min_overlap):
    """a 3 x 1 block that moves one cell: two cells of overlap"""
    return Scenario("overlap %d" % min_overlap, [Frame(10, 4).block(2, 1, 3, 1), Frame(10, 4).block(3, 1, 3, 1)], min_overlap=min_overlap, gate=0)


def random_history(seed, nx, nz, steps=5, density=0.08, **kw):
    """blobs that drift, appear and vanish, with a window that scrolls now and then"""
    rng = np.random.default_rng(seed)
    n = max(2, int(density * nx * nz / 6))
    pos = np.stack([rng.integers(0, nx, n), rng.integers(0, nz, n)], 1)
    size = rng.integers(1, 4, (n, 2))
    off, frames = np.zeros(2, np.int64), []
    for _ in range(steps):
        f = Frame(nx, nz, off=tuple(off))
        for (a, b), (w, h) in zip(pos, size):
            if rng.random() < 0.15:
                continue
            for ib in range(b, b + h):
                for ia in range(a, a + w):
                    if 0 <= ia - off[0] < nx and 0 <= ib - off[1] < nz:
                        f.put(ia - off[0], ib - off[1], 0.25 + 0.25 * int(rng.integers(0, 8)), int(rng.integers(1, 5)))
        frames.append(f)
        pos += rng.integers(-2, 3, pos.shape)
        if rng.random() < 0.4:
            off += rng.integers(-3, 4, 2)
    kw = dict(dict(min_size=int(rng.integers(1, 4)), max_size=int(rng.integers(6, 40)), min_height=float(rng.choice([0.0, 0.5, 1.0])),
                   max_tracks=int(rng.choice([3, 16, 4096])), min_overlap=int(rng.integers(1, 3)), gate=int(rng.choice([0, 2, 6])),
                   max_missed=int(rng.integers(0, 3)), min_age=int(rng.integers(0, 3)), move_cells=int(rng.integers(1, 4)),
                   smooth_shift=int(rng.integers(0, 5))), **kw)
    return Scenario("random %d" % seed, frames, **kw)


SCENARIOS = [moving_block, lambda: merge_and_split(0), lambda: merge_and_split(4), lambda: jump(0), lambda: jump(6), scrolled, leaving, full_table,
             lambda: missed(0), lambda: missed(2), lambda: overlap_bound(2), lambda: overlap_bound(3)]

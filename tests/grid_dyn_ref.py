"""The dynamics of the ground grid (stereo-vision_amd/csrc/grid_dyn_core.h; include/svh_grid.h, "DYNAMICS") restated in numpy
and plain Python integers, on top of tests/grid_local_ref.py: the three phases of an observation -- the frame record, the sight
lines with their heights, the settle -- the planes of the layer, its statistics and its render.  tests/test_grid_dyn.py pins it
by hand and compares the header with it; tests/test_grid_dyn_gpu.py compares the device with it, bit for bit.

Every plane is kept in logical order (there is no torus here); a scroll is an array shift."""
import numpy as np

import grid_local_ref as LR
import grid_ref as R

F = R.F
CLEARED, AGED, CONFIRMED = 1, 2, 4
EVENT_COLOUR = (255, 0, 255)
STAMP_LIMIT = 2 ** 31 - 1
MARGIN_LIMIT = F(1048576.0)
STATS = ("observations", "cleared", "aged", "confirmed")


class DynParams:
    """svh_grid_dyn_params with margin_q; ValueError where svh_grid_set_dynamics says SVH_ERR_BAD_ARG"""

    def __init__(self, clear_frames=2, min_through=3, margin=0.1, max_age=0):
        with np.errstate(all="ignore"):
            m = F(margin)
        ok = (0 <= clear_frames <= 65535 and min_through >= 1 and np.isfinite(m) and F(0) <= m < MARGIN_LIMIT and max_age >= 0 and
              max(clear_frames, min_through, max_age) < 2 ** 31)
        if not ok:
            raise ValueError("dyn parameters out of range")
        self.clear_frames, self.min_through, self.margin, self.max_age = int(clear_frames), int(min_through), m, int(max_age)
        self.margin_q = int(np.rint(m * F(1024.0)))


def rdiv64(p, n):
    """floor((2 p + n) / (2 n)) on Python integers (or int64 arrays well inside their range): // floors, also below zero"""
    return (2 * p + n) // (2 * n)


def q_of_key(key):
    """a key's height in 1/1024: int64 array"""
    return np.rint(R.height_of(key) * F(1024.0)).astype(np.int64)


def line_height(q_o, q_e, n, k):
    return q_o + rdiv64(k * (q_e - q_o), n)


def body(P, D, count, kmin, kmax):
    """(lo, hi) int64 per stored cell; (1, 0) where the cell is not tall"""
    count = np.asarray(count)
    with np.errstate(invalid="ignore"):
        tall = (count > 0) & (R.height_of(kmax).reshape(count.shape) > P.step)
    lo = np.where(tall, q_of_key(np.where(tall, kmin, R.key_of(F(0)))).reshape(count.shape), 1)
    hi = np.where(tall, q_of_key(np.where(tall, kmax, R.key_of(F(0)))).reshape(count.shape) - D.margin_q, 0)
    return lo.astype(np.int64), hi.astype(np.int64)


def settle_cell(P, D, stamp, cell, contra, last, frame, through):
    """settle() on one cell, plain Python: cell and frame are [count, overhead, kmin, kmax, hsum, vsum]; returns (cell', contra',
    last', event)"""
    count, over, kmin, kmax, hsum, vsum = (int(v) for v in cell)
    fc, fo, fkmin, fkmax, fhs, fvs = (int(v) for v in frame)
    step = P.step

    def height(key):
        return R.height_of(np.uint32(key))[()]

    ev = 0
    if fc > 0 and height(fkmax) > step:
        contra, ev = 0, ev | CONFIRMED
    elif count > 0 and height(kmax) > step and through >= D.min_through:
        contra += 1
    if D.clear_frames > 0 and contra >= D.clear_frames:
        count, kmin, kmax, hsum, vsum = 0, int(R.KMIN_EMPTY), int(R.KMAX_EMPTY), 0, 0
        contra, ev = 0, ev | CLEARED
    if D.max_age > 0 and (count > 0 or over > 0) and stamp - last > D.max_age:
        count, over, kmin, kmax, hsum, vsum = 0, 0, int(R.KMIN_EMPTY), int(R.KMAX_EMPTY), 0, 0
        contra = 0
        if not ev & CLEARED:
            ev |= AGED
    cell = [count + fc, over + fo, min(kmin, fkmin), max(kmax, fkmax), hsum + fhs, vsum + fvs]
    if fc > 0 or fo > 0:
        last = stamp
    return cell, contra, last, ev


class Grid(LR.Grid):
    """grid_local_ref.Grid with the dynamics: set_dynamics, observe, the three planes, the statistics, the render"""

    def __init__(self, P, D=None):
        self.D = D
        super().__init__(P)

    def clear(self):
        super().clear()
        n = self.P.nx * self.P.nz
        self.contra, self.last, self.kept = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.event = np.zeros(n, np.uint8)
        self.stamp = 0
        self.dyn_stats = dict.fromkeys(STATS, 0)

    def set_dynamics(self, D):
        """None drops the layer: its planes are empty when it is set again"""
        if D is None or self.D is None:
            n = self.P.nx * self.P.nz
            self.contra, self.last, self.kept = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
            self.event = np.zeros(n, np.uint8)
        self.D = D

    def scroll(self, da, db):
        super().scroll(da, db)
        sh = (self.P.nz, self.P.nx)
        for name in ("contra", "last", "kept", "event"):
            setattr(self, name, LR.shifted(getattr(self, name).reshape(sh), da, db, 0).ravel())
        return self

    def observe(self, pts, origin):
        P, D, nx = self.P, self.D, self.P.nx
        if D is None:
            raise ValueError("the dynamics are not set")
        oc = self.origin_cell(origin)
        if self.stamp >= STAMP_LIMIT:
            raise ValueError("out of stamps")
        o = np.asarray(origin, np.float64).reshape(3)
        q_o = int(LR.place(P, self.oa, self.ob, np.array([[o[0], o[1], o[2], 0.0]]).astype(F))[3][0])
        stamp = self.stamp + 1
        n = nx * P.nz
        # phase 1: the frame record
        fate, cell, key, q, v = LR.place(P, self.oa, self.ob, pts)
        low, ov = fate == R.LOW, fate == R.OVERHEAD
        c = cell[low].astype(np.int64)
        fcount, fover = np.zeros(n, np.int32), np.zeros(n, np.int32)
        fkmin, fkmax = np.full(n, R.KMIN_EMPTY, np.uint32), np.full(n, R.KMAX_EMPTY, np.uint32)
        fhsum, fvsum = np.zeros(n, np.int64), np.zeros(n, np.uint64)
        np.add.at(fcount, c, 1)
        np.minimum.at(fkmin, c, key[low])
        np.maximum.at(fkmax, c, key[low])
        np.add.at(fhsum, c, q[low].astype(np.int64))
        np.add.at(fvsum, c, v[low].astype(np.uint64))
        np.add.at(fover, cell[ov].astype(np.int64), 1)
        for name, f in (("binned", R.LOW), ("overhead", R.OVERHEAD), ("outside", R.OUTSIDE), ("unplaced", R.UNPLACED)):
            self.stats[name] += int((fate == f).sum())
        self.stats["added"] += len(fate)
        # phase 2: the sight lines, the closed form for 1024 end cells at a time, all their k at once
        lo, hi = body(P, D, self.count, self.kmin, self.kmax)
        through = np.zeros(n, np.int64)
        ends = np.nonzero(fcount > 0)[0]
        w = fcount[ends].astype(np.int64)
        self.rays += int(w.sum())
        oa, ob = oc % nx, oc // nx
        for at in range(0, len(ends), 1024):
            e, we = ends[at:at + 1024], w[at:at + 1024]
            dx, dz = e % nx - oa, e // nx - ob
            ln = np.maximum(np.abs(dx), np.abs(dz))
            k = np.arange(max(int(ln.max()), 1), dtype=np.int64)[None, :]
            nn = np.maximum(ln, 1)[:, None]
            ca = oa + (2 * k * dx[:, None] + nn) // (2 * nn)
            cb = ob + (2 * k * dz[:, None] + nn) // (2 * nn)
            dq = (q_of_key(fkmin[e]) - q_o)[:, None]          # |k dq| < 2^13 * 2^31: int64 holds it twice over
            qk = q_o + (2 * k * dq + nn) // (2 * nn)
            live = k < ln[:, None]
            idx = np.where(live, cb * nx + ca, 0)
            assert ((ca >= 0) & (ca < nx) & (cb >= 0) & (cb < P.nz))[live].all()
            wk = np.broadcast_to(we[:, None], live.shape)
            np.add.at(self.passed, idx[live], wk[live].astype(np.int32))
            thr = live & (lo[idx] <= qk) & (qk <= hi[idx])
            np.add.at(through, idx[thr], wk[thr])
            self.ray_cells += int((we * ln).sum())
        # phase 3: settle, vectorised in the order of settle_cell
        with np.errstate(invalid="ignore"):
            confirm = (fcount > 0) & (R.height_of(fkmax) > P.step)
            tall = (self.count > 0) & (R.height_of(self.kmax) > P.step)
        contra = self.contra.astype(np.int64)
        contra = np.where(confirm, 0, np.where(tall & (through >= D.min_through), contra + 1, contra))
        cleared = (contra >= D.clear_frames) if D.clear_frames > 0 else np.zeros(n, bool)
        for name, empty in (("count", 0), ("kmin", R.KMIN_EMPTY), ("kmax", R.KMAX_EMPTY), ("hsum", 0), ("vsum", 0)):
            a = getattr(self, name)
            a[cleared] = empty
        contra[cleared] = 0
        old = (((self.count > 0) | (self.over > 0)) & (stamp - self.last.astype(np.int64) > D.max_age)) if D.max_age > 0 else np.zeros(n, bool)
        for name, empty in (("count", 0), ("over", 0), ("kmin", R.KMIN_EMPTY), ("kmax", R.KMAX_EMPTY), ("hsum", 0), ("vsum", 0)):
            a = getattr(self, name)
            a[old] = empty
        contra[old] = 0
        aged = old & ~cleared
        self.count += fcount
        self.over += fover
        self.kmin, self.kmax = np.minimum(self.kmin, fkmin), np.maximum(self.kmax, fkmax)
        self.hsum += fhsum
        self.vsum += fvsum
        self.last = np.where((fcount > 0) | (fover > 0), stamp, self.last).astype(np.int32)
        self.contra = contra.astype(np.int32)
        self.kept = through.astype(np.int32)
        self.event = (np.where(confirm, CONFIRMED, 0) | np.where(cleared, CLEARED, 0) | np.where(aged, AGED, 0)).astype(np.uint8)
        self.stamp = stamp
        self.dyn_stats["observations"] = stamp
        self.dyn_stats["cleared"] += int(cleared.sum())
        self.dyn_stats["aged"] += int(aged.sum())
        self.dyn_stats["confirmed"] += int(confirm.sum())
        return self

    def dyn_planes(self):
        sh = (self.P.nz, self.P.nx)
        age = np.where(self.last == 0, -1, self.stamp - self.last.astype(np.int64)).astype(np.int32)
        return dict(age=age.reshape(sh), contra=self.contra.reshape(sh).copy(), through=self.kept.reshape(sh).copy())

    def render_dyn(self):
        return colour_dyn(self.render_local()[::-1], self.contra.reshape(self.P.nz, self.P.nx), self.event.reshape(self.P.nz, self.P.nx))[::-1].copy()


def colour_dyn(local_rgb, contra, event):
    """[..., 3] uint8 in cell order from the local colours: the tint of CONTRA > 0, then the event colour"""
    rgb = np.array(local_rgb, np.uint8)
    c = rgb[..., :2].astype(np.int64)
    rgb[..., :2] = np.where((np.asarray(contra) > 0)[..., None], c + (255 - c) // 2, c).astype(np.uint8)
    rgb[(np.asarray(event) & (CLEARED | AGED)) != 0] = EVENT_COLOUR
    return rgb

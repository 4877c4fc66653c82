"""GPU: scene `collide` (tests/golden/recon_collide.npz; what it contains is asserted in tests/test_recon_collide.py)
through the resident track table (k_rt_* of recon_track_kernels.hip) and through a host-table object, against the
reference's record.  Only committed fixtures are read.

The comparisons are Runner.check's of tests/test_recon_resident_gpu.py, after EVERY update of every setting: the
number of active tracks, the outcome code of every lost track in order, the appended points as float32 bytes, and at
the end the whole point array.  No tolerance.

In the batch test `collide` objects run beside `shared` and `edge` objects in one svh_recon_update_batch per step:
sizes from 0 to 3000 side by side under grids sized by the largest, a second `collide` object two updates behind the
first (so 3000 tracks are lost in one object while another extends 2049), and objects that sit out."""
import os

import numpy as np
import pytest

import helpers as H
import recon_ref as R
from test_recon_resident_gpu import Runner

pytestmark = pytest.mark.gpu

SHARED = os.path.join(H.GOLDEN, "recon_shared.npz")


@pytest.fixture(scope="module")
def Z():
    """the three fixtures as one"""
    out = {}
    for path in (R.GOLDEN, SHARED, R.COLLIDE_GOLDEN):
        with np.load(path) as z:
            if "calib" in out:
                assert np.array_equal(z["calib"], out["calib"])
            names = list(out.get("scene_names", [])) + list(z["scene_names"])
            out.update({k: z[k] for k in z.files})
            out["scene_names"] = np.array(names)
    return out


@pytest.fixture(scope="module")
def S():
    import svhip
    return svhip


def settings_of(Z):
    return range(len(Z["collide_settings"]))


def test_resident_object_from_host_matches(S, Z):
    for j in settings_of(Z):
        Runner(S, Z, "collide", j).run()


def test_resident_object_from_device_matches(S, Z):
    for j in settings_of(Z):
        Runner(S, Z, "collide", j, how="device").run()


def test_host_table_object(S, Z):
    for j in settings_of(Z):
        Runner(S, Z, "collide", j, resident=False).run()


def index_of(Z, name, setting):
    hit = [j for j, s in enumerate(Z["%s_settings" % name]) if tuple(s) == tuple(setting)]
    assert len(hit) == 1, (name, setting)
    return hit[0]


@pytest.mark.parametrize("setting", [(0.0, 2.0, 30.0, 2.0), (1.0, 3.0, 30.0, 2.0)])
def test_batch_beside_shared_and_edge(S, Z, setting):
    """object i joins at step start[i]; every fourth step one live object sits out and catches up later"""
    names = ["collide", "shared", "edge", "collide", "shared", "collide"]
    start = [0, 0, 0, 2, 5, 7]
    group = [Runner(S, Z, n, index_of(Z, n, setting)) for n in names]
    sizes, step = set(), 0
    while not all(g.done() for g in group):
        live = [step >= s0 and not g.done() for g, s0 in zip(group, start)]
        if step % 4 == 3:
            on = [i for i, ok in enumerate(live) if ok]
            live[on[(step // 4) % len(on)]] = False
        ms = [g.matches() if ok else None for g, ok in zip(group, live)]
        Trs = [g.scene[g.k][0] if ok else None for g, ok in zip(group, live)]
        before = [(g.rec.num_points(), g.rec.num_tracks()) for g in group]
        sizes.add((min(len(m) for m in ms if m is not None), max(len(m) for m in ms if m is not None)) if any(live)
                  else (0, 0))
        status = S.Reconstruction.update_batch([g.rec for g in group], ms, Trs, *group[0].settings())
        assert status == [0] * len(group), step
        for g, ok, b in zip(group, live, before):
            if ok:
                g.check(b[0])
            else:
                assert (g.rec.num_points(), g.rec.num_tracks()) == b
        step += 1
    assert any(lo <= 1 and hi >= 3000 for lo, hi in sizes), sorted(sizes)     # 0 or 1 matches beside 3000
    for g in group:
        g.finish()

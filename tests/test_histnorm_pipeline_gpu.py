"""GPU: tools/stereomapper_pipeline.py --normalize.  The pipeline that equalises every pair on the device, in place
where ELAS and the visual odometry read it, gives bit for bit what the plain pipeline gives on pairs equalised by the
numpy restatement (tests/histnorm_ref.py): visual odometry status, poses and both point lists per frame -- host frames,
resident frames, and two drives in lockstep."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import helpers as H
import histnorm_ref as R

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
pytestmark = pytest.mark.gpu

CALIB = (645.24, 635.96, 194.13, 0.5707)                               # libviso2 demo.cpp calibration


def darker(img, num, den):
    return (img.astype(np.int64) * num // den).astype(np.uint8)


@pytest.fixture(scope="module")
def drives():
    """two drives of 4 frames from the reference's two consecutive quad pairs; the right camera is exposed differently,
    which is what the equalisation is for"""
    quad = [H.read_pgm(os.path.join(H.GOLDEN, "viso_%s.pgm" % n)) for n in ("I1p", "I2p", "I1c", "I2c")]
    a = [(quad[0], darker(quad[1], 3, 4)), (quad[2], darker(quad[3], 3, 4))] * 2
    b = [(darker(l, 7, 8), r) for l, r in a]
    return [a, b]


def run_single(SP, drive, resident, normalize):
    p = SP.Pipeline(*CALIB, resident=resident, normalize=normalize)
    p.vo.lib.svh_vo_set_private_rand.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
    p.vo.lib.svh_vo_set_private_rand(p.vo.h, 1, 0)
    out = []
    for l, r in drive:
        ok, n0, n1 = p.push(l.copy(), r.copy())
        out.append((ok, n0, n1, p.poses[-1].tobytes(), p.map.points(0).tobytes(), p.map.points(1).tobytes()))
    return out


@pytest.fixture(scope="module")
def want(drives):
    """per drive: the plain resident pipeline on pairs equalised by the restatement"""
    import stereomapper_pipeline as SP
    out = [run_single(SP, [(R.normalize(l)[0], R.normalize(r)[0]) for l, r in d], True, False) for d in drives]
    assert out[0][0][0] is False and any(x[0] for x in out[0][1:]) and out[0][-1][2] > 1000
    return out


@pytest.mark.parametrize("resident", [False, True])
def test_normalize_in_the_pipeline_equals_equalised_input(drives, want, resident):
    import stereomapper_pipeline as SP
    got = run_single(SP, drives[0], resident, True)
    plain = run_single(SP, drives[0], resident, False)
    for k in range(4):
        assert got[k][:3] == want[0][k][:3], (k, got[k][:3], want[0][k][:3])
        assert got[k][3:] == want[0][k][3:], k
    assert plain[-1][5] != got[-1][5]                                  # ... and the flag is not a no-op


def test_normalize_in_lockstep_equals_single_pipelines(drives, want):
    import stereomapper_pipeline as SP
    lp = SP.LockstepPipeline(2, *CALIB, private_rand=0, normalize=True)
    for k in range(4):
        res = lp.push([d[k] for d in drives])
        for i in range(2):
            got = res[i] + (lp.poses[i][-1].tobytes(), lp.maps[i].points(0).tobytes(), lp.maps[i].points(1).tobytes())
            assert got[:3] == want[i][k][:3], (k, i, got[:3], want[i][k][:3])
            assert got[3:] == want[i][k][3:], (k, i)

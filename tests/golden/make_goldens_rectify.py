"""Writes tests/golden/rectify.npz: calibrations, small sources, expected maps and expected outputs of the rectification
(include/svh_rectify.h).

PRODUCED BY THE RESTATEMENT tests/rectify_ref.py, and labelled so inside the file: the reference's two OpenCV calls
(stereomapper/framecapturethread.cpp:100-131, 328-349) cannot be compiled or run here.  The fixture therefore pins the
kernels and the C++ core to the stated arithmetic; the arithmetic itself is pinned by the hand-derived answers and the
round trip of tests/test_rectify.py.

    python tests/golden/make_goldens_rectify.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rectify_ref as R  # noqa: E402


def pack_cam(cam):
    return np.concatenate([cam["K"].ravel(), cam["D"], cam["R"].ravel(), cam["P"].ravel()])


def main():
    z = {"produced_by": np.array("tests/rectify_ref.py (numpy restatement; NOT an OpenCV run)")}
    S = R.distinct_source(R.HAND_W, R.HAND_H)
    z["hand_src"] = S
    z["hand_names"] = np.array([n for n, _ in R.hand_cases()])
    for name, cam in R.hand_cases():
        mx, my = R.maps(cam, R.HAND_W, R.HAND_H)
        z[name + "_cam"], z[name + "_mx"], z[name + "_my"] = pack_cam(cam), mx, my
        for border in (R.WRAP, R.ZERO):
            z["%s_out%d" % (name, border)] = R.remap(S, mx, my, border)
    z["shape_names"] = np.array([n for n, _ in R.shape_cases()])
    for k, (name, (cam, sw, sh, dw, dh)) in enumerate(R.shape_cases()):
        S = R.source(sw, sh, seed=k)
        mx, my = R.maps(cam, dw, dh)
        z[name + "_cam"], z[name + "_size"] = pack_cam(cam), np.array([sw, sh, dw, dh], np.int32)
        z[name + "_src"], z[name + "_mx"], z[name + "_my"] = S, mx, my
        outs = [R.remap(S, mx, my, border) for border in (R.WRAP, R.ZERO)]
        z[name + "_out0"], z[name + "_out1"] = outs
        inside = (mx >= 0) & (mx < sw - 1) & (my >= 0) & (my < sh - 1)
        if name == "outside":
            assert not inside.any() and not outs[1].any() and outs[0].any()
        elif name == "seam":                      # both axes cross the seam inside the destination
            x0, y0 = np.floor(mx).astype(int), np.floor(my).astype(int)
            assert (x0 == sw - 1).any() and (y0 == sh - 1).any() and (x0 >= sw).any() and (y0 >= sh).any()
        elif dw * dh >= 300:                      # the larger shapes sample inside and beyond the source
            assert inside.any() and not inside.all() and not np.array_equal(*outs)
    for c, cam in enumerate(R.RIG):
        mx, my = R.maps(cam, *R.RIG_DST)
        S = R.source(*R.RIG_SRC, seed=c)
        z["rig%d_cam" % c] = pack_cam(cam)
        z["rig%d_mx" % c], z["rig%d_my" % c] = R.window(mx), R.window(my)
        for border in (R.WRAP, R.ZERO):
            z["rig%d_out%d" % (c, border)] = R.window(R.remap(S, mx, my, border))
    z["rig_window"] = np.array(R.RIG_WINDOW, np.int32)
    np.savez_compressed(R.GOLDEN, **z)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

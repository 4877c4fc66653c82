#!/usr/bin/env python3
"""Time the 2-D panes (include/svh_view2d.h) on the device.

Per pane size (1242 x 375, the KITTI frame, and 621 x 188) and content:

    grey          svh_view2d_set_image from a device frame (viso_I1c, 1344 x 391) + render, no matches
    grey_matches  the same + svh_view2d_set_matches from device arrays: the Matcher's quad matches of the golden libviso2
                  frames (at most 3000 of them), inlier flags from the visual odometry run on exactly those
    disparity     svh_view2d_set_disparity from a device map (1242 x 375 floats, the golden urban D1 tiled) + render
    disparity_via_host   the same pane by the only route there was before: svh_disparity_colormap from the device map
                  to three floats per pixel on the host, then quantisation and nearest resampling in numpy

Per case 5 warm-up and 20 timed repetitions of the WHOLE sequence set_* + render into a device buffer, each bracketed by
two HIP events -- the object's own stream is not exposed, so the events go to the null stream and a device
synchronisation orders them around the calls; the interval therefore contains everything the calls do, host work
included.  Reported: median, minimum, maximum in ms.  One JSON line per case goes to
profiles/view2d_render_times.jsonl.

    python tools/gpu_view2d.py [--out FILE]

There is no threshold: this is a measurement.  No kernel trace is taken, so the split over the kernels is not known."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_view import TIMED, WARMUP, Timer   # noqa: E402

SIZES = [(1242, 375), (621, 188)]
MATCHES = 3000


def upload(timer, a):
    a = np.ascontiguousarray(a)
    p = timer.malloc(max(a.nbytes, 16))
    assert timer.hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p


def real_matches():
    """(matches, flags): the first MATCHES quad matches of the golden frames and their inliers"""
    import helpers as H
    frames = [[H.read_pgm(os.path.join(H.GOLDEN, "viso_I%d%s.pgm" % (k, t))) for k in (1, 2)] for t in ("p", "c")]
    mt = H.ProductMatcher(H.matcher_defaults())
    mt.push_back(*frames[0])
    mt.push_back(*frames[1])
    mt.match(2)
    m = mt.matches()[:MATCHES]
    vo = H.ProductVo(H.vo_defaults())
    flags = np.zeros(len(m), np.uint8)
    if vo.process_matches(m) == 1:
        flags[vo.inliers()] = 1
    return m, flags, frames[1][0]


def measure(timer, call):
    for _ in range(WARMUP):
        call()
    ms = sorted(timer.ms(call) for _ in range(TIMED))
    return 0.5 * (ms[TIMED // 2 - 1] + ms[TIMED // 2]), ms[0], ms[-1]


def main():
    import helpers as H
    import svhip
    from svhip import mapper, view2d
    out = os.path.join(ROOT, "profiles", "view2d_render_times.jsonl")
    args = sys.argv[1:]
    while args:
        a = args.pop(0)
        if a == "--out":
            out = args.pop(0)
        else:
            raise SystemExit(__doc__)
    if svhip.device_count() < 1:
        raise SystemExit("gpu_view2d needs a GPU: libsvhip has no CPU fallback")
    timer = Timer()
    build = svhip.lib().svh_version().decode()
    m, flags, I = real_matches()
    ih, iw = I.shape
    z = np.load(os.path.join(H.GOLDEN, "urban3_demo.npz"))
    l, _ = H.golden_pair(str(z["crop"]))
    D = np.tile(z["d1"].reshape(l.shape), (2, 2))[:375, :1242].copy()
    dh, dw = D.shape
    dI, dD, dm, df = upload(timer, I), upload(timer, D), upload(timer, m), upload(timer, flags)
    rgb = timer.malloc(1242 * 375 * 3)
    L = mapper._bind()
    lines = []
    for W, Ht in SIZES:
        v = view2d.View2D(W, Ht)

        def grey():
            v.set_image_device(dI.value, iw, ih, iw)
            v.render(device_ptr=rgb.value)

        def grey_matches():
            v.set_image_device(dI.value, iw, ih, iw)
            v.set_matches_device(dm.value, len(m), df.value, True)
            v.render(device_ptr=rgb.value)

        def disparity():
            v.clear_matches()          # set_disparity keeps the matches of the case before
            v.set_disparity_device(dD.value, dw, dh)
            v.render(device_ptr=rgb.value)

        floats = np.empty((dh, dw, 3), np.float32)
        sy = ((2 * np.arange(Ht) + 1) * dh) // (2 * Ht)
        sx = ((2 * np.arange(W) + 1) * dw) // (2 * W)

        def disparity_via_host():
            assert L.svh_disparity_colormap(dD.value, 1, dw * dh, floats.ctypes.data) == 0
            tex = np.floor(np.clip(floats, 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
            return tex[sy][:, sx]

        for name, call, n in (("grey", grey, 0), ("grey_matches", grey_matches, len(m)), ("disparity", disparity, 0),
                              ("disparity_via_host", disparity_via_host, 0)):
            med, lo, hi = measure(timer, call)
            rec = {"case": name, "width": W, "height": Ht, "matches": n, "inliers": int(flags.sum()) if n else 0,
                   "source": [dw, dh] if name.startswith("disparity") else [iw, ih], "warmup": WARMUP, "timed": TIMED,
                   "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                   "timed_with": "HIP events around the whole sequence of calls", "build": build}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        # the two routes show the same pane
        disparity()
        got = np.zeros(W * Ht * 3, np.uint8)
        assert timer.hip.hipMemcpy(C.c_void_p(got.ctypes.data), rgb, C.c_size_t(got.nbytes), 2) == 0
        assert np.array_equal(got.reshape(Ht, W, 3), disparity_via_host())
        v.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

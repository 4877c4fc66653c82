#!/usr/bin/env python3
"""Times svh_rectify_pairs_device (include/svh_rectify.h) on the GPU: a 1392x512 source rectified to 1242x375 with the
KITTI-like rig of tests/rectify_ref.py, n = 1, 4 and 32 pairs per call, both border modes.  Appends one JSON line per
run to profiles/rectify_times.jsonl (or --out): ms per call (median of the device time between HIP events, and the
host's wall time), ms per pair, the bytes of the kernel's byte model and the GB/s they amount to.

Byte model per image: 8 bytes of table in and 1 byte out per output pixel, and the source image once
(1392 * 512 / (1242 * 375) = 1.53 source bytes per output pixel).

Every configuration runs in a child process of its own under `timeout`; the parent stops at the first child that does
not end cleanly.

    python tools/gpu_rectify.py [--calls 30] [--out profiles/rectify_times.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def worker(n, border, calls):
    import numpy as np
    import rectify_ref as R
    import svhip
    from svhip import rectify as SR
    hip = C.CDLL("libamdhip64.so")
    (sw, sh), (dw, dh) = R.RIG_SRC, R.RIG_DST

    def dev(nbytes, fill=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        if fill is not None:
            assert hip.hipMemcpy(p, C.c_void_p(fill.ctypes.data), C.c_size_t(fill.nbytes), 1) == 0
        return p

    src = [np.stack([R.source(sw, sh, seed=2 * k + c) for k in range(n)]) for c in range(2)]
    dS = [dev(s.nbytes, s) for s in src]
    dI = [dev(n * dw * dh) for _ in range(2)]
    r = SR.Rectifier(SR.params((sw, sh), (dw, dh), R.RIG, border))
    r.set_timing(True)

    def call():
        t = time.perf_counter()
        r.pairs_device(n, dS[0].value, dS[1].value, sw, sw * sh, dI[0].value, dI[1].value, dw, dw * dh)
        return 1e3 * (time.perf_counter() - t), float(r.timing()[0])

    _, maps_ms = call()[0], float(r.timing()[1])
    for _ in range(3):
        call()
    t = np.array([call() for _ in range(calls)])
    # one image back, against the restatement: a timing of wrong output is worth nothing
    out = np.zeros(dw * dh, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), dI[1], C.c_size_t(out.nbytes), 2) == 0
    mx, my = R.maps(R.RIG[1], dw, dh)
    assert np.array_equal(out.reshape(dh, dw), R.remap(src[1][0], mx, my, border))
    model = 2 * n * (9 * dw * dh + sw * sh)
    dev_ms = float(np.median(t[:, 1]))
    line = {"tool": "gpu_rectify", "version": svhip.lib().svh_version().decode(), "src": [sw, sh], "dst": [dw, dh],
            "pairs": n, "border": "wrap" if border == SR.WRAP else "zero", "calls": calls,
            "ms_per_call_device": round(dev_ms, 5), "ms_per_call_device_min": round(float(t[:, 1].min()), 5),
            "ms_per_call_wall": round(float(np.median(t[:, 0])), 5), "ms_per_pair_device": round(dev_ms / n, 6),
            "maps_kernel_ms": round(maps_ms, 5), "model_bytes": model, "model_GBps": round(model / dev_ms / 1e6, 1)}
    for p in dS + dI:
        hip.hipFree(p)
    r.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_times.jsonl"))
    ap.add_argument("--worker", nargs=2, type=int, metavar=("PAIRS", "BORDER"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], a.worker[1], a.calls)
    for border in (0, 1):
        for n in (1, 4, 32):
            cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--calls", str(a.calls),
                   "--worker", str(n), str(border)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            sys.stderr.write(p.stderr)
            if p.returncode != 0:
                sys.exit("gpu_rectify: n = %d border = %d ended with status %d; stopping" % (n, border, p.returncode))
            line = p.stdout.strip().splitlines()[-1]
            json.loads(line)
            print(line, flush=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""What the 16-bit and left-only outputs are worth to a host caller: the host-buffer stream and the batch entry with
{f32, both} (the existing entries), {u16, both} and {u16, left}, in one process.

    python tools/gpu_stream_u16.py [--frames 430] [--passes 4] [--reps 7] [--limit 60] [--out profiles/stream_u16_times.jsonl]

Input: the four urban 1242 x 375 crops of tests/golden, repeated to --frames pairs in pinned host memory; the maps come
back to pinned host memory too.  Library defaults otherwise (workers, pairs per launch, stage), svh_init before the HIP
runtime starts.
    stream   ElasStream.push_n in rings of 43 frames with a consumer thread in pop_n, --passes x --frames pairs as one
             stream, timed from the first push to the last pop
    batch    one svh_elas_process_batch[_out] call of --frames pairs
After a warm-up of every variant (whose 16-bit maps must equal the float maps passed through the numpy restatement of the
encoding, tests/disp_u16_ref.py, or the tool stops) the three variants ALTERNATE, --reps rounds, the order rotating
from round to round, so each round is a paired comparison under the same conditions.  Every timed step runs under its
own time limit (--limit seconds: a step that does not come back ends the process with status 124, nothing else is
started), and the tool stops at the first step that fails.

One JSON line per entry and variant: pairs/s as median, 10th and 90th percentile, the paired ratio against {f32, both}
of the same round (median, p10, p90), and the bytes of maps copied down per pair as the engine counted them
(svh_test_d2h_map_bytes).  The file is rewritten by every run.  Method: a host clock around whole calls that end in the
library's own waits."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CROPS = ["urban1_1242x375", "urban2_1242x375", "urban3_1242x375", "urban4_1242x375"]
VARIANTS = [("f32", "both"), ("u16", "both"), ("u16", "left")]
RING = 43


class step_limit:
    """a time limit of its own for one step: the process ends with status 124 if the step does not come back"""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self.expired, (seconds, what))
        self.t.daemon = True

    @staticmethod
    def expired(seconds, what):
        sys.stderr.write("gpu_stream_u16: %s did not finish within %d s: stopping\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()


def pinned(hip, nbytes):
    p = C.c_void_p()
    if hip.hipHostMalloc(C.byref(p), C.c_size_t(nbytes), C.c_uint(0)) != 0:
        raise SystemExit("hipHostMalloc of %d bytes failed" % nbytes)
    return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p.value))


def quantiles(x):
    x = np.sort(np.asarray(x, np.float64))
    q = lambda f: float(x[int(f * (len(x) - 1))])
    return {"median": round(float(np.median(x)), 4), "p10": round(q(0.1), 4), "p90": round(q(0.9), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=430)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=60, help="seconds a single step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_u16_times.jsonl"))
    a = ap.parse_args()

    import svhip as S
    import disp_u16_ref as R
    import helpers as H
    info = S.init()                       # before the first HIP call: the hardware-queue count is asked for here
    if S.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    L = S.lib()
    hip = C.CDLL("libamdhip64.so")
    prm = H.robotics()
    e = S.Elas(prm)
    crops = [H.golden_pair(c) for c in CROPS]
    h, w = crops[0][0].shape
    n, dn = a.frames, w * h

    I1 = pinned(hip, n * dn).reshape(n, h, w)
    I2 = pinned(hip, n * dn).reshape(n, h, w)
    for i in range(n):
        I1[i], I2[i] = crops[i % 4]
    raw1, raw2 = pinned(hip, n * dn * 4), pinned(hip, n * dn * 4)     # the maps of every variant in turn
    maps = {}
    for out, which in VARIANTS:
        dt, size = (np.uint16, 2) if out == "u16" else (np.float32, 4)
        maps[(out, which)] = (raw1[:n * dn * size].view(dt).reshape(n, h, w),
                              raw2[:n * dn * size].view(dt).reshape(n, h, w) if which == "both" else None)
    arr = C.c_void_p * n
    a1 = arr(*[int(I1[i].ctypes.data) for i in range(n)])
    a2 = arr(*[int(I2[i].ctypes.data) for i in range(n)])
    ptrs = {v: (arr(*[int(D1[i].ctypes.data) for i in range(n)]),
                arr(*[int(D2[i].ctypes.data) for i in range(n)]) if D2 is not None else None)
            for v, (D1, D2) in maps.items()}
    dims = (C.c_int32 * 3)(w, h, w)
    streams = {v: e.stream(w, h, out=v[0], maps=v[1]) for v in VARIANTS}

    def sub(p, r0, k):
        return (C.c_void_p * k)(*p[r0:r0 + k]) if p is not None else None

    def run_stream(v, passes):
        s, (d1, d2), got = streams[v], ptrs[v], []
        cons = threading.Thread(target=lambda: got.extend(s.pop_n(passes * n)))
        t0 = time.perf_counter()
        cons.start()
        for _ in range(passes):
            for r0 in range(0, n, RING):
                k = min(RING, n - r0)
                s.push_n_raw(k, sub(a1, r0, k), sub(a2, r0, k), sub(d1, r0, k), sub(d2, r0, k))
        s.flush()
        cons.join()
        dt = time.perf_counter() - t0
        if got != [0] * (passes * n):
            raise SystemExit("stream %s/%s: a pair failed: %r" % (v[0], v[1], [x for x in got if x][:4]))
        return passes * n / dt

    def run_batch(v, passes):
        st = (C.c_int32 * n)()
        t0 = time.perf_counter()
        if v == ("f32", "both"):
            rc = L.svh_elas_process_batch(e._h, n, a1, a2, ptrs[v][0], ptrs[v][1], dims, st)
        else:
            rc = L.svh_elas_process_batch_out(e._h, n, a1, a2, ptrs[v][0], ptrs[v][1], dims, st,
                                              C.byref(S.ElasOutput(S.DISP_U16 if v[0] == "u16" else S.DISP_F32,
                                                                   S.MAPS_LEFT if v[1] == "left" else S.MAPS_BOTH)))
        dt = time.perf_counter() - t0
        if rc != 0 or list(st) != [0] * n:
            raise SystemExit("batch %s/%s: status %d: %s" % (v[0], v[1], rc, S.last_error()))
        return n / dt

    counts = (C.c_int64 * 2)()
    lines = []
    for entry, run, passes in (("stream", run_stream, a.passes), ("batch", run_batch, 1)):
        # warm-up of every variant, and the check of what came back
        want = {}
        per_pair = {}
        for v in VARIANTS:
            raw1[:] = 0
            raw2[:] = 0
            with step_limit(a.limit, "%s warm-up %s/%s" % (entry, *v)):
                run(v, 1)
                L.svh_test_d2h_map_bytes(counts, 1)
                run(v, 1)
            L.svh_test_d2h_map_bytes(counts, 1)
            per_pair[v] = counts[0] / n
            D1, D2 = maps[v]
            if v == ("f32", "both"):
                want = {i: (R.pack(D1[i]), R.pack(D2[i])) for i in (0, 1, 2, 3, n // 2, n - 1)}
            else:
                for i, (u1, u2) in want.items():
                    if not np.array_equal(D1[i], u1) or (D2 is not None and not np.array_equal(D2[i], u2)):
                        raise SystemExit("%s %s/%s: frame %d differs from the packed float maps" % (entry, *v, i))
        rates = {v: [] for v in VARIANTS}
        for rep in range(a.reps):
            for k in range(len(VARIANTS)):
                v = VARIANTS[(k + rep) % len(VARIANTS)]
                with step_limit(a.limit, "%s round %d %s/%s" % (entry, rep, *v)):
                    rates[v].append(run(v, passes))
        base = np.asarray(rates[("f32", "both")])
        for v in VARIANTS:
            line = {"tool": "gpu_stream_u16", "entry": entry, "format": v[0], "maps": v[1], "frames": n,
                    "pairs_per_timed_step": passes * n, "rounds": a.reps, "size": [w, h],
                    "pairs_per_s": quantiles(rates[v]), "ratio_to_f32_both": quantiles(np.asarray(rates[v]) / base),
                    "map_bytes_down_per_pair": per_pair[v], "image_bytes_up_per_pair": 2 * dn,
                    "settings": S.elas_settings(), "runtime": info,
                    "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "build": L.svh_version().decode()}
            lines.append(line)
            print(json.dumps(line), flush=True)
    for s in streams.values():
        s.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
